"""Measures the MS-SSIM forward + backward (hyres_hip.metrics.ms_ssim under autograd, csrc/msssim.hip) in one run on
the GPU, by scripts/msssim_bench.py's protocol (HIP events, ``--warmup`` calls, ``--iters`` timed calls, the best of
three alternating windows):

  * accuracy: the gradient's error against autograd through the fp64 restatement for the tests' cases
    (tests/msssim_bwd_ref.py), with d, the bound and the scale;
  * time: 1x3x512x768 and 16x3x256x256, forward + backward towards the second image, the HIP path against autograd
    through the fp32 torch-op restatement on the same GPU, eager and as replays of a captured graph; the per-kernel
    trace of one HIP call, and the level-0 backward kernels' achieved bytes/s against their algorithmic minimum;
  * with ``--step``: the captured training step at 16x3x256x256 (fp32) with metric="ms-ssim" against metric="mse".

The result goes to ``--out`` (default profiles/msssim_bwd.json) and to stdout.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from msssim_bench import HBM_PEAK, REPO, graphed, kernel_trace, timed  # noqa: E402  (also sets sys.path)


def accuracy(torch, metrics, dev):
    import msssim_bwd_ref as G
    acc = {}
    cases = [(s, d, None) for s, d in G.PARITY] + [(s, "noise", w) for s, w in G.REDUCED]
    for shape, dist, w in cases:
        ref = G.case(shape, dist, w) if w else G.case(shape, dist)
        row = {"max_abs_g64": float(ref["g64"].abs().max()), "d": ref["d"], "s": ref["s"], "bound": ref["tol"]}
        for tag, D in (("device", dev), ("host", torch.device("cpu"))):
            g = G.device_grad(metrics, ref["x"].to(D), ref["y"].to(D), w)
            row[f"{tag}_err"] = float((g.cpu().double() - ref["g64"]).abs().max())
            row[f"{tag}_within_bound"] = row[f"{tag}_err"] <= ref["tol"]
        acc["x".join(map(str, shape)) + "-" + dist + (f"-levels{len(w)}" if w else "")] = row
    return acc


def step_cost(torch, args, dev):
    """The captured training step (bs 16, 256 x 256, fp32) with each criterion, alternating, best of three windows."""
    import msssim_ref as R
    from hyres_hip.graphs import CapturedStep
    from hyres_hip.loss import RateDistortionLoss
    from hyres_hip.weights import synthetic_state_dict
    from models import ResidualJPEGCompression
    import torch.nn.functional as F
    net = ResidualJPEGCompression(jpeg_quality=50)
    torch.nn.Module.load_state_dict(net, synthetic_state_dict(net.state_dict()), strict=True)
    net = net.to(dev).train()
    x = R.smooth_field((16, 3, 256, 256), 3)
    j = F.conv2d(F.pad(x, (2, 2, 2, 2), mode="replicate"), torch.full((3, 1, 5, 5), 1 / 25.0), groups=3)
    x, j = x.to(dev), j.to(dev)
    params = [p for p in net.parameters() if p.requires_grad]

    def zero():
        for p in params:
            if p.grad is not None:
                p.grad.zero_()

    caps = {m: CapturedStep(net, x, j, 0.25, criterion=RateDistortionLoss(lmbda=0.045 if m == "mse" else 8.0, alpha=0,
                                                                          metric=m), zero_grad=zero)
            for m in ("mse", "ms-ssim")}
    t = {m: [] for m in caps}
    for _ in range(3):
        for m, cap in caps.items():
            t[m].append(timed(torch, cap.replay, 5, args.step_iters))
    r = {f"{m}_step_ms": round(min(v), 4) for m, v in t.items()}
    r.update({f"{m}_step_ms_windows": [round(u, 4) for u in v] for m, v in t.items()})
    r["ms_ssim_cost_ms"] = round(r["ms-ssim_step_ms"] - r["mse_step_ms"], 4)
    for cap in caps.values():
        cap.close()
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "msssim_bwd.json"))
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--step", action="store_true", help="also time the captured training step with each criterion")
    ap.add_argument("--step-iters", type=int, default=20)
    args = ap.parse_args()

    import torch
    import msssim_ref as R
    from hyres_hip import metrics
    assert torch.cuda.is_available(), "this benchmark needs the GPU"
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "iters": args.iters, "warmup": args.warmup,
           "bound": "max(8 * d, 16 * 2^-24 * s); d = max|g32 - g64| of the case, s = max|g64| of the shape's noise case",
           "accuracy": accuracy(torch, metrics, dev), "timing": {}}

    for shape in ((1, 3, 512, 768), (16, 3, 256, 256)):
        x, y = (t.to(dev) for t in R.make_pair(shape, "noise", seed=5))
        y.requires_grad_(True)
        hip = lambda: torch.autograd.grad(metrics.ms_ssim(x, y), y)[0]  # noqa: E731
        ops = lambda: torch.autograd.grad(R.ms_ssim_ref(x, y, torch.float32)[0].mean(), y)[0]  # noqa: E731
        r = {"max_abs_diff_of_the_two_gradients": float((hip() - ops()).abs().max()),
             "max_abs_gradient": float(ops().abs().max())}
        hip_g = graphed(torch, hip)
        try:
            ops_g = graphed(torch, ops)
        except Exception as exc:  # the torch-op form is the baseline; if it cannot be captured, only eager is compared
            print(f"torch-op form not captured: {exc!r}", file=sys.stderr)
            ops_g = None
        t = {"hip_eager": [], "torch_ops_eager": [], "hip_graph": [], "torch_ops_graph": []}
        for _ in range(3):
            t["hip_eager"].append(timed(torch, hip, args.warmup, args.iters))
            t["torch_ops_eager"].append(timed(torch, ops, args.warmup, args.iters))
            t["hip_graph"].append(timed(torch, hip_g, args.warmup, args.iters))
            if ops_g is not None:
                t["torch_ops_graph"].append(timed(torch, ops_g, args.warmup, args.iters))
        for k, v in t.items():
            r[f"{k}_ms"] = round(min(v), 5) if v else "not measured"
            r[f"{k}_ms_windows"] = [round(u, 5) for u in v]
        r["speedup_eager"] = round(r["torch_ops_eager_ms"] / r["hip_eager_ms"], 2)
        if ops_g is not None:
            r["speedup_graph"] = round(r["torch_ops_graph_ms"] / r["hip_graph_ms"], 2)

        n = 5
        tr = kernel_trace(torch, hip, n)
        tr_ops = kernel_trace(torch, ops, n)
        r["launches_per_call_torch_ops"] = len(tr_ops) // n if tr_ops else "not measured"
        if tr and len(tr) % n == 0:
            per = len(tr) // n
            r["launches_per_call_hip"] = per
            # one call's kernels in start order, each the median of n calls
            r["kernel_trace_us"] = [[tr[k][0].split("(")[0], round(sorted(u for _, u in tr[k::per])[n // 2], 2)]
                                    for k in range(per)]
            B, C, H, W = shape
            planes, outs = B * C * H * W, B * C * (H - 10) * (W - 10)
            coef = [u for name, u in r["kernel_trace_us"] if "msssim_coef" in name]
            grad = [u for name, u in r["kernel_trace_us"] if "msssim_grad" in name]
            if len(coef) == 5 and len(grad) == 5:  # level 0 runs last
                # coef: reads X, Y, writes three maps; grad: reads three maps, X, Y and a quarter-size plane, writes G
                cb, gb = 4 * (2 * planes + 3 * outs), 4 * (3 * outs + 3 * planes + planes // 4)
                r["level0_coef_kernel"] = {"us": coef[-1], "min_bytes": cb, "bytes_per_s": round(cb / (coef[-1] * 1e-6), 1),
                                           "fraction_of_hbm_peak_8TBs": round(cb / (coef[-1] * 1e-6) / HBM_PEAK, 4)}
                r["level0_grad_kernel"] = {"us": grad[-1], "min_bytes": gb, "bytes_per_s": round(gb / (grad[-1] * 1e-6), 1),
                                           "fraction_of_hbm_peak_8TBs": round(gb / (grad[-1] * 1e-6) / HBM_PEAK, 4)}
        else:
            r["kernel_trace_us"] = "not measured"
        res["timing"]["x".join(map(str, shape))] = r

    if args.step:
        res["train_step_16x3x256x256_fp32_captured"] = step_cost(torch, args, dev)

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
