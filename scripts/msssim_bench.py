"""Measures the HIP MS-SSIM metric (hyres_hip.metrics.ms_ssim, csrc/msssim.hip) in one run on the GPU:

  * accuracy: every shape x distortion of tests/msssim_ref.py — the fp64 restatement's value, d = |restatement in
    fp32 - in fp64| (the reference's own rounding error, which sets the tests' bound max(8 d, 16 * 2^-24)), and the
    error of the device path and of the host twin against the fp64 restatement, for ``out`` and for ``per_level``;
  * time: 1x3x512x768 (one Kodak image as the CLI sees it) and 16x3x256x256 — the HIP path against the torch-op
    restatement run in fp32 on the same GPU (what pytorch_msssim's call executes there), each as ``--iters`` eager
    calls between HIP events after ``--warmup`` calls, and as replays of a captured graph (device time without the
    host's launch cost); kernel launches per call and the level-0 kernel's own time from a kernel trace
    (torch.profiler) taken after the timed loops, and from it level 0's achieved bytes/s against its algorithmic
    minimum: one read of X and Y plus one write of the pooled pair.

The HIP path must not be slower than the torch-op form at either shape (eager and graph), else the script exits 1.
The result goes to ``--out`` (default profiles/msssim.json) and to stdout.

    python scripts/msssim_bench.py [--out profiles/msssim.json]
"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "hyres-residual-enhanced-hybrid-image-compression_amd")
for _p in (PKG, REPO, os.path.join(REPO, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

HBM_PEAK = 8.0e12  # bytes/s, MI355X spec


def timed(torch, call, warmup, iters):
    for _ in range(warmup):
        call()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(iters):
        call()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def graphed(torch, call):
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        call()
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        call()
    return g.replay


def kernel_trace(torch, call, n=5):
    """[(kernel name, microseconds)] of ``n`` calls in start order, or None where the tracer gives no device events."""
    try:
        from torch.autograd import DeviceType
        from torch.profiler import ProfilerActivity, profile
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            for _ in range(n):
                call()
            torch.cuda.synchronize()
        ev = [e for e in prof.events() if e.device_type == DeviceType.CUDA and "emcpy" not in e.name]
        ev.sort(key=lambda e: e.time_range.start)
        return [(e.name, float(e.device_time)) for e in ev] or None
    except Exception as exc:  # the trace is a report, never a gate
        print(f"kernel trace unavailable: {exc!r}", file=sys.stderr)
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "msssim.json"))
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--no-accuracy", action="store_true")
    args = ap.parse_args()

    import torch
    import msssim_ref as R
    from hyres_hip import metrics
    assert torch.cuda.is_available(), "this benchmark needs the GPU"
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "iters": args.iters, "warmup": args.warmup,
           "bound": "max(8 * d, 16 * 2^-24); d per case for out, per case and level for per_level"}

    if not args.no_accuracy:
        acc = {}
        for shape in R.SHAPES:
            for dist in R.DISTORTIONS:
                ref = R.case(shape, dist)
                row = {"ref": [round(v, 7) for v in ref["out"].tolist()], "d_out": float(ref["d_out"].max()),
                       "d_per_level": [float(v) for v in ref["d_raw"][:, 0, 0]]}
                for tag, (x, y) in (("device", (ref["x"].to(dev), ref["y"].to(dev))), ("host", (ref["x"], ref["y"]))):
                    out, raw = metrics.per_level(x, y)
                    e_raw = (raw.cpu().double() - ref["raw"]).abs()
                    row[f"{tag}_err_out"] = float((out.cpu().double() - ref["out"]).abs().max())
                    row[f"{tag}_err_per_level"] = [float(v) for v in e_raw.flatten(1).max(1).values]
                    row[f"{tag}_within_bound"] = bool(((out.cpu().double() - ref["out"]).abs() <= ref["tol_out"]).all()
                                                      and (e_raw <= ref["tol_raw"]).all())
                acc["x".join(map(str, shape)) + "-" + dist] = row
        res["accuracy"] = acc

    ok = True
    res["timing"] = {}
    for shape in ((1, 3, 512, 768), (16, 3, 256, 256)):
        x, y = (t.to(dev) for t in R.make_pair(shape, "noise", seed=5))
        hip = lambda: metrics.ms_ssim(x, y)  # noqa: E731
        ops = lambda: R.ms_ssim_ref(x, y, torch.float32)[0].mean()  # noqa: E731
        r = {"ms_ssim_hip": float(hip()), "ms_ssim_torch_ops_fp32": float(ops())}
        hip_g = graphed(torch, hip)
        try:
            ops_g = graphed(torch, ops)
        except Exception as exc:  # the torch-op form is the baseline; if it cannot be captured, only eager is compared
            print(f"torch-op form not captured: {exc!r}", file=sys.stderr)
            ops_g = None
        # alternate the two versions; keep the best of three windows each
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
        ok = ok and r["hip_eager_ms"] <= r["torch_ops_eager_ms"]
        if ops_g is not None:
            r["speedup_graph"] = round(r["torch_ops_graph_ms"] / r["hip_graph_ms"], 2)
            ok = ok and r["hip_graph_ms"] <= r["torch_ops_graph_ms"]

        n = 5
        tr_hip, tr_ops = kernel_trace(torch, hip, n), kernel_trace(torch, ops, n)
        B, C, H, W = shape
        Hp, Wp = (H + 2 * (H % 2) - 2) // 2 + 1, (W + 2 * (W % 2) - 2) // 2 + 1
        min_bytes = 4 * B * C * (2 * H * W + 2 * Hp * Wp)
        r["level0_min_bytes"] = min_bytes
        r["launches_per_call_hip"] = len(tr_hip) // n if tr_hip else "not measured (by construction: 5 level kernels + 1 finalize + torch's mean)"
        r["launches_per_call_torch_ops"] = len(tr_ops) // n if tr_ops else "not measured"
        lv = [us for name, us in tr_hip if "msssim_level" in name] if tr_hip else []
        if len(lv) == 5 * n:
            l0 = sorted(lv[0::5])[n // 2]  # the first level kernel of each call; median of n
            r["level0_kernel_us"] = round(l0, 2)
            r["level_kernels_us"] = [round(sorted(lv[k::5])[n // 2], 2) for k in range(5)]
            r["level0_achieved_bytes_per_s"] = round(min_bytes / (l0 * 1e-6), 1)
            r["level0_fraction_of_hbm_peak_8TBs"] = round(min_bytes / (l0 * 1e-6) / HBM_PEAK, 4)
            fin = [us for name, us in tr_hip if "msssim_finalize" in name]
            r["finalize_kernel_us"] = round(sorted(fin)[len(fin) // 2], 2) if fin else None
        else:
            r["level0_kernel_us"] = r["level0_achieved_bytes_per_s"] = "not measured"
        res["timing"]["x".join(map(str, shape))] = r

    res["pass"] = bool(ok)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
