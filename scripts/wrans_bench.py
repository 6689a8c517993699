"""Times LightWeightCheckerboard.compress / decompress with the host rANS coder (compressai's
format, thread pool) and with the device coder (HRW1, csrc/wrans.hip), in one run on the GPU and on the same build:

  * shapes 1 x 3 x 512 x 768 and 16 x 3 x 256 x 256, recipe weights, update() run, a seeded residual-like input;
  * wall time per call: a host clock from the call to a device synchronise after it, ``--iters`` calls per coder after
    ``--warmup`` calls, the two coders alternating call by call; median, minimum and maximum are reported;
  * the total bytes of the strings of each coder, and whether decompress gives the same x_hat with both.

Nothing is required of the ratio: the device coder is opt-in whatever it shows.  The result goes to ``--out`` (default
profiles/wrans.json) and to stdout.

    python scripts/wrans_bench.py [--out profiles/wrans.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "hyres-residual-enhanced-hybrid-image-compression_amd")
for _p in (PKG, REPO):
    if _p not in sys.path:
        sys.path.insert(0, _p)

SHAPES = ((1, 3, 512, 768), (16, 3, 256, 256))


def residual_like(shape, seed):
    """A smooth field plus noise in about [-0.3, 0.3]: what x - jpeg_decoded looks like at a low JPEG quality."""
    import torch
    g = torch.Generator().manual_seed(seed)
    low = torch.nn.functional.interpolate(torch.randn((shape[0], 3, shape[2] // 16, shape[3] // 16), generator=g),
                                          size=shape[2:], mode="bilinear", align_corners=False)
    return (0.1 * low + 0.03 * torch.randn(shape, generator=g)).clamp(-0.5, 0.5)


def stats(ms):
    return {"median_ms": round(statistics.median(ms), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "wrans.json"))
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()

    import torch
    from hyres_hip.weights import synthetic_state_dict
    from models import ResidualJPEGCompression
    assert torch.cuda.is_available(), "this benchmark needs the GPU"
    dev = torch.device("cuda:0")
    net = ResidualJPEGCompression(jpeg_quality=1)
    torch.nn.Module.load_state_dict(net, synthetic_state_dict(net.state_dict()), strict=True)
    rm = net.residual_model.to(dev).eval()
    rm.update(force=True)
    res = {"device": torch.cuda.get_device_name(0), "iters": args.iters, "warmup": args.warmup,
           "timed": "LightWeightCheckerboard.compress / .decompress, host clock to a device synchronise after the call",
           "weights": "recipe (hyres_hip.weights.synthetic_state_dict)", "input": "seeded smooth field + noise",
           "shapes": {}}

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1000, out

    for shape in SHAPES:
        x = residual_like(shape, 1).to(dev)
        ms = {(c, op): [] for c in ("host", "device") for op in ("compress", "decompress")}
        last = {}
        for it in range(args.warmup + args.iters):
            for coder in ("host", "device"):
                rm.device_coder = coder == "device"
                tc, c = timed(lambda: rm.compress(x))
                td, d = timed(lambda: rm.decompress(c["strings"], c["shape"]))
                if it >= args.warmup:
                    ms[(coder, "compress")].append(tc)
                    ms[(coder, "decompress")].append(td)
                last[coder] = (c, d)
        r = {}
        for coder in ("host", "device"):
            c, d = last[coder]
            (a, na), z = c["strings"]
            r[coder] = {"compress": stats(ms[(coder, "compress")]), "decompress": stats(ms[(coder, "decompress")]),
                        "string_bytes": sum(len(s) for s in a + na + z),
                        "string_bytes_y_z": [sum(len(s) for s in a + na), sum(len(s) for s in z)]}
        r["x_hat_equal"] = bool(torch.equal(last["host"][1]["x_hat"], last["device"][1]["x_hat"]))
        r["device_over_host"] = {op: round(r["device"][op]["median_ms"] / r["host"][op]["median_ms"], 3)
                                 for op in ("compress", "decompress")}
        res["shapes"]["x".join(map(str, shape))] = r
    rm.device_coder = False

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
    return 0 if all(r["x_hat_equal"] for r in res["shapes"].values()) else 1


if __name__ == "__main__":
    sys.exit(main())
