"""Times LightWeightCheckerboard.compress / decompress with the host rANS coder, the device coder's format HRW1 (one
wave per string) and its segmented format HRW2 (one wave per segment of R rows) at R in {128, 256, 512, 1024} and at an
R that leaves every string one segment, in one run on the GPU and on the same build. The protocol is that of
scripts/wrans_bench.py:

  * shapes 1 x 3 x 512 x 768 and 16 x 3 x 256 x 256, recipe weights, update() run, a seeded residual-like input;
  * wall time per call: a host clock from the call to a device synchronise after it, ``--iters`` calls per coder after
    ``--warmup`` calls, the coders alternating call by call; median, quartiles and interquartile range are reported;
  * the total bytes of the strings of each coder, and whether decompress gives the same x_hat as the host coder.

``comparisons`` holds what the acceptance of HRW2 reads, against HRW1 in the same run: at one image and R = 512 both
medians below HRW1's by more than the larger of the two interquartile ranges; at 16 x 256^2 and R = 512 (one segment per
string) not above HRW1's by more than that spread. The result goes to ``--out`` (default profiles/wrans2.json) and to
stdout; the exit status is 0 if every x_hat is equal, whatever the timings show.

    python scripts/wrans2_bench.py [--out profiles/wrans2.json]
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

from wrans_bench import SHAPES, residual_like  # noqa: E402  (scripts/ is sys.path[0])

ONE_SEGMENT = 1 << 21
# name -> (device_coder, coder_segment_rows)
CODERS = {"host": (False, 0), "hrw1": (True, 0), "hrw2_r128": (True, 128), "hrw2_r256": (True, 256),
          "hrw2_r512": (True, 512), "hrw2_r1024": (True, 1024), "hrw2_one_segment": (True, ONE_SEGMENT)}
OPS = ("compress", "decompress")


def stats(ms):
    q1, med, q3 = statistics.quantiles(ms, n=4)
    return {"median_ms": round(med, 3), "q1_ms": round(q1, 3), "q3_ms": round(q3, 3), "iqr_ms": round(q3 - q1, 3),
            "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3)}


def compare(r, a, b):
    """Medians of coder ``a`` against ``b`` with the larger of their interquartile ranges as the run's spread."""
    out = {}
    for op in OPS:
        sa, sb = r[a][op], r[b][op]
        spread = max(sa["iqr_ms"], sb["iqr_ms"])
        diff = round(sa["median_ms"] - sb["median_ms"], 3)
        out[op] = {"median_ms": sa["median_ms"], "against_median_ms": sb["median_ms"], "difference_ms": diff,
                   "spread_ms": spread, "below_by_more_than_spread": diff < -spread,
                   "not_above_by_more_than_spread": diff <= spread}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "wrans2.json"))
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
           "coders": {k: {"device_coder": v[0], "coder_segment_rows": v[1]} for k, v in CODERS.items()},
           "shapes": {}}

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1000, out

    for shape in SHAPES:
        x = residual_like(shape, 1).to(dev)
        ms = {(c, op): [] for c in CODERS for op in OPS}
        last = {}
        for it in range(args.warmup + args.iters):
            for coder, (on_device, rows) in CODERS.items():
                rm.device_coder, rm.coder_segment_rows = on_device, rows
                tc, c = timed(lambda: rm.compress(x))
                td, d = timed(lambda: rm.decompress(c["strings"], c["shape"]))
                if it >= args.warmup:
                    ms[(coder, "compress")].append(tc)
                    ms[(coder, "decompress")].append(td)
                last[coder] = (c, d)
        r = {}
        for coder in CODERS:
            c, d = last[coder]
            (a, na), z = c["strings"]
            r[coder] = {"compress": stats(ms[(coder, "compress")]), "decompress": stats(ms[(coder, "decompress")]),
                        "string_bytes": sum(len(s) for s in a + na + z),
                        "string_bytes_y_z": [sum(len(s) for s in a + na), sum(len(s) for s in z)],
                        "x_hat_equals_host": bool(torch.equal(last["host"][1]["x_hat"], d["x_hat"]))}
        npix = shape[0] * shape[2] * shape[3]
        for coder in CODERS:
            r[coder]["bytes_over_hrw1"] = r[coder]["string_bytes"] - r["hrw1"]["string_bytes"]
            r[coder]["bytes_over_host"] = r[coder]["string_bytes"] - r["host"]["string_bytes"]
            r[coder]["bpp_over_hrw1"] = round(8 * r[coder]["bytes_over_hrw1"] / npix, 5)
        r["comparisons"] = {"hrw2_r512_vs_hrw1": compare(r, "hrw2_r512", "hrw1"),
                            "hrw2_r512_vs_host": compare(r, "hrw2_r512", "host")}
        res["shapes"]["x".join(map(str, shape))] = r
    rm.device_coder, rm.coder_segment_rows = False, 0

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
    return 0 if all(r[c]["x_hat_equals_host"] for r in res["shapes"].values() for c in CODERS) else 1


if __name__ == "__main__":
    sys.exit(main())
