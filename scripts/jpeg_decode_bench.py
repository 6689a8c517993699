"""Times ``TurboJPEGCompression.decompress`` from BytesIO buffers to a device tensor, in one run on the GPU:

  * the device decoder (hyres_hip.jpeg_device.decode: header parse, one pinned upload, the HIP kernels, the status
    read-back) against the host path (Pillow on the thread pool, stack, pageable upload), on 1 x 3 x 512 x 768 and
    16 x 3 x 256 x 256, qualities 1 / 50 / 95, on the fixture's Kodak crop tiled to the size and on uniform noise;
  * the kernels alone (decode_tensors on a staged batch) over sub_bits x work-group size — the sweep the library's
    defaults were picked from;
  * ``net.decompress`` of one 512 x 768 image with both device coders on (device JPEG codec, device rANS coder with
    512-row segments): with the JPEG files decoded by Pillow, which is what ``decompress`` did before the device
    decoder existed, and with the device decoder.

Every figure is the median and the interquartile range of ``--iters`` (>= 50) calls after ``--warmup`` calls, each
call between two HIP events on an otherwise idle stream (the events see the host's share too: the stream waits for
it).  Reads nothing outside the repository.  Writes ``--out`` (default profiles/jpeg_decode.json) and stdout.

    python scripts/jpeg_decode_bench.py [--out profiles/jpeg_decode.json]

``--shape B H W`` (repeatable), ``--qualities``, ``--contents`` and ``--no-sweep`` narrow the run; a shape that is
not whole 16x8 MCUs is coded and decoded through the any-size entry points (``any_size=True``).
"""
import argparse
import io
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "hyres-residual-enhanced-hybrid-image-compression_amd")
for _p in (PKG, REPO):
    if _p not in sys.path:
        sys.path.insert(0, _p)


def timed(fn, iters, warmup):
    import numpy as np
    import torch
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    q1, med, q3 = np.percentile(ms, [25, 50, 75])
    return {"median_ms": round(float(med), 4), "iqr_ms": round(float(q3 - q1), 4)}


def content(kind, B, H, W):
    """[B,3,H,W] fp32 of bytes / 255: the fixture's 64 x 64 Kodak crop mirrored out to the size, or uniform noise."""
    import numpy as np
    import torch
    if kind == "noise":
        return torch.randint(0, 256, (B, 3, H, W), generator=torch.Generator().manual_seed(1)).float() / 255.0
    with np.load(os.path.join(REPO, "tests", "golden", "jpeg_device_cases.npz"), allow_pickle=False) as z:
        crop = z["in_kodim01_0"]
    tile = np.concatenate([np.concatenate([crop, crop[:, ::-1]], 1), np.concatenate([crop[::-1], crop[::-1, ::-1]], 1)])
    img = np.tile(tile, (-(-H // 128), -(-W // 128), 1))[:H, :W]
    x = torch.from_numpy(np.ascontiguousarray(img)).permute(2, 0, 1).float() / 255.0
    return torch.stack([torch.roll(x, 8 * b, dims=2) for b in range(B)])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "jpeg_decode.json"))
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--no-model", action="store_true")
    ap.add_argument("--no-sweep", action="store_true")
    ap.add_argument("--shape", type=int, nargs=3, action="append", default=None, metavar=("B", "H", "W"))
    ap.add_argument("--qualities", type=int, nargs="+", default=[1, 50, 95])
    ap.add_argument("--contents", nargs="+", default=["kodak_crop_tiled", "noise"])
    args = ap.parse_args()
    assert args.iters >= 50, "--iters: at least 50 calls"

    import torch
    from hyres_hip import jpeg_device
    from models.utils.turbo_jpeg_compression import TurboJPEGCompression
    assert torch.cuda.is_available(), "this benchmark needs the GPU"
    dev = torch.device("cuda:0")
    host = TurboJPEGCompression(device_codec=False)
    devc = TurboJPEGCompression(device_codec=True)
    res = {"device": torch.cuda.get_device_name(0), "iters": args.iters, "warmup": args.warmup,
           "host_threads": host.workers, "backend": host.backend, "decompress": [], "sweep": []}
    shapes = tuple(map(tuple, args.shape)) if args.shape else ((1, 512, 768), (16, 256, 256))
    for B, H, W in shapes:
        ragged = H % 8 != 0 or W % 16 != 0
        kw = {"any_size": True} if ragged else {}
        devc = TurboJPEGCompression(device_codec=True, **kw)
        for kind in args.contents:
            x = content(kind, B, H, W).to(dev)
            for q in args.qualities:
                files = jpeg_device.encode(x, q, **kw)[1]
                bufs = [io.BytesIO(f) for f in files]
                assert devc.decode_on_device(files, dev)
                d, h = devc.decompress(bufs, dev), host.decompress(bufs, dev)
                r = {"batch": [B, 3, H, W], "any_size": ragged, "content": kind, "quality": q,
                     "bytes_per_image": round(sum(map(len, files)) / B, 1), "equal": bool(torch.equal(d, h)),
                     "device": timed(lambda: devc.decompress(bufs, dev), args.iters, args.warmup),
                     "host": timed(lambda: host.decompress(bufs, dev), args.iters, args.warmup)}
                st = jpeg_device.stage(files, dev, **kw)
                r["device_kernels_only"] = timed(lambda: jpeg_device.decode_tensors(st), args.iters, args.warmup)
                r["speedup"] = round(r["host"]["median_ms"] / r["device"]["median_ms"], 2)
                res["decompress"].append(r)
                print(json.dumps(r), flush=True)
                if not args.no_sweep and (kind == "kodak_crop_tiled" or q == 95):
                    for sub_bits in (256, 512, 1024, 2048):
                        for threads in (128, 256, 512, 1024):
                            t = timed(lambda: jpeg_device.decode_tensors(st, sub_bits, threads), args.iters, args.warmup)
                            _, _, rounds = jpeg_device.decode_tensors(st, sub_bits, threads)
                            res["sweep"].append({"batch": [B, 3, H, W], "content": kind, "quality": q,
                                                 "sub_bits": sub_bits, "block_threads": threads,
                                                 "max_rounds": int(rounds.max()), **t})
    best = {}
    for s in res["sweep"]:
        best.setdefault((s["sub_bits"], s["block_threads"]), []).append(s["median_ms"])
    res["sweep_sum_of_medians_ms"] = {f"{k[0]}x{k[1]}": round(sum(v), 4) for k, v in sorted(best.items())}

    if not args.no_model:
        from hyres_hip.weights import synthetic_state_dict
        from models import ResidualJPEGCompression
        from models.checkerboard import LightWeightCheckerboard
        net = ResidualJPEGCompression(base_model=LightWeightCheckerboard(device_coder=True, coder_segment_rows=512),
                                      jpeg_quality=1)
        torch.nn.Module.load_state_dict(net, synthetic_state_dict(net.state_dict()), strict=True)
        net = net.to(dev).eval()
        net.update(force=True)
        net.jpeg.device_codec = True
        x = content("kodak_crop_tiled", 1, 512, 768).to(dev)
        with torch.no_grad():
            comp = net.compress(x)
            after = net.decompress(comp)["x_hat"]
            m = {"image": [1, 3, 512, 768], "jpeg_quality": 1, "coder": "device, HRW2, 512-row segments",
                 "after_device_jpeg_decode": timed(lambda: net.decompress(comp), args.iters, args.warmup)}
            net.jpeg.decode_on_device = lambda datas, device: False  # what decompress did before: Pillow + upload
            m["before_host_jpeg_decode"] = timed(lambda: net.decompress(comp), args.iters, args.warmup)
            m["equal"] = bool(torch.equal(after, net.decompress(comp)["x_hat"]))
        res["net_decompress"] = m
        print(json.dumps(m), flush=True)

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({k: res[k] for k in ("sweep_sum_of_medians_ms",)}))
    return 0 if all(r["equal"] for r in res["decompress"]) else 1


if __name__ == "__main__":
    sys.exit(main())
