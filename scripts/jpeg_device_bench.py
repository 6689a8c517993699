"""Times the JPEG base layer of one 16 x 3 x 256 x 256 batch, in one run on the GPU:

  * the device round trip (hyres_hip.jpeg_device.roundtrip) at quality 1 and 50: HIP events around ``--iters``
    calls after ``--warmup`` calls; also with the files written (the ``compress`` path, without its D2H copy);
  * the process-pool host round trip (hyres_hip.jpeg_host, TurboJPEGCompression on a CPU batch) of the same batch;
  * the drop-in graphed training loop (src/utils/engine.py train_one_epoch) with each codec: ms per step over the
    tail of one epoch, from a device synchronise when the loop fetches batch ``--loop-steps[0]`` (capture and
    warm-up are behind it) to a synchronise after the last of ``--loop-steps[1]`` steps.

The device round trip must be at least ``--min-speedup`` (5) times faster than the process pool at both qualities,
else the script exits 1.  The result goes to ``--out`` (default profiles/jpeg_device.json) and to stdout.

    python scripts/jpeg_device_bench.py [--out profiles/jpeg_device.json]

``--shape B H W`` times another batch; one that is not whole 16x8 MCUs goes through the any-size entry points
(``any_size=True``, also forced by ``--any-size``) and is compared with the host stage's Pillow path on the same
bytes.  The graphed loop needs sides that are multiples of 32 and is skipped otherwise.
"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "hyres-residual-enhanced-hybrid-image-compression_amd")
for _p in (PKG, REPO):
    if _p not in sys.path:
        sys.path.insert(0, _p)


class _Batches:
    """A list of CPU batches with the two attributes train_one_epoch's progress line reads.  Fetching batch ``mark``
    synchronises the device and records the time: the loop fetches batch i + 1 before it issues step i, so steps
    mark - 1 .. n - 1 lie after that point."""

    def __init__(self, batches, mark):
        self.batches, self.mark, self.t_mark = batches, mark, None
        self.dataset = range(sum(len(b) for b in batches))

    def __iter__(self):
        import torch
        for i, b in enumerate(self.batches):
            if i == self.mark:
                torch.cuda.synchronize()
                self.t_mark = time.perf_counter()
            yield b

    def __len__(self):
        return len(self.batches)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "jpeg_device.json"))
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--procs", type=int, default=8)
    ap.add_argument("--loop-steps", type=int, nargs=2, default=[8, 40])
    ap.add_argument("--min-speedup", type=float, default=5.0)
    ap.add_argument("--no-loop", action="store_true")
    ap.add_argument("--shape", type=int, nargs=3, default=None, metavar=("B", "H", "W"))
    ap.add_argument("--any-size", action="store_true")
    args = ap.parse_args()

    from hyres_hip import jpeg_host
    nprocs = jpeg_host.start(args.procs)  # before the process touches the GPU

    import torch
    from hyres_hip import jpeg_device
    from models.utils.turbo_jpeg_compression import TurboJPEGCompression
    assert torch.cuda.is_available(), "this benchmark needs the GPU"
    dev = torch.device("cuda:0")
    B, H, W = args.shape if args.shape else (args.batch, args.size, args.size)
    any_size = args.any_size or H % 8 != 0 or W % 16 != 0
    kw = {"any_size": True} if any_size else {}
    if H % 32 or W % 32:
        args.no_loop = True
    x_cpu = torch.randint(0, 256, (B, 3, H, W), generator=torch.Generator().manual_seed(1)).float() / 255.0
    x = x_cpu.to(dev)
    res = {"batch": [B, 3, H, W], "any_size": any_size, "data": "uniform 8-bit noise", "iters": args.iters, "host_procs": nprocs,
           "device": torch.cuda.get_device_name(0)}

    for q in (1, 50):
        r = {}
        for tag, fn in (("roundtrip", jpeg_device.roundtrip), ("roundtrip_with_files", jpeg_device._run)):
            call = (lambda: fn(x, q, **kw)) if tag == "roundtrip" else (lambda: fn(x, q, True, **kw))
            for _ in range(args.warmup):
                call()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(args.iters):
                call()
            e1.record()
            torch.cuda.synchronize()
            r[f"device_{tag}_ms"] = round(e0.elapsed_time(e1) / args.iters, 4)
        j = TurboJPEGCompression(quality=q)
        dec_h, bpp_h = j(x_cpu)
        t0 = time.perf_counter()
        for _ in range(5):
            j(x_cpu)
        r["host_pool_roundtrip_ms"] = round((time.perf_counter() - t0) * 1000 / 5, 3)
        dec_d, sizes = jpeg_device.roundtrip(x, q, **kw)
        r["equal_to_host"] = bool(torch.equal(dec_d.cpu(), dec_h)) and float(jpeg_device.bpp(sizes, x)) == float(
            torch.tensor(bpp_h, dtype=torch.float32))
        r["bytes_per_image"] = round(float(sizes.sum()) / B, 1)
        r["speedup"] = round(r["host_pool_roundtrip_ms"] / r["device_roundtrip_ms"], 1)
        res[f"quality_{q}"] = r

    if not args.no_loop:
        from hyres_hip.loss import RateDistortionLoss
        from hyres_hip.optim import FusedAdam
        from hyres_hip.weights import synthetic_state_dict
        from models import ResidualJPEGCompression
        from src.utils.engine import train_one_epoch
        n0, n1 = args.loop_steps
        batches = [torch.roll(x_cpu, i, dims=3).contiguous() for i in range(n1)]
        loop = {"steps_timed": n1 - n0 + 1, "steps": n1, "quality": 1}
        for codec in ("host", "device"):
            net = ResidualJPEGCompression(jpeg_quality=1)
            torch.nn.Module.load_state_dict(net, synthetic_state_dict(net.state_dict()), strict=True)
            net = net.to(dev)
            net.jpeg.device_codec = codec == "device"
            named = sorted(net.named_parameters())
            opt = FusedAdam([p for n, p in named if not n.endswith(".quantiles")], lr=1e-4, max_grad_norm=1.0)
            aux = FusedAdam([p for n, p in named if n.endswith(".quantiles")], lr=1e-3)
            crit = RateDistortionLoss(lmbda=0.045, alpha=0)
            loader = _Batches(batches, n0)
            train_one_epoch(net, crit, loader, opt, aux, 0, 1.0, noisequant=False, log_every=10 ** 9)
            torch.cuda.synchronize()
            loop[f"{codec}_codec_ms_per_step"] = round((time.perf_counter() - loader.t_mark) * 1000 / (n1 - n0 + 1), 3)
            del net, opt, aux
        res["graphed_loop"] = loop

    jpeg_host.shutdown()
    res["min_speedup"] = args.min_speedup
    res["pass"] = all(res[f"quality_{q}"]["speedup"] >= args.min_speedup and res[f"quality_{q}"]["equal_to_host"]
                      for q in (1, 50))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
    return 0 if res["pass"] else 1


if __name__ == "__main__":
    sys.exit(main())
