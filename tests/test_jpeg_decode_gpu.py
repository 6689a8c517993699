"""Device decoding of JPEG 4:2:2 files on the GPU: the kernels of csrc/jpeg.hip (unstuffing, the self-synchronising
Huffman decoder, DC scan, IDCT) against Pillow's libjpeg-turbo (tests/golden/jpeg_device_cases.npz), against the host
twin that runs the same schedule, and inside the model's ``decompress``.  Integer work: every comparison is equality.
"""
import io
from collections import defaultdict

import pytest
import torch

from helpers import build_model, load_npz
from test_jpeg_decode_cpu import (case_named, corrupt_files, noise_64x128_q95, pillow_file, refused_files, want_of)
from test_jpeg_device_cpu import CASES

pytestmark = pytest.mark.gpu


def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


@pytest.mark.parametrize("sub_bits", (32, 0))
def test_fixture_files_decode_on_the_device(sub_bits):
    """All 100 files, batched by shape: pixels equal Pillow's and the host twin's, rounds equal the host twin's."""
    from hyres_hip import jpeg_device
    by_shape = defaultdict(list)
    for c in CASES:
        by_shape[c["u8"].shape[:2]].append(c)
    assert sum(len(v) for v in by_shape.values()) == 100
    for cs in by_shape.values():
        files = [c["file"] for c in cs]
        dec, status, rounds = jpeg_device.decode_tensors(jpeg_device.stage(files, dev()), sub_bits)
        dec_h, rounds_h = jpeg_device.decode_host(files, sub_bits, return_rounds=True)
        assert status.cpu().tolist() == [0] * len(cs)
        assert torch.equal(dec.cpu(), torch.cat([want_of(c) for c in cs]))
        assert torch.equal(dec.cpu(), dec_h) and torch.equal(rounds.cpu(), rounds_h)
        assert torch.equal(jpeg_device.decode(files, dev(), sub_bits), dec)


def test_more_subsequences_than_block_threads():
    """64 x 128 noise at quality 95 with 32-bit subsequences: about 3 300 of them on the strided loop, at the default
    block and at the largest."""
    from hyres_hip import jpeg_device
    f, want = noise_64x128_q95()
    _, rounds_h = jpeg_device.decode_host([f], 32, return_rounds=True)
    for threads in (0, 1024, 64):
        dec, status, rounds = jpeg_device.decode_tensors(jpeg_device.stage([f], dev()), 32, threads)
        assert status.item() == 0 and torch.equal(dec.cpu(), want) and torch.equal(rounds.cpu(), rounds_h)


def test_batch_of_files_of_different_lengths():
    from hyres_hip import jpeg_device
    cs = [case_named(f"{n}_q50") for n in ("noise_64x64", "ramp_64x64", "kodim01_0")]
    assert len({len(c["file"]) for c in cs}) == 3
    dec = jpeg_device.decode([c["file"] for c in cs], dev())
    for i, c in enumerate(cs):
        assert torch.equal(dec[i:i + 1].cpu(), want_of(c)), c["name"]


@pytest.mark.parametrize("quality", (1, 95))
def test_decode_inverts_the_device_encoder(quality):
    from hyres_hip import jpeg_device
    imgs = [torch.randint(0, 256, (3, 64, 128), generator=torch.Generator().manual_seed(40 + i)) for i in range(2)]
    x = (torch.stack(imgs).float() / 255.0).to(dev())
    dec = jpeg_device.decode(jpeg_device.encode(x, quality)[1], dev())
    assert torch.equal(dec, jpeg_device.roundtrip(x, quality)[0])


def test_decode_is_capture_legal():
    """decode_tensors captured over a static staged buffer and replayed after the buffer was refilled with files of
    other lengths and another quality gives the eager result."""
    from hyres_hip import jpeg_device
    D = dev()
    set1 = [case_named(n)["file"] for n in ("noise_64x64_q50", "ramp_64x64_q50")]
    set2 = [case_named(n)["file"] for n in ("primaries_64x64_q95", "noise_64x64_q95")]
    cap, room = 8192, 20000
    assert max(len(f) for f in set1 + set2) - 625 <= cap
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        static = jpeg_device.stage(set1, D, capacity=cap, room=room)
        jpeg_device.decode_tensors(static)  # warm-up: the workspace of this stream exists before the capture
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        dec, status, rounds = jpeg_device.decode_tensors(static)
    for files in (set2, set1):
        static.buf.copy_(jpeg_device.stage(files, None, capacity=cap, room=room).buf)
        graph.replay()
        torch.cuda.synchronize()
        eager = jpeg_device.decode(files, D)
        assert status.cpu().tolist() == [0, 0] and torch.equal(dec, eager)
        assert torch.equal(dec.cpu(), jpeg_device.decode_host(files))


def test_model_decompress_decodes_on_the_device(monkeypatch):
    g = load_npz("kodim01_crop64_eval.npz")
    net, _ = build_model()
    net = net.to(dev()).eval()
    assert net.update(force=True)
    x = g["x"].to(dev())
    with torch.no_grad():
        net.jpeg.device_codec = False
        comp = net.compress(x)
        host = net.decompress(comp)["x_hat"]
        net.jpeg.device_codec = True
        comp_d = net.compress(x)
        assert [b.getvalue() for b in comp_d["jpeg_buffers"]] == [b.getvalue() for b in comp["jpeg_buffers"]]
        calls = []

        def pillow(data):
            calls.append(len(data))
            raise AssertionError("the device path must not call Pillow")

        real = net.jpeg.jpeg.decode
        monkeypatch.setattr(net.jpeg.jpeg, "decode", pillow)
        devc = net.decompress(comp_d)["x_hat"]
        assert not calls and torch.equal(devc, host)
        assert torch.equal(net.decompress(comp)["x_hat"], host)  # the host codec's buffers, decoded on the device
        # one buffer re-encoded with optimised Huffman tables: the whole call falls back to Pillow
        from PIL import Image
        im = Image.open(io.BytesIO(comp["jpeg_buffers"][0].getvalue()))
        buf = io.BytesIO()
        im.save(buf, format="JPEG", quality="keep", subsampling="keep", optimize=True)
        from hyres_hip import jpeg_device
        assert not jpeg_device.supported_file(buf.getvalue())
        mixed = dict(comp, jpeg_buffers=[buf] + list(comp["jpeg_buffers"][1:]))

        def counting(data):
            calls.append(len(data))
            return real(data)

        monkeypatch.setattr(net.jpeg.jpeg, "decode", counting)
        fell_back = net.decompress(mixed)["x_hat"]
        assert len(calls) == len(mixed["jpeg_buffers"])
        net.jpeg.device_codec = False
        assert torch.equal(fell_back, net.decompress(mixed)["x_hat"])


def test_refused_files_fall_back_with_a_gpu_target():
    from models.utils.turbo_jpeg_compression import TurboJPEGCompression
    host = TurboJPEGCompression(workers=1, device_codec=False)
    devc = TurboJPEGCompression(workers=1, device_codec=True)
    for name, f in refused_files().items():
        got = devc.decompress([io.BytesIO(f)], dev())
        assert got.is_cuda and torch.equal(got, host.decompress([io.BytesIO(f)], dev())), name
    good = pillow_file(case_named("kodim01_0_q50")["u8"], quality=75)
    assert devc.decode_on_device([good], dev())
    assert torch.equal(devc.decompress([io.BytesIO(good)], dev()), host.decompress([io.BytesIO(good)], dev()))


@pytest.mark.parametrize("name", ["truncated", "zeroed_tail", "planted_rst"])
def test_corrupt_files_on_the_device(name):
    """Once each: ValueError, or the host twin's pixels where the file happens to decode; the next call on the same
    stream decodes a good file."""
    from hyres_hip import jpeg_device
    f = corrupt_files()[name]
    dec_h, status_h = jpeg_device.decode_host([f], check=False)
    dec, status = jpeg_device.decode([f], dev(), check=False)
    assert status.cpu().tolist() == status_h.tolist()
    if int(status_h[0]):
        with pytest.raises(ValueError, match="image"):
            jpeg_device._raise_on_status(status.cpu().tolist())
    else:
        assert torch.equal(dec.cpu(), dec_h)
    good = case_named("noise_64x64_q50")
    assert torch.equal(jpeg_device.decode([good["file"]], dev()).cpu(), want_of(good))
