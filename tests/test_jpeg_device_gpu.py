"""Row f2, device codec on the GPU: the HIP kernels of csrc/jpeg.hip against Pillow's libjpeg-turbo
(tests/golden/jpeg_device_cases.npz), the reference fixtures, the pure-host round trip and the host JPEG stage of
the model.  Integer work throughout, so every comparison is equality.
"""
import numpy as np
import pytest
import torch

from helpers import build_model, load_npz
from test_jpeg_device_cpu import CASES, as_input
from test_jpeg_host import FIXTURES

pytestmark = pytest.mark.gpu


def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def noise(shape, seed):
    """bytes / 255 with a different seed per image, so the images' stream lengths differ"""
    imgs = [torch.randint(0, 256, shape[1:], generator=torch.Generator().manual_seed(seed + i)) for i in range(shape[0])]
    return torch.stack(imgs).float() / 255.0


@pytest.mark.parametrize("fixture", FIXTURES)
def test_device_roundtrip_reproduces_reference_fixtures(fixture):
    from hyres_hip import jpeg_device
    g = load_npz(fixture)
    x = g["x"].to(dev())
    dec, sizes = jpeg_device.roundtrip(x, 50)
    bpp = jpeg_device.bpp(sizes, x)
    assert dec.is_cuda and dec.dtype == torch.float32 and sizes.is_cuda and sizes.dtype == torch.int32
    assert bpp.is_cuda and bpp.dim() == 0 and bpp.dtype == torch.float32
    assert torch.equal(dec.cpu(), g["jpeg_decoded"]), int((dec.cpu() != g["jpeg_decoded"]).sum())
    if "jpeg_bpp" in g:
        assert bpp.cpu().numpy() == g["jpeg_bpp"].numpy(), (float(bpp), float(g["jpeg_bpp"]))


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_device_codec_equals_pillow(case):
    from hyres_hip import jpeg_device
    x = as_input(case["u8"]).to(dev())
    dec, files = jpeg_device.encode(x, case["quality"])
    _, sizes = jpeg_device.roundtrip(x, case["quality"])  # the sizes-only path (no file buffer)
    assert sizes.tolist() == [len(case["file"])]
    assert files[0][:623] == case["file"][:623], "header"
    assert files[0] == case["file"], (len(files[0]), len(case["file"]))
    want = torch.from_numpy(case["dec"]).permute(2, 0, 1).unsqueeze(0)
    got_u8 = (dec.cpu() * 255).round().to(torch.uint8)
    assert torch.equal(got_u8, want), int((got_u8 != want).sum())
    assert torch.equal(dec.cpu(), want.float() / 255.0)


def test_device_equals_host_on_a_nonsquare_batch():
    """B = 3 of 64 x 128 noise at quality 1: H / W swaps, per-image scan offsets, differing sizes."""
    from hyres_hip import jpeg_device
    x = noise((3, 3, 64, 128), 7)
    dec_h, files_h = jpeg_device.encode_host(x, 1)
    dec_d, files_d = jpeg_device.encode(x.to(dev()), 1)
    assert len({len(f) for f in files_h}) == 3
    assert files_d == files_h
    assert torch.equal(dec_d.cpu(), dec_h)
    dec_r, sizes = jpeg_device.roundtrip(x.to(dev()), 1)
    assert sizes.tolist() == [len(f) for f in files_h] and torch.equal(dec_r, dec_d)


def test_roundtrip_is_capture_legal():
    """Captured once on a single stream and replayed on a second input, the round trip gives the eager result bit
    for bit: no sync, no allocation outside the graph's pool, no host read inside."""
    from hyres_hip import jpeg_device
    D = dev()
    x1, x2 = noise((2, 3, 64, 64), 11).to(D), noise((2, 3, 64, 64), 23).to(D)
    static = x1.clone()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        jpeg_device.roundtrip(static, 50)  # warm-up: the workspace of this stream exists before the capture
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        dec, sizes = jpeg_device.roundtrip(static, 50)
        bpp = jpeg_device.bpp(sizes, static)
    for x in (x2, x1):
        static.copy_(x)
        graph.replay()
        torch.cuda.synchronize()
        got = (dec.clone(), sizes.clone(), bpp.clone())
        dec_e, sizes_e = jpeg_device.roundtrip(x, 50)
        assert torch.equal(got[0], dec_e) and torch.equal(got[1], sizes_e)
        assert torch.equal(got[2], jpeg_device.bpp(sizes_e, x))
    dec_h, sizes_h = jpeg_device.roundtrip_host(x1.cpu(), 50)
    assert torch.equal(got[0].cpu(), dec_h) and torch.equal(got[1].cpu(), sizes_h)


def test_model_with_device_codec_equals_host_codec():
    """forward / compress / decompress of the model at 64 x 64, eval: every returned tensor and every JPEG buffer
    equal with either codec; with the device codec jpeg_bpp_loss never visits the host."""
    g = load_npz("kodim01_crop64_eval.npz")
    net, _ = build_model()
    net = net.to(dev()).eval()
    assert net.update(force=True)
    x = g["x"].to(dev())
    out, comp, dcmp = {}, {}, {}
    for codec in (False, True):
        net.jpeg.device_codec = codec
        assert net.jpeg.on_device(x) is codec
        with torch.no_grad():
            out[codec] = net(x)
            comp[codec] = net.compress(x)
            dcmp[codec] = net.decompress(comp[codec])
    flat = lambda o: {"x_hat": o["x_hat"], "y": o["likelihoods"]["y"], "z": o["likelihoods"]["z"],  # noqa: E731
                      "jpeg_bpp_loss": o["jpeg_bpp_loss"], "jpeg_decoded": o["jpeg_decoded"],
                      "residual": o["residual"], "residual_hat": o["residual_hat"]}
    host, devc = flat(out[False]), flat(out[True])
    for k in host:
        assert devc[k].is_cuda and devc[k].dtype == host[k].dtype and devc[k].shape == host[k].shape, k
        assert torch.equal(devc[k], host[k]), k
    assert torch.equal(devc["jpeg_decoded"].cpu(), g["jpeg_decoded"])
    assert ([b.getvalue() for b in comp[True]["jpeg_buffers"]] == [b.getvalue() for b in comp[False]["jpeg_buffers"]])
    assert comp[True]["strings"] == comp[False]["strings"] and comp[True]["shape"] == comp[False]["shape"]
    assert torch.equal(dcmp[True]["x_hat"], dcmp[False]["x_hat"])


def test_unsupported_inputs_fall_back_to_the_host_path():
    from models.utils.turbo_jpeg_compression import TurboJPEGCompression
    host = TurboJPEGCompression(quality=50, workers=1)
    devc = TurboJPEGCompression(quality=50, workers=1, device_codec=True)
    x = noise((2, 3, 64, 128), 3)
    for t in (x[..., :72].contiguous(), x[:, :1].contiguous()):  # W = 72; one channel
        t = t.to(dev())
        assert not devc.on_device(t)
        d0, b0 = host(t)
        d1, b1 = devc(t)
        assert isinstance(b1, float) and b1 == b0 and d1.is_cuda and torch.equal(d1, d0)
        assert [b.getvalue() for b in devc.compress(t)] == [b.getvalue() for b in host.compress(t)]
    t = x.to(dev())
    assert devc.on_device(t)
    d0, b0 = host(t)
    d1, b1 = devc(t)
    assert isinstance(b1, torch.Tensor) and b1.is_cuda and b1.cpu().numpy() == np.float32(b0)
    assert torch.equal(d1, d0)
