"""Row f2, device codec, the part that needs no GPU: csrc/jpeg_core.h — the arithmetic the HIP kernels
and the pure-host C-ABI round trip share — against Pillow's bundled libjpeg-turbo.

tests/golden/jpeg_device_cases.npz (tests/golden/make_jpeg_device_golden.py) holds, per case, the input bytes, the
quality, the JPEG file Pillow wrote with the host stage's settings and Pillow's decode of it.  The codec is integer
work, so every comparison is equality: file bytes, decoded bytes, the fp32 output (= byte / 255, a true division)
and ``jpeg_bpp``.  The four reference fixtures of tests/test_jpeg_host.py must come out of it bit for bit as well.
"""
import json
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from helpers import load_npz
from test_jpeg_host import FIXTURES

QUALITIES = (1, 25, 50, 95)


def load_cases():
    with np.load(os.path.join(GOLDEN, "jpeg_device_cases.npz"), allow_pickle=False) as z:
        meta = json.loads(bytes(z["meta"]).decode())
        return [dict(m, u8=z["in_" + m["input"]].copy(), file=bytes(z[f"file_{i}"]), dec=z[f"dec_{i}"].copy())
                for i, m in enumerate(meta)]


CASES = load_cases()


def as_input(u8):
    """[H,W,3] bytes -> the [1,3,H,W] fp32 image whose (x * 255).byte() gives those bytes back."""
    x = torch.from_numpy(u8).permute(2, 0, 1).float().div(255.0).unsqueeze(0).contiguous()
    assert torch.equal((x * 255).byte()[0].permute(1, 2, 0), torch.from_numpy(u8))
    return x


def dqt_payloads(data):
    """The 64-byte tables of a file's two DQT segments, by table id."""
    out, i = {}, 2
    while data[i + 1] != 0xDA:
        n = (data[i + 2] << 8) | data[i + 3]
        if data[i + 1] == 0xDB:
            out[data[i + 4]] = np.frombuffer(data[i + 5:i + 2 + n], np.uint8)
        i += 2 + n
    return out


def test_fixture_covers_the_issue_grid():
    sizes = {c["u8"].shape[:2] for c in CASES}
    assert {(8, 16), (16, 32), (24, 48), (64, 64), (64, 128)} <= sizes
    assert {c["quality"] for c in CASES} == set(QUALITIES)
    for q in QUALITIES:  # noise exercises 0xFF stuffing at every quality
        f = next(c["file"] for c in CASES if c["name"] == f"noise_64x64_q{q}")
        assert f[623:].count(b"\xff\x00") >= 4


@pytest.mark.parametrize("quality", QUALITIES)
def test_quant_tables_equal_the_dqt_payloads(quality):
    from hyres_hip import jpeg_device
    lum, chr_ = jpeg_device.quant_tables(quality)
    for c in (c for c in CASES if c["quality"] == quality):
        dqt = dqt_payloads(c["file"])
        assert np.array_equal(lum, dqt[0]) and np.array_equal(chr_, dqt[1])
    if quality == 1:
        assert (lum == 255).all() and (chr_ == 255).all()


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_host_roundtrip_equals_pillow(case):
    from hyres_hip import jpeg_device
    x = as_input(case["u8"])
    dec, files = jpeg_device.encode_host(x, case["quality"])
    assert files[0][:623] == case["file"][:623], "header"
    assert files[0] == case["file"], (len(files[0]), len(case["file"]))
    want = torch.from_numpy(case["dec"]).permute(2, 0, 1).unsqueeze(0)
    got_u8 = (dec * 255).round().to(torch.uint8)
    assert torch.equal(got_u8, want), int((got_u8 != want).sum())
    assert torch.equal(dec, want.float() / 255.0)
    dec2, sizes = jpeg_device.roundtrip_host(x, case["quality"])
    assert torch.equal(dec2, dec) and sizes.tolist() == [len(case["file"])]


@pytest.mark.parametrize("fixture", FIXTURES)
def test_host_roundtrip_reproduces_reference_fixtures(fixture):
    from hyres_hip import jpeg_device
    g = load_npz(fixture)
    dec, sizes = jpeg_device.roundtrip_host(g["x"], 50)
    assert dec.dtype == torch.float32 and torch.equal(dec, g["jpeg_decoded"]), int((dec != g["jpeg_decoded"]).sum())
    bpp = jpeg_device.bpp(sizes, g["x"])
    assert bpp.dtype == torch.float32 and bpp.dim() == 0
    if "jpeg_bpp" in g:
        assert bpp.numpy() == g["jpeg_bpp"].numpy(), (float(bpp), float(g["jpeg_bpp"]))


def test_host_roundtrip_batches_images_independently():
    """B > 1 through the C-ABI: per-image sizes and files, different per image."""
    from hyres_hip import jpeg_device
    cs = [c for c in CASES if c["input"] in ("noise_64x64", "ramp_64x64", "kodim01_0") and c["quality"] == 50]
    x = torch.cat([as_input(c["u8"]) for c in cs])
    dec, files = jpeg_device.encode_host(x, 50)
    assert files == [c["file"] for c in cs] and len({len(f) for f in files}) == len(cs)
    for i, c in enumerate(cs):
        assert torch.equal(dec[i], torch.from_numpy(c["dec"]).permute(2, 0, 1).float() / 255.0)


def test_unsupported_shapes_are_refused_by_the_library():
    from hyres_hip import _lib as L
    from hyres_hip import jpeg_device
    assert L.load().hyres_jpeg_workspace_bytes(1, 64, 72) == -1
    assert b"W % 16" in L.load().hyres_last_error_string()
    assert L.load().hyres_jpeg_workspace_bytes(2, 64, 64) > 0
    with pytest.raises(L.HipError):
        jpeg_device.roundtrip_host(torch.zeros(1, 3, 12, 16), 50)
    assert not jpeg_device.supported(torch.zeros(1, 3, 64, 64))  # a CPU tensor never takes the device path
    assert jpeg_device.supported_shape(torch.zeros(1, 3, 64, 64))
    assert not jpeg_device.supported_shape(torch.zeros(1, 1, 64, 64))
    assert not jpeg_device.supported_shape(torch.zeros(1, 3, 64, 72))


def test_default_codec_is_the_host_backend(monkeypatch):
    from models.utils.turbo_jpeg_compression import TurboJPEGCompression
    monkeypatch.delenv("HYRES_JPEG_CODEC", raising=False)
    j = TurboJPEGCompression()
    assert j.device_codec is False and j.backend in ("pillow-libjpeg-turbo", "pyturbojpeg")
    monkeypatch.setenv("HYRES_JPEG_CODEC", "device")
    assert TurboJPEGCompression().device_codec is True
    assert TurboJPEGCompression(device_codec=False).device_codec is False  # the argument wins over the environment
    monkeypatch.setenv("HYRES_JPEG_CODEC", "host")
    assert TurboJPEGCompression().device_codec is False
    monkeypatch.setenv("HYRES_JPEG_CODEC", "gpu")
    with pytest.raises(ValueError):
        TurboJPEGCompression()


def test_cpu_tensor_with_device_codec_takes_the_host_path():
    from models.utils.turbo_jpeg_compression import TurboJPEGCompression
    g = load_npz("hyres_eval_b2_64.npz")
    host, devc = TurboJPEGCompression(quality=50, workers=1), TurboJPEGCompression(quality=50, workers=1,
                                                                                 device_codec=True)
    assert not devc.on_device(g["x"])
    d0, b0 = host(g["x"])
    d1, b1 = devc(g["x"])
    assert isinstance(b1, float) and b1 == b0 and torch.equal(d1, d0) and torch.equal(d1, g["jpeg_decoded"])
    assert [b.getvalue() for b in devc.compress(g["x"])] == [b.getvalue() for b in host.compress(g["x"])]
    # and the codec's own host round trip writes those very files
    from hyres_hip import jpeg_device
    assert jpeg_device.encode_host(g["x"], 50)[1] == [b.getvalue() for b in host.compress(g["x"])]
