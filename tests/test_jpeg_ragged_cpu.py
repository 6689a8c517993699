"""The any-size JPEG codec (``any_size=True``, the ``hyres_jpeg_*_any`` entry points), the part that needs no GPU:
the host twins of the encoder and of the decoder against Pillow's libjpeg-turbo on images that are not whole 16x8
MCUs -- edge replication, dummy blocks, odd widths, the narrow-chroma rule.

tests/golden/jpeg_ragged_cases.npz (tests/golden/make_jpeg_ragged_golden.py) holds, per case, the input bytes, the
quality, Pillow's file and Pillow's decode.  Integer work throughout, so every comparison is equality.
"""
import io
import json
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN

HEADER = 623
QUALITIES = (1, 25, 50, 95)
SIZES = {(8, 24), (9, 16), (16, 17), (13, 21), (15, 31), (33, 47), (60, 72), (64, 72), (3, 5), (2, 2)}
SUB_BITS = (32, 128, 0)  # 0 = the library's default


def load_cases():
    with np.load(os.path.join(GOLDEN, "jpeg_ragged_cases.npz"), allow_pickle=False) as z:
        meta = json.loads(bytes(z["meta"]).decode())
        return [dict(m, u8=z["in_" + m["input"]].copy(), file=bytes(z[f"file_{i}"]), dec=z[f"dec_{i}"].copy())
                for i, m in enumerate(meta)]


CASES = load_cases()


def as_input(u8):
    """[H,W,3] bytes -> the [1,3,H,W] fp32 image whose (x * 255).byte() gives those bytes back."""
    x = torch.from_numpy(u8).permute(2, 0, 1).float().div(255.0).unsqueeze(0).contiguous()
    assert torch.equal((x * 255).byte()[0].permute(1, 2, 0), torch.from_numpy(u8))
    return x


def want_of(case):
    return torch.from_numpy(case["dec"]).permute(2, 0, 1).unsqueeze(0).float() / 255.0


def case_named(name):
    return next(c for c in CASES if c["name"] == name)


def corrupt_files():
    """The three corrupt versions of the 33x47 noise file at quality 50: all parse, none may crash or hang."""
    f = case_named("noise_33x47_q50")["file"]
    scan = f[HEADER:-2]
    mid = HEADER + len(scan) // 2
    return {
        "truncated": f[:mid] + b"\xff\xd9",
        "zeroed_tail": f[:-34] + bytes(32) + f[-2:],
        "planted_rst": f[:mid] + b"\xff\xd0" + f[mid + 2:],
    }


def unstuffed_bits(f):
    scan = f[HEADER:-2]
    return 8 * (len(scan) - scan.count(b"\xff\x00"))


def test_fixture_covers_the_issue_grid():
    assert {c["u8"].shape[:2] for c in CASES} == SIZES
    assert {c["quality"] for c in CASES} == set(QUALITIES)
    for kind in ("noise", "ramp", "primaries", "edge"):
        assert {c["u8"].shape[:2] for c in CASES if c["input"].startswith(kind)} == SIZES
    for c in CASES:  # Pillow's header is the codec's 623 bytes with the true size in SOF0
        H, W = c["u8"].shape[:2]
        assert c["file"][HEADER - 14:HEADER - 12] == b"\xff\xda" and c["file"].count(b"\xff\xc0") >= 1
        i = c["file"].index(b"\xff\xc0")
        assert c["file"][i + 5:i + 9] == bytes([H >> 8, H & 255, W >> 8, W & 255]), c["name"]


def test_roundtrip_host_equals_pillow():
    from hyres_hip import jpeg_device
    for c in CASES:
        x = as_input(c["u8"])
        dec, files = jpeg_device.encode_host(x, c["quality"], any_size=True)
        f = files[0]
        assert f[:HEADER] == c["file"][:HEADER], c["name"]
        assert f == c["file"], (c["name"], len(f), len(c["file"]))
        want = want_of(c)
        assert dec.dtype == torch.float32 and dec.shape == want.shape, c["name"]
        assert torch.equal((dec * 255).round().to(torch.uint8)[0].permute(1, 2, 0), torch.from_numpy(c["dec"])), c["name"]
        assert torch.equal(dec, want), (c["name"], int((dec != want).sum()))
        dec2, sizes = jpeg_device.roundtrip_host(x, c["quality"], any_size=True)
        assert torch.equal(dec2, dec) and sizes.dtype == torch.int32 and sizes.tolist() == [len(c["file"])], c["name"]


@pytest.mark.parametrize("sub_bits", SUB_BITS)
def test_decode_host_equals_pillow(sub_bits):
    from hyres_hip import jpeg_device
    for c in CASES:
        assert jpeg_device.supported_file(c["file"], any_size=True), \
            (c["name"], jpeg_device.unsupported_reason(c["file"], any_size=True))
        dec, rounds = jpeg_device.decode_host([c["file"]], sub_bits, return_rounds=True, any_size=True)
        want = want_of(c)
        assert dec.dtype == torch.float32 and dec.shape == want.shape, c["name"]
        assert torch.equal(dec, want), (c["name"], sub_bits, int((dec != want).sum()))
        nsub = -(-unstuffed_bits(c["file"]) // (sub_bits or 512))
        r = int(rounds[0])
        assert 0 <= r <= nsub and r <= max(nsub - 1, 0), (c["name"], r, nsub)


def test_batch_of_three_equals_the_single_images():
    from hyres_hip import jpeg_device
    for size in ("13x21", "33x47"):
        cs = [case_named(f"{k}_{size}_q50") for k in ("noise", "ramp", "edge")]
        x = torch.cat([as_input(c["u8"]) for c in cs])
        for q in (1, 50):
            dec, files = jpeg_device.encode_host(x, q, any_size=True)
            for i in range(3):
                d1, f1 = jpeg_device.encode_host(x[i:i + 1], q, any_size=True)
                assert files[i] == f1[0] and torch.equal(dec[i:i + 1], d1), (size, q, i)
            assert files[0] != files[1] != files[2]
            assert torch.equal(jpeg_device.decode_host(files, any_size=True), dec)
        assert [f for f in jpeg_device.encode_host(x, 50, any_size=True)[1]] == [c["file"] for c in cs]


def test_strict_entry_points_answer_as_before():
    from hyres_hip import _lib as L
    from hyres_hip import jpeg_device
    lib = L.load()
    assert lib.hyres_jpeg_workspace_bytes(1, 64, 72) == -1 and lib.hyres_jpeg_workspace_bytes_any(1, 64, 72) > 0
    assert lib.hyres_jpeg_stream_bytes(13, 21) == -1 and lib.hyres_jpeg_stream_bytes_any(13, 21) > 0
    assert lib.hyres_jpeg_decode_workspace_bytes(1, 13, 21, 4096) == -1
    assert lib.hyres_jpeg_decode_any_workspace_bytes(1, 13, 21, 4096) > 0
    assert lib.hyres_jpeg_workspace_bytes_any(1, 0, 16) == -1 and lib.hyres_jpeg_workspace_bytes_any(1, 8, 65536) == -1
    # on whole MCUs the pair is one computation
    assert lib.hyres_jpeg_workspace_bytes(2, 64, 64) == lib.hyres_jpeg_workspace_bytes_any(2, 64, 64)
    assert lib.hyres_jpeg_stream_bytes(64, 64) == lib.hyres_jpeg_stream_bytes_any(64, 64)
    c = case_named("noise_13x21_q50")
    x = as_input(c["u8"])
    assert not jpeg_device.supported_shape(x) and jpeg_device.supported_shape(x, any_size=True)
    assert not jpeg_device.supported_file(c["file"]) and "MCU" in jpeg_device.unsupported_reason(c["file"])
    assert jpeg_device.unsupported_reason(c["file"], any_size=True) is None
    with pytest.raises(L.HipError):
        jpeg_device.roundtrip_host(x, 50)
    with pytest.raises(ValueError):
        jpeg_device.decode_host([c["file"]])
    a = torch.rand(2, 3, 16, 32)
    for q in (1, 95):
        d0, f0 = jpeg_device.encode_host(a, q)
        d1, f1 = jpeg_device.encode_host(a, q, any_size=True)
        assert f0 == f1 and torch.equal(d0, d1)
        assert torch.equal(jpeg_device.decode_host(f0), jpeg_device.decode_host(f0, any_size=True))


def test_the_stage_opts_in_twice(monkeypatch):
    from models.utils.turbo_jpeg_compression import TurboJPEGCompression
    f = case_named("noise_13x21_q50")["file"]
    assert not TurboJPEGCompression(workers=1, device_codec=True).decode_on_device([f], "cuda")
    assert TurboJPEGCompression(workers=1, device_codec=True, any_size=True).decode_on_device([f], "cuda")
    assert not TurboJPEGCompression(workers=1, device_codec=False, any_size=True).decode_on_device([f], "cuda")
    monkeypatch.setenv("HYRES_JPEG_ANY_SIZE", "1")
    monkeypatch.setenv("HYRES_JPEG_CODEC", "device")
    j = TurboJPEGCompression(workers=1)
    assert j.device_codec and j.any_size and j.decode_on_device([f], "cuda")
    assert not j.on_device(torch.zeros(1, 3, 13, 21))  # a CPU tensor keeps the host path
    monkeypatch.setenv("HYRES_JPEG_CODEC", "host")
    assert not TurboJPEGCompression(workers=1).decode_on_device([f], "cuda")  # no effect without the device codec
    monkeypatch.setenv("HYRES_JPEG_ANY_SIZE", "yes")
    with pytest.raises(ValueError):
        TurboJPEGCompression(workers=1)


@pytest.mark.parametrize("name", ["truncated", "zeroed_tail", "planted_rst"])
def test_corrupt_ragged_files_are_refused(name):
    from hyres_hip import jpeg_device
    f = corrupt_files()[name]
    assert jpeg_device.supported_file(f, any_size=True)  # the markers are intact: the entropy decoder has to notice
    for sub_bits in SUB_BITS:
        dec, status = jpeg_device.decode_host([f], sub_bits, check=False, any_size=True)
        assert dec.shape == (1, 3, 33, 47)
        assert int(status[0]) != 0, (name, sub_bits)
        with pytest.raises(ValueError, match="image"):
            jpeg_device.decode_host([f], sub_bits, any_size=True)
    good = case_named("noise_33x47_q50")["file"]
    _, status = jpeg_device.decode_host([good, f, good], check=False, any_size=True)
    assert status[0] == 0 and status[2] == 0 and status[1] != 0
    assert jpeg_device.unsupported_reason(good[:-2], any_size=True) is not None  # no EOI
    assert jpeg_device.unsupported_reason(good[:300], any_size=True) is not None


def test_model_pads_to_the_stride():
    from models import ResidualJPEGCompression
    net = ResidualJPEGCompression()
    assert net.residual_model.stride == 32
    assert net.padded_size(40, 56) == (64, 64) and net.padded_size(33, 47) == (64, 64)
    assert net.padded_size(64, 96) == (64, 96) and net.padded_size(1, 65) == (32, 96)
