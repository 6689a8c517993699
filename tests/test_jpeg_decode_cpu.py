"""Device decoding of JPEG 4:2:2 files, the part that needs no GPU: the marker parser and the host twin of the
self-synchronising parallel Huffman decoder (csrc/jpeg_core.h: the same symbol step, rounds, write pass, DC scan and
IDCT the kernels run, with a loop over subsequences where the kernel has threads) against Pillow's libjpeg-turbo.

Integer work throughout, so every comparison is equality.  tests/golden/jpeg_device_cases.npz holds 100
Pillow-written files with Pillow's decode of each; other files are written here with the installed Pillow.
"""
import io

import numpy as np
import pytest
import torch

from test_jpeg_device_cpu import CASES, QUALITIES, as_input

HEADER = 623
SUB_BITS = (32, 128, 0)  # 0 = the library's default


def want_of(case):
    return torch.from_numpy(case["dec"]).permute(2, 0, 1).unsqueeze(0).float() / 255.0


def case_named(name):
    return next(c for c in CASES if c["name"] == name)


def image_u8(h, w, seed=0):
    """A smooth gradient under noise: short and long code words, DC steps in every component."""
    g = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    base = np.stack([xx * 255 // max(w - 1, 1), yy * 255 // max(h - 1, 1), (xx + yy) * 255 // (h + w)], -1)
    return np.clip(base * 0.6 + g.integers(0, 103, (h, w, 3)), 0, 255).astype(np.uint8)


def pillow_file(u8, mode="RGB", **opts):
    from PIL import Image
    im = Image.fromarray(u8 if mode == "RGB" else u8[..., 0], mode)
    buf = io.BytesIO()
    im.save(buf, format="JPEG", **{"quality": 50, "subsampling": 1, **opts})
    return buf.getvalue()


def host_decode(files):
    """The host JPEG stage's decompress (Pillow), one image per call so that sizes may differ."""
    from models.utils.turbo_jpeg_compression import TurboJPEGCompression
    j = TurboJPEGCompression(workers=1, device_codec=False)
    return [j.decompress([io.BytesIO(f)], "cpu") for f in files]


def refused_files():
    """name -> file the device decoder must leave to the host path"""
    from PIL import Image
    u8 = image_u8(64, 64, 1)
    ex = Image.Exif()
    ex[0x010E] = "x"
    return {
        "optimize": pillow_file(u8, optimize=True),
        "restart": pillow_file(u8, restart_marker_blocks=4),
        "444": pillow_file(u8, subsampling=0),
        "420": pillow_file(u8, subsampling=2),
        "grey": pillow_file(u8, mode="L", subsampling=-1),
        "progressive": pillow_file(u8, progressive=True),
        "60x72": pillow_file(image_u8(60, 72, 2)),
    }


def corrupt_files():
    """The three corrupt versions of the 64x64 noise file at quality 50: all parse, none may crash or hang."""
    f = case_named("noise_64x64_q50")["file"]
    scan = f[HEADER:-2]
    mid = HEADER + len(scan) // 2
    return {
        "truncated": f[:mid] + b"\xff\xd9",
        "zeroed_tail": f[:-34] + bytes(32) + f[-2:],
        "planted_rst": f[:mid] + b"\xff\xd0" + f[mid + 2:],
    }


def noise_64x128_q95():
    """(file, Pillow's decode) of the fixture's 64 x 128 noise input at quality 95, which the fixture stores only up
    to quality 50: about 3 300 subsequences of 32 bits."""
    from models.utils.turbo_jpeg_compression import _PillowTurbo
    u8 = next(c["u8"] for c in CASES if c["input"] == "noise_64x128")
    f = _PillowTurbo().encode(u8, quality=95)
    return f, host_decode([f])[0]


def unstuffed_bits(f):
    scan = f[HEADER:-2]
    return 8 * (len(scan) - scan.count(b"\xff\x00"))


@pytest.mark.parametrize("sub_bits", SUB_BITS)
def test_fixture_files_decode_to_pillows_pixels(sub_bits):
    from hyres_hip import jpeg_device
    for c in CASES:
        assert jpeg_device.supported_file(c["file"]), (c["name"], jpeg_device.unsupported_reason(c["file"]))
        dec = jpeg_device.decode_host([c["file"]], sub_bits)
        want = want_of(c)
        assert dec.dtype == torch.float32 and dec.shape == want.shape, c["name"]
        assert torch.equal(dec, want), (c["name"], sub_bits, int((dec != want).sum()))
        assert torch.equal((dec * 255).round().to(torch.uint8)[0].permute(1, 2, 0), torch.from_numpy(c["dec"]))


@pytest.mark.parametrize("quality", QUALITIES)
def test_decode_inverts_the_codecs_own_files(quality):
    from hyres_hip import jpeg_device
    cs = [case_named(f"{n}_q50") for n in ("noise_64x64", "ramp_64x64", "kodim01_0")]
    x = torch.cat([as_input(c["u8"]) for c in cs])
    dec, files = jpeg_device.encode_host(x, quality)
    for sub_bits in (32, 0):
        assert torch.equal(jpeg_device.decode_host(files, sub_bits), dec)


def test_foreign_supported_files_equal_pillow():
    from PIL import Image
    from hyres_hip import jpeg_device
    ex = Image.Exif()
    ex[0x010E] = "a description"
    u8 = image_u8(64, 64, 3)
    files = {
        "q75": pillow_file(u8, quality=75),
        "q100": pillow_file(u8, quality=100),
        "comment_exif": pillow_file(u8, comment=b"made by a test", exif=ex.tobytes()),
        "24x48": pillow_file(image_u8(24, 48, 4), quality=90),
        "64x128": pillow_file(image_u8(64, 128, 5), quality=30),
    }
    assert b"made by a test" in files["comment_exif"] and b"Exif" in files["comment_exif"]
    assert files["comment_exif"][:HEADER] != pillow_file(u8)[:HEADER]  # the segments are really there
    for name, f in files.items():
        assert jpeg_device.supported_file(f), (name, jpeg_device.unsupported_reason(f))
        want = host_decode([f])[0]
        for sub_bits in (32, 0):
            got = jpeg_device.decode_host([f], sub_bits)
            assert torch.equal(got, want), (name, sub_bits, int((got != want).sum()))


def test_refused_files_keep_the_host_path():
    from hyres_hip import jpeg_device
    from models.utils.turbo_jpeg_compression import TurboJPEGCompression
    devc = TurboJPEGCompression(workers=1, device_codec=True)
    for name, f in refused_files().items():
        assert not jpeg_device.supported_file(f), name
        why = jpeg_device.unsupported_reason(f)
        assert isinstance(why, str) and len(why) > 8, (name, why)
        with pytest.raises(ValueError):
            jpeg_device.decode_host([f])
        assert not devc.decode_on_device([f], "cuda"), name
        assert torch.equal(devc.decompress([io.BytesIO(f)], "cpu"), host_decode([f])[0]), name
    why = {n: jpeg_device.unsupported_reason(f) for n, f in refused_files().items()}
    assert "Huffman" in why["optimize"] and "restart" in why["restart"] and "progressive" in why["progressive"]
    assert "subsampling" in why["444"] and "subsampling" in why["420"] and "three components" in why["grey"]
    assert "MCU" in why["60x72"]
    # a batch mixing 64 x 64 and 64 x 128: each file is supported, the batch is not
    mixed = [case_named("noise_64x64_q50")["file"], case_named("noise_64x128_q50")["file"]]
    assert all(jpeg_device.supported_file(f) for f in mixed)
    assert not devc.decode_on_device(mixed, "cuda")
    with pytest.raises(ValueError):
        jpeg_device.decode_host(mixed)
    with pytest.raises((ValueError, RuntimeError)):  # np.stack of two sizes: the host path's own answer, unchanged
        devc.decompress([io.BytesIO(f) for f in mixed], "cpu")
    # supported files with a GPU target take the device path, with a CPU target the host path
    assert devc.decode_on_device(mixed[:1], "cuda") and not devc.decode_on_device(mixed[:1], "cpu")
    assert not TurboJPEGCompression(workers=1, device_codec=False).decode_on_device(mixed[:1], "cuda")
    assert jpeg_device.unsupported_reason(mixed[0][:-2]) is not None  # no EOI
    assert jpeg_device.unsupported_reason(b"") is not None and jpeg_device.unsupported_reason(b"\xff\xd8\xff") is not None


def test_rounds_are_bounded_by_the_subsequence_count():
    from hyres_hip import jpeg_device
    one = 0
    for c in CASES:
        _, rounds = jpeg_device.decode_host([c["file"]], 32, return_rounds=True)
        nsub = -(-unstuffed_bits(c["file"]) // 32)
        r = int(rounds[0])
        assert 0 <= r <= nsub and r <= max(nsub - 1, 0), (c["name"], r, nsub)
        if nsub == 1:  # nothing to synchronise: the loop runs no round
            assert c["u8"].shape[:2] == (8, 16) and r == 0, c["name"]
            one += 1
    assert one >= 1
    # more subsequences than a work-group has threads: the strided loop of the kernel is a tested path
    assert -(-unstuffed_bits(case_named("noise_64x64_q95")["file"]) // 32) > 1024
    f, want = noise_64x128_q95()
    nsub = -(-unstuffed_bits(f) // 32)
    dec, rounds = jpeg_device.decode_host([f], 32, return_rounds=True)
    assert nsub > 3000 and int(rounds[0]) <= nsub - 1 and torch.equal(dec, want)


@pytest.mark.parametrize("name", ["truncated", "zeroed_tail", "planted_rst"])
def test_corrupt_files_are_refused_or_decode(name):
    from hyres_hip import jpeg_device
    f = corrupt_files()[name]
    assert jpeg_device.supported_file(f)  # the markers are intact: the entropy decoder has to notice
    for sub_bits in (32, 0):
        dec, status = jpeg_device.decode_host([f], sub_bits, check=False)
        assert dec.shape == (1, 3, 64, 64)
        if int(status[0]):
            with pytest.raises(ValueError, match="image"):
                jpeg_device.decode_host([f], sub_bits)
        else:
            assert torch.equal(jpeg_device.decode_host([f], sub_bits), dec)
    # the status names the image inside a batch
    good = case_named("noise_64x64_q50")["file"]
    _, status = jpeg_device.decode_host([good, f, good], check=False)
    assert status[0] == 0 and status[2] == 0
    if name in ("truncated", "planted_rst"):  # half the blocks are missing / a marker sits in the segment
        assert status[1] != 0
        with pytest.raises(ValueError, match=r"image\(s\) 1 "):
            jpeg_device.decode_host([good, f, good])


def test_library_refuses_bad_decode_arguments():
    from hyres_hip import _lib as L
    lib = L.load()
    assert lib.hyres_jpeg_decode_workspace_bytes(2, 64, 64, 4096) > 0
    assert lib.hyres_jpeg_decode_workspace_bytes(2, 64, 72, 4096) == -1
    assert lib.hyres_jpeg_decode_workspace_bytes(2, 64, 64, 0) == -1
    from hyres_hip import jpeg_device
    good = case_named("noise_64x64_q50")["file"]
    for bad in (16, 48, 16384):
        with pytest.raises(L.HipError):
            jpeg_device.decode_host([good], bad)
