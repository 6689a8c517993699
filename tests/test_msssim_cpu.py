"""MS-SSIM / SSIM on the CPU: the pure-host twin of csrc/msssim.hip (same arithmetic, csrc/msssim_core.h) against the
fp64 torch-op restatement of pytorch_msssim's ms_ssim (tests/msssim_ref.py), the argument checks of the C-ABI and of
hyres_hip.metrics, and src/utils/metrics.py's CompressionMetrics on CPU tensors.  No GPU call is made."""
import ctypes
import math
import sys

import pytest
import torch

import msssim_ref as R

CASES = [(s, d) for s in R.SHAPES for d in R.DISTORTIONS]
IDS = [f"{'x'.join(map(str, s))}-{d}" for s, d in CASES]


@pytest.mark.parametrize("shape,dist", CASES, ids=IDS)
def test_host_twin_matches_restatement(shape, dist):
    from hyres_hip import metrics
    ref = R.case(shape, dist)
    out, raw = metrics.per_level(ref["x"], ref["y"])
    assert out.dtype == torch.float32 and out.shape == (shape[0],) and raw.shape == (5, shape[0], shape[1])
    R.check(out, raw, ref, f"host {shape} {dist}")
    if dist == "same":
        assert torch.equal(out, torch.ones_like(out))
    if dist == "inverted":
        assert (ref["raw"][0] < 0).all(), "the restatement's level-0 cs must be negative for the clamp to be exercised"
        assert (raw[0] < 0).all() and torch.equal(out, torch.zeros_like(out))
    got = metrics.ms_ssim(ref["x"], ref["y"])
    assert got.dim() == 0 and abs(float(got) - float(ref["out"].mean())) <= float(ref["tol_out"].max())
    assert torch.equal(metrics.ms_ssim(ref["x"], ref["y"], size_average=False), out)


def test_default_weights_equal_explicit_weights():
    from hyres_hip import metrics
    ref = R.case(R.SHAPES[0], "noise")
    a = metrics.ms_ssim(ref["x"], ref["y"], size_average=False)
    b = metrics.ms_ssim(ref["x"], ref["y"], size_average=False, weights=list(R.WEIGHTS))
    assert torch.equal(a, b)


@pytest.mark.parametrize("dist", ["noise", "blur", "inverted"])
def test_ssim_is_the_raw_level0_mean(dist):
    from hyres_hip import metrics
    shape = R.SHAPES[1]
    ref = R.case(shape, dist)
    want = R.ssim_ref(ref["x"], ref["y"])
    d = (R.ssim_ref(ref["x"], ref["y"], torch.float32).double() - want).abs().max()
    got = metrics.ssim(ref["x"], ref["y"], size_average=False)
    err = (got.double() - want).abs().max()
    print(f"ssim {dist}: ref {want.tolist()} d {d:.3e} err {err:.3e}")
    assert err <= R.bound(d)
    if dist == "inverted":
        assert (got < 0).all(), "ssim() is not clamped"
    assert abs(float(metrics.ssim(ref["x"], ref["y"])) - float(want.mean())) <= float(R.bound(d))


def test_fp64_and_noncontiguous_inputs_are_converted():
    from hyres_hip import metrics
    ref = R.case(R.SHAPES[2], "noise")
    want = metrics.ms_ssim(ref["x"], ref["y"], size_average=False)
    xcl = ref["x"].contiguous(memory_format=torch.channels_last)
    wide = torch.zeros(1, 3, 180, 216)
    wide[:, :, 2:178, 5:213] = ref["y"]
    assert torch.equal(metrics.ms_ssim(xcl.double(), wide[:, :, 2:178, 5:213], size_average=False), want)


def _native(name, x, y, levels, ws_bytes=0):
    from hyres_hip import _lib as L
    B, C, H, W = x.shape
    out = torch.empty(B)
    w = (ctypes.c_float * 5)(*R.WEIGHTS)
    rc = getattr(L.load(), name)(x.data_ptr(), y.data_ptr(), B, C, H, W, levels, w, 1.0, out.data_ptr(), None,
                                 out.data_ptr() if ws_bytes else None, ws_bytes, None)
    return rc, L.load().hyres_last_error_string().decode(), out


def test_minimum_size(monkeypatch):
    from hyres_hip import _lib as L
    from hyres_hip import metrics
    x = torch.rand(1, 3, 160, 200)
    rc, msg, _ = _native("hyres_msssim_host", x, x, 5)
    assert rc == 1001 and "160" in msg, (rc, msg)
    assert L.load().hyres_msssim_workspace_bytes(1, 3, 160, 200, 5) == -1
    assert L.load().hyres_msssim_workspace_bytes(1, 3, 161, 161, 5) > 0
    # ... and the Python entry raises before any native call
    monkeypatch.setattr(L, "call", lambda *a, **k: pytest.fail("native call on a bad shape"))
    with pytest.raises(ValueError, match="160"):
        metrics.ms_ssim(x, x)
    with pytest.raises(ValueError, match="160"):
        metrics.ms_ssim(x.transpose(2, 3), x.transpose(2, 3))
    with pytest.raises(ValueError):
        metrics.ms_ssim(x[0], x[0])
    with pytest.raises(ValueError):
        metrics.ms_ssim(torch.zeros(1, 3, 170, 170), torch.zeros(1, 3, 170, 171))
    with pytest.raises(ValueError):
        metrics.ms_ssim(torch.zeros(1, 3, 170, 170, dtype=torch.int32), torch.zeros(1, 3, 170, 170, dtype=torch.int32))
    with pytest.raises(ValueError):
        metrics.ms_ssim(torch.zeros(1, 3, 170, 170), torch.zeros(1, 3, 170, 170), weights=[0.2] * 6)
    with pytest.raises(ValueError, match="10"):
        metrics.ssim(torch.zeros(1, 1, 10, 64), torch.zeros(1, 1, 10, 64))


def test_161_passes_and_ssim_takes_eleven():
    from hyres_hip import metrics
    x = torch.rand(1, 1, 161, 161, generator=torch.Generator().manual_seed(3))
    assert float(metrics.ms_ssim(x, x)) == 1.0
    rc, _, out = _native("hyres_msssim_host", x, x, 5)
    assert rc == 0 and float(out) == 1.0
    s = torch.rand(1, 2, 11, 13, generator=torch.Generator().manual_seed(4))
    t = torch.rand(1, 2, 11, 13, generator=torch.Generator().manual_seed(5))
    want = R.ssim_ref(s, t)
    d = (R.ssim_ref(s, t, torch.float32).double() - want).abs().max()
    assert abs(float(metrics.ssim(s, t)) - float(want)) <= float(R.bound(d))


def test_device_entry_rejects_bad_arguments_without_a_gpu():
    """hyres_msssim validates before it launches: a short workspace, NULL pointers, the size limit, levels."""
    from hyres_hip import _lib as L
    x = torch.rand(1, 3, 161, 161)
    need = L.load().hyres_msssim_workspace_bytes(1, 3, 161, 161, 5)
    assert need > 0
    rc, msg, _ = _native("hyres_msssim", x, x, 5, ws_bytes=need - 1)
    assert rc == 1004 and str(need) in msg, (rc, msg)
    rc, _, _ = _native("hyres_msssim", x, x, 5, ws_bytes=0)  # ws == NULL
    assert rc == 1004
    rc, msg, _ = _native("hyres_msssim", x[..., :160, :], x[..., :160, :], 5, ws_bytes=need)
    assert rc == 1001 and "160" in msg
    lib = L.load()
    w = (ctypes.c_float * 5)(*R.WEIGHTS)
    out = torch.empty(1)
    for args in ((None, x.data_ptr(), w, out.data_ptr()), (x.data_ptr(), None, w, out.data_ptr()),
                 (x.data_ptr(), x.data_ptr(), None, out.data_ptr()), (x.data_ptr(), x.data_ptr(), w, None)):
        for fn in (lib.hyres_msssim, lib.hyres_msssim_host):
            assert fn(args[0], args[1], 1, 3, 161, 161, 5, args[2], 1.0, args[3], None, None, 0, None) == 1003
    assert lib.hyres_msssim_host(x.data_ptr(), x.data_ptr(), 1, 3, 161, 161, 6, w, 1.0, out.data_ptr(), None, None, 0,
                                 None) == 1003


def test_compression_metrics_on_cpu_tensors():
    from src.utils import CompressionMetrics
    assert "lpips" not in sys.modules and "pytorch_msssim" not in sys.modules
    ref = R.case(R.SHAPES[0], "noise")
    x, y = ref["x"], ref["y"]
    m = CompressionMetrics(device="cpu")
    v = m.msssim(x, y)
    assert isinstance(v, float) and abs(v - float(ref["out"].mean())) <= float(ref["tol_out"].max())
    mse = ((x.double() - y.double()) ** 2).mean(dim=[1, 2, 3])
    want = float((10 * torch.log10(1 / mse)).mean())
    p = m.psnr(x, y)
    assert isinstance(p, float) and math.isclose(p, want, rel_tol=1e-5) and 20 < p < 40
    with pytest.raises(RuntimeError, match="LPIPS"):
        m.lpips(x, y)
    allm = m.compute_all(x, y)
    assert set(allm) == {"psnr", "ms-ssim"} and allm["ms-ssim"] == v and allm["psnr"] == p
