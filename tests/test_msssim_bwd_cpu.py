"""MS-SSIM backward on the CPU: the host twin hyres_msssim_bwd_host (the kernels' arithmetic, csrc/msssim_core.h)
through hyres_hip.metrics' autograd function, against autograd through the fp64 torch-op restatement
(tests/msssim_bwd_ref.py); the argument checks of the new C-ABI entries, RateDistortionLoss's metric argument and the
training CLI's guard. No GPU call is made."""
import ctypes

import pytest
import torch

import msssim_bwd_ref as G
import msssim_ref as R


@pytest.mark.parametrize("shape,dist", G.PARITY, ids=G.PARITY_IDS)
def test_host_twin_gradient_matches_autograd_of_the_restatement(shape, dist):
    from hyres_hip import metrics
    ref = G.case(shape, dist)
    g = G.device_grad(metrics, ref["x"], ref["y"])
    assert g.shape == ref["y"].shape
    G.check(g, ref, f"host {shape} {dist}")


@pytest.mark.parametrize("shape", R.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_identical_images_give_a_negligible_gradient(shape):
    """x == y is the maximum: the fp64 gradient is ~1e-18 and any fp32 evaluation leaves rounding noise, so the bound
    is 1e-3 of the shape's gradient scale, which only a wrong sign or a missing term exceeds."""
    from hyres_hip import metrics
    x, y = R.make_pair(shape, "same", seed=R.SHAPES.index(shape))
    g = G.device_grad(metrics, x, y)
    s = G.case(shape, "noise")["s"]
    print(f"same {shape}: max|g| {float(g.abs().max()):.3e} s {s:.3e}")
    assert torch.isfinite(g).all() and float(g.abs().max()) <= 1e-3 * s


@pytest.mark.parametrize("shape", R.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_negative_level_means_give_an_exactly_zero_gradient(shape):
    """y = 1 - x: the level-0 means are about -0.99, relu clamps them, and the gradient is 0 everywhere (not NaN from
    0 * inf in the pow's backward)."""
    from hyres_hip import metrics
    x, y = R.make_pair(shape, "inverted", seed=R.SHAPES.index(shape))
    assert (metrics.per_level(x, y)[1][0] < 0).all()
    g = G.device_grad(metrics, x, y)
    assert torch.equal(g, torch.zeros_like(g))


@pytest.mark.parametrize("shape,weights", G.REDUCED, ids=["ssim-12x43", "two-levels-21x21"])
def test_reduced_levels_at_the_smallest_shapes(shape, weights):
    from hyres_hip import metrics
    ref = G.case(shape, "noise", weights)  # ms_ssim_ref accepts these shapes: the reference is built from it
    assert ref["s"] > 0 and torch.isfinite(ref["g64"]).all()
    G.check(G.device_grad(metrics, ref["x"], ref["y"], weights), ref, f"host {shape} levels {len(weights)}")


def test_ssim_is_differentiable_and_keeps_its_value():
    from hyres_hip import metrics
    shape, w = G.REDUCED[0]
    ref = G.case(shape, "noise", w)
    y = ref["y"].clone().requires_grad_(True)
    v = metrics.ssim(ref["x"], y, size_average=False)
    assert torch.equal(v.detach(), metrics.ssim(ref["x"], ref["y"], size_average=False))
    (v * G.grad_out(1)).sum().backward()
    G.check(y.grad, ref, "host ssim")


def test_first_argument_both_arguments_and_dtypes():
    from hyres_hip import metrics
    ref = G.case(R.SHAPES[0], "noise")
    x, y = ref["x"], ref["y"]
    gy = G.device_grad(metrics, x, y)
    # the gradient towards the first argument is the swapped call's gradient towards the second, bit for bit
    assert torch.equal(G.device_grad(metrics, y, x, wrt="x"), gy)
    a, b = x.clone().requires_grad_(True), y.clone().requires_grad_(True)
    (metrics.ms_ssim(a, b, size_average=False) * G.grad_out(2)).sum().backward()
    assert torch.equal(b.grad, gy) and torch.equal(a.grad, G.device_grad(metrics, x, y, wrt="x"))
    # fp64 and non-contiguous inputs: the gradient comes back in the input's dtype and layout-independent
    d = y.double().contiguous(memory_format=torch.channels_last).requires_grad_(True)
    (metrics.ms_ssim(x, d, size_average=False) * G.grad_out(2)).sum().backward()
    assert d.grad.dtype == torch.float64 and torch.equal(d.grad.float(), gy)
    # size_average: the mean's 1 / B reaches every image
    m = y.clone().requires_grad_(True)
    metrics.ms_ssim(x, m).backward()
    n = y.clone().requires_grad_(True)
    metrics.ms_ssim(x, n, size_average=False).mean().backward()
    assert torch.equal(m.grad, n.grad) and float(m.grad.abs().max()) > 0


def test_no_grad_path_is_unchanged_and_means_carry_no_gradient():
    from hyres_hip import metrics
    ref = R.case(R.SHAPES[0], "noise")
    x, y = ref["x"], ref["y"]
    want, means = metrics.per_level(x, y)
    assert want.grad_fn is None and not want.requires_grad
    yg = y.clone().requires_grad_(True)
    with torch.no_grad():
        out = metrics.ms_ssim(x, yg, size_average=False)
    assert out.grad_fn is None and torch.equal(out, want)
    out, m = metrics.per_level(x, yg)
    assert out.grad_fn is not None and torch.equal(out.detach(), want)
    assert not m.requires_grad and torch.equal(m, means)


def test_double_backward_is_refused():
    from hyres_hip import metrics
    ref = R.case(R.SHAPES[0], "noise")
    y = ref["y"].clone().requires_grad_(True)
    with pytest.raises(RuntimeError, match="double backward is not supported"):
        torch.autograd.grad(metrics.ms_ssim(ref["x"], y), y, create_graph=True)
    g, = torch.autograd.grad(metrics.ms_ssim(ref["x"], y), y)
    assert not g.requires_grad


def test_bwd_entries_check_their_arguments_without_a_gpu():
    from hyres_hip import _lib as L
    lib = L.load()
    x = torch.rand(1, 3, 161, 161)
    g, go = torch.empty_like(x), torch.ones(1)
    w = (ctypes.c_float * 5)(*R.WEIGHTS)
    need = lib.hyres_msssim_bwd_workspace_bytes(1, 3, 161, 161, 5)
    assert need > lib.hyres_msssim_workspace_bytes(1, 3, 161, 161, 5) > 0
    assert lib.hyres_msssim_bwd_workspace_bytes(1, 3, 160, 200, 5) == -1

    def call(fn, xp=x.data_ptr(), go_p=go.data_ptr(), g_p=g.data_ptr(), H=161, levels=5, ws=None, n=0):
        rc = fn(xp, x.data_ptr(), 1, 3, H, 161, levels, w, 1.0, go_p, g_p, ws, n, None)
        return rc, lib.hyres_last_error_string().decode()

    for fn in (lib.hyres_msssim_bwd, lib.hyres_msssim_bwd_host):
        assert call(fn, xp=None)[0] == 1003 and call(fn, go_p=None)[0] == 1003 and call(fn, g_p=None)[0] == 1003
        assert call(fn, levels=6)[0] == 1003
        rc, msg = call(fn, H=160)
        assert rc == 1001 and "160" in msg
    rc, msg = call(lib.hyres_msssim_bwd, ws=g.data_ptr(), n=need - 1)  # validated before any launch
    assert rc == 1004 and str(need) in msg
    assert call(lib.hyres_msssim_bwd)[0] == 1004  # ws == NULL


def test_rate_distortion_loss_metric_argument():
    from hyres_hip.loss import RateDistortionLoss
    assert RateDistortionLoss(lmbda=0.5, alpha=0).metric == "mse"
    assert RateDistortionLoss(lmbda=0.5, alpha=0, metric="ms-ssim").metric == "ms-ssim"
    for bad in ("msssim", "MS-SSIM", "psnr", None):
        with pytest.raises(ValueError, match="metric"):
            RateDistortionLoss(lmbda=0.5, alpha=0, metric=bad)


def test_training_cli_refuses_small_patches_for_ms_ssim(monkeypatch, tmp_path):
    """--metric ms-ssim --patch-size 128 128 stops in the argument parser, before the dataset is looked at."""
    import src.training as T
    monkeypatch.setattr(T, "ImageFolder", lambda *a, **k: pytest.fail("the dataset was touched"))
    missing = str(tmp_path / "no_such_dataset")
    with pytest.raises(SystemExit, match="160"):
        T.main(["-d", missing, "--alpha", "0", "--metric", "ms-ssim", "--patch-size", "128", "128"])
    with pytest.raises(SystemExit, match="160"):
        T.parse_args(["-d", missing, "--metric", "ms-ssim", "--patch-size", "256", "160"])
    assert T.parse_args(["-d", missing, "--metric", "ms-ssim"]).metric == "ms-ssim"
    assert T.parse_args(["-d", missing, "--metric", "ms-ssim", "--patch-size", "161", "256"]).patch_size == [161, 256]
    assert T.parse_args(["-d", missing, "--patch-size", "128", "128"]).metric == "mse"
    with pytest.raises(SystemExit):
        T.parse_args(["-d", missing, "--metric", "psnr"])
