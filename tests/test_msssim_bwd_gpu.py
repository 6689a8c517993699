"""MS-SSIM backward on the GPU: hyres_msssim_bwd (csrc/msssim.hip) through hyres_hip.metrics' autograd function against
autograd through the fp64 torch-op restatement (tests/msssim_bwd_ref.py, bound from the restatement's own fp32 error);
symmetry, repeatability, batch independence, layouts, fp16, graph capture; RateDistortionLoss(metric="ms-ssim") and a
captured training step with it.

Measured on an MI355X (max|g - g64| / bound, worst case per group): see DESIGN.md section 8, "Backward"."""
import math

import pytest
import torch

import msssim_bwd_ref as G
import msssim_ref as R
from helpers import build_model

pytestmark = pytest.mark.gpu


def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def grad(x, y, weights=None, wrt="y"):
    from hyres_hip import metrics
    return G.device_grad(metrics, x.to(dev()), y.to(dev()), weights, wrt)


@pytest.mark.parametrize("shape,dist", G.PARITY, ids=G.PARITY_IDS)
def test_device_gradient_matches_autograd_of_the_restatement(shape, dist):
    ref = G.case(shape, dist)
    g = grad(ref["x"], ref["y"])
    assert g.is_cuda and g.shape == ref["y"].shape
    G.check(g, ref, f"device {shape} {dist}")


@pytest.mark.parametrize("shape", R.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_identical_and_inverted_images(shape):
    """x == y: rounding noise only, below 1e-3 of the shape's gradient scale (a wrong sign or a missing term is of the
    order of the scale). y = 1 - x: every level-0 mean is about -0.99 and the gradient is exactly zero."""
    seed = R.SHAPES.index(shape)
    s = G.case(shape, "noise")["s"]
    g = grad(*R.make_pair(shape, "same", seed=seed))
    print(f"same {shape}: max|g| {float(g.abs().max()):.3e} s {s:.3e}")
    assert torch.isfinite(g).all() and float(g.abs().max()) <= 1e-3 * s
    g = grad(*R.make_pair(shape, "inverted", seed=seed))
    assert torch.equal(g, torch.zeros_like(g))


@pytest.mark.parametrize("shape,weights", G.REDUCED, ids=["ssim-12x43", "two-levels-21x21"])
def test_reduced_levels_at_the_smallest_shapes(shape, weights):
    ref = G.case(shape, "noise", weights)
    G.check(grad(ref["x"], ref["y"], weights), ref, f"device {shape} levels {len(weights)}")


def test_ssim_is_differentiable_on_device():
    from hyres_hip import metrics
    shape, w = G.REDUCED[0]
    ref = G.case(shape, "noise", w)
    x, y = ref["x"].to(dev()), ref["y"].to(dev()).requires_grad_(True)
    v = metrics.ssim(x, y, size_average=False)
    assert torch.equal(v.detach(), metrics.ssim(x, y.detach(), size_average=False))
    (v * G.grad_out(1).to(dev())).sum().backward()
    G.check(y.grad, ref, "device ssim")


def test_first_argument_gradient_is_the_swapped_call():
    from hyres_hip import metrics
    ref = G.case(R.SHAPES[1], "blur")
    x, y = ref["x"].to(dev()), ref["y"].to(dev())
    gx = grad(x, y, wrt="x")
    assert torch.equal(gx, grad(y, x)) and not torch.equal(gx, grad(x, y))
    a, b = x.clone().requires_grad_(True), y.clone().requires_grad_(True)
    (metrics.ms_ssim(a, b, size_average=False) * G.grad_out(2).to(dev())).sum().backward()
    assert torch.equal(a.grad, gx) and torch.equal(b.grad, grad(x, y))
    G.check(b.grad, ref, "both require grad")


@pytest.mark.parametrize("shape", R.SHAPES[:2], ids=lambda s: "x".join(map(str, s)))
def test_repeatable_and_independent_of_the_batch(shape):
    """Two calls give the same bits, and with an explicit grad_out image b of a batch gets the bits it gets alone."""
    from hyres_hip import metrics
    ref = G.case(shape, "noise")
    x, y = ref["x"].to(dev()), ref["y"].to(dev())
    g = grad(x, y)
    assert torch.equal(g, grad(x, y))
    go = G.grad_out(shape[0]).to(dev())
    for b in range(shape[0]):
        yb = y[b:b + 1].clone().requires_grad_(True)
        metrics.ms_ssim(x[b:b + 1], yb, size_average=False).backward(go[b:b + 1])
        assert torch.equal(yb.grad[0], g[b]), b


def test_noncontiguous_and_fp16_inputs():
    from hyres_hip import metrics
    ref = G.case(R.SHAPES[2], "noise")
    x, y = ref["x"].to(dev()), ref["y"].to(dev())
    want = grad(x, y)
    xcl = x.contiguous(memory_format=torch.channels_last)
    wide = torch.zeros(1, 3, 180, 216, device=dev())
    wide[:, :, 2:178, 5:213] = y
    wide.requires_grad_(True)
    ysl = wide[:, :, 2:178, 5:213]
    assert not xcl.is_contiguous() and not ysl.is_contiguous()
    metrics.ms_ssim(xcl, ysl, size_average=False).backward(G.grad_out(1).to(dev()))
    assert torch.equal(wide.grad[:, :, 2:178, 5:213], want)
    ycl = y.contiguous(memory_format=torch.channels_last).requires_grad_(True)
    metrics.ms_ssim(x, ycl, size_average=False).backward(G.grad_out(1).to(dev()))
    assert torch.equal(ycl.grad, want)
    # fp16 in, fp16 gradient out: the fp32 gradient of the fp16 values, rounded
    h = y.half().requires_grad_(True)
    metrics.ms_ssim(x, h, size_average=False).backward(G.grad_out(1).to(dev()))
    assert h.grad.dtype == torch.float16 and torch.equal(h.grad, grad(x, y.half().float()).half())


def test_forward_and_backward_are_capture_legal():
    """Forward + backward captured once, replayed on a second pair and on the first again: each replay gives that
    pair's eager gradient bits."""
    from hyres_hip import metrics
    D = dev()
    shape = R.SHAPES[0]
    a, b = G.case(shape, "noise"), G.case(shape, "blur")
    pairs = [(a["x"].to(D), a["y"].to(D)), (b["x"].to(D), b["y"].to(D))]
    go = G.grad_out(shape[0]).to(D)
    eager = [grad(x, y) for x, y in pairs]
    assert not torch.equal(eager[0], eager[1])
    sx, sy = pairs[0][0].clone(), pairs[0][1].clone().requires_grad_(True)

    def step():
        g, = torch.autograd.grad((metrics.ms_ssim(sx, sy, size_average=False) * go).sum(), sy)
        return g

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step()  # warm-up: this stream's workspaces exist before the capture
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        g = step()
    for k in (1, 0):
        with torch.no_grad():
            sx.copy_(pairs[k][0])
            sy.copy_(pairs[k][1])
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(g, eager[k]), k
    G.check(g, a, "replayed")


def test_no_grad_path_is_unchanged():
    from hyres_hip import metrics
    ref = R.case(R.SHAPES[0], "noise")
    x, y = ref["x"].to(dev()), ref["y"].to(dev())
    want, _ = metrics.per_level(x, y)
    assert want.grad_fn is None
    yg = y.clone().requires_grad_(True)
    with torch.no_grad():
        out = metrics.ms_ssim(x, yg, size_average=False)
    assert out.grad_fn is None and torch.equal(out, want)
    assert metrics.ms_ssim(x, y, size_average=False).grad_fn is None
    assert torch.equal(metrics.ms_ssim(x, yg, size_average=False).detach(), want)


# ------------------------------------------------------------------ RateDistortionLoss(metric="ms-ssim")
def _synthetic_output(D):
    g = torch.Generator().manual_seed(21)
    ref = G.case(R.SHAPES[0], "noise")
    lik = {"y": (torch.rand((2, 24, 11, 11), generator=g) * 0.95 + 0.05).to(D),
           "z": (torch.rand((2, 16, 3, 3), generator=g) * 0.95 + 0.05).to(D)}
    return ref, {"likelihoods": lik, "x_hat": ref["y"].to(D).requires_grad_(True),
                 "jpeg_bpp_loss": torch.tensor(0.125, device=D)}


def test_ms_ssim_loss_matches_the_restatement():
    """loss = lmbda * (1 - ms_ssim(x_hat, target)) + bpp_loss. ms_ssim_loss is held to the forward's bound; loss to
    lmbda times it plus two fp32 roundings at the loss's magnitude (the product and the sum with bpp_loss, which is
    taken as the criterion reports it: its own parity is tests/test_parity_gpu.py's). The x_hat gradient is lmbda / B
    times the per-image gradients, held to lmbda times the backward's bound."""
    from hyres_hip.loss import RateDistortionLoss
    D = dev()
    lmbda = 0.5
    ref, output = _synthetic_output(D)
    target = ref["x"].to(D)
    c = RateDistortionLoss(lmbda=lmbda, alpha=0, metric="ms-ssim")(output, target)
    gx, = torch.autograd.grad(c["loss"], output["x_hat"])
    c = {k: v.detach() for k, v in c.items()}
    assert set(c) == {"loss", "bpp_loss", "residual_bpp_loss", "y_bpp_loss", "z_bpp_loss", "mse_loss", "vgg_loss",
                      "ms_ssim_loss"}
    fwd = R.case(R.SHAPES[0], "noise")  # symmetric: ms_ssim(x_hat = y, target = x)
    want = 1 - float(fwd["out"].mean())
    tol = float(fwd["tol_out"].max())
    print(f"ms_ssim_loss {float(c['ms_ssim_loss']):.7f} want {want:.7f} tol {tol:.3e}")
    assert abs(float(c["ms_ssim_loss"]) - want) <= tol
    want_loss = lmbda * want + float(c["bpp_loss"].double())
    assert abs(float(c["loss"]) - want_loss) <= lmbda * tol + 2.0 ** -23 * abs(want_loss)
    mse = float(((ref["y"].double() - ref["x"].double()) ** 2).mean()) * 255 ** 2
    assert math.isclose(float(c["mse_loss"]), mse, rel_tol=1e-5)  # still reported
    # d loss / d x_hat = -lmbda / B * sum_b d out[b] / d x_hat: the reference with a uniform grad_out
    yy = ref["y"].double().requires_grad_(True)
    R.ms_ssim_ref(ref["x"], yy)[0].mean().backward()
    y32 = ref["y"].clone().requires_grad_(True)
    R.ms_ssim_ref(ref["x"], y32, torch.float32)[0].mean().backward()
    d = float((y32.grad.double() - yy.grad).abs().max())
    err = float((gx.cpu().double() + lmbda * yy.grad).abs().max())
    bound = lmbda * G.bound(d, yy.grad.abs().max())
    print(f"x_hat gradient: err {err:.3e} bound {bound:.3e}")
    assert err <= bound


def test_default_metric_is_untouched():
    import sys
    from hyres_hip.loss import RateDistortionLoss
    D = dev()
    ref, output = _synthetic_output(D)
    target = ref["x"].to(D)
    a = RateDistortionLoss(lmbda=0.5, alpha=0)(output, target)
    b = RateDistortionLoss(lmbda=0.5, alpha=0, metric="mse")(output, target)
    assert list(a) == list(b) == ["loss", "bpp_loss", "residual_bpp_loss", "y_bpp_loss", "z_bpp_loss", "mse_loss",
                                  "vgg_loss"]
    assert all(torch.equal(a[k], b[k]) for k in a)
    ga, = torch.autograd.grad(a["loss"], output["x_hat"])
    gb, = torch.autograd.grad(b["loss"], output["x_hat"])
    assert torch.equal(ga, gb)
    with pytest.raises(ValueError, match="metric"):
        RateDistortionLoss(lmbda=0.5, alpha=0, metric="ssim")


def test_training_step_with_ms_ssim_eager_and_captured():
    """An eager step with the ms-ssim criterion gives a finite loss and a finite gradient wherever the mse criterion
    gives one; CapturedStep with the same criterion replays to the eager step's loss and gradient bits."""
    from hyres_hip.graphs import CapturedStep
    from hyres_hip.loss import RateDistortionLoss
    import torch.nn.functional as F
    D = dev()
    net, _ = build_model()
    net = net.to(D).train()
    x = R.smooth_field((1, 3, 192, 192), 17)
    j = F.conv2d(F.pad(x, (2, 2, 2, 2), mode="replicate"), torch.full((3, 1, 5, 5), 1 / 25.0), groups=3)
    x, j = x.to(D), j.to(D)
    # the training draws (EntropyBottleneck z, GaussianConditional y) injected, so that a replay repeats the eager step
    gen = torch.Generator().manual_seed(23)
    net.residual_model.noise.injected = {"z": (torch.rand((1, 6, 6, 128), generator=gen) - 0.5).to(D),
                                         "y": (torch.rand((1, 24, 24, 192), generator=gen) - 0.5).to(D)}
    params = [p for p in net.parameters() if p.requires_grad]

    def zero():
        for p in params:
            if p.grad is not None:
                p.grad.zero_()

    def eager(crit):
        for p in params:
            p.grad = None
        c = crit(net.forward_device(x, j, 0.25), x)
        c["loss"].backward()
        torch.cuda.synchronize()
        return c

    eager(RateDistortionLoss(lmbda=0.045, alpha=0))
    with_mse = [p.grad is not None for p in params]
    crit = RateDistortionLoss(lmbda=8.0, alpha=0, metric="ms-ssim")
    c = {k: v.detach() for k, v in eager(crit).items()}
    loss_e = float(c["loss"])
    assert math.isfinite(loss_e) and 0 < float(c["ms_ssim_loss"]) < 1
    assert loss_e == float(crit.lmbda * c["ms_ssim_loss"] + c["bpp_loss"])
    for p, had in zip(params, with_mse):
        assert (p.grad is not None) == had and (not had or torch.isfinite(p.grad).all()), p.shape
    assert any(float(p.grad.abs().max()) > 0 for p in params if p.grad is not None)
    grads_e = [None if p.grad is None else p.grad.detach().clone() for p in params]
    c = None
    zero()
    cap = CapturedStep(net, x, j, 0.25, criterion=crit, zero_grad=zero)
    cc = cap.replay()[1]
    torch.cuda.synchronize()
    assert float(cc["loss"].detach()) == loss_e
    for p, ge in zip(params, grads_e):
        assert ge is None or torch.equal(p.grad, ge), p.shape
    cc = None
    cap.close()
