"""The references of tests/refine_ref.py checked against torch on the CPU (no GPU, no HIP): the explicit bilinear
matrices and their transpose against F.interpolate and its autograd in fp64 (1e-6: the fp32 source index of the
reference against torch's fp64 one is the only difference), torch.max's tie rule, and the closed form of the folded
SpatialAttention / PReLU backward against autograd."""
import pytest
import torch
import torch.nn.functional as F

import refine_ref as RR
from helpers import rel_err

ALL_SHAPES = RR.BILINEAR_SHAPES + RR.PRELU_UP_SHAPES


def _interp(x_nhwc, s, conv):
    (hi, wi), (ho, wo), _, sf = s
    xc = x_nhwc.permute(0, 3, 1, 2)
    if conv == "size":
        y = F.interpolate(xc, size=(ho, wo), mode="bilinear", align_corners=False)
    else:
        y = F.interpolate(xc, scale_factor=sf, mode="bilinear", align_corners=False)
    assert tuple(y.shape[2:]) == (ho, wo)
    return y.permute(0, 2, 3, 1)


@pytest.mark.parametrize("conv", ["size", "sf"])
@pytest.mark.parametrize("s", ALL_SHAPES, ids=RR.shape_id)
def test_bilinear_ref_matches_interpolate_fwd_and_adjoint(s, conv):
    (hi, wi), (ho, wo), _, _ = s
    sh, sw = RR.scales_of(s, conv)
    x = RR.rand((2, hi, wi, 8), 1).double().requires_grad_()
    y = _interp(x, s, conv)
    gy = RR.rand((2, ho, wo, 8), 2).double()
    y.backward(gy)
    assert rel_err(RR.bilinear_ref(x.detach(), ho, wo, sh, sw), y.detach()) < 1e-6
    assert rel_err(RR.bilinear_bwd_ref(gy, hi, wi, sh, sw), x.grad) < 1e-6


def test_bilinear_adjoint_is_the_transpose():
    """<M x, g> == <x, M^T g> to fp64 rounding, on a non-integer scale."""
    x, g = RR.rand((1, 13, 9, 3), 3).double(), RR.rand((1, 5, 7, 3), 4).double()
    a = (RR.bilinear_ref(x, 5, 7, 13 / 5, 9 / 7) * g).sum()
    b = (x * RR.bilinear_bwd_ref(g, 13, 9, 13 / 5, 9 / 7)).sum()
    assert abs(float(a - b)) < 1e-12 * max(1.0, abs(float(a)))


@pytest.mark.parametrize("C", [4, 20, 64, 192, 260])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64, torch.float16])
def test_torch_max_keeps_the_first_maximal_index_on_ties(C, dtype):
    x = RR.tie_input((2, 17, 33, C), 5).to(dtype)
    first = RR.first_argmax(x)
    ties = (x == x.max(-1, keepdim=True)[0]).sum(-1)
    assert int((ties > 1).sum()) > x.shape[0] * 17 * 33 // 4 and bool((x.view(-1, C)[0::5] == 0).all())
    assert int((first[(x == 0).all(-1)] != 0).sum()) == 0
    if dtype != torch.float16:  # the references run in fp64 (fp16 inputs are widened first)
        assert torch.equal(x.permute(0, 3, 1, 2).max(1)[1], first)
        assert torch.equal(RR.sa_ref(x.double(), RR.rand((1, 2, 7, 7), 6).double())[3], first)
    # a duplicated maximum in the last channel does not win
    dup = x.view(-1, C)[3::7]
    assert bool((dup[:, -1] == dup.max(-1)[0]).all()) and bool((RR.first_argmax(dup) <= C - 1).all())
    nz = dup.max(-1)[0] > 0
    assert bool((RR.first_argmax(dup)[nz & (dup[:, :-1].max(-1)[0] == dup[:, -1])] < C - 1).all())


def test_sa_ref_routes_the_max_gradient_to_the_first_index():
    x = RR.tie_input((1, 5, 3, 20), 7).double().requires_grad_()
    w = RR.rand((1, 2, 7, 7), 8, 0.3).double()
    w[:, 0] = 0  # no mean path: the gradient beyond gy * attn lands on one channel per pixel
    y, attn, _, idx = RR.sa_ref(x, w)
    gy = RR.rand(y.shape, 9).double()
    y.backward(gy)
    r = x.grad - gy * attn.detach()[..., None]
    hot = torch.zeros_like(r, dtype=torch.bool).scatter_(-1, RR.first_argmax(x.detach())[..., None], True)
    assert float(r[~hot].abs().max()) == 0.0 and float(r[hot].abs().min()) > 0.0
    assert torch.equal(idx, RR.first_argmax(x.detach()))


@pytest.mark.parametrize("P,C", [(7, 4), (1000, 20), (300, 64)])
def test_sa_fold_closed_form_matches_autograd(P, C):
    z = RR.rand((P, C), 10).double().requires_grad_()
    logit = RR.rand((P,), 11, 2.0).double().requires_grad_()
    bias = RR.rand((C,), 12, 0.5).double()
    bias[0] = 0.0
    with torch.no_grad():
        z[::3, 0] = 0.0  # pre == 0 exactly there
    bias.requires_grad_()
    slope = torch.tensor([0.25], dtype=torch.float64, requires_grad=True)
    attn = torch.sigmoid(logit)
    pre = attn[:, None] * z + bias
    assert int((pre == 0).sum()) >= P // 3 and bool((pre > 0).any()) and bool((pre < 0).any())
    gy = RR.rand((P, C), 13).double()
    F.prelu(pre, slope).backward(gy)
    gs, glogit, dbias, dslope = RR.sa_fold_bwd_ref(pre.detach(), gy, attn.detach(), bias.detach(), 0.25)
    assert rel_err(gs, z.grad) < 1e-12
    assert rel_err(glogit, logit.grad) < 1e-12
    assert rel_err(dbias, bias.grad) < 1e-12
    assert rel_err(dslope, slope.grad[0]) < 1e-12


def test_prelu_bwd_ref_matches_autograd():
    pre = RR.rand((50, 8), 14).double()
    pre[::4] = 0.0
    pre.requires_grad_()
    slope = torch.tensor([0.2], dtype=torch.float64, requires_grad=True)
    g = RR.rand((50, 8), 15).double()
    F.prelu(pre, slope).backward(g)
    gi, ds = RR.prelu_bwd_ref(pre.detach(), g, 0.2)
    assert rel_err(gi, pre.grad) < 1e-14 and rel_err(ds, slope.grad[0]) < 1e-12


def test_se_ref_matches_module_formulation():
    x = RR.rand((2, 37, 16), 16).double()
    w1, w2 = RR.rand((2, 16), 17).double(), RR.rand((16, 2), 18).double()
    y, pooled, hidden, gate = RR.se_ref(x, w1, w2)
    xc = x.permute(0, 2, 1)[..., None]  # [B, C, HW, 1]
    s = torch.sigmoid(F.conv2d(F.relu(F.conv2d(F.adaptive_avg_pool2d(xc, 1), w1[:, :, None, None])), w2[:, :, None, None]))
    assert rel_err(y, (xc * s)[..., 0].permute(0, 2, 1)) < 1e-14
