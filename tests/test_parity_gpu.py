"""GPU parity: every HIP kernel family vs a CPU fp32 reference on the same seeded inputs, then the
whole model vs the oracle / golden fixtures produced by the reference's own code.

Tolerances (fp32 everywhere, BASELINE.json north_star: "within 1e-4 relative fp32"):
  * per-op:  max|hip - ref| <= 1e-4 * max|ref|  (normwise relative)
  * end-to-end x_hat / likelihoods: same bound, on elements whose quantisation decision agrees with the
    reference (a round() boundary flip changes y_hat by exactly 1 — reported as a fraction, must be rare).
"""
import contextlib
import ctypes

import pytest
import torch
import torch.nn.functional as F

from helpers import load_meta, load_npz, oracle_from, recipe_state_dict, rel_err

pytestmark = pytest.mark.gpu

TOL = 1e-4


def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def _rand(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(shape, generator=g) * 2 - 1) * scale


@pytest.fixture(params=["native", "bf16x6"])
def fp32_gemm(request):
    """The fp32 convs' GEMM (hyres_conv_tuning key 7): the native fp32 MFMA and the bf16x6 split on the bf16 MFMA —
    every test taking this fixture holds its fp32 bars on both, with the concurrent branch streams on."""
    from hyres_hip import _lib as L
    old = ctypes.c_int(0)
    L.call("hyres_conv_tuning", 7, 1 if request.param == "bf16x6" else 0, ctypes.byref(old))
    try:
        yield request.param
    finally:
        L.call("hyres_conv_tuning", 7, old.value, None)


# ------------------------------------------------------------------------------------------------ ops
CONV_CASES = [
    # B, Ci, Co, H, W, K, stride, pad, dil
    (2, 64, 64, 16, 16, 3, 1, 1, 1),
    (2, 128, 64, 16, 16, 1, 1, 0, 1),
    (2, 64, 128, 16, 16, 1, 1, 0, 1),
    (2, 128, 128, 16, 16, 5, 2, 2, 1),
    (2, 128, 192, 16, 16, 5, 2, 2, 1),
    (2, 3, 128, 32, 32, 5, 2, 2, 1),
    (2, 3, 64, 16, 16, 3, 1, 1, 1),
    (2, 64, 3, 16, 16, 3, 1, 1, 1),
    (2, 64, 64, 16, 16, 3, 1, 2, 2),
    (2, 192, 384, 8, 8, 5, 1, 2, 1),
    (1, 768, 640, 4, 4, 1, 1, 0, 1),
    (2, 192, 128, 8, 8, 3, 1, 1, 1),
    (3, 96, 40, 12, 20, 3, 1, 1, 1),
    (2, 64, 96, 16, 16, 5, 1, 2, 1),   # wgrad: 5 fused taps per block
    (2, 5, 48, 12, 12, 3, 1, 1, 1),    # wgrad: taps folded into N (N=5)
    (2, 48, 5, 12, 12, 3, 1, 1, 1),    # wgrad: small-M swap (M=5)
    # thin-operand weight gradient (wgrad_thin_kernel): N <= 4, M in {64, 128}
    (2, 1, 64, 20, 36, 3, 1, 1, 1),    # N = 1 (4-channel accumulator variant)
    (2, 64, 2, 20, 36, 3, 1, 1, 1),    # swapped (M = 2 -> wide 64, thin 2)
    (1, 3, 64, 6, 256, 3, 1, 2, 2),    # 256-wide row window, dilation 2
    (1, 3, 64, 4, 300, 3, 1, 1, 1),    # window wider than the LDS stage: generic tap-folded path
    (2, 3, 128, 16, 40, 5, 2, 2, 1),   # two tap groups, stride 2
    # halo-staged weight gradient (wgrad_halo_kernel; bf16x6: wgrad_halo_bf6[_pf2]_kernel): base rows a multiple of
    # 32 pixels
    (2, 64, 64, 32, 32, 3, 1, 1, 1),   # 3x3, one kernel row of 3 taps per block
    (2, 64, 64, 20, 64, 3, 1, 2, 2),   # dilated 3x3 (MultiScaleRefine): halo rows 2 apart, all 9 taps per block
    (1, 96, 64, 32, 32, 3, 1, 2, 2),
    (1, 96, 64, 8, 64, 3, 1, 1, 1),    # partial N tile (Ci = 96), two 32-px chunks per row
    (2, 64, 64, 64, 64, 5, 2, 2, 1),   # 5x5 stride 2 (Q stride 2), one kernel row per block
    (2, 64, 128, 32, 64, 5, 1, 2, 1),  # 5x5 stride 1, two M tiles
    # weight-resident persistent fp32 3x3 (conv3x3_wres_f32_kernel): Ci = 64, >= 2 tiles of 4 x 64 pixels per
    # block; forward and input-gradient; a partial last row tile; one 32-channel output slice (Co = 32)
    (2, 64, 64, 128, 256, 3, 1, 1, 1),
    (2, 64, 64, 126, 256, 3, 1, 1, 1),
    (4, 64, 32, 128, 256, 3, 1, 1, 1),
    # the tile walk's ragged case: 3 x 31 x 4 = 372 tiles (372 % 8 = 4, a partial last row tile) over 2 channel
    # groups x 128 blocks, so blocks of one launch walk 2 or 3 tiles
    (3, 64, 64, 122, 256, 3, 1, 1, 1),
]

# the weight-gradient kernel the cases above name in their comments, as hyres_wgrad_kernel_name reports it (under
# either fp32 GEMM mode): a case that drifts to another kernel no longer tests what it says
_HALO3 = r"wgrad_halo_(kernel<1, 3, 1, 1, 1>|bf6_pf2_kernel<3, 1, 1, 2>)"
_HALO3D = r"wgrad_halo_(bf6_)?kernel<3, 3, 1, 2(, 1)?>"
WGRAD_KERNELS = {
    (2, 64, 96, 16, 16, 5, 1, 2, 1): r"wgrad_kernel<1, 1, 2, 2, 5, true, true, false>",
    (2, 5, 48, 12, 12, 3, 1, 1, 1): r"wgrad_kernel<1, 1, 2, 2, 1, true, false, false>",   # folded: scalar Q loads
    (2, 48, 5, 12, 12, 3, 1, 1, 1): r"wgrad_kernel<1, 1, 2, 2, 1, true, false, false>",   # swapped: the same
    (2, 1, 64, 20, 36, 3, 1, 1, 1): r"wgrad_thin_kernel<1, 4, 9, 1, false>",
    (2, 64, 2, 20, 36, 3, 1, 1, 1): r"wgrad_thin_kernel<1, 4, 9, 1, false>",
    (1, 3, 64, 6, 256, 3, 1, 2, 2): r"wgrad_thin_kernel<1, 3, 9, 1, false>",
    (1, 3, 64, 4, 300, 3, 1, 1, 1): r"wgrad_kernel<1, 1, 4, 1, 1, true, false, false>",
    (2, 3, 128, 16, 40, 5, 2, 2, 1): r"wgrad_thin_kernel<2, 3, 13, 2, false>",
    (2, 64, 64, 32, 32, 3, 1, 1, 1): _HALO3,
    (2, 64, 64, 20, 64, 3, 1, 2, 2): _HALO3D,
    (1, 96, 64, 32, 32, 3, 1, 2, 2): _HALO3D,
    (1, 96, 64, 8, 64, 3, 1, 1, 1): _HALO3,
    (2, 64, 64, 64, 64, 5, 2, 2, 1): r"wgrad_halo_(bf6_)?kernel<1, 5, 2, 1(, 1)?>",
    (2, 64, 128, 32, 64, 5, 1, 2, 1): r"wgrad_halo_(bf6_)?kernel<1, 5, 1, 1(, 1)?>",
}


def _assert_wgrad_kernel(pattern, fn, *args, f16=False):
    import re
    from hyres_hip import _lib as L
    from hyres_hip import ops as O
    d = L.WgradDesc()
    L.call(fn, ctypes.byref(d), *args)
    d.f16_operands = int(f16)
    assert re.fullmatch(pattern, O.wgrad_variant(d)), (O.wgrad_variant(d), pattern)


@pytest.mark.parametrize("case", CONV_CASES)
def test_conv2d_fwd_bwd(case, fp32_gemm):
    from hyres_hip import _lib as L
    from hyres_hip import ops as O
    B, Ci, Co, H, W, K, s, p, d = case
    if case in WGRAD_KERNELS:
        _assert_wgrad_kernel(WGRAD_KERNELS[case], "hyres_wgrad_desc_conv2d", B, H, W, Ci, Ci, Co, Co, K, K, s, p, d)
    x = _rand((B, Ci, H, W), 1)
    w = _rand((Co, Ci, K, K), 2, 1.0 / (Ci * K * K) ** 0.5)
    b = _rand((Co,), 3, 0.1)
    xr, wr, br = x.clone().requires_grad_(), w.clone().requires_grad_(), b.clone().requires_grad_()
    yr = F.conv2d(xr, wr, br, stride=s, padding=p, dilation=d)
    gy = _rand(yr.shape, 4)
    yr.backward(gy)
    D = dev()
    wd = torch.nn.Parameter(w.to(D))
    bd = torch.nn.Parameter(b.to(D))
    tape = O.Tape()
    xn = O.to_nhwc(x.to(D), rg=True)
    yn = O.conv2d(tape, xn, wd, bd, stride=s, pad=p, dil=d)
    y = O.to_nchw(yn)
    yn.set_grad(O.nchw_grad_to_nhwc(gy.to(D)))
    tape.backward()
    torch.cuda.synchronize()
    assert rel_err(y.cpu(), yr) < TOL
    assert rel_err(O.to_nchw_grad(xn).cpu(), xr.grad) < TOL
    assert rel_err(wd.grad.cpu(), wr.grad) < TOL
    assert rel_err(bd.grad.cpu(), br.grad) < TOL


@pytest.mark.parametrize("case", [(2, 183, 183, 64, 128, 96), (1, 260, 260, 128, 64, 64), (2, 16, 16, 64, 128, 64),
                                  (1, 9, 23, 96, 96, 128)])
def test_conv1x1_epilogue_chain(case, fp32_gemm):
    """1x1 convs through a chain that exercises every streamed epilogue operand: a = relu(conv1(x) + r)
    (residual), b = relu(conv2(a)) (its dgrad takes the ReLU mask), y = conv3(b) + conv4(x) (x fans out:
    conv4's dgrad accumulates into conv1's). In the first two cases (>= 65536 pixels, K in {64, 96, 128})
    the layers without a streamed epilogue operand (conv2, conv3 forward, several dgrads) run on
    conv1x1_stream_kernel with ragged last 32-pixel tiles; the rest on the tiled kernel.
    Reference: torch fp64 with the ReLU decisions of the HIP forward (at 67k pixels x 128 channels a
    pre-activation within fp32 rounding of 0 occurs, and its flipped mask bit is a kink, not an error)."""
    from hyres_hip import _lib as L
    from hyres_hip import ops as O
    B, H, W, C0, C1, C2 = case
    x = _rand((B, C0, H, W), 11)
    r = _rand((B, C1, H, W), 12)
    ws = [_rand(sh, 13 + i, 1.0 / sh[1] ** 0.5) for i, sh in
          enumerate([(C1, C0, 1, 1), (C0, C1, 1, 1), (C2, C0, 1, 1), (C2, C0, 1, 1)])]
    bs = [_rand((sh,), 20 + i, 0.1) for i, sh in enumerate([C1, C0, C2, C2])]
    gy = _rand((B, C2, H, W), 30)
    D = dev()
    wd = [torch.nn.Parameter(w.to(D)) for w in ws]
    bd = [torch.nn.Parameter(b.to(D)) for b in bs]
    tape = O.Tape()
    xn = O.to_nhwc(x.to(D), rg=True)
    rn = O.to_nhwc(r.to(D), rg=True)
    an = O.conv2d(tape, xn, wd[0], bd[0], act=L.ACT_RELU, res=rn)
    bn = O.conv2d(tape, an, wd[1], bd[1], act=L.ACT_RELU)
    cn = O.conv2d(tape, bn, wd[2], bd[2])
    yn = O.conv2d(tape, xn, wd[3], bd[3], res=cn)
    y = O.to_nchw(yn)
    ma = (O.to_nchw(an) > 0).cpu()
    mb = (O.to_nchw(bn) > 0).cpu()
    yn.set_grad(O.nchw_grad_to_nhwc(gy.to(D)))
    tape.backward()
    torch.cuda.synchronize()
    xr, rr = x.double().requires_grad_(), r.double().requires_grad_()
    wr = [w.double().requires_grad_() for w in ws]
    br = [b.double().requires_grad_() for b in bs]
    a = (F.conv2d(xr, wr[0], br[0]) + rr) * ma
    b_ = F.conv2d(a, wr[1], br[1]) * mb
    yr = F.conv2d(b_, wr[2], br[2]) + F.conv2d(xr, wr[3], br[3])
    yr.backward(gy.double())
    assert rel_err(y.cpu().double(), yr) < TOL
    assert rel_err(O.to_nchw_grad(xn).cpu().double(), xr.grad) < TOL
    assert rel_err(O.to_nchw_grad(rn).cpu().double(), rr.grad) < TOL
    for i in range(4):
        assert rel_err(wd[i].grad.cpu().double(), wr[i].grad) < TOL, i
        assert rel_err(bd[i].grad.cpu().double(), br[i].grad) < TOL, i


@pytest.mark.parametrize("case", [(2, 192, 128, 4, 4), (2, 128, 128, 8, 8), (2, 128, 3, 16, 16),
                                  (2, 128, 192, 4, 4), (2, 64, 64, 32, 32)])  # last: halo wgrad, Q stride 2
def test_deconv2d_fwd_bwd(case, fp32_gemm):
    from hyres_hip import ops as O
    B, Ci, Co, H, W = case
    if case == (2, 64, 64, 32, 32):
        _assert_wgrad_kernel(r"wgrad_halo_(bf6_)?kernel<1, 5, 2, 1(, 1)?>", "hyres_wgrad_desc_deconv2d", B, H, W, Ci, Ci,
                             Co, Co, 5, 2)
    x = _rand((B, Ci, H, W), 5)
    w = _rand((Ci, Co, 5, 5), 6, 1.0 / (Ci * 25 / 4) ** 0.5)
    b = _rand((Co,), 7, 0.1)
    xr, wr, br = x.clone().requires_grad_(), w.clone().requires_grad_(), b.clone().requires_grad_()
    yr = F.conv_transpose2d(xr, wr, br, stride=2, padding=2, output_padding=1)
    gy = _rand(yr.shape, 8)
    yr.backward(gy)
    D = dev()
    wd = torch.nn.Parameter(w.to(D))
    bd = torch.nn.Parameter(b.to(D))
    tape = O.Tape()
    xn = O.to_nhwc(x.to(D), rg=True)
    yn = O.deconv2d(tape, xn, wd, bd)
    y = O.to_nchw(yn)
    yn.set_grad(O.nchw_grad_to_nhwc(gy.to(D)))
    tape.backward()
    torch.cuda.synchronize()
    assert rel_err(y.cpu(), yr) < TOL
    assert rel_err(O.to_nchw_grad(xn).cpu(), xr.grad) < TOL
    assert rel_err(wd.grad.cpu(), wr.grad) < TOL
    assert rel_err(bd.grad.cpu(), br.grad) < TOL


@pytest.mark.parametrize("inverse", [False, True])
def test_gdn_fwd_bwd(inverse, fp32_gemm):
    from oracle.compressai_restated import GDN as RefGDN
    from hyres_hip.layers import GDN
    from hyres_hip import ops as O
    C = 128
    ref = RefGDN(C, inverse=inverse)
    with torch.no_grad():
        ref.beta.copy_(torch.sqrt(1 + torch.rand(C) * 0.5))
        ref.gamma.copy_(torch.sqrt(0.1 * torch.eye(C) + torch.rand(C, C) * 0.02))
    x = _rand((2, C, 8, 8), 9)
    xr = x.clone().requires_grad_()
    yr = ref(xr)
    gy = _rand(yr.shape, 10)
    yr.backward(gy)
    D = dev()
    m = GDN(C, inverse=inverse).to(D)
    m.load_state_dict(ref.state_dict())
    tape = O.Tape()
    xn = O.to_nhwc(x.to(D), rg=True)
    yn = m.hip(tape, xn)
    y = O.to_nchw(yn)
    yn.set_grad(O.nchw_grad_to_nhwc(gy.to(D)))
    tape.backward()
    torch.cuda.synchronize()
    assert rel_err(y.cpu(), yr) < TOL
    assert rel_err(O.to_nchw_grad(xn).cpu(), xr.grad) < TOL
    assert rel_err(m.beta.grad.cpu(), ref.beta.grad) < TOL
    assert rel_err(m.gamma.grad.cpu(), ref.gamma.grad) < TOL


def test_bilinear_se_spatial_attention():
    from hyres_hip import ops as O
    from hyres_hip import refine_ops as R
    D = dev()
    B, C, H, W = 2, 64, 16, 16
    x = _rand((B, C, H, W), 11)
    for (Ho, Wo, scale, sf) in [(8, 8, 2.0, 0.5), (4, 4, 4.0, 0.25)]:
        xr = x.clone().requires_grad_()
        yr = F.interpolate(xr, scale_factor=sf, mode="bilinear", align_corners=False)
        up = F.interpolate(yr, size=(H, W), mode="bilinear", align_corners=False)
        gy = _rand(up.shape, 12)
        up.backward(gy)
        tape = O.Tape()
        xn = O.to_nhwc(x.to(D), rg=True)
        dn = R.bilinear(tape, xn, Ho, Wo, scale, scale)
        un = R.bilinear(tape, dn, H, W, Ho / H, Wo / W)
        un.set_grad(O.nchw_grad_to_nhwc(gy.to(D)))
        tape.backward()
        assert rel_err(O.to_nchw(un).cpu(), up) < TOL
        assert rel_err(O.to_nchw_grad(xn).cpu(), xr.grad) < TOL
    # SE block
    w1 = _rand((4, C), 13, 0.125)
    w2 = _rand((C, 4), 14, 0.5)
    xr = x.clone().requires_grad_()
    w1r, w2r = w1.clone().requires_grad_(), w2.clone().requires_grad_()
    s = torch.sigmoid(F.linear(F.relu(F.linear(xr.mean((2, 3)), w1r)), w2r))
    yr = xr * s[:, :, None, None]
    gy = _rand(yr.shape, 15)
    yr.backward(gy)
    w1d, w2d = torch.nn.Parameter(w1.to(D)), torch.nn.Parameter(w2.to(D))
    tape = O.Tape()
    xn = O.to_nhwc(x.to(D), rg=True)
    yn = R.se_block(tape, xn, w1d, w2d)
    yn.set_grad(O.nchw_grad_to_nhwc(gy.to(D)))
    tape.backward()
    assert rel_err(O.to_nchw(yn).cpu(), yr) < TOL
    assert rel_err(O.to_nchw_grad(xn).cpu(), xr.grad) < TOL
    assert rel_err(w1d.grad.cpu(), w1r.grad) < TOL
    assert rel_err(w2d.grad.cpu(), w2r.grad) < TOL
    # spatial attention (192 channels, 7x7)
    C2 = 192
    x2 = _rand((B, C2, H, W), 16)
    wsa = _rand((1, 2, 7, 7), 17, 0.3)
    xr = x2.clone().requires_grad_()
    wr = wsa.clone().requires_grad_()
    a = torch.sigmoid(F.conv2d(torch.cat([xr.mean(1, keepdim=True), xr.max(1, keepdim=True)[0]], 1), wr,
                               None, padding=3))
    yr = xr * a
    gy = _rand(yr.shape, 18)
    yr.backward(gy)
    wd = torch.nn.Parameter(wsa.to(D))
    tape = O.Tape()
    xn = O.to_nhwc(x2.to(D), rg=True)
    yn = R.spatial_attention_mul(tape, xn, wd)
    yn.set_grad(O.nchw_grad_to_nhwc(gy.to(D)))
    tape.backward()
    assert rel_err(O.to_nchw(yn).cpu(), yr) < TOL
    assert rel_err(O.to_nchw_grad(xn).cpu(), xr.grad) < TOL
    assert rel_err(wd.grad.cpu(), wr.grad) < TOL


def test_checkerboard_masked_conv(fp32_gemm):
    """CheckboardMaskedConv2d: weight masked in place, forward/dgrad on the 12 live taps, dense dW."""
    from hyres_hip import ops as O
    from models.layers.checkerboard import CheckboardMaskedConv2d
    D = dev()
    torch.manual_seed(5)
    m = CheckboardMaskedConv2d(192, 384, kernel_size=5, padding=2, stride=1)
    w0 = m.weight.detach().clone()
    x = _rand((2, 192, 8, 8), 31)
    gy = _rand((2, 384, 8, 8), 32)
    wr = w0.clone().requires_grad_(True)
    br = m.bias.detach().clone().requires_grad_(True)
    xr = x.clone().requires_grad_(True)
    with torch.no_grad():
        wr.mul_(m.mask)  # reference: weight.data *= mask, then a dense conv
    yr = F.conv2d(xr, wr, br, padding=2)
    yr.backward(gy)
    m = m.to(D)
    tape = O.Tape()
    xn = O.to_nhwc(x.to(D), rg=True)
    yn = m.hip(tape, xn)
    yn.set_grad(O.nchw_grad_to_nhwc(gy.to(D)))
    tape.backward()
    torch.cuda.synchronize()
    assert torch.equal(m.weight.detach().cpu(), (w0 * m.mask.cpu()))  # in-place mask applied
    assert rel_err(O.to_nchw(yn).cpu(), yr) < TOL
    assert rel_err(O.to_nchw_grad(xn).cpu(), xr.grad) < TOL
    assert rel_err(m.weight.grad.cpu(), wr.grad) < TOL  # dense over all 25 taps
    assert float(wr.grad[:, :, 0, 0].abs().max()) > 0  # (a masked tap still gets a gradient)
    assert rel_err(m.bias.grad.cpu(), br.grad) < TOL


@pytest.mark.parametrize("fold", [True, False])
def test_refine_fusion_head_sa_fold_fwd_bwd(fp32_gemm, fold):
    """MultiScaleRefine's head in training (enhancement.py:105-109): fusion[2](PReLU(fusion[0](multi *
    SpatialAttention(multi)))) forward and backward vs fp64 torch — with the attention multiply folded into the fusion
    1x1 (refine_ops.sa_fold_fusion: ROWSCALE forward, hyres_sa_fold_bwd, hyres_spatial_attn_bwd_map, the SA_BWD
    input-gradient epilogue) and unfused (spatial_attention_mul + Sequential). Output, d multi, and every parameter
    gradient (both 1x1 / 3x3 weights and biases, the PReLU slope, the 7x7 attention weight) at 1e-4 max-norm; the slope
    at 1e-3 (one cancelled sum). 2 x 192 x 40 x 48: a partial last tile of pixels, both PReLU branches populated."""
    import models.layers.enhancement as EH
    from hyres_hip import ops as O
    D = dev()
    B, C, H, W = 2, 192, 40, 48
    torch.manual_seed(11)
    m = EH.MultiScaleRefine(3, 64)
    multi = _rand((B, C, H, W), 41, 1.0)
    gy = _rand((B, 3, H, W), 42)
    sd = {k: v.detach().double().clone().requires_grad_(True) for k, v in m.state_dict().items()
          if k.startswith(("fusion", "spatial_att"))}
    sd["fusion.0.bias"].data.add_(0.05)  # the bias shifts pre-activations across 0: both PReLU sides
    xr = multi.double().requires_grad_(True)
    a = torch.sigmoid(F.conv2d(torch.cat([xr.mean(1, keepdim=True), xr.max(1, keepdim=True)[0]], 1),
                               sd["spatial_att.conv.weight"], None, padding=3))
    h = F.prelu(F.conv2d(xr * a, sd["fusion.0.weight"], sd["fusion.0.bias"]), sd["fusion.1.weight"])
    yr = F.conv2d(h, sd["fusion.2.weight"], sd["fusion.2.bias"], padding=1)
    yr.backward(gy.double())
    m = m.to(D)
    with torch.no_grad():
        for k, v in m.named_parameters():
            if k in sd:
                v.copy_(sd[k].detach().float())
    for p in m.parameters():
        p.grad = None
    tape = O.Tape()
    xn = O.to_nhwc(multi.to(D), rg=True)
    hn = R_sa_fold(tape, xn, m) if fold else _unfused_head(tape, xn, m)
    yn = m.fusion[2].hip(tape, hn)
    yn.set_grad(O.nchw_grad_to_nhwc(gy.to(D)))
    tape.backward()
    torch.cuda.synchronize()
    neg = float((F.conv2d(xr * a, sd["fusion.0.weight"], sd["fusion.0.bias"]) < 0).double().mean())
    assert 0.05 < neg < 0.95, neg
    errs = {"y": rel_err(O.to_nchw(yn).cpu(), yr), "dmulti": rel_err(O.to_nchw_grad(xn).cpu(), xr.grad)}
    for k, p in m.named_parameters():
        if k in sd:
            errs[k] = rel_err(p.grad.cpu(), sd[k].grad)
    print("fold" if fold else "unfused", {k: f"{v:.1e}" for k, v in errs.items()})
    bad = {k: v for k, v in errs.items() if v > (1e-3 if k == "fusion.1.weight" else TOL)}
    assert not bad, errs


def R_sa_fold(tape, xn, m):
    from hyres_hip import refine_ops as R
    return R.sa_fold_fusion(tape, xn, m.spatial_att.conv.weight, m.fusion[0].weight, m.fusion[0].bias,
                            m.fusion[1].weight)


def _unfused_head(tape, xn, m):
    from hyres_hip import _lib as L
    mm = m.spatial_att.hip_mul(tape, xn)
    return m.fusion[0].hip(tape, mm, act=L.ACT_PRELU, slope=m.fusion[1].weight)


@pytest.mark.parametrize("branch", ["scale1", "scale2", "scale3"])
def test_refine_branch_fwd_bwd(branch):
    """One MultiScaleRefine branch (bilinear down -> conv+PReLU -> dilated conv+PReLU -> bilinear up) vs fp64."""
    from hyres_hip import ops as O
    from hyres_hip import refine_ops as R
    from hyres_hip.layers import Sequential, PReLU
    from models.layers.enhancement import dilated_conv
    D = dev()
    B, C, H, W = 2, 64, 64, 64
    f = {"scale1": 1, "scale2": 2, "scale3": 4}[branch]
    torch.manual_seed(3)
    blk = Sequential(dilated_conv(C, C, 1), PReLU(), dilated_conv(C, C, 2), PReLU())
    x = _rand((B, C, H, W), 21)
    gy = _rand((B, C, H, W), 22)
    # fp64 torch reference
    ref = {k: v.detach().double().clone().requires_grad_(True) for k, v in blk.state_dict().items()}
    xr = x.double().requires_grad_(True)
    t = xr if f == 1 else F.interpolate(xr, scale_factor=1.0 / f, mode="bilinear", align_corners=False)
    t = F.prelu(F.conv2d(t, ref["0.weight"], ref["0.bias"], padding=1), ref["1.weight"])
    t = F.prelu(F.conv2d(t, ref["2.weight"], ref["2.bias"], padding=2, dilation=2), ref["3.weight"])
    yr = t if f == 1 else F.interpolate(t, size=(H, W), mode="bilinear", align_corners=False)
    yr.backward(gy.double())
    blk = blk.to(D)
    for p in blk.parameters():
        p.grad = None
    tape = O.Tape()
    xn = O.to_nhwc(x.to(D), rg=True)
    t = xn if f == 1 else R.bilinear(tape, xn, H // f, W // f, float(f), float(f))
    t = blk.hip(tape, t)
    yn = t if f == 1 else R.bilinear(tape, t, H, W, (H // f) / H, (W // f) / W)
    yn.set_grad(O.nchw_grad_to_nhwc(gy.to(D)))
    tape.backward()
    torch.cuda.synchronize()
    errs = {"y": rel_err(O.to_nchw(yn).cpu(), yr), "dx": rel_err(O.to_nchw_grad(xn).cpu(), xr.grad)}
    for k, p in blk.named_parameters():
        errs[k] = rel_err(p.grad.cpu(), ref[k].grad)
    bad = {k: v for k, v in errs.items() if v > (1e-3 if k in ("1.weight", "3.weight") else TOL)}
    assert not bad, errs


@pytest.mark.parametrize("amp", [False, True])
def test_multiscale_refine_prelu_folds_match_unfused(amp, monkeypatch):
    """The whole MultiScaleRefine (enhancement.py:84-110) in training with every PReLU-backward fold on — round 6's
    last one included: scale 1's PReLU applied by the SA_BWD streaming input-gradient that writes multi[..., 0:64]
    (conv1x1_stream_b6_kernel / conv1x1_stream_hf_kernel <6, 4, 40>) — against HYRES_FOLD_PRELU=0 on the same inputs:
    d x and every weight / bias gradient bit for bit in fp32 (2e-3 under AMP, fp16 activations and gradients), the
    PReLU slopes (the same products summed in other orders) at 1e-5 (AMP 2e-3). The scale-1 fold must fire."""
    import models.layers.enhancement as EH
    from hyres_hip import ops as O
    D = dev()
    B, C, H, W = 4, 3, 128, 128
    torch.manual_seed(5)
    m = EH.MultiScaleRefine(C, 64).to(D)
    with torch.no_grad():
        for mod in m.modules():
            if isinstance(mod, torch.nn.Conv2d) and mod.bias is not None:
                mod.bias.add_(0.02)
    x = _rand((B, C, H, W), 91)
    gy = _rand((B, C, H, W), 92)
    names = []
    orig = O.conv_variant

    def spy(g, e, sk):
        r = orig(g, e, sk)
        names.append(r)
        return r

    monkeypatch.setattr(O, "conv_variant", spy)

    def run(fold):
        monkeypatch.setattr(O, "FOLD_PRELU", fold)
        for p in m.parameters():
            p.grad = None
        names.clear()
        tape = O.Tape()
        xn = O.to_nhwc(x.to(D), rg=True)
        with contextlib.ExitStack() as st:
            if amp:
                st.enter_context(torch.autocast("cuda", dtype=torch.float16))
                st.enter_context(O.f16_region())
            yn = m.hip(tape, xn)
        yn.set_grad(O.nchw_grad_to_nhwc(gy.to(D)))
        tape.backward()
        torch.cuda.synchronize()
        return (O.to_nchw_grad(xn).float().cpu(), {k: p.grad.cpu().clone() for k, p in m.named_parameters()},
                any(", 40" in n for n in names))

    dx0, g0, f0 = run(False)
    dx1, g1, f1 = run(True)
    assert f1 and not f0, (f0, f1)
    slopes = [k for k, p in m.named_parameters() if p.numel() == 1]
    assert len(slopes) >= 5, slopes
    for k in g0:
        if k in slopes:
            assert rel_err(g1[k], g0[k]) < (2e-3 if amp else 1e-5), k
        elif amp:
            assert rel_err(g1[k], g0[k]) < 2e-3, k
        else:
            assert torch.equal(g1[k], g0[k]), k
    assert torch.equal(dx1, dx0) if not amp else rel_err(dx1, dx0) < 2e-3


@pytest.mark.parametrize("amp", [False, True])
def test_bilinear_up_prelu_fold_matches_unfused(amp, monkeypatch):
    """MultiScaleRefine's scales 2 / 3 (enhancement.py:89-103): conv + PReLU, then the bilinear up-sample. Round 6
    folds the PReLU backward into the up-sample's backward (hyres_bilinear_bwd_prelu, refine_ops.bilinear) — against
    the unfused prelu_bwd pass (HYRES_FOLD_PRELU=0) on the same inputs: d x and the conv's weight / bias gradients bit
    for bit in fp32 (within fp16 rounding, 2e-3, under AMP with fp16 activations and gradients: the folded and the
    separate kernel may contract slope * g into the fp16 store differently); the slope's gradient (the same products
    summed in another order) at 1e-5 (AMP 1e-3). Both PReLU sides are populated and the fold must fire."""
    from hyres_hip import _lib as L
    from hyres_hip import ops as O
    from hyres_hip import refine_ops as R
    from hyres_hip.layers import Conv2d, PReLU, Sequential
    D = dev()
    B, C, H, W = 2, 64, 48, 40
    torch.manual_seed(9)
    blk = Sequential(Conv2d(C, C, 3, padding=1), PReLU()).to(D)
    with torch.no_grad():
        blk[0].bias.add_(0.02)
    x = _rand((B, C, H, W), 61)
    gy = _rand((B, C, 2 * H, 2 * W), 62)
    calls = []
    orig = L.call

    def spy(fn, *a):
        calls.append(fn)
        return orig(fn, *a)

    def run(fold):
        monkeypatch.setattr(O, "FOLD_PRELU", fold)
        for p in blk.parameters():
            p.grad = None
        calls.clear()
        tape = O.Tape()
        xn = O.to_nhwc(x.to(D), rg=True)
        ctx = (torch.autocast("cuda", dtype=torch.float16), O.f16_region()) if amp else ()
        with contextlib.ExitStack() as st:
            for c in ctx:
                st.enter_context(c)
            h = blk.hip(tape, xn)
            assert h.half == amp
            yn = R.bilinear(tape, h, 2 * H, 2 * W, 0.5, 0.5)
        yn.set_grad(O.nchw_grad_to_nhwc(gy.to(D)))
        monkeypatch.setattr(L, "call", spy)
        tape.backward()
        monkeypatch.setattr(L, "call", orig)
        torch.cuda.synchronize()
        return (O.to_nchw_grad(xn).float().cpu(), {k: p.grad.cpu().clone() for k, p in blk.named_parameters()},
                "hyres_bilinear_bwd_prelu" in calls)

    dx0, g0, f0 = run(False)
    dx1, g1, f1 = run(True)
    assert f1 and not f0
    for k in g0:
        if k.endswith("1.weight"):  # the PReLU slope
            assert rel_err(g1[k], g0[k]) < (1e-3 if amp else 1e-5), k
        elif amp:
            assert rel_err(g1[k], g0[k]) < 2e-3, k
        else:
            assert torch.equal(g1[k], g0[k]), k
    assert torch.equal(dx1, dx0) if not amp else rel_err(dx1, dx0) < 2e-3


@pytest.mark.parametrize("shape", [(2, 256, 128), (4, 128, 128)])
def test_refine_block_prelu_fold_matches_unfused(shape, monkeypatch):
    """A MultiScaleRefine scale block in training (enhancement.py:89-95) with its first PReLU's backward folded into the
    dilation-2 conv's input-gradient (HYRES_ACT_PRELU_MASK on conv3x3_wres_bf6_kernel, ops.Node.prelu_mask_epilogue)
    against the unfused prelu_bwd pass (HYRES_FOLD_PRELU=0) on the same inputs: d x, both conv weight / bias
    gradients and the second PReLU's slope gradient bit for bit; the folded slope's gradient (the same products
    summed in another order) at 1e-5. Sizes at the weight-resident kernel's tile floor (>= 2 tiles per block); the
    fold must fire, and both PReLU sides are populated."""
    from hyres_hip import _lib as L
    from hyres_hip import ops as O
    from hyres_hip.layers import Sequential, PReLU
    from models.layers.enhancement import dilated_conv
    D = dev()
    B, H, W = shape
    C = 64
    torch.manual_seed(7)
    blk = Sequential(dilated_conv(C, C, 1), PReLU(), dilated_conv(C, C, 2), PReLU()).to(D)
    with torch.no_grad():
        blk[0].bias.add_(0.02)
    x = _rand((B, C, H, W), 51)
    gy = _rand((B, C, H, W), 52)
    fired = []
    orig = O.Node.prelu_mask_epilogue

    def spy(self, e, acc, g):
        orig(self, e, acc, g)
        fired.append(self.pmasked)

    monkeypatch.setattr(O.Node, "prelu_mask_epilogue", spy)
    old = ctypes.c_int(0)
    L.call("hyres_conv_tuning", 7, 1, ctypes.byref(old))  # the bf16x6 GEMM (the default)

    def run(fold):
        monkeypatch.setattr(O, "FOLD_PRELU", fold)
        for p in blk.parameters():
            p.grad = None
        fired.clear()
        tape = O.Tape()
        xn = O.to_nhwc(x.to(D), rg=True)
        yn = blk.hip(tape, xn)
        yn.set_grad(O.nchw_grad_to_nhwc(gy.to(D)))
        tape.backward()
        torch.cuda.synchronize()
        return (O.to_nchw_grad(xn).cpu(), {k: p.grad.cpu().clone() for k, p in blk.named_parameters()},
                any(fired))

    try:
        dx0, g0, f0 = run(False)
        dx1, g1, f1 = run(True)
    finally:
        L.call("hyres_conv_tuning", 7, old.value, None)
    assert f1 and not f0, (f0, f1)
    pre = F.conv2d(x.to(D), blk[0].weight, blk[0].bias, padding=1)
    neg = float((pre < 0).float().mean())
    assert 0.05 < neg < 0.95, neg
    assert torch.equal(dx0, dx1), float((dx0 - dx1).abs().max())
    for k in g0:
        if k == "1.weight":
            assert rel_err(g1[k], g0[k]) < 1e-5, (k, g0[k], g1[k])
        else:
            assert torch.equal(g0[k], g1[k]), (k, float((g0[k] - g1[k]).abs().max()))


def test_refine_input_se_prelu_fold_matches_unfused(monkeypatch):
    """MultiScaleRefine's input stage in training, SE(PReLU(conv_in(x))) (enhancement.py:107-110), with act_in's
    backward folded into the SE block's input-gradient (hyres_se_bwd_prelu) against the unfused prelu_bwd pass
    (HYRES_FOLD_PRELU=0): d x, conv_in's weight / bias and both SE weights bit for bit; act_in's slope gradient (same
    products, another summation order) at 1e-5; the fold fires; both PReLU sides populated. Against fp64 torch too."""
    import models.layers.enhancement as EH
    from hyres_hip import _lib as L
    from hyres_hip import ops as O
    from hyres_hip import refine_ops as R
    D = dev()
    B, H, W = 2, 64, 96
    torch.manual_seed(9)
    m = EH.MultiScaleRefine(3, 64).to(D)
    x = _rand((B, 3, H, W), 61)
    gy = _rand((B, 64, H, W), 62)
    calls = []
    orig_call = L.call

    def spy(name, *args):
        calls.append(name)
        return orig_call(name, *args)

    monkeypatch.setattr(L, "call", spy)

    def run(fold):
        monkeypatch.setattr(O, "FOLD_PRELU", fold)
        for p in m.parameters():
            p.grad = None
        calls.clear()
        tape = O.Tape()
        xn = O.to_nhwc(x.to(D), rg=True)
        feat = m.conv_in.hip(tape, xn, act=L.ACT_PRELU, slope=m.act_in.weight)
        yn = m.se_block.hip(tape, feat)
        yn.set_grad(O.nchw_grad_to_nhwc(gy.to(D)))
        tape.backward()
        torch.cuda.synchronize()
        names = ("conv_in.weight", "conv_in.bias", "act_in.weight", "se_block.fc.0.weight", "se_block.fc.2.weight")
        grads = {k: p.grad.cpu().clone() for k, p in m.named_parameters() if k in names}
        return O.to_nchw_grad(xn).cpu(), grads, O.to_nchw(yn).cpu(), list(calls)

    dx0, g0, y0, c0 = run(False)
    dx1, g1, y1, c1 = run(True)
    assert "hyres_se_bwd_prelu" in c1 and "hyres_prelu_bwd" not in c1, c1
    assert "hyres_prelu_bwd" in c0 and "hyres_se_bwd_prelu" not in c0, c0
    assert torch.equal(y0, y1) and torch.equal(dx0, dx1), float((dx0 - dx1).abs().max())
    for k in g0:
        if k == "act_in.weight":
            assert rel_err(g1[k], g0[k]) < 1e-5, (g0[k], g1[k])
        else:
            assert torch.equal(g0[k], g1[k]), (k, float((g0[k] - g1[k]).abs().max()))
    # fp64 torch reference of the same stage
    sd = {k: v.detach().cpu().double().clone().requires_grad_(True) for k, v in m.state_dict().items()
          if k.startswith(("conv_in", "act_in", "se_block"))}
    xr = x.double().requires_grad_(True)
    pre = F.conv2d(xr, sd["conv_in.weight"], sd["conv_in.bias"], padding=1)
    neg = float((pre < 0).double().mean())
    assert 0.05 < neg < 0.95, neg
    f = F.prelu(pre, sd["act_in.weight"])
    s = torch.sigmoid(F.linear(F.relu(F.linear(f.mean((2, 3)), sd["se_block.fc.0.weight"])),
                               sd["se_block.fc.2.weight"]))
    (f * s[:, :, None, None]).backward(gy.double())
    assert rel_err(dx1, xr.grad) < TOL
    for k in g1:
        assert rel_err(g1[k], sd[k].grad) < (1e-3 if k == "act_in.weight" else TOL), k


def test_attn_gate_float4_and_relu_fold():
    """AttentionBlock's gate (models/layers/attention.py:44-47) on the round-6 float4 kernels: forward a * sigmoid(b) + x
    and backward vs fp64 torch (1e-6), and the backward with the last ResidualUnit's ReLU folded in
    (hyres_attn_gate_bwd_relu) equal bit for bit to the gate backward followed by the ReLU backward."""
    from hyres_hip import _lib as L
    D = dev()
    P, C = 16 * 32 * 32, 192
    a = torch.relu(_rand((P, C), 81)).to(D)
    b = _rand((P, C), 82, 3.0).to(D)
    x = _rand((P, C), 83).to(D)
    g = _rand((P, C), 84).to(D)
    out = torch.empty_like(a)
    L.call("hyres_attn_gate_fwd", a.data_ptr(), b.data_ptr(), x.data_ptr(), out.data_ptr(), P * C, 0, L.stream())
    ga, gb, gam, gbm, gar = (torch.empty_like(a) for _ in range(5))
    L.call("hyres_attn_gate_bwd", a.data_ptr(), b.data_ptr(), g.data_ptr(), ga.data_ptr(), gb.data_ptr(), P * C, 0,
           L.stream())
    L.call("hyres_relu_bwd_2d", a.data_ptr(), C, ga.data_ptr(), C, gar.data_ptr(), C, P, C, 0, L.stream())
    L.call("hyres_attn_gate_bwd_relu", a.data_ptr(), b.data_ptr(), g.data_ptr(), gam.data_ptr(), gbm.data_ptr(), P * C,
           0, L.stream())
    torch.cuda.synchronize()
    s = torch.sigmoid(b.double())
    assert rel_err(out.double().cpu(), (a.double() * s + x.double()).cpu()) < 1e-6
    assert rel_err(ga.double().cpu(), (g.double() * s).cpu()) < 1e-6
    assert rel_err(gb.double().cpu(), (g.double() * a.double() * s * (1 - s)).cpu()) < 1e-6
    assert torch.equal(gam, gar) and torch.equal(gbm, gb)
    assert float((gam[a == 0]).abs().max()) == 0.0 and bool((a == 0).any())


@pytest.mark.parametrize("g16", [0, 1])
def test_attn_gate_f16_vector_and_relu_fold(g16):
    """The AMP gate backward (fp16 a, b; fp16 or fp32 gradients) on the round-6 vector kernel equals the scalar kernel
    (the one a ragged n runs on) bit for bit with fp32 gradients and within 1 fp16 ulp with fp16 ones, and the ReLU-folded variant (hyres_attn_gate_bwd_relu) equals
    the gate backward followed by hyres_relu_bwd_2d, both with the same dtype mask, bit for bit."""
    from hyres_hip import _lib as L
    D = dev()
    P, C = 8 * 32 * 32, 192
    n = P * C
    gdt = torch.float16 if g16 else torch.float32
    a = torch.relu(_rand((P, C), 91)).to(D).half()
    b = _rand((P, C), 92, 3.0).to(D).half()
    g = _rand((P, C), 93).to(D).to(gdt)
    ga, gb, gam, gbm, gar = (torch.empty(P, C, device=D, dtype=gdt) for _ in range(5))
    gas, gbs = (torch.zeros(P, C, device=D, dtype=gdt) for _ in range(2))
    dt = L.DT_ACT16 | (L.DT_GRAD16 if g16 else 0)
    L.call("hyres_attn_gate_bwd", a.data_ptr(), b.data_ptr(), g.data_ptr(), ga.data_ptr(), gb.data_ptr(), n, dt,
           L.stream())
    # n - 1: not a multiple of 4, the scalar kernel; the last element is compared separately below
    L.call("hyres_attn_gate_bwd", a.data_ptr(), b.data_ptr(), g.data_ptr(), gas.data_ptr(), gbs.data_ptr(), n - 1,
           dt, L.stream())
    L.call("hyres_relu_bwd_2d", a.data_ptr(), C, ga.data_ptr(), C, gar.data_ptr(), C, P, C, dt, L.stream())
    L.call("hyres_attn_gate_bwd_relu", a.data_ptr(), b.data_ptr(), g.data_ptr(), gam.data_ptr(), gbm.data_ptr(), n,
           dt, L.stream())
    torch.cuda.synchronize()
    if g16:
        # the scalar kernel's fp16 stores compile to v_fma_mixlo_f16 (product rounded once, straight to fp16: the
        # contraction -ffp-contract=fast allows); the vector kernel rounds the fp32 product, then packs to fp16 (the
        # source's literal semantics) — at most 1 fp16 ulp apart (zeros' signs aside), on a small fraction of the elements
        for u, v in ((ga, gas), (gb, gbs)):
            u, v = u.view(-1)[:-1] + 0, v.view(-1)[:-1] + 0  # -0 -> +0 (gb = g * a * ... at a == 0 keeps g's sign)
            du = (u.view(torch.int16).int() - v.view(torch.int16).int()).abs()
            assert int(du.max()) <= 1 and float((du > 0).float().mean()) < 0.05
    else:
        assert torch.equal(ga.view(-1)[:-1], gas.view(-1)[:-1]) and torch.equal(gb.view(-1)[:-1], gbs.view(-1)[:-1])
    s = torch.sigmoid(b.double())
    tol = 2e-3 if g16 else 1e-6
    assert rel_err(ga.double().cpu(), (g.double() * s).cpu()) < tol
    assert rel_err(gb.double().cpu(), (g.double() * a.double() * s * (1 - s)).cpu()) < tol
    assert torch.equal(gam, gar) and torch.equal(gbm, gb)
    assert bool((a == 0).any()) and float(gam[a == 0].abs().max()) == 0.0


def test_prelu_mask_epilogue_refused_off_the_weight_resident_kernel():
    """HYRES_ACT_PRELU_MASK is implemented by conv3x3_wres_bf6_kernel only: a 1x1 input-gradient asking for it gets
    HYRES_E_ARG, nothing launched (the caller, ops.Node.prelu_mask_epilogue, checks the route first)."""
    from hyres_hip import _lib as L
    from hyres_hip import ops as O
    D = dev()
    P, C = 4096, 64
    x = torch.randn(P, C, device=D)
    w = torch.randn(C, C, device=D)
    y = torch.zeros(P, C, device=D)
    pre = torch.randn(P, C, device=D)
    slope = torch.full((1,), 0.25, device=D)
    ds = torch.zeros(1, device=D)
    part = torch.zeros(L.PRELU_PARTIALS, device=D)
    g = O._geom("hyres_geom_conv2d", 1, 64, 64, C, C, C, C, 1, 1, 1, 0, 1)
    e = L.Epilogue()
    e.kind = L.EPI_BIAS
    e.act = L.ACT_PRELU_MASK
    e.aux0, e.ld0 = pre.data_ptr(), C
    e.slope, e.aux1 = slope.data_ptr(), ds.data_ptr()
    e.aux2, e.ld2 = part.data_ptr(), L.PRELU_PARTIALS
    assert not O.conv_variant(g, e, False).startswith("conv3x3_wres_bf6_kernel")
    with pytest.raises(L.HipError, match="conv3x3_wres_bf6_kernel only"):
        L.call("hyres_conv_forward", ctypes.byref(g), x.data_ptr(), w.data_ptr(), C, y.data_ptr(), ctypes.byref(e),
               None, 0, L.stream())
    torch.cuda.synchronize()
    assert float(y.abs().max()) == 0.0 and float(ds[0]) == 0.0


# ------------------------------------------------------------------------------------------------ model
def _hip_model():
    from models import ResidualJPEGCompression
    from hyres_hip.weights import synthetic_state_dict
    net = ResidualJPEGCompression(jpeg_quality=50)
    sd = synthetic_state_dict(net.state_dict())
    torch.nn.Module.load_state_dict(net, sd, strict=True)
    return net.to(dev()), sd


@pytest.mark.parametrize("fixture", ["hyres_eval_b2_64.npz", "kodim01_crop64_eval.npz"])
def test_model_eval_matches_reference(fixture):
    g = load_npz(fixture)
    net, sd = _hip_model()
    net.eval()
    D = dev()
    with torch.no_grad():
        out = net(g["x"], jpeg=(g["jpeg_decoded"], float(g["jpeg_bpp"])))
    torch.cuda.synchronize()
    # decision-level: y_hat is round(y - mu) + mu: compare likelihoods / outputs normwise
    assert rel_err(out["likelihoods"]["z"].cpu(), g["z_likelihoods"]) < TOL
    # y likelihoods: 1e-4 (north_star) on every element whose round(y - mu) decision agrees with the reference;
    # a decision flip (y - mu within fp32 noise of k + 1/2) is counted separately and must not occur here
    ly, lr_ = out["likelihoods"]["y"].cpu().double(), g["y_likelihoods"].double()
    flips = (ly - lr_).abs() > 1e-3 * lr_.abs().clamp_min(1e-9)
    assert int(flips.sum()) == 0, int(flips.sum())
    assert rel_err(ly, lr_) < TOL
    assert rel_err(out["residual_hat"].cpu(), g["residual_hat"]) < TOL
    assert rel_err(out["x_hat"].cpu(), g["x_hat"]) < TOL
    # PSNR parity (north_star: within 0.01 dB of the CPU reference)
    mse_h = F.mse_loss(out["x_hat"].cpu(), g["x"]).item()
    mse_r = F.mse_loss(g["x_hat"], g["x"]).item()
    import math
    assert abs(10 * math.log10(1 / mse_h) - 10 * math.log10(1 / mse_r)) < 0.01


def _nhwc_noise(g, keys, D):
    return {k: g[src].permute(0, 2, 3, 1).contiguous().to(D) for k, src in keys.items()}


def _hip_train_step(net, x, jpeg, jb, noisequant, injected, lmbda):
    """One HIP train step (forward, RD loss, backward) recording the branch decisions the oracle must
    follow at the kinks: every fused ReLU / PReLU's pre-activation sign, and the round() results behind
    z_hat / y_anchor_hat / y_hat (STE)."""
    from hyres_hip import ops as O
    from hyres_hip.loss import RateDistortionLoss
    D = dev()
    net.residual_model.noise.injected = injected
    O.Trace.nodes, O.Trace.acts = {}, []
    try:
        out = net(x, noisequant=noisequant, jpeg=(jpeg, jb))
        crit = RateDistortionLoss(lmbda=lmbda, alpha=0)(out, x.to(D))
        crit["loss"].backward()
        torch.cuda.synchronize()
        dec = O.Trace.decisions()
        hats = {k: O.Trace.value(k).cpu() for k in ("z_hat", "y_anchor_hat", "y_hat")}
    finally:
        O.Trace.nodes, O.Trace.acts = None, None
    return out, crit, dec, hats


def _oracle_following(fx, jb, noisequant, noise, lmbda, dec, hats, dtype=torch.float64, tol_act=1e-4,
                      tol_ste=1e-4):
    """Oracle train step (``dtype``) that takes the HIP run's branch at every kink: a ReLU / PReLU input
    with |x| < tol_act*max|x| follows the HIP pre-activation sign, and a round() argument within tol_ste of
    a half-integer follows the HIP rounding.  Anywhere else the decisions must agree (asserted), so the
    comparison stays decision-exact without masking real errors.  Returns (grads, prelu |g*x| sums, loss,
    number of followed decisions)."""
    from oracle import Oracle, rd_loss
    sd = recipe_state_dict()
    sd2, params = {}, []
    for k, v in sd.items():
        t = v.clone().to(dtype) if v.is_floating_point() else v.clone()
        if t.is_floating_point() and not k.endswith(("pedestal", "bound", "mask", "target", "scale_bound",
                                                      "scale_table")):
            t.requires_grad_(True)
            params.append(k)
        sd2[k] = t
    calls = {"relu": 0, "prelu": 0}
    followed = {"relu": 0, "prelu": 0, "ste": 0}
    captured = []

    def branch(kind, x):
        i = calls[kind]
        calls[kind] += 1
        d = dec[kind][i]
        assert tuple(d.shape) == tuple(x.shape), (kind, i, tuple(d.shape), tuple(x.shape))
        own = x.detach() > 0
        near = x.detach().abs() < tol_act * float(x.detach().abs().max())
        bad = (own != d) & ~near
        assert not bool(bad.any()), (kind, i, int(bad.sum()), float(x.detach()[bad].abs().max()))
        followed[kind] += int(((own != d) & near).sum())
        return torch.where(near, d, own)

    class Follow(Oracle):
        @staticmethod
        def relu(x):
            return torch.where(branch("relu", x), x, torch.zeros_like(x))

        @staticmethod
        def prelu(x, a):
            y = torch.where(branch("prelu", x), x, a * x)
            if y.requires_grad:
                y.register_hook(lambda gg, x=x: captured.append((a, x.detach(), gg.detach())))
            return y

        def quant_ste(self, v, m, key):
            t = v - m
            r = torch.round(t.detach())
            if key == "z":
                hat = hats["z_hat"]
            elif key == "y_anchor":
                hat = hats["y_anchor_hat"]
            else:
                hat = hats["y_hat"] - hats["y_anchor_hat"]
            rh = torch.round(hat.to(t.dtype) - m.detach())
            frac = (t.detach() - torch.floor(t.detach()) - 0.5).abs()
            near = frac < tol_ste
            bad = (r != rh) & ~near
            assert not bool(bad.any()), (key, int(bad.sum()))
            followed["ste"] += int(((r != rh) & near).sum())
            r = torch.where(near, rh, r)
            return (r - t.detach() + t) + m

    orc = Follow(sd2)
    out = orc.forward(fx["x"].to(dtype), fx["jpeg_decoded"].to(dtype), 0.0, training=True, noisequant=noisequant,
                      noise={k: v.to(dtype) for k, v in noise.items()})
    assert calls["relu"] == len(dec["relu"]) and calls["prelu"] == len(dec["prelu"]), (calls, len(dec["relu"]))
    out["jpeg_bpp_loss"] = torch.tensor(jb, dtype=dtype)
    crit = rd_loss(out, fx["x"].to(dtype), lmbda)
    crit["loss"].backward()
    grads = {k: sd2[k].grad for k in params if sd2[k].grad is not None}
    by_id = {id(sd2[k]): k for k in params}
    terms = {}
    for a, x, gg in captured:
        k = by_id[id(a)]
        terms[k] = terms.get(k, 0.0) + float((gg * x).abs()[x <= 0].sum())
    return grads, terms, float(crit["loss"].detach()), followed


def _check_grads(net, ref, terms, tol=1e-3, slope_tol=5e-4):
    """Every parameter gradient normwise within ``tol`` of the oracle's; PReLU slopes (cancelled sums of
    g*x over many pixels) within ``slope_tol`` * sum|g*x|.  Returns the sorted (err, name) rows."""
    params = dict(net.named_parameters())
    bad, rows = [], []
    for k, r in ref.items():
        p = params[k]
        gd = p.grad.detach().double().cpu() if p.grad is not None else torch.zeros(p.shape, dtype=torch.float64)
        scale = float(r.abs().max())
        if scale == 0.0:
            continue
        err = float((gd - r.double()).abs().max())
        lim = tol * scale
        if k in terms:
            lim = max(lim, slope_tol * terms[k])
        rows.append((err / scale, k))
        if err > lim:
            bad.append((k, err / scale))
    rows.sort(reverse=True)
    assert not bad, bad[:8]
    return rows


def test_model_train_step_matches_reference(fp32_gemm):
    """C2 semantics: train mode, noisequant=False, lambda=0.045, recorded noise -> loss and aux loss vs the
    reference fixture (1e-4), every parameter gradient vs the fp64 oracle (pinned to the fixture's gradient
    summaries in test_oracle_golden.py) within 1e-3 normwise.  Decision-exact: where a ReLU / PReLU input or
    a round() argument sits within fp32 rounding of its kink, the oracle takes the HIP run's branch (on this
    fixture one input of refine.scale3's second PReLU is 1.4e-8: its branch alone moves
    refine.scale3.2.weight's gradient by 1.9e-3)."""
    g = load_npz("hyres_train_b2_64.npz")
    meta = load_meta()
    net, sd = _hip_model()
    net.train()
    D = dev()
    jb = float(g["loss"]) - (meta["train_lambda"] * float(g["mse_loss"]) + float(g["y_bpp"]) + float(g["z_bpp"]))
    keys = {"z": "noise_z", "y": "noise_y"}
    _, crit, dec, hats = _hip_train_step(net, g["x"], g["jpeg_decoded"], jb, False, _nhwc_noise(g, keys, D),
                                         meta["train_lambda"])
    aux = net.aux_loss()
    assert abs(float(crit["loss"]) - float(g["loss"])) <= TOL * abs(float(g["loss"]))
    assert abs(float(aux) - float(g["aux_loss"])) <= TOL * abs(float(g["aux_loss"]))
    torch.set_num_threads(16)
    ref, terms, _, followed = _oracle_following(g, jb, False, {k: g[v] for k, v in keys.items()},
                                                meta["train_lambda"], dec, hats)
    rows = _check_grads(net, ref, terms)
    print("followed decisions", followed, "worst", rows[:3])


NQ_KEYS = {"z": "noise_z", "y_anchor": "noise_y_anchor", "y_non_anchor": "noise_y_non_anchor", "y": "noise_y"}


def test_model_train_step_noisequant_matches_reference():
    """noisequant=True (the reference's training default for epochs <= 400, src/training.py:238-243): the
    Quantizer "noise" branch (models/utils/quantization.py:6-10) on the anchor / non-anchor halves
    (models/checkerboard.py:121-122,132-133) plus EB/GC noise, all four draws recorded by the reference run
    (tests/golden/make_golden.py train_step_noisequant) and injected here.  Loss, aux loss, x_hat and
    likelihoods within 1e-4 of the reference fixture; every parameter gradient vs the fp64 oracle (pinned to
    the fixture's gradient summaries in test_oracle_golden.py) within 1e-3, decision-exact (on this fixture
    one ReLU input of g_s.2.conv1 is 2e-6 of its layer's max: its branch alone moves g_s.2.conv1.weight's
    gradient by 3.4e-3 and, through y, every g_a gradient by ~1e-3)."""
    import json
    import os
    from conftest import GOLDEN
    g = load_npz("hyres_train_nq_b2_64.npz")
    with open(os.path.join(GOLDEN, "hyres_train_nq_b2_64.json")) as f:
        meta = json.load(f)
    net, _ = _hip_model()
    net.train()
    D = dev()
    jb = float(g["jpeg_bpp"])
    out, crit, dec, hats = _hip_train_step(net, g["x"], g["jpeg_decoded"], jb, True, _nhwc_noise(g, NQ_KEYS, D),
                                           meta["lambda"])
    aux = net.aux_loss()
    for k, r in (("loss", "loss"), ("mse_loss", "mse_loss"), ("y_bpp_loss", "y_bpp"), ("z_bpp_loss", "z_bpp")):
        assert abs(float(crit[k]) - float(g[r])) <= TOL * abs(float(g[r])), k
    assert abs(float(aux) - float(g["aux_loss"])) <= TOL * abs(float(g["aux_loss"]))
    assert rel_err(out["x_hat"].detach().cpu(), g["x_hat"]) < TOL
    assert rel_err(out["residual_hat"].detach().cpu(), g["residual_hat"]) < TOL
    assert rel_err(out["likelihoods"]["y"].detach().cpu(), g["y_likelihoods"]) < TOL
    assert rel_err(out["likelihoods"]["z"].detach().cpu(), g["z_likelihoods"]) < TOL
    # noisequant: the EB quantiles get no main-loss gradient (z_hat = z + U feeds h_s, no medians)
    q = net.residual_model.entropy_bottleneck.quantiles
    assert q.grad is None or float(q.grad.abs().max()) == 0.0
    torch.set_num_threads(16)
    ref, terms, _, followed = _oracle_following(g, jb, True, {k: g[v] for k, v in NQ_KEYS.items()}, meta["lambda"],
                                                dec, hats)
    rows = _check_grads(net, ref, terms)
    print("followed decisions", followed, "worst", rows[:3])


TRACE_KEYS = ["residual", "y", "z", "z_hat", "latent_params", "y_anchor_hat", "ctx_params", "y_hat", "residual_hat",
              "x_hat_initial", "refine_feat", "refine_f2", "refine_f3", "refine_multi", "refine_multi_att", "refined",
              "x_hat"]


def test_train_stagewise_vs_fp64():
    """Stage-wise forward values (1e-4) and activation gradients (1e-2: kink flips, see above) of the
    train step vs the fp64 oracle."""
    from hyres_hip.loss import RateDistortionLoss
    from hyres_hip import ops as O
    from oracle import Oracle, rd_loss
    g = load_npz("hyres_train_b2_64.npz")
    meta = load_meta()
    jb = float(g["loss"]) - (meta["train_lambda"] * float(g["mse_loss"]) + float(g["y_bpp"]) + float(g["z_bpp"]))
    net, sd = _hip_model()
    net.train()
    D = dev()
    net.residual_model.noise.injected = {"z": g["noise_z"].permute(0, 2, 3, 1).contiguous().to(D),
                                         "y": g["noise_y"].permute(0, 2, 3, 1).contiguous().to(D)}
    O.Trace.nodes = {}
    try:
        out = net(g["x"], noisequant=False, jpeg=(g["jpeg_decoded"], jb))
        crit = RateDistortionLoss(lmbda=meta["train_lambda"], alpha=0)(out, g["x"].to(D))
        crit["loss"].backward()
        hv = {k: O.Trace.value(k).cpu() for k in O.Trace.nodes if k in TRACE_KEYS}
        hg = {}
        for k in hv:
            gg = O.Trace.grad(k)
            hg[k] = None if gg is None else gg.cpu()
    finally:
        O.Trace.nodes = None
    sd64 = {k: (v.clone().double() if v.is_floating_point() else v.clone()) for k, v in recipe_state_dict().items()}
    for k, v in sd64.items():
        if v.is_floating_point() and k.endswith(("weight", "bias")):
            v.requires_grad_(True)
    T = {}
    o = Oracle(sd64).forward(g["x"].double(), g["jpeg_decoded"].double(), jb, training=True,
                             noise={"z": g["noise_z"].double(), "y": g["noise_y"].double()}, trace=T)
    rd_loss(o, g["x"].double(), meta["train_lambda"])["loss"].backward()
    rows, bad = [], []
    for k in TRACE_KEYS:
        if k not in hv or k not in T:
            continue
        fe = rel_err(hv[k], T[k].detach())
        ge = None
        # y_anchor_hat's HIP node carries only the context-model gradient (the y_hat path is routed to y
        # directly), so its gradient is not comparable to the oracle's total
        if k != "y_anchor_hat" and hg.get(k) is not None and T[k].grad is not None:
            ge = rel_err(hg[k], T[k].grad)
        rows.append((k, fe, ge))
        if fe > TOL or (ge is not None and ge > 1e-2):
            bad.append((k, fe, ge))
    print("\n".join(f"{k:18s} fwd {fe:.2e} grad {ge if ge is None else f'{ge:.2e}'}" for k, fe, ge in rows))
    assert not bad, bad


def _lik_flip_fraction(a, b, tol=1e-3):
    """Fraction of likelihood elements that disagree beyond ``tol`` relative: a round() boundary flip of
    y - mu (|t - (k + .5)| within fp32 noise) changes that element's likelihood entirely; such flips
    must be rare (<= 1e-5 of the elements)."""
    a = a.double()
    b = b.double()
    bad = (a - b).abs() > tol * b.abs().clamp_min(1e-9)
    return float(bad.double().mean())


def _bpp_per_image(lik_y, lik_z, H, W):
    """Ideal code length per image (src/losses/rd_loss.py:23-26 without the batch mean)."""
    import math
    s = lik_y.double().log().flatten(1).sum(1) + lik_z.double().log().flatten(1).sum(1)
    return s / (-math.log(2) * H * W)


def _psnr(a, b):
    import math
    return 10 * math.log10(1.0 / F.mse_loss(a.double(), b.double()).item())


def _check_against_oracle(out, idx, x, jpeg, jpeg_bpp, y_hat=None):
    """Oracle (reference math, CPU fp32) on images ``idx``: z-likelihoods 1e-4; y-likelihoods and x_hat
    decision-aware; per-image bpp 1e-4 relative; PSNR within 0.01 dB (north_star).

    Decision-aware: a round() of y - mu within fp32 noise of k + .5 may go either way (~1 such latent per 6e5
    elements). ``y_hat`` (the HIP run's, traced) lets the check count those ROOT flips (|dy_hat| = 1, each at a
    near-tie of the oracle's own y - mu) and their cascade: an anchor flip moves the context-model parameters of the
    non-anchors in its 5x5 window (every channel), whose y_hat = round(y - mu) + mu then move continuously (or flip
    once more), and g_s spreads every moved latent over a 64x64-pixel window. So the likelihood mismatches must stay
    within the moved latents' count and the x_hat values beyond 1e-4 within 64 x 64 x 3 per moved latent."""
    orc, _ = oracle_from(recipe_state_dict())
    torch.set_num_threads(16)
    tr = {}
    with torch.no_grad():
        ref = orc.forward(x[idx], jpeg[idx], jpeg_bpp, training=False, trace=tr)
    H, W = x.shape[-2:]
    xh = out["x_hat"].cpu()[idx]
    ly_h, ly_r = out["likelihoods"]["y"].cpu()[idx].double(), ref["likelihoods"]["y"].double()
    nflip = int(((ly_h - ly_r).abs() > 1e-3 * ly_r.abs().clamp_min(1e-9)).sum())
    dx = (xh.double() - ref["x_hat"].double()).abs() / ref["x_hat"].abs().max()
    nbad = int((dx > TOL).sum())
    nroot = nmoved = 0
    if y_hat is not None:
        dy = (y_hat[idx].double() - tr["y_hat"].double()).abs()
        nroot = int((dy > 0.5).sum())
        nmoved = int((dy > 1e-4).sum())
    print(f"vs oracle: {nroot} root round() flips, {nmoved} moved latents, {nflip} y-likelihood mismatches, {nbad} "
          f"x_hat values beyond {TOL} (max {float(dx.max()):.2e}, normwise {rel_err(xh.double(), ref['x_hat'].double()):.2e})")
    cap = max(2, 1e-5 * ly_r.numel())
    assert nroot <= cap, nroot
    assert nflip <= cap + nmoved, (nflip, nmoved)
    assert nbad <= (max(nflip, nmoved)) * 64 * 64 * 3, (nbad, nflip, nmoved)
    assert rel_err(out["likelihoods"]["z"].cpu()[idx], ref["likelihoods"]["z"]) < TOL
    bh = _bpp_per_image(out["likelihoods"]["y"].cpu()[idx], out["likelihoods"]["z"].cpu()[idx], H, W)
    br = _bpp_per_image(ref["likelihoods"]["y"], ref["likelihoods"]["z"], H, W)
    assert float(((bh - br).abs() / br.abs()).max()) < 1e-4 * (1 + nmoved), (bh, br)
    for k in range(len(idx)):
        assert abs(_psnr(xh[k], x[idx][k]) - _psnr(ref["x_hat"][k], x[idx][k])) < 0.01


def test_c3_bs32_eval_gc_path_parity():
    """BASELINE config C3: checkerboard two-pass context + GaussianConditional on the HIP path, bs=32,
    256x256 synthetic (seed 1926, 8-bit exact), eval; bpp/PSNR parity vs the CPU reference math on the
    first and last image, and batch independence (the same images run as a batch of 2)."""
    net, _ = _hip_model()
    net.eval()
    g = torch.Generator().manual_seed(1926)
    x = torch.randint(0, 256, (32, 3, 256, 256), generator=g).float() / 255
    jpeg, jpeg_bpp = net.jpeg(x)
    from hyres_hip import ops as O
    O.Trace.nodes = {}
    with torch.no_grad():
        out = net(x, jpeg=(jpeg, jpeg_bpp))
        y_hat = O.Trace.value("y_hat").cpu()
        O.Trace.nodes = None
        idx = [0, 31]
        out2 = net(x[idx], jpeg=(jpeg[idx], jpeg_bpp))
    torch.cuda.synchronize()
    # batch independence, decision-aware as _check_against_oracle: bs 32 and bs 2 take different kernels (the
    # weight-resident 3x3 needs >= 2 tiles per CU, split-K factors follow the grid), so fp32 rounding differs and a
    # y - mu within that noise of k + .5 may round the other way; each such flip perturbs x_hat only in its
    # receptive field
    ly2, ly = out2["likelihoods"]["y"].cpu().double(), out["likelihoods"]["y"].cpu()[idx].double()
    nflip = int(((ly2 - ly).abs() > 1e-3 * ly.abs().clamp_min(1e-9)).sum())
    assert nflip <= max(2, 1e-5 * ly.numel()), nflip
    xa, xb = out2["x_hat"].cpu().double(), out["x_hat"].cpu()[idx].double()
    nbad = int(((xa - xb).abs() / xb.abs().max() > TOL).sum())
    print(f"bs32 vs bs2: {nflip} likelihood flips, {nbad} x_hat values beyond {TOL}, "
          f"x_hat normwise {rel_err(xa, xb):.2e}")
    assert nbad <= nflip * 64 * 64 * 3, (nbad, nflip)
    _check_against_oracle(out, idx, x, jpeg, float(jpeg_bpp), y_hat)


def test_c5_kodak_size_eval_parity(fp32_gemm):
    """BASELINE config C5 shape: one 768x512 image (Kodak size, W != H; latents 96x64 / 24x16), eval,
    MultiScaleRefine on the HIP path, fp32 (the fp16-operand variant: test_c5_fp16_autocast_eval)."""
    net, _ = _hip_model()
    net.eval()
    g = torch.Generator().manual_seed(7)
    # smooth synthetic content (low-frequency field + 8-bit noise), so JPEG and the codec see image-like data
    base = F.interpolate(torch.rand(1, 3, 16, 24, generator=g), size=(512, 768), mode="bilinear",
                         align_corners=False)
    x = ((base * 0.8 + 0.2 * torch.rand(1, 3, 512, 768, generator=g)) * 255).floor() / 255
    jpeg, jpeg_bpp = net.jpeg(x)
    from hyres_hip import ops as O
    O.Trace.nodes = {}
    with torch.no_grad():
        out = net(x, jpeg=(jpeg, jpeg_bpp))
        y_hat = O.Trace.value("y_hat").cpu()
        O.Trace.nodes = None
    torch.cuda.synchronize()
    assert out["likelihoods"]["y"].shape == (1, 192, 64, 96)
    assert out["likelihoods"]["z"].shape == (1, 128, 16, 24)
    _check_against_oracle(out, [0], x, jpeg, float(jpeg_bpp), y_hat)


@pytest.mark.parametrize("case", [(2, 64, 64, 16, 16, 3, 1, 1, 1), (2, 128, 192, 16, 16, 5, 2, 2, 1),
                                  (2, 192, 96, 8, 8, 1, 1, 0, 1), (2, 96, 96, 8, 8, 3, 1, 1, 1)])
def test_conv2d_fp16_operands(case):
    """Forward conv under torch.autocast(float16), no tape: fp16-rounded operands on the f16 MFMA with fp32
    accumulation == torch fp32 conv of the fp16-rounded operands (2e-6: only the summation order
    differs), and within 4e-3 of the fp32 conv (operand rounding 2^-11)."""
    from hyres_hip import ops as O
    B, Ci, Co, H, W, K, s, p, d = case
    x = _rand((B, Ci, H, W), 11)
    w = _rand((Co, Ci, K, K), 12, 1.0 / (Ci * K * K) ** 0.5)
    b = _rand((Co,), 13, 0.1)
    y32 = F.conv2d(x, w, b, stride=s, padding=p, dilation=d)
    yh = F.conv2d(x.half().float(), w.half().float(), b, stride=s, padding=p, dilation=d)
    D = dev()
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
        yn = O.conv2d(None, O.to_nhwc(x.to(D)), w.to(D), b.to(D), stride=s, pad=p, dil=d)
        y = O.to_nchw(yn).cpu()
    assert y.dtype == torch.float32
    assert rel_err(y, yh) < 2e-6
    assert rel_err(y, y32) < 4e-3


def _nhwc16(t):
    from hyres_hip import ops as O
    return O.Node(t.permute(0, 2, 3, 1).contiguous().half().to(dev()), rg=False)


def test_fp16_activation_ops():
    """configs[4] "fp16 activations": every forward kernel of the fp16 region (conv / deconv / GDN / IGDN
    epilogues incl. residual + ReLU / PReLU, split-K, the Ci=3 image-side conv, the Co=3 narrow convs,
    bilinear, SE, spatial attention, the attention gate) reads / writes fp16 activations and computes in
    fp32. Reference: the same HIP op with fp32 activations holding the fp16-rounded inputs (fp16 MFMA
    operands in both); bound 2e-3 normwise = the output's own fp16 rounding (2^-11) plus margin."""
    from hyres_hip import _lib as L
    from hyres_hip import ops as O
    from hyres_hip import refine_ops as R
    D = dev()
    TOLH = 2e-3

    def f32(n):  # fp16 node -> fp32 node (same values)
        return O.Node(n.v.float(), rg=False)

    def chk(yh, y32, what):
        assert yh.half, what
        assert rel_err(O.to_nchw(yh).cpu(), O.to_nchw(y32).cpu()) < TOLH, what

    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
        x = _nhwc16(_rand((2, 64, 24, 20), 1))
        r = _nhwc16(_rand((2, 64, 24, 20), 2))
        w = _rand((64, 64, 3, 3), 3, 1.0 / 24).to(D)
        b = _rand((64,), 4, 0.1).to(D)
        slope = torch.full((1,), 0.25, device=D)
        with O.f16_region():
            y = O.conv2d(None, x, w, b, pad=1, act=L.ACT_RELU, res=r)
            yp = O.conv2d(None, x, w, b, pad=2, dil=2, act=L.ACT_PRELU, slope=slope)
        chk(y, O.conv2d(None, f32(x), w, b, pad=1, act=L.ACT_RELU, res=f32(r)), "conv res relu")
        chk(yp, O.conv2d(None, f32(x), w, b, pad=2, dil=2, act=L.ACT_PRELU, slope=slope), "conv prelu")
        # fp16 X -> fp32 Y outside the region (g_a's conv(N, M) into the latent)
        yo = O.conv2d(None, x, w, b, pad=1)
        assert not yo.half
        assert rel_err(O.to_nchw(yo).cpu(), O.to_nchw(O.conv2d(None, f32(x), w, b, pad=1)).cpu()) < 1e-5
        # W % 64 == 0: the halo-staged f16 3x3 kernel with fp16 X and Y (IO 3) and fp16 X -> fp32 Y (IO 1)
        x64, r64 = _nhwc16(_rand((2, 64, 12, 64), 7)), _nhwc16(_rand((2, 64, 12, 64), 8))
        with O.f16_region():
            y64 = O.conv2d(None, x64, w, b, pad=1, act=L.ACT_RELU, res=r64)
        chk(y64, O.conv2d(None, f32(x64), w, b, pad=1, act=L.ACT_RELU, res=f32(r64)), "halo conv res relu")
        yo64 = O.conv2d(None, x64, w, b, pad=1)
        assert not yo64.half
        assert rel_err(O.to_nchw(yo64).cpu(), O.to_nchw(O.conv2d(None, f32(x64), w, b, pad=1)).cpu()) < 1e-5
        # enough tiles for the weight-resident persistent kernel (IO 3 and IO 1)
        xw, rw = _nhwc16(_rand((4, 64, 128, 256), 9)), _nhwc16(_rand((4, 64, 128, 256), 10))
        with O.f16_region():
            yw = O.conv2d(None, xw, w, b, pad=1, act=L.ACT_RELU, res=rw)
        chk(yw, O.conv2d(None, f32(xw), w, b, pad=1, act=L.ACT_RELU, res=f32(rw)), "wres conv res relu")
        yow = O.conv2d(None, xw, w, b, pad=1)
        assert rel_err(O.to_nchw(yow).cpu(), O.to_nchw(O.conv2d(None, f32(xw), w, b, pad=1)).cpu()) < 1e-5
        # image side: fp32 X (Ci=3, scalar path) -> fp16 Y; 5x5 s2
        xi = O.to_nhwc(_rand((2, 3, 32, 40), 5).to(D))
        wi = _rand((128, 3, 5, 5), 6, 1.0 / 75 ** 0.5).to(D)
        with O.f16_region():
            yi = O.conv2d(None, xi, wi, None, stride=2, pad=2)
        chk(yi, O.conv2d(None, xi, wi, None, stride=2, pad=2), "conv 3->128 s2")
        # small grid with split-K (192 -> 384 3x3 at 8x8) and the 1x1 GDN square prologue
        xs = _nhwc16(_rand((2, 192, 8, 8), 7))
        ws = _rand((384, 192, 3, 3), 8, 1.0 / 1728 ** 0.5).to(D)
        with O.f16_region():
            ys = O.conv2d(None, xs, ws, None, pad=1)
        chk(ys, O.conv2d(None, f32(xs), ws, None, pad=1), "split-K conv")
        xg = _nhwc16(_rand((2, 128, 16, 12), 9))
        beta = (torch.rand(128, generator=torch.Generator().manual_seed(10)) + 0.5).to(D)
        gamma = (0.1 * torch.eye(128) + 0.01).to(D)
        for inv in (False, True):
            yg = O.gdn(None, xg, beta, gamma, inv)
            chk(yg, O.gdn(None, f32(xg), beta, gamma, inv), "gdn inverse=%d" % inv)
        # deconv 5x5 s2 fp16 -> fp16, then the narrow Co=3 deconv fp16 -> fp32
        wd = _rand((128, 128, 5, 5), 11, 1.0 / (128 * 25 / 4) ** 0.5).to(D)
        with O.f16_region():
            yd = O.deconv2d(None, xg, wd, b[:1].repeat(128))
        chk(yd, O.deconv2d(None, f32(xg), wd, b[:1].repeat(128)), "deconv")
        w3 = _rand((128, 3, 5, 5), 12, 1.0 / (128 * 25 / 4) ** 0.5).to(D)
        with O.f16_region():
            y3 = O.deconv2d(None, xg, w3, None)
        assert not y3.half
        assert rel_err(O.to_nchw(y3).cpu(), O.to_nchw(O.deconv2d(None, f32(xg), w3, None)).cpu()) < 1e-5
        wn = _rand((3, 64, 3, 3), 13, 1.0 / 24).to(D)
        yn = O.conv2d(None, x, wn, None, pad=1)
        assert rel_err(O.to_nchw(yn).cpu(), O.to_nchw(O.conv2d(None, f32(x), wn, None, pad=1)).cpu()) < 1e-5
        # MultiScaleRefine pieces and the AttentionBlock gate
        chk(R.bilinear(None, x, 12, 10, 2.0, 2.0), R.bilinear(None, f32(x), 12, 10, 2.0, 2.0), "bilinear down")
        chk(R.bilinear(None, x, 48, 40, 0.5, 0.5), R.bilinear(None, f32(x), 48, 40, 0.5, 0.5), "bilinear up")
        w1 = _rand((4, 64), 14, 0.2).to(D)
        w2 = _rand((64, 4), 15, 0.2).to(D)
        chk(R.se_block(None, x, w1, w2), R.se_block(None, f32(x), w1, w2), "SE")
        wsa = _rand((1, 2, 7, 7), 16, 0.2).to(D)
        chk(R.spatial_attention_mul(None, x, wsa), R.spatial_attention_mul(None, f32(x), wsa), "spatial attention")
        chk(O.attn_gate(None, x, r, y), O.attn_gate(None, f32(x), f32(r), f32(y)), "attention gate")


@pytest.mark.parametrize("f16_act", [True, False])
def test_c5_fp16_autocast_eval(f16_act, monkeypatch):
    """BASELINE configs[4]: Kodak-size inference under torch.autocast("cuda", float16) — forward convs take
    fp16 operands on v_mfma_f32_32x32x16_f16 (fp32 accumulation), and (f16_act) g_a / g_s above the latent
    resolution and MultiScaleRefine keep their activations as fp16 in HBM. No fp16 golden exists
    (the reference's AMP path needs CUDA): parity is unpinned against the reference's fp16 run and checked
    against this build's fp32 path, which is pinned to the reference fixtures. Tolerances (fp16 operands,
    2^-11 relative rounding, which also flips a few round() decisions of y_hat, each perturbing a local
    window of x_hat): PSNR within 0.05 dB, bpp within 1 %, mean |x_hat diff| < 1e-2 (measured 6.7e-3 with
    fp32 activations)."""
    import math
    from hyres_hip import ops as O
    monkeypatch.setattr(O, "F16_ACT", f16_act)
    halves = []
    real_new = O.Node.new

    def spy(*a, **k):
        n = real_new(*a, **k)
        halves.append(n.half)
        return n
    monkeypatch.setattr(O.Node, "new", staticmethod(spy))
    net, _ = _hip_model()
    net.eval()
    g = torch.Generator().manual_seed(7)
    base = F.interpolate(torch.rand(1, 3, 16, 24, generator=g), size=(512, 768), mode="bilinear",
                         align_corners=False)
    x = ((base * 0.8 + 0.2 * torch.rand(1, 3, 512, 768, generator=g)) * 255).floor() / 255
    jpeg, jpeg_bpp = net.jpeg(x)
    with torch.no_grad():
        o32 = net(x, jpeg=(jpeg, jpeg_bpp))
        with torch.autocast("cuda", dtype=torch.float16):
            o16 = net(x, jpeg=(jpeg, jpeg_bpp))
    torch.cuda.synchronize()
    assert o16["x_hat"].dtype == torch.float32 and o16["likelihoods"]["y"].shape == (1, 192, 64, 96)
    assert not torch.equal(o16["x_hat"], o32["x_hat"]), "fp16 operand path did not engage"
    assert any(halves) == f16_act, "fp16 activations engaged iff enabled"
    xd = x.to(o32["x_hat"].device)

    def psnr(a):
        return 10 * math.log10(1.0 / float(F.mse_loss(a, xd)))

    def bits(o):
        return sum(float((-torch.log2(v)).sum()) for v in o["likelihoods"].values())

    assert abs(psnr(o16["x_hat"]) - psnr(o32["x_hat"])) < 0.05
    assert abs(bits(o16) - bits(o32)) < 0.01 * bits(o32)
    assert float((o16["x_hat"] - o32["x_hat"]).abs().mean()) < 1e-2


# ------------------------------------------------------------------------------------------------ graphs
def test_captured_eval_matches_eager_and_reference():
    """hyres_hip.graphs.CapturedStep (eval): the replayed HIP graph computes exactly what the eager
    launches compute, for the captured input and for new inputs copied into the static buffers."""
    from hyres_hip.graphs import CapturedStep
    g = load_npz("hyres_eval_b2_64.npz")
    net, _ = _hip_model()
    net.eval()
    D = dev()
    x, j, bpp = g["x"].to(D), g["jpeg_decoded"].to(D), float(g["jpeg_bpp"])
    with torch.no_grad():
        eager = net.forward_device(x, j, bpp)["x_hat"].clone()
    cap = CapturedStep(net, x, j, bpp)
    out, _ = cap.replay()
    torch.cuda.synchronize()
    assert torch.equal(out["x_hat"], eager)
    assert rel_err(out["x_hat"].cpu(), g["x_hat"]) < TOL
    x2 = torch.flip(x, dims=[3]).contiguous()
    j2 = torch.flip(j, dims=[3]).contiguous()
    with torch.no_grad():
        eager2 = net.forward_device(x2, j2, bpp)
    out, _ = cap.replay(x2, j2, bpp)
    torch.cuda.synchronize()
    assert torch.equal(out["x_hat"], eager2["x_hat"])
    assert torch.equal(out["likelihoods"]["y"], eager2["likelihoods"]["y"])
    out = None
    cap.close()


def test_captured_train_step_matches_eager():
    """CapturedStep (train, recorded noise injected): loss and every parameter gradient of a replay equal
    the eager step's; without injection every replay draws fresh noise (device-resident seed)."""
    from hyres_hip.graphs import CapturedStep
    from hyres_hip.loss import RateDistortionLoss
    g = load_npz("hyres_train_b2_64.npz")
    net, _ = _hip_model()
    net.train()
    D = dev()
    x, j = g["x"].to(D), g["jpeg_decoded"].to(D)
    rm = net.residual_model
    rm.noise.injected = {"z": g["noise_z"].permute(0, 2, 3, 1).contiguous().to(D),
                         "y": g["noise_y"].permute(0, 2, 3, 1).contiguous().to(D)}
    crit = RateDistortionLoss(lmbda=0.045, alpha=0)
    params = [p for p in net.parameters() if p.requires_grad]

    def zero():
        for p in params:
            if p.grad is not None:
                p.grad.zero_()

    zero()
    c = crit(net.forward_device(x, j, 0.25), x)
    c["loss"].backward()
    torch.cuda.synchronize()
    loss_e = float(c["loss"])
    grads_e = [p.grad.detach().clone() for p in params]
    zero()
    cap = CapturedStep(net, x, j, 0.25, criterion=crit, zero_grad=zero)
    cc = cap.replay()[1]
    torch.cuda.synchronize()
    assert float(cc["loss"]) == loss_e
    for p, ge in zip(params, grads_e):
        assert torch.equal(p.grad, ge), p.shape
    # fresh noise per replay when nothing is injected
    rm.noise.injected = None
    cap2 = CapturedStep(net, x, j, 0.25, criterion=crit, zero_grad=zero)
    l1 = float(cap2.replay()[1]["loss"])
    l2 = float(cap2.replay()[1]["loss"])
    assert l1 != l2 and abs(l1 - l2) < 0.05 * abs(l1)
    cc = None
    cap.close()
    cap2.close()


def test_captured_step_close_refuses_live_outputs():
    """The graph-lifetime rule (hyres_hip/graphs.py CapturedStep.close): a replay's outputs live in the
    graph's private pool, so close() with one of them still referenced raises GraphOutputsAlive and leaves the graph
    alone (no reset: the held tensor keeps its values); once the reference is dropped close() resets the graph. The
    static inputs the forward passes through (jpeg_decoded, jpeg_bpp_loss) are the step's own and are not tracked.
    Reference loop the rule serves: /root/reference/src/utils/engine.py:28-56."""
    from hyres_hip.graphs import CapturedStep, GraphOutputsAlive
    from hyres_hip.loss import RateDistortionLoss
    g = load_npz("hyres_train_b2_64.npz")
    net, _ = _hip_model()
    net.train()
    D = dev()
    x, j = g["x"].to(D), g["jpeg_decoded"].to(D)
    crit = RateDistortionLoss(lmbda=0.045, alpha=0)
    params = [p for p in net.parameters() if p.requires_grad]

    def zero():
        for p in params:
            if p.grad is not None:
                p.grad.zero_()

    cap = CapturedStep(net, x, j, 0.25, criterion=crit, zero_grad=zero)
    assert cap.live_outputs() > 5  # x_hat, both likelihoods, residual(s), the loss terms
    out, c = cap.replay()
    torch.cuda.synchronize()
    loss = c["loss"]  # one held output is enough
    want = float(loss)
    x_hat = out["x_hat"].clone()
    del out, c
    with pytest.raises(GraphOutputsAlive):
        cap.close()
    assert cap.graph is not None, "close() must not reset the graph while an output is referenced"
    assert cap.live_outputs() == 1
    assert float(loss) == want  # the pool was not released under the held tensor
    del loss
    cap.close()
    assert cap.graph is None and cap.live_outputs() == 0
    # eval capture: outputs include the step's own static jpeg buffer, which close() does not count
    net.eval()
    cap = CapturedStep(net, x, j, 0.25)
    out, _ = cap.replay()
    jd = out["jpeg_decoded"]
    assert jd.data_ptr() == cap.jpeg.data_ptr()
    del out
    cap.close()
    assert cap.graph is None
    assert x_hat.isfinite().all()


def test_captured_step_survives_eager_step_with_new_layouts_and_bigger_workspace():
    """Regression (round 4, commit 5e08bd4): an eager step between two replays that registers NEW weight layouts
    (rebuilding the batched re-layout's descriptor table) and GROWS a workspace slot (replacing its buffer) must not
    free what the graph recorded: the graph's weight_prep_batch_kernel read the freed descriptor table (illegal
    address) before CapturedStep kept both alive. Capture at bs 2 64x64; eager step at bs 4 128x128; replay; the
    replay's loss and every parameter gradient equal a fresh eager step's, bit for bit (src/utils/engine.py:33,50-53
    mixes eager and graphed steps the same way)."""
    from hyres_hip import ops as O
    from hyres_hip.graphs import CapturedStep
    from hyres_hip.loss import RateDistortionLoss
    g = load_npz("hyres_train_b2_64.npz")
    net, _ = _hip_model()
    net.train()
    D = dev()
    x, j = g["x"].to(D), g["jpeg_decoded"].to(D)
    rm = net.residual_model
    injected = {"z": g["noise_z"].permute(0, 2, 3, 1).contiguous().to(D),
                "y": g["noise_y"].permute(0, 2, 3, 1).contiguous().to(D)}
    crit = RateDistortionLoss(lmbda=0.045, alpha=0)
    params = [p for p in net.parameters() if p.requires_grad]

    def zero():
        for p in params:
            if p.grad is not None:
                p.grad.zero_()

    rm.noise.injected = injected
    zero()
    cap = CapturedStep(net, x, j, 0.25, criterion=crit, zero_grad=zero)
    st = O.PrepBatch._state[D.index]
    old_table = st["table"]
    ws_before = {k: (b.data_ptr(), b.numel()) for k, b in O.Workspace._bufs.items()}
    # eager work in between: a conv with a weight the graph never saw registers a NEW layout (the descriptor table
    # is rebuilt), and a train step at a bigger geometry grows the workspace slots
    extra_w = torch.nn.Parameter(_rand((64, 3, 3, 3), 91, 0.2).to(D))
    O.conv2d(None, O.to_nhwc(_rand((1, 3, 32, 32), 92).to(D)), extra_w, None, pad=1)
    rm.noise.injected = None
    gen = torch.Generator().manual_seed(11)
    xb = torch.rand((4, 3, 128, 128), generator=gen).to(D)
    jb = (xb + 0.02 * torch.randn((4, 3, 128, 128), generator=gen).to(D)).clamp(0, 1)
    crit(net.forward_device(xb, jb, 0.3), xb)["loss"].backward()
    O.PrepBatch.prepare(D)  # what the next capture / batch run would do: rebuild the table from the new entries
    torch.cuda.synchronize()
    grew = [k for k, b in O.Workspace._bufs.items() if k not in ws_before or ws_before[k][1] < b.numel()]
    assert st["table"] is not old_table, "descriptor table not rebuilt"
    assert grew, "no workspace slot grew"
    del xb, jb, old_table
    torch.cuda.empty_cache()  # hand the replaced buffers back to the device: a dangling read would now fault
    rm.noise.injected = injected
    zero()
    cc = cap.replay()[1]
    torch.cuda.synchronize()
    loss_r = float(cc["loss"])
    grads_r = [p.grad.detach().clone() for p in params]
    zero()
    c = crit(net.forward_device(x, j, 0.25), x)
    c["loss"].backward()
    torch.cuda.synchronize()
    assert float(c["loss"]) == loss_r
    for p, gr in zip(params, grads_r):
        assert torch.equal(p.grad, gr), p.shape
    rm.noise.injected = None
    del cc
    cap.close()


def test_overlapped_rccl_reducer_single_rank():
    """The RCCL path of hyres_hip.ddp.FlatGradReducer with backward-overlapped segments, on a one-rank
    nccl (= RCCL) group: markers fire during the real model's tape backward, collectives are enqueued
    behind the weight-gradient side stream, and the reduced gradients equal the un-reduced ones."""
    import os
    import socket
    import torch.distributed as tdist
    from hyres_hip.ddp import FlatGradReducer, HYRES_SEGMENTS
    from hyres_hip.loss import RateDistortionLoss
    from hyres_hip.ops import GradReady
    from hyres_hip.optim import FusedAdam
    g = load_npz("hyres_train_b2_64.npz")
    net, _ = _hip_model()
    net.train()
    D = dev()
    x, j = g["x"].to(D), g["jpeg_decoded"].to(D)
    names = [n for n, p in sorted(net.named_parameters()) if not n.endswith(".quantiles")]
    opt = FusedAdam([p for n, p in sorted(net.named_parameters()) if not n.endswith(".quantiles")], lr=0.0)
    crit = RateDistortionLoss(lmbda=0.045, alpha=0)
    net.residual_model.noise.injected = {"z": g["noise_z"].permute(0, 2, 3, 1).contiguous().to(D),
                                         "y": g["noise_y"].permute(0, 2, 3, 1).contiguous().to(D)}
    opt.zero_grad()
    crit(net.forward_device(x, j, 0.0), x)["loss"].backward()
    ref = opt.flat.grad.clone()
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    tdist.init_process_group("nccl", rank=0, world_size=1)
    try:
        red = FlatGradReducer(opt.flat, 1, names=names, segments=HYRES_SEGMENTS).overlap()
        opt.zero_grad()
        crit(net.forward_device(x, j, 0.0), x)["loss"].backward()
        assert red.fired == ["refine", "g_s", "hyper"]
        red.all_reduce()
        torch.cuda.synchronize()
        assert torch.equal(opt.flat.grad, ref)
    finally:
        GradReady.listeners = []
        tdist.destroy_process_group()


@pytest.mark.parametrize("split", [False, True])
def test_captured_step_with_rccl_group_single_rank(split):
    """The N > 1 bench path: the train step captured (capture_error_mode thread_local) while an RCCL
    process group is live, replayed, then the flat gradients all-reduced after the replay in buckets; the
    reduced gradients equal the eager step's. split (graph+overlap, the default N > 1 mode): the capture cut at the
    "hyper" marker into two graphs, the finished segments' RCCL all-reduce started between the replays."""
    import os
    import socket
    import torch.distributed as tdist
    from hyres_hip.ddp import FlatGradReducer, HYRES_SEGMENTS
    from hyres_hip.graphs import CapturedStep
    from hyres_hip.loss import RateDistortionLoss
    from hyres_hip.optim import FusedAdam
    g = load_npz("hyres_train_b2_64.npz")
    net, _ = _hip_model()
    net.train()
    D = dev()
    x, j = g["x"].to(D), g["jpeg_decoded"].to(D)
    names = [n for n, p in sorted(net.named_parameters()) if not n.endswith(".quantiles")]
    opt = FusedAdam([p for n, p in sorted(net.named_parameters()) if not n.endswith(".quantiles")], lr=0.0)
    crit = RateDistortionLoss(lmbda=0.045, alpha=0)
    net.residual_model.noise.injected = {"z": g["noise_z"].permute(0, 2, 3, 1).contiguous().to(D),
                                         "y": g["noise_y"].permute(0, 2, 3, 1).contiguous().to(D)}
    opt.zero_grad()
    crit(net.forward_device(x, j, 0.0), x)["loss"].backward()
    torch.cuda.synchronize()
    ref = opt.flat.grad.clone()
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    tdist.init_process_group("nccl", rank=0, world_size=1)
    try:
        red = FlatGradReducer(opt.flat, 1, names=names, segments=HYRES_SEGMENTS)
        red.all_reduce()  # a completed collective before the capture (the watchdog has work to poll)
        opt.zero_grad()
        cap = CapturedStep(net, x, j, 0.0, criterion=crit, zero_grad=opt.zero_grad,
                           capture_error_mode="thread_local", split_at=("hyper",) if split else ())
        assert len(cap.graphs) == (2 if split else 1)
        for _ in range(2):
            opt.zero_grad()
            cap.replay(between=red.launch_segments if split else None)
            if split:
                assert red.fired == ["refine", "g_s", "hyper"]
            red.all_reduce()
            torch.cuda.synchronize()
            assert red.fired == []
            assert torch.equal(opt.flat.grad, ref)
        cap.close()
    finally:
        tdist.destroy_process_group()


def test_batched_weight_relayout_matches_individual():
    """hyres_hip.ops.PrepBatch: after an optimiser-style weight update (new epoch) every cached conv
    re-layout is refreshed by ONE batched launch, bit-identical to the per-layer re-layout kernel."""
    import ctypes
    from hyres_hip import _lib as L
    from hyres_hip import ops as O
    g = load_npz("hyres_eval_b2_64.npz")
    net, _ = _hip_model()
    net.eval()
    D = dev()
    x, j = g["x"].to(D), g["jpeg_decoded"].to(D)
    with torch.no_grad():
        ref = net.forward_device(x, j, 0.0)["x_hat"].clone()
        W = net.residual_model.g_a[4].weight
        W.data.add_(0.01)
        O.bump_weight_epoch()
        out = net.forward_device(x, j, 0.0)["x_hat"].clone()
    torch.cuda.synchronize()
    st = O.PrepBatch._state[D.index]
    assert st["epoch"] == O._WEIGHT_EPOCH[0] and st["n"] > 10, "batched re-layout did not run"
    assert not torch.equal(out, ref)
    for wr, key, br, _, _ in st["order"]:
        w, buf = wr(), br()
        ent = [e for e in st["entries"].values() if e[0]() is w and e[1] == key][0]
        _, _, geom, _, mode, Ci, Co, KH, KW, _, _ = ent
        one = torch.empty_like(buf)
        L.call("hyres_conv_weight_prep", ctypes.byref(geom), w.data_ptr(), one.data_ptr(), mode, Ci, Co, KH, KW, 0,
               None, L.stream())
        torch.cuda.synchronize()
        assert torch.equal(one, buf), key
    with torch.no_grad():
        W.data.sub_(0.01)
        O.bump_weight_epoch()
        back = net.forward_device(x, j, 0.0)["x_hat"]
    torch.cuda.synchronize()
    assert torch.equal(back, ref)


# ------------------------------------------------------------------------------------------------ entropy coding
@pytest.mark.parametrize("amp", [False, True])
def test_compress_decompress_roundtrip(amp):
    """update() -> compress -> decompress (amp: all under torch.autocast(float16), i.e. fp16
    operands and the fp16-activation region of configs[4] on both sides). The decoded residual equals the eval forward's
    residual_hat (clamped as the reference's LightWeightCheckerboard.decompress does) to 1e-6 — the
    checkerboard two-pass decode reproduces y_hat exactly — the final x_hat equals the reference formula on
    it, the strings' length is in the range of the forward's ideal code length, and decoding inside compress
    (the reference's literal order) writes the same strings. Bitstream parity with compressai itself is
    unpinned (not installed); the coder is bit-exact to the restatement (tests/test_lib_cpu.py)."""
    import math
    g = load_npz("kodim01_crop64_eval.npz")
    net, _ = _hip_model()
    net.eval()
    D = dev()
    assert net.update(force=True)
    rm = net.residual_model
    assert rm.gaussian_conditional._quantized_cdf.shape[0] == 64 and rm.entropy_bottleneck._offset.numel() == 128
    x = g["x"]
    ctx = torch.autocast("cuda", dtype=torch.float16) if amp else torch.autocast("cuda", enabled=False)
    with torch.no_grad(), ctx:
        fwd = net(x)
        c = net.compress(x)
        d = net.decompress(c)
        dres = rm.decompress(c["strings"], c["shape"])
        x0 = fwd["jpeg_decoded"].to(D) + dres["x_hat"]
        from hyres_hip import ops as O
        with O.f16_region():
            want = torch.clamp(x0 + net.refine(x0), 0, 1)
    torch.cuda.synchronize()
    assert tuple(c["shape"]) == (x.shape[2] // 32, x.shape[3] // 32)
    res_ref = fwd["residual_hat"].clamp(0, 1)
    assert float((dres["x_hat"] - res_ref).abs().max()) <= 1e-6
    assert float((d["x_hat"] - want).abs().max()) <= 1e-6
    nbytes = sum(len(s) for part in (c["strings"][0][0], c["strings"][0][1], c["strings"][1]) for s in part)
    nstr = sum(len(part) for part in (c["strings"][0][0], c["strings"][0][1], c["strings"][1]))
    ideal = sum(float((-torch.log2(v)).sum()) for v in fwd["likelihoods"].values()) / 8
    # the reference codes BOTH checkerboard passes over all positions (anchor pass: y*mask_a with the anchor
    # parameters, non-anchor pass likewise), while the forward's likelihood uses the combined y_hat with
    # summed scales/means (models/checkerboard.py:136-142), so the two lengths agree only loosely
    assert 0.5 * ideal <= nbytes <= 2.0 * ideal + 8 * nstr, (nbytes, ideal)
    rm.decode_in_compress = True
    try:
        with torch.no_grad(), ctx:
            c2 = net.compress(x)
    finally:
        rm.decode_in_compress = False
    assert c2["strings"] == c["strings"]
    assert math.isfinite(c["time"]) and math.isfinite(d["time"])


def test_inference_cli_compress_decompress(tmp_path):
    """src/inference.py end to end on one 64x64 PNG: checkpoint load (weights_only), update(), compress ->
    decompress, the reference's metrics.csv columns with bpp from the real strings and JPEG bytes."""
    import csv
    import numpy as np
    from PIL import Image
    from src.inference import main as infer_main
    g = load_npz("kodim01_crop64_eval.npz")
    net, sd = _hip_model()
    ck = tmp_path / "ckpt.pth.tar"
    torch.save({"state_dict": {k: v.cpu() for k, v in net.state_dict().items()}}, ck)
    img = (g["x"][0].permute(1, 2, 0).numpy() * 255).round().astype(np.uint8)
    Image.fromarray(img).save(tmp_path / "img.png")
    out = tmp_path / "out"
    infer_main(["--checkpoint", str(ck), "--input", str(tmp_path / "img.png"), "--output", str(out),
                "--jpeg-quality", "50", "--save-components"])
    rows = list(csv.DictReader(open(out / "metrics.csv")))
    assert len(rows) == 1 and rows[0]["filename"] == "img.png"
    r = rows[0]
    assert float(r["y_bpp"]) > 0 and float(r["z_bpp"]) > 0 and float(r["jpeg_bpp"]) > 0
    assert abs(float(r["total_bpp"]) - (float(r["jpeg_bpp"]) + float(r["y_bpp"]) + float(r["z_bpp"]))) < 1e-9
    assert 5.0 < float(r["psnr"]) < 80.0
    assert (out / "img_recon.png").exists() and (out / "img_residual_hat.png").exists()


# ------------------------------------------------------------------------------------------------ more parity
def test_checkerboard_index_sets_bit_exact_on_gpu():
    """north_star: the anchor / non-anchor index sets must be bit-exact.  An arange y with zero means goes
    through the HIP kernels (hyres_ckbd_anchor_fwd: y_anchor_hat = STE(y*anchor - 0) + 0; the non-anchor
    kernel with y_anchor_hat = 0: y_hat = y*non_anchor) and is compared with torch.equal against the sets
    the reference's own _split_tensor produced (tests/golden/checkerboard_sets.npz) and, on a ragged
    multi-image shape, against (h + w) even / odd."""
    from hyres_hip import _lib as L
    from hyres_hip.ops import _empty, zeros
    D = dev()
    sets = load_npz("checkerboard_sets.npz")

    def run(B, H, W, C):
        y = torch.arange(B * H * W * C, dtype=torch.float32).remainder(4093.0).reshape(B, H, W, C).to(D)
        params = zeros((B, H, W, 2 * C), D)  # scales | means = 0
        ya = _empty((B, H, W, C), D)
        L.call("hyres_ckbd_anchor_fwd", y.data_ptr(), params[..., C:].data_ptr(), 2 * C, None, ya.data_ptr(), B, H, W,
               C, L.stream())
        z = zeros((B, H, W, C), D)
        outs = [_empty((B, H, W, C), D) for _ in range(5)]
        L.call("hyres_ckbd_nonanchor_gc_fwd", y.data_ptr(), z.data_ptr(), params.data_ptr(), 2 * C, params.data_ptr(),
               2 * C, None, None, *[o.data_ptr() for o in outs], B, H, W, C, L.stream())
        torch.cuda.synchronize()
        return y.cpu(), ya.cpu(), outs[0].cpu()

    y, ya, yna = run(1, 4, 4, 1)
    yy = torch.arange(16.0).view(4, 4)
    assert torch.equal(y[0, :, :, 0], yy)
    assert torch.equal(ya[0, :, :, 0], sets["anchor"].float())
    assert torch.equal(yna[0, :, :, 0], sets["non_anchor"].float())
    y, ya, yna = run(3, 6, 10, 5)
    i = torch.arange(6).view(6, 1)
    j = torch.arange(10).view(1, 10)
    anchor = ((i + j) % 2 == 0).view(1, 6, 10, 1)
    assert torch.equal(ya, y * anchor)
    assert torch.equal(yna, y * ~anchor)


def test_c2_size_train_step_vs_fp64_oracle(fp32_gemm):
    """BASELINE config C2 at its full size (bs=16, 256x256, train, noisequant=False, lambda=0.045): the HIP
    train step (the bench's tile routing, split-K factors and XCD-ordered grids) vs the fp64 oracle on the
    host with the same recorded noise: loss within 1e-4 and every parameter gradient normwise within 1e-3,
    decision-exact as in test_model_train_step_matches_reference (at this size thousands of ReLU / PReLU
    inputs and a few round() arguments sit within fp32 rounding of their kinks; the number followed is
    printed and each is checked to be a near-tie)."""
    net, _ = _hip_model()
    net.train()
    D = dev()
    g = torch.Generator().manual_seed(1926)
    x = torch.randint(0, 256, (16, 3, 256, 256), generator=g).float() / 255
    jpeg, jb = net.jpeg(x)
    jb = float(jb)
    ng = torch.Generator().manual_seed(45)
    noise = {"z": torch.rand((16, 128, 8, 8), generator=ng) - 0.5, "y": torch.rand((16, 192, 32, 32), generator=ng) - 0.5}
    _, crit, dec, hats = _hip_train_step(net, x, jpeg, jb, False, _nhwc_noise(noise, {"z": "z", "y": "y"}, D), 0.045)
    torch.set_num_threads(16)
    ref, terms, loss64, followed = _oracle_following({"x": x, "jpeg_decoded": jpeg}, jb, False, noise, 0.045, dec,
                                                     hats)
    assert abs(float(crit["loss"]) - loss64) <= TOL * abs(loss64), (float(crit["loss"]), loss64)
    rows = _check_grads(net, ref, terms)
    print(f"C2 loss hip {float(crit['loss']):.6f} oracle {loss64:.6f}; followed {followed}; worst grads",
          [f"{e:.2e} {k}" for e, k in rows[:5]])


def test_compress_bitstream_matches_oracle():
    """LightWeightCheckerboard.compress (models/checkerboard.py:167-198) on the Kodak crop's
    residual writes strings byte-equal to the oracle's restatement (oracle/entropy_coding.py
    reference_compress: the fp32 oracle transforms, compressai 1.2.6 build_indexes / symbols / rANS and CDF
    tables) — the scale-index choice, the symbols and the coder are all pinned, not only the round trip."""
    import numpy as np
    from oracle.entropy_coding import reference_compress
    g = load_npz("kodim01_crop64_eval.npz")
    net, sd = _hip_model()
    net.eval()
    rm = net.residual_model
    assert net.update(force=True)
    residual = g["x"] - g["jpeg_decoded"]
    with torch.no_grad():
        c = rm.compress(residual)
    orc, _ = oracle_from(recipe_state_dict())
    torch.set_num_threads(16)
    want, inter = reference_compress(orc, residual, rm.gaussian_conditional.scale_table.cpu().numpy())
    assert tuple(c["shape"]) == tuple(inter["z"].shape[-2:])
    for name, a, b in (("anchor", c["strings"][0][0], want[0][0]), ("non_anchor", c["strings"][0][1], want[0][1]),
                       ("z", c["strings"][1], want[1])):
        assert len(a) == len(b) == residual.shape[0], name
        for i, (sa, sb) in enumerate(zip(a, b)):
            assert sa == sb, (name, i, len(sa), len(sb))
    assert np.array_equal(rm.gaussian_conditional._quantized_cdf.cpu().numpy(), inter["gc_tables"][0])


# ------------------------------------------------------------------------------------------------ AMP
AMP_CASES = [(2, 64, 64, 16, 16, 3, 1, 1, 1), (2, 128, 192, 16, 16, 5, 2, 2, 1), (2, 192, 96, 8, 8, 1, 1, 0, 1),
             (2, 64, 64, 16, 16, 3, 1, 2, 2), (2, 128, 128, 32, 32, 1, 1, 0, 1), (2, 192, 384, 8, 8, 5, 1, 2, 1),
             # odd spatial sizes, Co a multiple of 32 but not of 64 (partial N tiles in fwd and dgrad)
             (2, 96, 96, 20, 20, 3, 1, 1, 1), (3, 64, 96, 36, 12, 3, 1, 1, 1), (1, 128, 128, 48, 40, 3, 1, 2, 2),
             # rows a multiple of 32 pixels: the f16 halo-staged weight gradient (3x3, dilated 3x3, 5x5 s2;
             # Co = 96: a partial second M tile)
             (2, 64, 64, 32, 32, 3, 1, 1, 1), (2, 64, 96, 32, 64, 3, 1, 2, 2), (2, 64, 96, 64, 64, 5, 2, 2, 1),
             # W a multiple of 64, Co of 64: the halo-staged f16 3x3 conv (conv3x3_halo_f16_kernel) in the forward
             # and (Ci = 64 / 128) the input gradient; H = 10 leaves a partial 4-row tile, Ci = 96 three chunks
             (2, 64, 64, 16, 64, 3, 1, 1, 1), (1, 96, 128, 10, 128, 3, 1, 1, 1), (2, 128, 64, 8, 64, 3, 1, 1, 1),
             # Ci = 64 with >= 2 tiles per CU: the weight-resident persistent kernel (conv3x3_wres_f16_kernel), one
             # and two 64-channel output groups, a partial last row tile
             (4, 64, 64, 128, 256, 3, 1, 1, 1), (2, 64, 128, 128, 256, 3, 1, 1, 1), (4, 64, 64, 126, 256, 3, 1, 1, 1),
             # >= 65536 pixels, 1x1: the streaming 1x1 kernel on fp16-rounded operands
             (4, 64, 128, 128, 128, 1, 1, 0, 1), (4, 128, 64, 128, 128, 1, 1, 0, 1),
             # conv3x3_wres_f16_kernel's ragged tile walk: 372 tiles (372 % 8 = 4, H % 4 = 2) over 2 channel groups x
             # 128 blocks, 2 or 3 tiles per block (last, so that the ids above keep their cases)
             (3, 64, 128, 122, 256, 3, 1, 1, 1)]


@pytest.mark.parametrize("case", AMP_CASES)
def test_conv2d_amp_fwd_bwd(case):
    """train.sh --mixed-precision: a conv recorded on the tape under torch.autocast(float16) takes fp16
    operands on the f16 MFMA for the forward, the input gradient AND the weight gradient (fp32 accumulation,
    fp32 bias sums).  Against torch fp32 on the fp16-rounded operands: y = conv(x_h, w_h) + b,
    dx = conv^T(gy_h, w_h), dw = sum gy_h x_h, db = sum gy (only the summation order differs: 1e-5)."""
    from hyres_hip import ops as O
    B, Ci, Co, H, W, K, s, p, d = case
    halo16 = {(2, 64, 64, 32, 32, 3, 1, 1, 1): "1, 3, 1, 1", (2, 64, 96, 32, 64, 3, 1, 2, 2): "3, 3, 1, 2",
              (2, 64, 96, 64, 64, 5, 2, 2, 1): "1, 5, 2, 1"}
    if case in halo16:
        _assert_wgrad_kernel(rf"wgrad_halo_f16_kernel<{halo16[case]}, \d, 1>", "hyres_wgrad_desc_conv2d", B, H, W, Ci,
                             Ci, Co, Co, K, K, s, p, d, f16=True)
    x = _rand((B, Ci, H, W), 41)
    w = _rand((Co, Ci, K, K), 42, 1.0 / (Ci * K * K) ** 0.5)
    b = _rand((Co,), 43, 0.1)
    xh, wh = x.half().float(), w.half().float()
    yr = F.conv2d(xh, wh, b, stride=s, padding=p, dilation=d)
    gy = _rand(yr.shape, 44)
    gyh = gy.half().float()
    xr, wr = xh.clone().requires_grad_(), wh.clone().requires_grad_()
    F.conv2d(xr, wr, None, stride=s, padding=p, dilation=d).backward(gyh)
    D = dev()
    wd = torch.nn.Parameter(w.to(D))
    bd = torch.nn.Parameter(b.to(D))
    tape = O.Tape()
    xn = O.to_nhwc(x.to(D), rg=True)
    with torch.autocast("cuda", dtype=torch.float16):
        yn = O.conv2d(tape, xn, wd, bd, stride=s, pad=p, dil=d)
    y = O.to_nchw(yn)
    yn.set_grad(O.nchw_grad_to_nhwc(gy.to(D)))
    tape.backward()
    torch.cuda.synchronize()
    assert rel_err(y.cpu(), yr) < 1e-5
    assert rel_err(O.to_nchw_grad(xn).cpu(), xr.grad) < 1e-5
    assert rel_err(wd.grad.cpu(), wr.grad) < 1e-5
    assert rel_err(bd.grad.cpu(), gy.sum((0, 2, 3))) < 1e-5


@pytest.mark.parametrize("hw", [8, 32])
def test_deconv2d_amp_fwd_bwd(hw):
    """Transposed conv (compressai deconv, 4 sub-pixel phases) under autocast: f16 forward, dgrad, wgrad
    (hw = 32: rows of 32 pixels, the f16 halo-staged weight gradient)."""
    from hyres_hip import ops as O
    B, Ci, Co, H, W = 2, 128, 128, hw, hw
    if hw == 32:
        _assert_wgrad_kernel(r"wgrad_halo_f16_kernel<1, 5, 2, 1, \d, 1>", "hyres_wgrad_desc_deconv2d", B, H, W, Ci, Ci,
                             Co, Co, 5, 2, f16=True)
    x = _rand((B, Ci, H, W), 45)
    w = _rand((Ci, Co, 5, 5), 46, 1.0 / (Ci * 25 / 4) ** 0.5)
    b = _rand((Co,), 47, 0.1)
    xh, wh = x.half().float(), w.half().float()
    yr = F.conv_transpose2d(xh, wh, b, stride=2, padding=2, output_padding=1)
    gy = _rand(yr.shape, 48)
    xr, wr = xh.clone().requires_grad_(), wh.clone().requires_grad_()
    F.conv_transpose2d(xr, wr, None, stride=2, padding=2, output_padding=1).backward(gy.half().float())
    D = dev()
    wd, bd = torch.nn.Parameter(w.to(D)), torch.nn.Parameter(b.to(D))
    tape = O.Tape()
    xn = O.to_nhwc(x.to(D), rg=True)
    with torch.autocast("cuda", dtype=torch.float16):
        yn = O.deconv2d(tape, xn, wd, bd)
    yn.set_grad(O.nchw_grad_to_nhwc(gy.to(D)))
    tape.backward()
    torch.cuda.synchronize()
    assert rel_err(O.to_nchw(yn).cpu(), yr) < 1e-5
    assert rel_err(O.to_nchw_grad(xn).cpu(), xr.grad) < 1e-5
    assert rel_err(wd.grad.cpu(), wr.grad) < 1e-5


def test_amp_train_step_vs_fp32():
    """The whole train step under autocast (noisequant=True fixture: no round() decisions to flip) against
    this build's fp32 HIP step, which is pinned to the reference: the reference's own AMP run needs CUDA, so
    parity with it is unpinned.  fp16 operands (2^-11 relative rounding) through ~150 convolutions, loss
    scaled by 2^16 as the GradScaler does: loss within 1e-3 relative (measured 4e-6); the whole flat gradient
    within 8e-2 relative in 2-norm (measured 3.7e-2); every weight / bias gradient within 0.15 in relative
    Frobenius norm (measured 0.068 worst: AttentionBlock conv_b gradients pass through sigmoid'(b) * a and
    cancel) — PReLU slopes, sums of cancelling g*x, excluded; x_hat PSNR within 0.05 dB.  Each f16 kernel is
    checked exactly (1e-5 against the fp16-rounded operands) in test_conv2d_amp_fwd_bwd."""
    import json
    import math
    import os
    from conftest import GOLDEN
    g = load_npz("hyres_train_nq_b2_64.npz")
    with open(os.path.join(GOLDEN, "hyres_train_nq_b2_64.json")) as f:
        meta = json.load(f)
    D = dev()
    from hyres_hip.loss import RateDistortionLoss
    res = {}
    for amp in (False, True):
        net, _ = _hip_model()
        net.train()
        net.residual_model.noise.injected = _nhwc_noise(g, NQ_KEYS, D)
        ctx = torch.autocast("cuda", dtype=torch.float16) if amp else torch.autocast("cuda", enabled=False)
        with ctx:
            out = net(g["x"], noisequant=True, jpeg=(g["jpeg_decoded"], float(g["jpeg_bpp"])))
            crit = RateDistortionLoss(lmbda=meta["lambda"], alpha=0)(out, g["x"].to(D))
        S = 65536.0 if amp else 1.0  # the GradScaler's initial scale (engine.py:23)
        (crit["loss"] * S).backward()
        torch.cuda.synchronize()
        grads = {k: p.grad.detach().double().cpu() / S for k, p in net.named_parameters() if p.grad is not None}
        res[amp] = (float(crit["loss"]), out["x_hat"].detach().cpu(), grads)
    l32, x32, g32 = res[False]
    l16, x16, g16 = res[True]
    assert abs(l16 - l32) <= 1e-3 * abs(l32), (l16, l32)
    psnr = lambda a: 10 * math.log10(1.0 / float(F.mse_loss(a.double(), g["x"].double())))  # noqa: E731
    assert abs(psnr(x16) - psnr(x32)) < 0.05
    worst, fro = [], []
    for k, r in g32.items():
        sc = float(r.abs().max())
        if sc > 0 and not k.endswith(("act_in.weight", ".1.weight", ".3.weight")):  # PReLU slopes: cancelled sums
            worst.append((float((g16[k] - r).abs().max()) / sc, k))
            fro.append((float((g16[k] - r).norm() / r.norm()), k))
    worst.sort(reverse=True)
    fro.sort(reverse=True)
    keys = [k for _, k in fro]
    flat16 = torch.cat([g16[k].flatten() for k in keys])
    flat32 = torch.cat([g32[k].flatten() for k in keys])
    glob = float((flat16 - flat32).norm() / flat32.norm())
    print("AMP vs fp32: loss", l16, l32, "global", glob, "worst max-norm", worst[:4], "worst frobenius", fro[:4])
    assert glob < 8e-2, glob
    assert fro[0][0] < 0.15, fro[:4]
    assert not torch.equal(x16, x32), "fp16 operand path did not engage"


# per-tensor direction / distance of the AMP train-step gradients from this build's fp32 ones (2x the worst measured)
# AMP vs this build's fp32, per gradient tensor (test_amp_matches_reference_autocast_fixture). Measured round 5 over
# 251 tensors (2 x 64^2, noisequant=False: fp16 rounding moves round(y - mu) decisions, so the gradients of the
# layers around the quantiser differ by more than rounding): worst 1 - cos 0.131 / normwise 0.510 (g_a.0.weight),
# median 0.0175 / 0.200, 90th percentile 0.044 / 0.302. Bars ~1.5x those: a tensor with a wrong sign pattern
# (1 - cos ~ 1) cannot pass, a scale error is caught by the norm check against the reference AMP (0.25), and a
# systematic drift of the whole model by the median / 90th-percentile bars
AMP_COS_GAP = 0.2
AMP_NORMWISE = 0.75
AMP_NORMWISE_MEDIAN = 0.3
AMP_NORMWISE_P90 = 0.45


def test_amp_matches_reference_autocast_fixture():
    """The AMP path (train.sh:19 ``--mixed-precision``; engine.py:32 forward + criterion under autocast) against
    the REFERENCE's own autocast run (tests/golden/make_golden.py ``amp_fixtures``: the reference under
    ``torch.autocast("cpu", float16)`` — the op lists that differ from CUDA's are stated there).  Eval forward:
    x_hat PSNR within 0.01 dB of the reference's AMP x_hat, y/z bits within 1 %, round() flips of y_hat counted
    and bounded.  Train step (noisequant=False, the fixture's recorded EB / GC noise injected): loss, mse and
    bpp terms within 1e-3 relative; the whole-model gradient norm within 5 % and the median per-tensor norm
    within 5 % — the size of the reference's OWN AMP-vs-fp32 gap (3.1 % global, 1.7 % median: fp16 rounding
    points differ between any two AMP implementations; measured here 3.0 % / 1.8 %). Per tensor, with this build's
    fp32 step on the same inputs as the yardstick: within 0.25 of the reference AMP unless the reference AMP is
    itself further than that from fp32 (then no further from fp32 than it); the PReLU slopes, each one cancelled
    sum, within 0.5 of fp32; sampled elements' sign disagreements counted once and only where fp32 sides with
    the reference."""
    import json
    import math
    import os
    from conftest import GOLDEN
    from hyres_hip.loss import RateDistortionLoss
    g = load_npz("hyres_amp_b2_64.npz")
    with open(os.path.join(GOLDEN, "hyres_amp_b2_64.json")) as f:
        meta = json.load(f)
    D = dev()
    x = g["x"]
    jpeg = (g["jpeg_decoded"], float(g["jpeg_bpp"]))

    def psnr(a):
        return 10 * math.log10(1.0 / float(F.mse_loss(a.double().cpu(), x.double())))

    def bits(lik):
        return float((-torch.log2(lik.double())).sum())

    net, _ = _hip_model()
    net.eval()
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
        out = net(x, jpeg=jpeg)
    torch.cuda.synchronize()
    dp = psnr(out["x_hat"]) - psnr(g["eval_x_hat"])
    ly, lz = out["likelihoods"]["y"].cpu(), out["likelihoods"]["z"].cpu()
    # a round(y - mu) decision flip moves that element's likelihood by O(1); fp16 rounding of the scales
    # alone moves likelihoods by ~1 % (counted separately, reported)
    dly = (ly.double() - g["eval_y_likelihoods"].double()).abs()
    flips = int((dly > 0.5 * g["eval_y_likelihoods"].double().clamp_min(1e-3)).sum())
    moved = int((dly > 1e-2 * g["eval_y_likelihoods"].double()).sum())
    by, bz = bits(ly) / bits(g["eval_y_likelihoods"]) - 1, bits(lz) / bits(g["eval_z_likelihoods"]) - 1
    print(f"AMP eval vs reference AMP: dPSNR {dp:.5f} dB, y bits {by:.2e}, z bits {bz:.2e}, "
          f"y flips {flips} (moved > 1 %: {moved}) of {ly.numel()}")
    eval_ok = abs(dp) < 0.01 and abs(by) < 0.01 and abs(bz) < 0.01 and flips <= 0.005 * ly.numel()

    net, _ = _hip_model()
    net.train()
    net.residual_model.noise.injected = {"z": g["noise_z"].permute(0, 2, 3, 1).contiguous().to(D),
                                         "y": g["noise_y"].permute(0, 2, 3, 1).contiguous().to(D)}
    with torch.autocast("cuda", dtype=torch.float16):
        out = net(x, noisequant=False, jpeg=jpeg)
        crit = RateDistortionLoss(lmbda=meta["lambda"], alpha=0)(out, x.to(D))
    crit["loss"].backward()
    torch.cuda.synchronize()
    terms = []
    for k, ref in (("loss", "loss"), ("mse_loss", "mse_loss"), ("y_bpp_loss", "y_bpp"), ("z_bpp_loss", "z_bpp")):
        v, r = float(crit[k].detach()), float(g[ref])
        print(f"AMP train {k}: {v:.6f} vs reference AMP {r:.6f}")
        terms.append(abs(v - r) <= 1e-3 * abs(r))
    amp = {n: p.grad.detach().double().cpu().reshape(-1) for n, p in net.named_parameters() if p.grad is not None}
    # the same step in fp32 on this build (pinned to the reference's fp32 fixtures and to the fp64 oracle): the
    # yardstick for how far EITHER AMP run is from exact arithmetic on these inputs
    net, _ = _hip_model()
    net.train()
    net.residual_model.noise.injected = {"z": g["noise_z"].permute(0, 2, 3, 1).contiguous().to(D),
                                         "y": g["noise_y"].permute(0, 2, 3, 1).contiguous().to(D)}
    out = net(x, noisequant=False, jpeg=jpeg)
    RateDistortionLoss(lmbda=meta["lambda"], alpha=0)(out, x.to(D))["loss"].backward()
    torch.cuda.synchronize()
    f32 = {n: p.grad.detach().double().cpu().reshape(-1) for n, p in net.named_parameters() if p.grad is not None}
    rel, tot_h, tot_r, own = [], 0.0, 0.0, {}
    for n, gh in amp.items():
        s = meta["train_grads"].get(n)
        if s is None:
            continue
        nh, nr, n32 = float(gh.norm()), math.sqrt(s["sumsq"]), float(f32[n].norm())
        tot_h += nh * nh
        tot_r += s["sumsq"]
        if s["sumsq"] > 0 and n32 > 0:
            rel.append((abs(nh - nr) / nr, n))
            # each AMP run's own distance from fp32 (norms; the reference's tensor is known by its norm)
            own[n] = (abs(nh - n32) / n32, abs(nr - n32) / n32)
    rel.sort(reverse=True)
    glob = abs(math.sqrt(tot_h) / math.sqrt(tot_r) - 1)
    med = rel[len(rel) // 2][0]
    print(f"AMP train gradient norms vs reference AMP: global {glob:.3e}, median {med:.3e}, worst {rel[:3]}")
    print("  the same tensors, distance from this build's fp32 step (this AMP, reference AMP):",
          [(n, "%.3f" % own[n][0], "%.3f" % own[n][1]) for _, n in rel[:6]])
    # direction, not only size: per tensor, the sum (|d sum| against sqrt(numel) * the reference
    # norm, the Cauchy-Schwarz scale of a normwise error) and the 8 sampled elements the fixture holds (|d val|
    # against the tensor's absmax; a sign disagreement counts only where the reference value is not tiny)
    dsum, bad_sign, nsamp, dval, signs = [], 0, 0, [], []
    for n, gh in amp.items():
        s = meta["train_grads"].get(n)
        if s is None or s["sumsq"] <= 0:
            continue
        dsum.append((abs(float(gh.sum()) - s["sum"]) / (math.sqrt(gh.numel() * s["sumsq"])), n))
        for i, v in zip(s["idx"], s["val"]):
            h, h32 = float(gh[i]), float(f32[n][i])
            nsamp += 1
            dval.append((abs(h - v) / s["absmax"], n))
            if abs(v) > 0.05 * s["absmax"] and h * v < 0:
                bad_sign += 1
                signs.append((n, v, h, h32))
    dsum.sort(reverse=True)
    dval.sort(reverse=True)
    # a sign disagreement where fp32 sides with this AMP run is the reference AMP's own rounding, not a defect here
    ours_wrong = sum(1 for _, v, h, h32 in signs if h * h32 < 0)
    print(f"AMP per-tensor sums (scaled): worst {dsum[:3]}; sampled elements: worst |d|/absmax {dval[:3]}, "
          f"median {dval[len(dval) // 2][0]:.3e}, sign disagreements {bad_sign} of {nsamp} "
          f"(fp32 disagrees with this AMP run on {ours_wrong} of them)")
    assert eval_ok and all(terms)
    assert glob < 0.05 and med < 0.05
    # worst single tensor: within 0.25 of the reference AMP, unless the reference AMP is itself further than that
    # from fp32 — then this run must be no further from fp32 than the reference AMP is (the PReLU slopes are
    # cancelled sums of g*x: fp16 rounding points decide them, see test_amp_train_step_vs_fp32)
    slopes = {f"{m}.weight" for m, mod in net.named_modules() if isinstance(mod, torch.nn.PReLU)}
    bad = [(e, n, own[n]) for e, n in rel if n not in slopes and e >= 0.25
           and not (own[n][1] >= 0.25 and own[n][0] <= own[n][1])]
    assert not bad, bad[:3]
    # PReLU slopes: each ONE cancelled sum of g*x over a whole activation (both AMP runs are far from fp32 on some:
    # the reference AMP 3.9x on refine.act_in, measured round 4) — this run within 0.5 of fp32, or no further from
    # fp32 than the reference AMP (the rule of every other tensor above). refine.act_in moves with the last bits of
    # the refine's 64->3 output: 0.354 with conv_narrow_kernel, 1.10 with conv_narrow_strip_kernel (same fp32
    # products, another summation order; both within 1e-5 of fp64), against the reference AMP's 3.86
    # (profiles/r5_ampfix_act_in_slope.log). Fixed bars, independent of the kernel that happens to run: refine.act_in
    # <= 1.5 (the reference AMP run itself is 3.86 from fp32 there), every other slope < 0.5
    sl = [(own[n][0], n, own[n][1]) for n in slopes if n in own]
    print("PReLU slopes, distance from fp32 (this AMP, reference AMP):", sorted(sl, reverse=True))
    assert any(n == "refine.act_in.weight" for _, n, _ in sl), sorted(slopes)
    assert all(e <= (1.5 if n == "refine.act_in.weight" else 0.5) for e, n, _ in sl), sl
    wrong = {(n, v) for n, v, h, h32 in signs if n not in slopes and h * h32 < 0}
    assert dval[len(dval) // 2][0] < 0.05 and len(wrong) <= max(2, nsamp // 100), (dval[:5], sorted(wrong)[:5])
    # every other tensor, whole, against this build's fp32 gradient (itself pinned to the reference's fp32 fixtures and
    # the fp64 oracle): direction (1 - cosine) and normwise distance, worst tensor and the bulk (AMP_* above)
    dirn = []
    for n, gh in amp.items():
        b32 = f32.get(n)
        if n in slopes or b32 is None or float(b32.norm()) == 0.0:
            continue
        nb = float(b32.norm())
        cos = float(gh @ b32) / max(float(gh.norm()) * nb, 1e-300)
        dirn.append((1.0 - cos, float((gh - b32).norm()) / nb, n))
    dirn.sort(reverse=True)
    nw = sorted(r for _, r, _ in dirn)
    cg = sorted(c for c, _, _ in dirn)
    pct = {q: (cg[int(q * (len(cg) - 1))], nw[int(q * (len(nw) - 1))]) for q in (0.5, 0.9)}
    print("AMP vs this build's fp32, per tensor: worst 1-cos", [("%.2e" % c, "%.3f" % r, n) for c, r, n in dirn[:4]],
          "worst normwise", sorted(((r, n) for _, r, n in dirn), reverse=True)[:3],
          "(1-cos, normwise) median %.2e %.3f, 90th percentile %.2e %.3f of %d tensors"
          % (pct[0.5][0], pct[0.5][1], pct[0.9][0], pct[0.9][1], len(dirn)))
    assert all(c <= AMP_COS_GAP and r <= AMP_NORMWISE for c, r, _ in dirn), dirn[:3]
    assert pct[0.5][1] <= AMP_NORMWISE_MEDIAN and pct[0.9][1] <= AMP_NORMWISE_P90, pct


@pytest.mark.parametrize("K,Ci,Co,H", [(3, 64, 64, 128), (1, 128, 64, 128), (1, 64, 128, 128)])
def test_wgrad_many_split_reduce_deterministic(K, Ci, Co, H):
    """Weight + bias gradients at bs 16 (hundreds of split-K slabs and the fused bias partials, reduced by
    wgrad_bias_reduce_kernel) against torch fp32 (1e-5), and bit-identical across two runs (the split reduce
    sums in a fixed order: no atomics)."""
    import ctypes
    from hyres_hip import _lib as L
    D = dev()
    B = 16
    x = _rand((B, H, H, Ci), 71).to(D)
    gy = _rand((B, H, H, Co), 72).to(D)
    d = L.WgradDesc()
    L.call("hyres_wgrad_desc_conv2d", ctypes.byref(d), B, H, H, Ci, Ci, Co, Co, K, K, 1, K // 2, 1)
    d.sm = Ci * K * K
    nb = L.load().hyres_wgrad_workspace_bytes(ctypes.byref(d))
    ws = torch.empty(nb // 4 + 16, device=D)
    outs = []
    for _ in range(2):
        dw = torch.zeros(Co, Ci, K, K, device=D)
        db = torch.zeros(Co, device=D)
        L.call("hyres_conv_wgrad", ctypes.byref(d), gy.data_ptr(), x.data_ptr(), dw.data_ptr(), db.data_ptr(),
               ws.data_ptr(), nb, L.stream())
        torch.cuda.synchronize()
        outs.append((dw.clone(), db.clone()))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    xr = x.cpu().permute(0, 3, 1, 2).contiguous().requires_grad_(False)
    gyr = gy.cpu().permute(0, 3, 1, 2).contiguous()
    wr = torch.zeros(Co, Ci, K, K, requires_grad=True)
    F.conv2d(xr, wr, None, padding=K // 2).backward(gyr)
    assert rel_err(outs[0][0].cpu(), wr.grad) < 1e-5
    assert rel_err(outs[0][1].cpu(), gyr.sum((0, 2, 3))) < 1e-5
