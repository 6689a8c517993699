"""Per-kernel fp64 parity of the MultiScaleRefine kernels (csrc/refine.hip) at ragged shapes.

Every case calls an entry point directly through ``_lib.call`` (so ``ld``, pointer offsets, accumulate flags and dtype
masks are the test's), compares with the fp64 references of tests/refine_ref.py computed from the same (for fp16: the
fp16-rounded) inputs, and names in its id the kernel it is meant to reach.  That name is DERIVED here from the host
predicates of refine.hip (C % 4, ld % 4, pointer alignment, 256 % (C / 4), C == 192, exact 2x / 4x down-sampling,
se_chunks(HW), the grid caps); the library has no query for these routes, so a changed predicate shows as a failed
comparison, not as a failed name.

Every output lives inside a larger buffer filled with a sentinel (for ``ld > C`` the columns outside the slice too), the
workspaces are guarded the same way at exactly the size the library's ``*_workspace_bytes`` functions ask for, and
after each call every sentinel must be unchanged.

Bars (max-norm, helpers.rel_err): 1e-6 for the few-operation fp32 kernels (bilinear forward, SE scale, SA multiply,
sa_bwd_x, se_bwd_x: at most ~6 roundings of O(1) values).  Where such a kernel consumes a reduction of the same launch
(the SE gate, the attention map, the pooled gradients), the 1e-6 check is made on the kernel's own arithmetic, with the
reduction's device result as its operand, and the end-to-end result is checked at the reductions' bar.  1e-4 for fp32
reductions and gathers (test_parity_gpu.TOL), 1e-3 for d slope (a cancelled sum; the existing fold tests' bar).  fp16
storage: 2^-11 (one rounding of the stored result) plus the fp32 bar; 2e-3 (the AMP bar) where fp16 gradients feed a
reduction.  Argmax, exact-down against the general gather and sentinels are compared exactly.

The 32-bit index guards (n / 4 < 2^31, B * Ho <= 65535, Wo * C < 2^30) cannot be reached at test sizes and are left
untested."""
import ctypes
import functools

import pytest
import torch

import refine_ref as RR
from helpers import rel_err

pytestmark = pytest.mark.gpu

TOL = 1e-4          # fp32 reductions and gathers
TOL_POINT = 1e-6    # few-operation fp32 kernels
TOL_SLOPE = 1e-3
H16 = 2.0 ** -11    # one fp16 rounding of a stored result
TOL_AMP = 2e-3
SENT = -777.0       # exact in fp32, fp16 and int32
PAD = 64            # guard elements on each side (keeps the 256-byte alignment of the allocation)
DT_ACT16, DT_GRAD16 = 1, 2


def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def _L():
    from hyres_hip import _lib as L
    return L


class Buf:
    """``rows`` x ``C`` values at columns [c0, c0 + C) of rows of ``ld`` elements, ``off`` elements past an aligned
    address, inside a buffer of sentinels."""

    def __init__(self, rows, C, dtype=torch.float32, ld=None, c0=0, off=0):
        self.ld = ld or C
        n = rows * self.ld
        self.buf = torch.full((PAD + off + n + PAD,), SENT, dtype=dtype, device=dev())
        self.v = self.buf[PAD + off:PAD + off + n].view(rows, self.ld)[:, c0:c0 + C]
        assert self.buf.data_ptr() % 256 == 0

    def set(self, t):
        self.v.copy_(t.reshape(self.v.shape).to(self.v.device, self.v.dtype))
        return self

    @property
    def ptr(self):
        return self.v.data_ptr()

    def take(self):
        """The values, after checking that nothing outside them was written."""
        torch.cuda.synchronize()
        out = self.v.detach().cpu().clone()
        self.v.fill_(SENT)
        assert bool((self.buf == SENT).all()), "a sentinel outside the output was overwritten"
        return out

    def untouched(self):
        torch.cuda.synchronize()
        return bool((self.buf == SENT).all())


def _ws(nbytes):
    return Buf((int(nbytes) + 3) // 4, 1)


def _show(name, err, bar):
    print(f"{name}: {err:.3e} (bar {bar:.1e})")
    return err


def _check(name, got, ref, bar):
    assert _show(name, rel_err(got, ref), bar) < bar, name


# ======================================================================================================= bilinear
# storage variants: (C, ld, c0, off, accumulate); ld None = C
VARIANTS = {
    "C8": (8, None, 0, 0, 0),
    "C6": (6, None, 0, 0, 0),
    "C8-ld10": (8, 10, 0, 0, 0),
    "C8-misaligned": (8, None, 0, 1, 0),
    "C8-cols64of192": (8, 192, 64, 0, 0),
    "C8-acc": (8, None, 0, 0, 1),
    "C6-acc": (6, None, 0, 0, 1),
}


def _vec(v):
    C, ld, c0, off, _ = VARIANTS[v]
    return C % 4 == 0 and (ld or C) % 4 == 0 and off % 4 == 0 and c0 % 4 == 0


def _bwd_kernel(s, v):
    """hyres_bilinear_bwd's route (bilinear_bwd_impl)."""
    (hi, wi), (ho, wo), _, _ = s
    sh, sw = RR.scales_of(s)
    if not _vec(v):
        return "bilinear_bwd_kernel<1>"
    for S in (2, 4):
        if sh == S and sw == S and hi == S * ho and wi == S * wo:
            return f"bilinear_down_bwd_kernel<{S}>"
    return "bilinear_bwd_kernel<4>"


BIL_FWD = [pytest.param(s, v, id=f"{RR.shape_id(s)}/{v}/bilinear_fwd_kernel<{4 if _vec(v) else 1}>")
           for s in RR.BILINEAR_SHAPES for v in VARIANTS]
BIL_BWD = [pytest.param(s, v, id=f"{RR.shape_id(s)}/{v}/{_bwd_kernel(s, v)}")
           for s in RR.BILINEAR_SHAPES for v in VARIANTS]
BIL_B = 2


@functools.lru_cache(maxsize=None)
def _bil_case(s):
    """x, gy (8 channels; a 6-channel case takes the first 6: resampling is per channel), the accumulate targets and
    the fp64 references, computed once per shape."""
    (hi, wi), (ho, wo), _, _ = s
    sh, sw = RR.scales_of(s)
    x, gy = RR.rand((BIL_B, hi, wi, 8), 101), RR.rand((BIL_B, ho, wo, 8), 102)
    y0, gx0 = RR.rand((BIL_B, ho, wo, 8), 103), RR.rand((BIL_B, hi, wi, 8), 104)
    return dict(x=x, gy=gy, y0=y0, gx0=gx0, y=RR.bilinear_ref(x, ho, wo, sh, sw),
                gx=RR.bilinear_bwd_ref(gy, hi, wi, sh, sw))


def _run_bilinear(which, s, v, f16=0, src=None):
    """One hyres_bilinear_fwd / _bwd launch in storage variant ``v``: the output [B, H, W, C] (checked for stray
    writes) and the fp64 reference."""
    L = _L()
    (hi, wi), (ho, wo), _, _ = s
    sh, sw = RR.scales_of(s)
    C, ld, c0, off, acc = VARIANTS[v]
    k = _bil_case(s)
    dt = torch.float16 if f16 else torch.float32
    fwd = which == "fwd"
    (ri, ro) = (hi * wi, ho * wo) if fwd else (ho * wo, hi * wi)
    inp = (k["x"] if fwd else k["gy"])[..., :C] if src is None else src
    tgt0 = (k["y0"] if fwd else k["gx0"])[..., :C]
    a = Buf(BIL_B * ri, C, dt, ld, c0, off).set(inp)
    o = Buf(BIL_B * ro, C, dt, ld, c0, off)
    if acc:
        o.set(tgt0)
    L.call("hyres_bilinear_fwd" if fwd else "hyres_bilinear_bwd", a.ptr, a.ld, o.ptr, o.ld, BIL_B, hi, wi, ho, wo, C,
           sh, sw, acc, f16, L.stream())
    out = o.take().view(BIL_B, *((ho, wo) if fwd else (hi, wi)), C)
    if f16:
        h = inp.half()
        ref = RR.bilinear_ref(h, ho, wo, sh, sw) if fwd else RR.bilinear_bwd_ref(h, hi, wi, sh, sw)
    else:
        ref = (k["y"] if fwd else k["gx"])[..., :C]
    return out, (ref + tgt0.double() if acc else ref)


@pytest.mark.parametrize("s,v", BIL_FWD)
def test_bilinear_fwd(s, v):
    """The compiled kernel forms the source index scale * (o + 0.5) - 0.5 as one fused multiply-add (one rounding);
    the reference rounds the product and the difference separately, as torch does on the CPU.  At 13x9 -> 5x7 (scale
    2.6, source indices up to 11) that alone moves the result by 6.8e-7 of its maximum (computed on the CPU from the two
    index rules); the kernel measures 7.0e-7 there and at most 1e-7 where the index is exact."""
    out, ref = _run_bilinear("fwd", s, v)
    _check("bilinear_fwd", out, ref, TOL_POINT)


@pytest.mark.parametrize("s,v", BIL_BWD)
def test_bilinear_bwd(s, v):
    """The general gather (bw_range / bw_weight) at non-integer scales, at scale 2 on an odd height (13 -> 6 must not
    take the exact-down kernel), the exact 2x / 4x kernels, strided slices and accumulate, against the transpose of the
    reference's weight matrices.  (bw_range keeps one output of slack below floor(v) + 1, the first output whose
    stencil can touch the pixel: moving lo up to that bound drops weights of at most 4e-6 over every size up to 71 in
    both scale conventions, so no comparison at these bars can, or should, tell the two apart.)"""
    out, ref = _run_bilinear("bwd", s, v)
    _check("bilinear_bwd", out, ref, TOL)


@pytest.mark.parametrize("s", [RR.BILINEAR_SHAPES[3], RR.BILINEAR_SHAPES[4]], ids=RR.shape_id)
def test_bilinear_exact_down_bwd_equals_general_gather_bitwise(s):
    """bilinear_down_bwd_kernel<S> (aligned) against bilinear_bwd_kernel<1> (the same data one float off alignment):
    the kernel's comment promises the same fp32 result."""
    assert _bwd_kernel(s, "C8").startswith("bilinear_down") and _bwd_kernel(s, "C8-misaligned") == "bilinear_bwd_kernel<1>"
    exact, _ = _run_bilinear("bwd", s, "C8")
    general, _ = _run_bilinear("bwd", s, "C8-misaligned")
    assert torch.equal(exact, general)
    assert int((exact != 0).sum()) > 0


F16_SHAPES = [RR.BILINEAR_SHAPES[1], RR.BILINEAR_SHAPES[3]]


@pytest.mark.parametrize("s", F16_SHAPES, ids=[RR.shape_id(s) + "/bilinear_fwd_kernel<4,H>" for s in F16_SHAPES])
def test_bilinear_fwd_f16(s):
    out, ref = _run_bilinear("fwd", s, "C8", f16=1)
    _check("bilinear_fwd f16", out, ref, H16 + TOL_POINT)


@pytest.mark.parametrize("s", F16_SHAPES, ids=[RR.shape_id(s) + "/" + _bwd_kernel(s, "C8").replace(">", ",G>")
                                               for s in F16_SHAPES])
def test_bilinear_bwd_f16(s):
    """fp16 gy and gx; the reference gathers the fp16-rounded gy, so the stored result's rounding is the only addition
    to the fp32 bar."""
    out, ref = _run_bilinear("bwd", s, "C8", f16=1)
    _check("bilinear_bwd f16", out, ref, H16 + TOL)


@pytest.mark.parametrize("v", ["C8-acc", "C6"])
def test_bilinear_fwd_f16_refusals(v):
    """fp16 with accumulate, and fp16 off the float4 path (C = 6): HipError, output untouched."""
    L = _L()
    C, _, _, _, acc = VARIANTS[v]
    x = Buf(BIL_B * 35, C, torch.float16).set(RR.rand((BIL_B * 35, C), 105))
    y = Buf(BIL_B * 117, C, torch.float16)
    with pytest.raises(L.HipError):
        L.call("hyres_bilinear_fwd", x.ptr, C, y.ptr, C, BIL_B, 5, 7, 13, 9, C, 5 / 13, 7 / 9, acc, 1, L.stream())
    assert y.untouched()


def _pre_with_zeros(shape, seed):
    pre = RR.rand(shape, seed)
    pre.view(-1)[::7] = 0.0
    assert bool((pre > 0).any()) and bool((pre < 0).any()) and bool((pre == 0).any())
    return pre


def _bilinear_bwd_prelu(B, hi, wi, ho, wo, C, sh, sw, dt):
    L = _L()
    gdt = torch.float16 if dt & DT_GRAD16 else torch.float32
    pdt = torch.float16 if dt & DT_ACT16 else torch.float32
    gy = RR.rand((B, ho, wo, C), 111).to(gdt)
    pre = _pre_with_zeros((B, hi, wi, C), 112).to(pdt)
    slope = torch.tensor([0.25])
    dslope0 = 0.625
    g = Buf(B * ho * wo, C, gdt).set(gy)
    p = Buf(B * hi * wi, C, pdt).set(pre)
    gx = Buf(B * hi * wi, C, gdt)
    ds = Buf(1, 1).set(torch.tensor([dslope0]))
    sl = slope.to(dev())
    ws = _ws(L.load().hyres_bilinear_bwd_prelu_workspace_bytes(B, hi, wi, C))
    L.call("hyres_bilinear_bwd_prelu", g.ptr, C, gx.ptr, C, B, hi, wi, ho, wo, C, sh, sw, p.ptr, C, sl.data_ptr(),
           ds.ptr, ws.ptr, ws.v.numel() * 4, dt, L.stream())
    ws.take()
    gi, dsl = RR.prelu_bwd_ref(pre, RR.bilinear_bwd_ref(gy, hi, wi, sh, sw), 0.25)
    g16 = bool(dt & DT_GRAD16)
    _check("gx", gx.take().view(B, hi, wi, C), gi, TOL_AMP if g16 else TOL)
    _check("dslope", ds.take().view(()), dsl + dslope0, TOL_AMP if g16 else TOL_SLOPE)


@pytest.mark.parametrize("s,dt", [(RR.PRELU_UP_SHAPES[0], 0), (RR.PRELU_UP_SHAPES[0], 1), (RR.PRELU_UP_SHAPES[0], 2),
                                  (RR.PRELU_UP_SHAPES[0], 3), (RR.PRELU_UP_SHAPES[1], 0)],
                         ids=lambda a: (RR.shape_id(a) if isinstance(a, tuple) else
                                        f"bilinear_bwd_kernel<4,G={a >> 1},PM={1 + (a & 1)}>+slope_sum8"))
def test_bilinear_bwd_prelu(s, dt):
    """The up-sample's gather with the producing PReLU's backward folded in, on a pre-activation with both signs and
    exact zeros, d slope added to a non-zero start; every mask of the two dtype bits."""
    (hi, wi), (ho, wo), _, _ = s
    sh, sw = RR.scales_of(s)
    _bilinear_bwd_prelu(2, hi, wi, ho, wo, 8, sh, sw, dt)


def test_bilinear_bwd_prelu_2100_partials_slope_sum8_tail():
    """B * Hi = 2100 one-block rows: sum_partials_kernel (the eight-in-flight order, reached through sum_partials8)
    folds one full pass of 2048 partials plus a ragged tail of 52."""
    _bilinear_bwd_prelu(3, 700, 4, 1400, 8, 4, 0.5, 0.5, 0)


# ======================================================================================================= SE block
def _se_chunks(HW):
    return max(1, min(64, (HW + 1023) // 1024))


def _se_kernels(B, HW, C, Cr, off=0):
    """hyres_se_fwd / hyres_se_bwd's routes in fp32."""
    al = off % 4 == 0
    pool4 = C % 4 == 0 and C <= 1024 and 256 % (C // 4) == 0 and al
    vec = C % 4 == 0 and al
    return (f"{'se_pool4' if pool4 else 'se_pool|se_bwd_pool'}(x{_se_chunks(HW)})+"
            f"{'se_scale4|se_bwd_x4' if vec else 'se_scale|se_bwd_x'}")


SE_CASES = [(2, 1500, 64, 4, 0), (2, 1025, 64, 4, 0), (3, 1, 64, 4, 0), (2, 3, 16, 1, 0), (2, 300, 48, 3, 0),
            (2, 300, 6, 1, 0), (2, 37, 4, 1, 0), (1, 5, 1024, 64, 0), (1, 5, 1028, 64, 0), (1, 66000, 4, 1, 0),
            (2, 300, 64, 4, 1),
            (2, 66000, 64, 4, 0)]  # n / 4 > 2048 * 1024: the grid-capped second pass of se_scale4 / se_bwd_x4


def _se_id(c):
    B, HW, C, Cr, off = c
    return f"{B}x{HW}x{C}r{Cr}{'-misaligned' if off else ''}/{_se_kernels(*c)}"


@functools.lru_cache(maxsize=2)
def _se_case(B, HW, C, Cr, half=False, prelu=False):
    """Inputs and the fp64 reference (autograd) of one SE case.  ``prelu``: x = PReLU(pre) and the gradients taken at
    pre.  w1's sign is chosen so that the first hidden unit is alive (with one or a few hidden units a dead ReLU would
    leave the weight gradients all zero)."""
    act = torch.float16 if half else torch.float32
    slope = 0.25
    pre = _pre_with_zeros((B, HW, C), 121).to(act) if prelu else None
    x = torch.where(pre > 0, pre, (slope * pre.float()).to(act)) if prelu else RR.rand((B, HW, C), 121).to(act)
    w1, w2 = RR.rand((Cr, C), 122, 4.0 / C ** 0.5), RR.rand((C, Cr), 123, 0.5)
    if float((x.double().mean(1) @ w1.double().t())[0, 0]) <= 0:
        w1 = -w1
    gy = RR.rand((B, HW, C), 124)
    xr = x.double().requires_grad_()
    w1r, w2r = w1.double().requires_grad_(), w2.double().requires_grad_()
    y, pooled, hidden, gate = RR.se_ref(xr, w1r, w2r)
    assert float(hidden.detach()[0, 0]) > 0
    return dict(x=x, pre=pre, w1=w1, w2=w2, gy=gy, slope=slope, xr=xr, w1r=w1r, w2r=w2r, y=y, pooled=pooled,
                hidden=hidden, gate=gate)


def _se_grads(k, gy):
    gx, g1, g2 = torch.autograd.grad(k["y"], (k["xr"], k["w1r"], k["w2r"]), gy.double(), retain_graph=True)
    return gx, g1, g2


def _run_se(c, dt=0, prelu=False, slope_bar=None):
    """hyres_se_fwd, then hyres_se_bwd (or hyres_se_bwd_prelu) on the forward's saved pooled / hidden / gate.
    ``slope_bar``: the bar on d slope when it is not the dtype's usual one."""
    L = _L()
    B, HW, C, Cr, off = c
    half, g16 = bool(dt & DT_ACT16), bool(dt & DT_GRAD16)
    act, gdt = (torch.float16 if half else torch.float32), (torch.float16 if g16 else torch.float32)
    k = _se_case(B, HW, C, Cr, half, prelu)
    D = dev()
    w1, w2 = k["w1"].to(D), k["w2"].to(D)
    x = Buf(B * HW, C, act, off=off).set(k["x"])
    y = Buf(B * HW, C, act, off=off)
    pooled, hidden, sgate = Buf(B, C), Buf(B, Cr), Buf(B, C)
    wsb = L.load().hyres_se_workspace_bytes(B, HW, C)
    ws = _ws(wsb)
    L.call("hyres_se_fwd", x.ptr, w1.data_ptr(), w2.data_ptr(), y.ptr, pooled.ptr, hidden.ptr, sgate.ptr, B, HW, C, Cr,
           ws.ptr, wsb, int(half), L.stream())
    ws.take()
    yv, pv, hv, sv = y.take().view(B, HW, C), pooled.take(), hidden.take(), sgate.take()
    h = H16 if half else 0.0
    _check("pooled", pv, k["pooled"].detach(), TOL)
    _check("hidden", hv, k["hidden"].detach(), TOL)
    _check("gate", sv, k["gate"].detach(), TOL)
    # the scale kernel's own arithmetic (x times the device gate), then end to end at the pool's bar
    _check("y | device gate", yv, k["x"].double() * sv.double()[:, None, :], h + TOL_POINT)
    _check("y", yv, k["y"].detach(), h + TOL)

    # backward: gw1 / gw2 (and d slope) are added to non-zero starts
    gy = k["gy"].to(gdt)
    gw10, gw20 = RR.rand((Cr, C), 125), RR.rand((C, Cr), 126)
    pooled.set(pv), hidden.set(hv), sgate.set(sv)
    g = Buf(B * HW, C, gdt, off=off).set(gy)
    gx = Buf(B * HW, C, gdt, off=off)
    gw1, gw2 = Buf(Cr, C).set(gw10), Buf(C, Cr).set(gw20)
    need = wsb + B * C * 4 + (2048 * 4 if prelu else 0)  # se_bwd_impl: the pool partials, g pooled, the slope partials
    ws = _ws(need)
    if prelu:
        p = Buf(B * HW, C, act).set(k["pre"])
        sl = torch.tensor([k["slope"]], device=D)
        ds = Buf(1, 1).set(torch.tensor([0.625]))
        L.call("hyres_se_bwd_prelu", x.ptr, g.ptr, w1.data_ptr(), w2.data_ptr(), pooled.ptr, hidden.ptr, sgate.ptr,
               gx.ptr, gw1.ptr, gw2.ptr, B, HW, C, Cr, p.ptr, sl.data_ptr(), ds.ptr, ws.ptr, need, dt, L.stream())
    else:
        L.call("hyres_se_bwd", x.ptr, g.ptr, w1.data_ptr(), w2.data_ptr(), pooled.ptr, hidden.ptr, sgate.ptr, gx.ptr,
               gw1.ptr, gw2.ptr, B, HW, C, Cr, ws.ptr, need, dt, L.stream())
    ws.take()
    gxr, g1r, g2r = _se_grads(k, gy)
    red = TOL_AMP if g16 else TOL
    _check("gw1", gw1.take(), g1r + gw10.double(), red)
    _check("gw2", gw2.take(), g2r + gw20.double(), red)
    gxv = gx.take().view(B, HW, C)
    if prelu:
        gi, dsl = RR.prelu_bwd_ref(k["pre"], gxr, k["slope"])
        _check("gx", gxv, gi, red)
        _check("dslope", ds.take().view(()), dsl + 0.625, slope_bar or (TOL_AMP if g16 else TOL_SLOPE))
        return
    _check("gx", gxv, gxr, red)
    if not g16:
        # se_bwd_x's own arithmetic: gx - gy * gate is g pooled[b][c], the same for every pixel
        r = gxv.double() - gy.double() * sv.double()[:, None, :]
        spread = float((r - r.mean(1, keepdim=True)).abs().max() / gxv.double().abs().max())
        assert _show("gx - gy * gate spread over pixels", spread, TOL_POINT) < TOL_POINT
        gpool = (gxr - gy.double() * k["gate"].detach()[:, None, :]).mean(1)
        _check("g pooled", r.mean(1), gpool, TOL)


@pytest.mark.parametrize("c", SE_CASES, ids=_se_id)
def test_se_fwd_bwd(c):
    """SEBlock forward and backward in fp32: pooling in one to 64 ragged chunks, the scalar and the float4 pool, scale
    and input-gradient kernels, weight gradients added to non-zero starts."""
    _run_se(c)


@pytest.mark.parametrize("dt", [DT_ACT16, DT_ACT16 | DT_GRAD16], ids=["act16", "act16-grad16"])
def test_se_fwd_bwd_f16(dt):
    _run_se((2, 1500, 64, 4, 0), dt)


@pytest.mark.parametrize("c,dt", [((2, 1500, 64, 4, 0), 0), ((2, 66000, 64, 4, 0), 0), ((2, 1500, 64, 4, 0), DT_ACT16),
                                  ((2, 1500, 64, 4, 0), DT_ACT16 | DT_GRAD16)],
                         ids=["2x1500x64/se_bwd_x4_prelu", "2x66000x64/se_bwd_x4_prelu-second-pass",
                              "2x1500x64-act16/se_bwd_x4_prelu<H>", "2x1500x64-act16-grad16/se_bwd_x4_prelu<H,G>"])
def test_se_bwd_prelu(c, dt):
    """hyres_se_bwd_prelu: the producing PReLU's backward on the input gradient, d slope added to a non-zero start; at
    2 x 66000 x 64 n / 4 exceeds 2048 x 1024 float4, so every thread makes a second pass. The kernel is
    se_bwd_x4_kernel<G, PRELU = true, H>; its partials are finished by sum_partials_serial_kernel."""
    _run_se(c, dt, prelu=True)


@pytest.mark.parametrize("dt", [0, DT_ACT16 | DT_GRAD16], ids=["fp32", "act16-grad16"])
def test_se_bwd_prelu_258_partials_serial_sum_tail(dt):
    """1 x (129 x 128) x 64: 264,192 float4 give 258 blocks of slope partials, so sum_partials_serial_kernel (one
    running sum per thread) makes one full pass of 256 and a ragged second pass of 2. d slope at TOL_SLOPE in both
    dtypes: the fp16 roundings of 1M gradients (2^-11 each, signs random) average far below it."""
    _run_se((1, 129 * 128, 64, 4, 0), dt, prelu=True, slope_bar=TOL_SLOPE)


def test_se_bwd_refuses_batch_beyond_lds():
    """B * (C + Cr) * 4 > 60000 bytes of LDS for se_fc_bwd_kernel: HipError before any launch."""
    L = _L()
    B, HW, C, Cr = 16, 1, 1024, 64
    D = dev()
    x, gy = Buf(B * HW, C).set(RR.rand((B, C), 131)), Buf(B * HW, C).set(RR.rand((B, C), 132))
    w1, w2 = RR.rand((Cr, C), 133).to(D), RR.rand((C, Cr), 134).to(D)
    pooled, hidden, sgate = (Buf(B, n).set(torch.rand(B, n)) for n in (C, Cr, C))
    gx, gw1, gw2 = Buf(B * HW, C), Buf(Cr, C), Buf(C, Cr)
    need = L.load().hyres_se_workspace_bytes(B, HW, C) + B * C * 4
    ws = _ws(need)
    with pytest.raises(L.HipError):
        L.call("hyres_se_bwd", x.ptr, gy.ptr, w1.data_ptr(), w2.data_ptr(), pooled.ptr, hidden.ptr, sgate.ptr, gx.ptr,
               gw1.ptr, gw2.ptr, B, HW, C, Cr, ws.ptr, need, 0, L.stream())
    assert gx.untouched() and gw1.untouched() and gw2.untouched() and ws.untouched()


# ======================================================================================================= SpatialAttention
SA_CASES = [((2, 1, 1), 4), ((2, 1, 1), 192), ((2, 5, 3), 20), ((2, 5, 3), 260), ((2, 16, 16), 64), ((2, 16, 16), 192),
            ((2, 17, 33), 20), ((2, 17, 33), 192), ((2, 17, 33), 256), ((1, 40, 48), 4), ((1, 40, 48), 64),
            ((1, 40, 48), 260), ((3, 17, 704), 4)]


def _sa_tiles(B, H, W):
    return B * ((H + 15) // 16) * ((W + 15) // 16)


def _sa_id(bhw, C):
    B, H, W = bhw
    return f"{B}x{H}x{W}xC{C}/sa_pool<NC={3 if C == 192 else 0}>+tiled7x7({_sa_tiles(B, H, W)} tiles)"


SA_PARAMS = [pytest.param(bhw, C, fam, id=f"{_sa_id(bhw, C)}/{fam}") for bhw, C in SA_CASES for fam in ("cont", "ties")]


@functools.lru_cache(maxsize=4)
def _sa_case(bhw, C, fam, half=False):
    B, H, W = bhw
    x = RR.rand((B, H, W, C), 141) if fam == "cont" else RR.tie_input((B, H, W, C), 141)
    if half:
        x = x.half()
    w = RR.rand((1, 2, 7, 7), 142, 0.3)
    xr, wr = x.double().requires_grad_(), w.double().requires_grad_()
    y, attn, pooled2, idx = RR.sa_ref(xr, wr)
    first = RR.first_argmax(x.double())
    assert torch.equal(idx, first)  # torch.max's tie rule (also checked on the CPU)
    return dict(x=x, w=w, xr=xr, wr=wr, y=y, attn=attn, pooled2=pooled2, idx=first.to(torch.int32),
                gy=RR.rand((B, H, W, C), 143), gw0=RR.rand((98,), 144))


def _sa_fwd(k, bhw, C, half, with_y=True):
    L = _L()
    B, H, W = bhw
    P = B * H * W
    act = torch.float16 if half else torch.float32
    x = Buf(P, C, act).set(k["x"])
    w = k["w"].to(dev())
    pooled2, amax, attn = Buf(P, 2), Buf(P, 1, torch.int32), Buf(P, 1)
    y = Buf(P, C, act) if with_y else None
    L.call("hyres_spatial_attn_fwd", x.ptr, w.data_ptr(), pooled2.ptr, amax.ptr, attn.ptr, y.ptr if with_y else None,
           B, H, W, C, int(half), L.stream())
    return (x, w, pooled2.take().view(B, H, W, 2), amax.take().view(B, H, W), attn.take().view(B, H, W),
            y.take().view(B, H, W, C) if with_y else None)


def _check_sa_fwd(k, bhw, C, half):
    _, _, p2, am, at, y = _sa_fwd(k, bhw, C, half)
    assert torch.equal(am, k["idx"]), "argmax: torch.max keeps the first maximal index"
    assert torch.equal(p2[..., 1].double(), k["pooled2"][..., 1].detach()), "the channel max is exact"
    _check("mean", p2[..., 0], k["pooled2"][..., 0].detach(), TOL)
    _check("attn", at, k["attn"].detach(), TOL)
    h = H16 if half else 0.0
    # sa_mul's own arithmetic on the device map, then end to end
    _check("y | device attn", y, k["x"].double() * at.double()[..., None], h + TOL_POINT)
    _check("y", y, k["y"].detach(), h + TOL)
    _, _, p2b, amb, atb, _ = _sa_fwd(k, bhw, C, half, with_y=False)  # the map alone (y NULL): the same bits
    assert torch.equal(p2b, p2) and torch.equal(amb, am) and torch.equal(atb, at)
    return p2, am, at


def _check_sa_bwd(k, bhw, C, dt):
    L = _L()
    B, H, W = bhw
    P = B * H * W
    half, g16 = bool(dt & DT_ACT16), bool(dt & DT_GRAD16)
    gdt = torch.float16 if g16 else torch.float32
    x, w, p2, am, at, _ = _sa_fwd(k, bhw, C, half)
    pooled2, amax, attn = Buf(P, 2).set(p2), Buf(P, 1, torch.int32).set(am), Buf(P, 1).set(at)
    gy = k["gy"].to(gdt)
    g, gx, gw = Buf(P, C, gdt).set(gy), Buf(P, C, gdt), Buf(98, 1).set(k["gw0"])
    wsb = L.load().hyres_spatial_attn_workspace_bytes(B, H, W)
    ws = _ws(wsb)
    L.call("hyres_spatial_attn_bwd", x.ptr, w.data_ptr(), pooled2.ptr, amax.ptr, attn.ptr, g.ptr, gx.ptr, gw.ptr, B, H,
           W, C, ws.ptr, wsb, dt, L.stream())
    ws.take()
    gxr, gwr = torch.autograd.grad(k["y"], (k["xr"], k["wr"]), gy.double(), retain_graph=True)
    red = TOL_AMP if g16 else TOL
    _check("gw", gw.take().view(-1), gwr.reshape(-1) + k["gw0"].double(), red)
    gxv = gx.take().view(B, H, W, C)
    _check("gx", gxv, gxr, red)
    if g16:
        return
    # sa_bwd_x's own arithmetic: gx - gy * attn is g_avg / C on every channel but the argmax, which alone adds g_max
    r = gxv.double() - gy.double() * at.double()[..., None]
    hot = torch.zeros_like(r, dtype=torch.bool).scatter_(-1, k["idx"].long()[..., None], True)
    scale = float(gxv.double().abs().max())
    if C > 1:
        cold = r.masked_fill(hot, float("nan"))
        base = cold.nanmean(-1, keepdim=True)
        spread = float((cold - base).abs().nan_to_num(0.0).max() / scale)
        assert _show("gx - gy * attn spread off the argmax", spread, TOL_POINT) < TOL_POINT
        rr = gxr - gy.double() * k["attn"].detach()[..., None]
        gmax_ref = (rr - rr.masked_fill(hot, float("nan")).nanmean(-1, keepdim=True))[hot]
        _check("g_max on the argmax channel", (r - base)[hot], gmax_ref, TOL)


@pytest.mark.parametrize("bhw,C,fam", SA_PARAMS)
def test_spatial_attn_fwd(bhw, C, fam):
    """Channel mean / max / first argmax, the tiled 7x7 and the multiply: images smaller than the filter, one-pixel
    partial tiles, 264 tiles, C below and off a multiple of 64 (lanes without data), the C == 192 build; with y and
    with y NULL (the map alone)."""
    _check_sa_fwd(_sa_case(bhw, C, fam), bhw, C, False)


@pytest.mark.parametrize("bhw,C,fam", SA_PARAMS)
def test_spatial_attn_bwd(bhw, C, fam):
    """gx routes g_max to the first maximal channel only; gw is added to a non-zero start; 264 tiles run
    sum_partials_cols_kernel's loop (the strided column sum, stride 98) into a second pass."""
    _check_sa_bwd(_sa_case(bhw, C, fam), bhw, C, 0)


@pytest.mark.parametrize("C", [192, 20])
@pytest.mark.parametrize("fam", ["cont", "ties"])
def test_spatial_attn_fwd_f16(C, fam):
    _check_sa_fwd(_sa_case((2, 17, 33), C, fam, True), (2, 17, 33), C, True)


@pytest.mark.parametrize("C", [192, 20])
@pytest.mark.parametrize("dt", [DT_ACT16, DT_ACT16 | DT_GRAD16], ids=["act16", "act16-grad16"])
def test_spatial_attn_bwd_f16(C, dt):
    _check_sa_bwd(_sa_case((2, 17, 33), C, "cont", True), (2, 17, 33), C, dt)


@pytest.mark.parametrize("bhw", [(2, 17, 33), (3, 17, 704)], ids=["2x17x33/6-tiles", "3x17x704/264-tiles-wfinal-loop"])
def test_spatial_attn_bwd_map(bhw):
    """hyres_spatial_attn_bwd_map with C > 0: gpooled2[..., 0] is the mean's gradient divided by C."""
    L = _L()
    B, H, W = bhw
    P, C = B * H * W, 192
    glogit, pooled2, w, gw0 = RR.rand((B, H, W), 151), RR.rand((B, H, W, 2), 152), RR.rand((1, 2, 7, 7), 153, 0.3), \
        RR.rand((98,), 154)
    gl, p2, gp2, gw = Buf(P, 1).set(glogit), Buf(P, 2).set(pooled2), Buf(P, 2), Buf(98, 1).set(gw0)
    wd = w.to(dev())
    wsb = L.load().hyres_spatial_attn_workspace_bytes(B, H, W)
    ws = _ws(wsb)
    L.call("hyres_spatial_attn_bwd_map", gl.ptr, p2.ptr, wd.data_ptr(), gp2.ptr, gw.ptr, B, H, W, C, ws.ptr, wsb,
           L.stream())
    ws.take()
    gpr, gwr = RR.sa_map_bwd_ref(glogit, pooled2, w)
    out = gp2.take().view(B, H, W, 2)
    _check("g mean / C", out[..., 0], gpr[..., 0] / C, TOL)
    _check("g max", out[..., 1], gpr[..., 1], TOL)
    _check("gw", gw.take().view(-1), gwr.reshape(-1) + gw0.double(), TOL)


def test_spatial_attn_pool_c192_build_against_loop_build():
    """sa_pool_kernel<NC = 3> against the runtime-loop build on the same data padded to C = 196.  -inf padding would
    poison the loop build's channel sum, so the comparison is made on the non-negative tie inputs padded with zeros:
    the maximum and the first argmax must agree bit for bit; the mean is s / 196 against s / 192 and is only compared to
    two fp32 roundings.  (The fp64 checks above are the requirement; this is not a clean bitwise comparison.)"""
    bhw = (2, 17, 33)
    k = dict(_sa_case(bhw, 192, "ties"))
    _, _, p2, am, _, _ = _sa_fwd(k, bhw, 192, False, with_y=False)
    k["x"] = torch.cat([k["x"], torch.zeros(*bhw, 4)], -1)
    _, _, p2l, aml, _, _ = _sa_fwd(k, bhw, 196, False, with_y=False)
    assert torch.equal(am, aml) and torch.equal(p2[..., 1], p2l[..., 1])
    _check("mean", p2l[..., 0].double() * 196, p2[..., 0].double() * 192, 2.0 ** -22)


# ======================================================================================================= SA fold
def _fold_kernel(dt):
    return {0: "sa_fold_bwd_kernel", 1: "sa_fold_bwd_h8_kernel<G=0>", 3: "sa_fold_bwd_h8_kernel<G=1>"}[dt]


def _fold_blocks(P):
    return max(1, min((P + 63) // 64, 1024))


FOLD = [pytest.param(P, C, 0, 0, id=f"P{P}xC{C}/{_fold_kernel(0)}({_fold_blocks(P)} blocks)")
        for C in (4, 20, 64) for P in (7, 1000, 70000)]
FOLD += [pytest.param(1000, 20, 4, 0, id=f"P1000xC20-ld24/{_fold_kernel(0)}")]
FOLD += [pytest.param(P, C, 0, dt, id=f"P{P}xC{C}/{_fold_kernel(dt)}({_fold_blocks(P)} blocks)")
         for dt in (1, 3) for C in (8, 24, 64) for P in (7, 1000, 70000)]


@pytest.mark.parametrize("P,C,extra_ld,dt", FOLD)
def test_sa_fold_bwd(P, C, extra_ld, dt):
    """hyres_sa_fold_bwd against its closed form: P below one group row, off a multiple of 16, and above the 1024-block
    cap (blocks stride); pre with exact zeros; d bias and d slope added to non-zero starts."""
    L = _L()
    half, g16 = bool(dt & DT_ACT16), bool(dt & DT_GRAD16)
    pdt, gdt = (torch.float16 if half else torch.float32), (torch.float16 if g16 else torch.float32)
    ld = C + extra_ld
    pre, gy = _pre_with_zeros((P, C), 161).to(pdt), RR.rand((P, C), 162).to(gdt)
    attn = torch.sigmoid(RR.rand((P,), 163, 3.0))
    bias, db0, ds0 = RR.rand((C,), 164, 0.5), RR.rand((C,), 165), -0.375
    D = dev()
    p, g = Buf(P, C, pdt, ld).set(pre), Buf(P, C, gdt, ld).set(gy)
    at, b, sl = attn.to(D), bias.to(D), torch.tensor([0.25], device=D)
    gs, gl, db, ds = Buf(P, C, gdt), Buf(P, 1), Buf(C, 1).set(db0), Buf(1, 1).set(torch.tensor([ds0]))
    wsb = L.load().hyres_sa_fold_workspace_bytes(P, C)
    ws = _ws(wsb)
    L.call("hyres_sa_fold_bwd", p.ptr, ld, g.ptr, ld, at.data_ptr(), b.data_ptr(), sl.data_ptr(), gs.ptr, gl.ptr,
           db.ptr, ds.ptr, P, C, ws.ptr, wsb, dt, L.stream())
    ws.take()
    gsr, glr, dbr, dsr = RR.sa_fold_bwd_ref(pre, gy, attn, bias, 0.25)
    # gs = attn * PReLU'(gy): two roundings
    _check("gs", gs.take(), gsr, (H16 if g16 else 0.0) + TOL_POINT)
    _check("glogit", gl.take().view(-1), glr, TOL_AMP if g16 else TOL)
    _check("dbias", db.take().view(-1), dbr + db0.double(), TOL_AMP if g16 else TOL)
    _check("dslope", ds.take().view(()), dsr + ds0, TOL_AMP if g16 else TOL_SLOPE)


@pytest.mark.parametrize("C,dt", [(68, 0), (6, 0), (12, DT_ACT16)], ids=["C68", "C6", "C12-act16"])
def test_sa_fold_bwd_refusals(C, dt):
    L = _L()
    P = 100
    D = dev()
    pdt = torch.float16 if dt else torch.float32
    p, g = Buf(P, C, pdt).set(RR.rand((P, C), 171)), Buf(P, C).set(RR.rand((P, C), 172))
    at, b, sl = torch.rand(P, device=D), torch.rand(72, device=D), torch.tensor([0.25], device=D)
    gs, gl, db, ds = Buf(P, C), Buf(P, 1), Buf(C, 1), Buf(1, 1)
    wsb = L.load().hyres_sa_fold_workspace_bytes(P, C)
    ws = _ws(wsb)
    with pytest.raises(L.HipError):
        L.call("hyres_sa_fold_bwd", p.ptr, C, g.ptr, C, at.data_ptr(), b.data_ptr(), sl.data_ptr(), gs.ptr, gl.ptr,
               db.ptr, ds.ptr, P, C, ws.ptr, wsb, dt, L.stream())
    assert gs.untouched() and gl.untouched() and db.untouched() and ds.untouched() and ws.untouched()
