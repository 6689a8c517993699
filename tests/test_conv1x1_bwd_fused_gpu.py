"""conv1x1_bwd_fused_b6_kernel (csrc/conv_stream.hip): the backward of a plain fp32 1x1 Conv2d (bf16x6) in one launch
— the input gradient of conv1x1_stream_b6_kernel and the weight / bias gradient partials of wgrad1x1_bf6_pf2_kernel
from one read of the output gradient — against the two kernels it replaces, through the C-ABI.

Per case the same operands go through hyres_conv_forward + hyres_conv_wgrad (hyres_conv_tuning key 24 = 2: the two
kernels, the streaming kernel's pixel floor lifted so that it is the unfused conv at these shapes) and through
hyres_conv1x1_bwd_fused + hyres_wgrad_reduce_jobs (key 24 = 7: bit 2 routes the 64 -> 128 gradients, which the default
leaves on the two kernels). Bars:
  * gx bit-identical (same bf16 pieces, same K order, same epilogue code);
  * dW and dbias of BOTH paths within test_wgrad_kernels_gpu.TOL (1e-5, max-norm) of an fp64 reference computed here.
Shapes: 2 x 8 x 64 pixels (32 chunks of 32 pixels), 1 x 7 x 40 (ragged last chunk), 1 x 2 x 16 (one chunk) — all with
fewer chunks than blocks, one chunk per block — and two with 3 and 4 chunks per block (146 x 153, ragged, and
2 x 100 x 131), where a block's loop runs both of its bodies and rotates its register sets. Channels 128 -> 64 and
64 -> 128, every combination of residual / ReLU mask / accumulate, with and without the bias gradient.
"""
import ctypes

import pytest
import torch

from helpers import rel_err
from test_wgrad_kernels_gpu import TOL

pytestmark = pytest.mark.gpu

KEY = 24


def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def _rand(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(shape, generator=g) * 2 - 1) * scale


def _tune(value):
    from hyres_hip import _lib as L
    old = ctypes.c_int(0)
    L.call("hyres_conv_tuning", KEY, value, ctypes.byref(old))
    return old.value


def _descs(B, H, W, KG, CX, F, ops):
    """The input-gradient conv (KG gradient channels -> CX) with the F operands and the weight gradient [KG][CX]."""
    from hyres_hip import _lib as L
    from hyres_hip import ops as O
    g = O._geom("hyres_geom_conv2d_dgrad", B, H, W, CX, CX, KG, KG, 1, 1, 1, 0, 1)
    e = L.Epilogue()
    e.kind = L.EPI_BIAS
    if F & 1:
        e.res, e.ldres = ops["res"].data_ptr(), CX
    if F & 2:
        e.act = L.ACT_RELU_MASK
        e.aux0, e.ld0 = ops["mask"].data_ptr(), CX
    e.accumulate = 1 if F & 4 else 0
    d = L.WgradDesc()
    L.call("hyres_wgrad_desc_conv2d", ctypes.byref(d), B, H, W, CX, CX, KG, KG, 1, 1, 1, 0, 1)
    d.accumulate = 1
    return g, e, d


_CACHE = {}


def _operands(B, H, W, KG, CX):
    """Inputs and fp64 references of one shape, computed once and shared by its F / bias variants (never written)."""
    key = (B, H, W, KG, CX)
    if key not in _CACHE:
        D = dev()
        P = B * H * W
        o = {"gp": _rand((P, KG), 1).to(D), "x": _rand((P, CX), 2).to(D),
             "w": _rand((KG, CX), 3, KG ** -0.5).to(D), "res": _rand((P, CX), 4).to(D),
             "mask": _rand((P, CX), 5).to(D), "old": _rand((P, CX), 6).to(D),
             "dw0": _rand((KG, CX), 7).to(D), "db0": _rand((KG,), 8).to(D)}
        o["w2d"] = o["w"].t().contiguous()  # WPREP_CONV_DGRAD of a 1x1: [Ci][Co]
        o["dw_ref"] = o["dw0"].double() + o["gp"].double().t() @ o["x"].double()
        o["db_ref"] = o["db0"].double() + o["gp"].double().sum(0)
        o["gx_lin"] = o["gp"].double() @ o["w"].double()
        _CACHE.clear()  # one shape's operands at a time
        _CACHE[key] = o
    return _CACHE[key]


def _gx_ref(o, F):
    r = o["gx_lin"]
    if F & 1:
        r = r + o["res"].double()
    if F & 2:
        r = torch.where(o["mask"].double() > 0, r, torch.zeros_like(r))
    if F & 4:
        r = r + o["old"].double()
    return r


def _run(B, H, W, KG, CX, F, bias, fused):
    from hyres_hip import _lib as L
    from hyres_hip import ops as O
    D = dev()
    o = _operands(B, H, W, KG, CX)
    P = B * H * W
    gx = o["old"].clone() if F & 4 else torch.full((P, CX), float("nan"), device=D)
    dw, db = o["dw0"].clone(), o["db0"].clone()
    g, e, d = _descs(B, H, W, KG, CX, F, o)
    lib = L.load()
    old = _tune(7 if fused else 2)
    try:
        ok = lib.hyres_conv1x1_bwd_fused_ok(ctypes.byref(g), ctypes.byref(e), ctypes.byref(d), o["gp"].data_ptr(),
                                            o["x"].data_ptr(), o["w2d"].data_ptr(), KG, gx.data_ptr())
        assert bool(ok) == fused
        if fused:
            name = O.bwd1x1_fused_variant(g, e, d)
            nb = int(lib.hyres_conv1x1_bwd_fused_workspace_bytes(ctypes.byref(d)))
            ws = torch.full((nb // 4,), float("nan"), device=D)
            jobs = (L.WgradJob * 2)()
            nj = ctypes.c_int(0)
            L.call("hyres_conv1x1_bwd_fused", ctypes.byref(g), o["gp"].data_ptr(), o["w2d"].data_ptr(), KG,
                   gx.data_ptr(), ctypes.byref(e), ctypes.byref(d), o["x"].data_ptr(), dw.data_ptr(),
                   db.data_ptr() if bias else None, ws.data_ptr(), nb, jobs, ctypes.byref(nj), L.stream())
            assert nj.value == (2 if bias else 1)
            L.call("hyres_wgrad_reduce_jobs", jobs, nj.value, L.stream())
        else:
            name = O.conv_variant(g, e, False) + " + " + O.wgrad_variant(d)
            L.call("hyres_conv_forward", ctypes.byref(g), o["gp"].data_ptr(), o["w2d"].data_ptr(), KG, gx.data_ptr(),
                   ctypes.byref(e), None, 0, L.stream())
            nb = int(lib.hyres_wgrad_workspace_bytes(ctypes.byref(d)))
            ws = torch.full((nb // 4 + 4,), float("nan"), device=D)
            L.call("hyres_conv_wgrad", ctypes.byref(d), o["gp"].data_ptr(), o["x"].data_ptr(), dw.data_ptr(),
                   db.data_ptr() if bias else None, ws.data_ptr(), 4 * ws.numel(), L.stream())
        torch.cuda.synchronize()
    finally:
        _tune(old)
    return name, gx, dw, db


SMALL = [(2, 8, 64), (1, 7, 40), (1, 2, 16)]
LARGE = [(1, 146, 153, 128, 64, 6, True), (2, 100, 131, 64, 128, 7, True)]
CASES = [(B, H, W, KG, CX, F, (F + H) % 2 == 0) for (B, H, W) in SMALL for (KG, CX) in ((128, 64), (64, 128))
         for F in range(8)] + LARGE


@pytest.mark.parametrize("B,H,W,KG,CX,F,bias", CASES)
def test_fused_matches_two_kernels(B, H, W, KG, CX, F, bias):
    o = _operands(B, H, W, KG, CX)
    name_u, gx_u, dw_u, db_u = _run(B, H, W, KG, CX, F, bias, False)
    name_f, gx_f, dw_f, db_f = _run(B, H, W, KG, CX, F, bias, True)
    nt, ks = CX // 32, KG // 16
    assert name_f == f"conv1x1_bwd_fused_b6_kernel<{nt}, {ks}, {F}>", name_f
    assert name_u.startswith(f"conv1x1_stream_b6_kernel<{nt}, {ks}, {F}, true> + wgrad1x1_bf6"), name_u
    gx_err = rel_err(gx_f.cpu(), _gx_ref(o, F).cpu())
    errs = {"dw_u": rel_err(dw_u.cpu(), o["dw_ref"].cpu()), "dw_f": rel_err(dw_f.cpu(), o["dw_ref"].cpu())}
    if bias:
        errs["db_u"] = rel_err(db_u.cpu(), o["db_ref"].cpu())
        errs["db_f"] = rel_err(db_f.cpu(), o["db_ref"].cpu())
    print(f"B{B} {H}x{W} {KG}->{CX} F={F} bias={bias}: gx vs fp64 {gx_err:.2e}, " +
          ", ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert torch.equal(gx_f, gx_u), "gx differs from conv1x1_stream_b6_kernel's"
    assert (gx_f.view(torch.int32) == gx_u.view(torch.int32)).all(), "gx differs in a zero's sign"
    assert gx_err < 2e-6  # test_stream_b6_gpu's bar for the streaming kernel: the operands reached the right places
    if not bias:
        assert torch.equal(db_f, o["db0"]) and torch.equal(db_u, o["db0"])
    for k, v in errs.items():
        assert v <= TOL, (k, v)


def test_key_off_restores_the_two_kernels():
    """hyres_conv_tuning key 24 = 0 at the flagship's shapes (B 16, 128^2): the predicate refuses and the conv / weight
    gradient labels are those of the two kernels; = 1 (the default) the fused kernel takes the 128 -> 64 gradients and
    = 5 the 64 -> 128 ones too. Host-only."""
    from hyres_hip import _lib as L
    from hyres_hip import ops as O
    lib = L.load()
    assert _tune(1) == 1, "key 24 defaults to 1"
    for (KG, CX, F) in ((128, 64, 2), (64, 128, 3), (64, 128, 5)):
        ops = {"res": torch.empty(4), "mask": torch.empty(4)}  # only the pointers' presence is read
        g, e, d = _descs(16, 128, 128, KG, CX, F, ops)
        args = (ctypes.byref(g), ctypes.byref(e), ctypes.byref(d), None, None, None, KG, None)
        assert lib.hyres_conv1x1_bwd_fused_ok(*args) == (1 if KG == 128 else 0)
        try:
            _tune(5)
            assert lib.hyres_conv1x1_bwd_fused_ok(*args) == 1
            assert O.bwd1x1_fused_variant(g, e, d) == f"conv1x1_bwd_fused_b6_kernel<{CX // 32}, {KG // 16}, {F}>"
            _tune(0)
            assert lib.hyres_conv1x1_bwd_fused_ok(*args) == 0
            assert O.conv_variant(g, e, False) == f"conv1x1_stream_b6_kernel<{CX // 32}, {KG // 16}, {F}, true>"
            assert O.wgrad_variant(d).startswith("wgrad1x1_bf6_pf2_kernel<")
        finally:
            _tune(1)
    # other shapes keep the two kernels with the key on: 64 -> 64, a small grid, fp16 operands
    g, e, d = _descs(16, 128, 128, 64, 64, 2, {"mask": torch.empty(4)})
    assert lib.hyres_conv1x1_bwd_fused_ok(ctypes.byref(g), ctypes.byref(e), ctypes.byref(d), None, None, None, 64, None) == 0
    g, e, d = _descs(2, 8, 64, 128, 64, 2, {"mask": torch.empty(4)})
    assert lib.hyres_conv1x1_bwd_fused_ok(ctypes.byref(g), ctypes.byref(e), ctypes.byref(d), None, None, None, 128, None) == 0
    g, e, d = _descs(16, 128, 128, 128, 64, 2, {"mask": torch.empty(4)})
    d.f16_operands = 1
    assert lib.hyres_conv1x1_bwd_fused_ok(ctypes.byref(g), ctypes.byref(e), ctypes.byref(d), None, None, None, 128, None) == 0


def test_conv2d_backward_takes_the_fused_kernel():
    """ops.conv2d's backward at 2 x 128 x 256 pixels (the pixel floor), 64 -> 128 with a bias: key on and key off give
    bit-identical input gradients, and weight / bias gradients within TOL of fp64 both ways (at this shape both paths
    split the pixels into the same 256 ranges of 8 chunks, so the gradients may agree bit for bit: which kernel ran is
    read from KernelTimer's labels)."""
    from hyres_hip import ops as O
    D = dev()
    B, H, W, Ci, Co = 2, 128, 256, 64, 128
    xv = _rand((B, Ci, H, W), 11).to(D)
    gy = _rand((B, Co, H, W), 12).to(D)
    g2 = gy.permute(0, 2, 3, 1).reshape(-1, Co).double()
    x2 = xv.permute(0, 2, 3, 1).reshape(-1, Ci).double()
    dw_ref, db_ref = g2.t() @ x2, g2.sum(0)
    outs = []
    for key in (1, 0):
        old = _tune(key)
        try:
            w = torch.nn.Parameter(_rand((Co, Ci, 1, 1), 13, Ci ** -0.5).to(D))
            b = torch.nn.Parameter(_rand((Co,), 14, 0.1).to(D))
            tape = O.Tape()
            xn = O.to_nhwc(xv, rg=True)
            yn = O.conv2d(tape, xn, w, b)
            yn.set_grad(O.nchw_grad_to_nhwc(gy))
            timed = O.KernelTimer.enabled
            O.KernelTimer.reset()
            O.KernelTimer.enabled = True
            try:
                tape.backward()
                torch.cuda.synchronize()
                names = [ev[4] for ev in O.KernelTimer.events]
            finally:
                O.KernelTimer.enabled = timed
                O.KernelTimer.reset()
            outs.append((O.to_nchw_grad(xn).clone(), w.grad.clone(), b.grad.clone()))
            assert names == (["conv1x1_bwd_fused_b6_kernel<2, 8, 0>"] if key else
                             ["conv1x1_stream_b6_kernel<2, 8, 0, true>"]), names
        finally:
            _tune(old)
    (gx1, dw1, db1), (gx0, dw0, db0) = outs
    assert torch.equal(gx1, gx0)
    for dw, db in ((dw1, db1), (dw0, db0)):
        assert rel_err(dw.reshape(Co, Ci).cpu(), dw_ref.cpu()) <= TOL and rel_err(db.cpu(), db_ref.cpu()) <= TOL
