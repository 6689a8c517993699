"""CPU (no GPU): the fp64 weight-gradient reference of tests/wgrad_ref.py against fp64 autograd at 1e-12, and the
coverage of the GPU case table of tests/test_wgrad_kernels_gpu.py: the kernel names it records are the ones the built
library reports (hyres_wgrad_kernel_name_at under both values of tuning key 7), and their union holds every
instantiation wgrad_route() can produce, listed below from with_tile, with_halo, with_io, launch_thin and launch_wgrad.

Instantiations the launcher compiles and the route never selects (they are not in the lists): with_halo's <1, 3, 1, 2>
(a dilated 3x3 always takes all nine taps per block, KR = 3) and <3, 3, 1, 1> (a dilation-1 3x3 always takes one tap row,
KR = 1), in each of wgrad_halo_kernel, wgrad_halo_bf6_kernel and wgrad_halo_f16_kernel (x 4 io masks), and
wgrad_halo_bf6_pf2_kernel<3, 1, 2, 2>.  wgrad_f16_kernel with NT = 9 / 5 is reachable, though the f16 plan never groups
taps: with f16_operands, an fp16 operand whose ld % 4 != 0 keeps the plan on the fp32 kernels, and its contiguous fp32
copy then makes the launch descriptor f16-eligible (the f16late/ cases)."""
import ctypes
import itertools

import pytest
import torch
import torch.nn.functional as F

import test_wgrad_kernels_gpu as T
import wgrad_ref as WR
from helpers import rel_err

TOL = 1e-12


def _L():
    from hyres_hip import _lib as L
    return L


def _nhwc(t):
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])


@pytest.mark.parametrize("B,H,W,Ci,Co,K,s,p,dil", [(2, 5, 7, 3, 4, 1, 1, 0, 1), (2, 5, 7, 3, 4, 1, 2, 0, 1),
                                                   (2, 5, 7, 3, 4, 3, 1, 1, 1), (3, 6, 9, 5, 2, 3, 2, 1, 1),
                                                   (2, 7, 5, 3, 4, 3, 1, 2, 2), (1, 9, 11, 2, 3, 3, 2, 2, 2),
                                                   (2, 5, 7, 3, 4, 5, 1, 2, 1), (2, 7, 9, 3, 4, 5, 2, 2, 1),
                                                   (1, 11, 13, 2, 3, 5, 1, 4, 2), (2, 4, 6, 3, 2, 3, 1, 0, 1)])
def test_ref_matches_conv2d_autograd(B, H, W, Ci, Co, K, s, p, dil):
    L = _L()
    x = WR.rand((B, Ci, H, W), 1).double()
    w = WR.rand((Co, Ci, K, K), 2).double().requires_grad_()
    b = torch.zeros(Co, dtype=torch.float64, requires_grad=True)
    y = F.conv2d(x, w, b, stride=s, padding=p, dilation=dil)
    gy = WR.rand(tuple(y.shape), 3).double()
    y.backward(gy)
    d = L.WgradDesc()
    L.call("hyres_wgrad_desc_conv2d", ctypes.byref(d), B, H, W, Ci, Ci, Co, Co, K, K, s, p, dil)
    dW, db = WR.wgrad_ref(d, _nhwc(gy), _nhwc(x))
    flat = torch.zeros(Co * Ci * K * K, dtype=torch.float64)
    flat[WR.dst_index(d)] = dW
    assert rel_err(flat.view(Co, Ci, K, K), w.grad) < TOL
    assert rel_err(db, b.grad) < TOL


@pytest.mark.parametrize("B,H,W,Ci,Co", [(2, 3, 5, 3, 4), (1, 7, 4, 2, 3), (3, 1, 1, 4, 2)])
def test_ref_matches_conv_transpose2d_autograd(B, H, W, Ci, Co):
    """K = 5, stride 2, padding 2, output_padding 1 (the model's up-sampling layers), hyres_wgrad_desc_deconv2d."""
    L = _L()
    x = WR.rand((B, Ci, H, W), 4).double()
    w = WR.rand((Ci, Co, 5, 5), 5).double().requires_grad_()
    y = F.conv_transpose2d(x, w, None, stride=2, padding=2, output_padding=1)
    assert tuple(y.shape[2:]) == (2 * H, 2 * W)
    gy = WR.rand(tuple(y.shape), 6).double()
    y.backward(gy)
    d = L.WgradDesc()
    L.call("hyres_wgrad_desc_deconv2d", ctypes.byref(d), B, H, W, Ci, Ci, Co, Co, 5, 2)
    dW, _ = WR.wgrad_ref(d, _nhwc(x), _nhwc(gy))
    flat = torch.zeros(Ci * Co * 25, dtype=torch.float64)
    flat[WR.dst_index(d)] = dW
    assert rel_err(flat.view(Ci, Co, 5, 5), w.grad) < TOL


@pytest.mark.parametrize("B,H,W,C", [(2, 5, 7, 3), (1, 1, 9, 6)])
def test_ref_matches_gdn_gamma_autograd(B, H, W, C):
    """norm[q][m] = sum_n gamma[m][n] x[q][n]^2: d gamma = sum_q dn[q][m] x[q][n]^2."""
    x = WR.rand((B * H * W, C), 7).double()
    gamma = WR.rand((C, C), 8).double().requires_grad_()
    dn = WR.rand((B * H * W, C), 9).double()
    ((x * x) @ gamma.t()).backward(dn)
    d = WR.Desc(B, H, W, C, C, H, W, 1, [0], [0], square_q=1)
    dW, _ = WR.wgrad_ref(d, dn, x)
    assert rel_err(dW[0], gamma.grad) < TOL


def test_ref_reversed_tap_list_and_strided_dst():
    """A tap list is data: the reversed 3x3 order gives the same taps at mirrored slots, at any destination stride."""
    fwd = WR.Desc(2, 5, 7, 4, 3, 5, 7, 1, [t // 3 - 1 for t in range(9)], [t % 3 - 1 for t in range(9)])
    rev = WR.Desc(2, 5, 7, 4, 3, 5, 7, 1, [1 - t // 3 for t in range(9)], [1 - t % 3 for t in range(9)], sm=70, sn=19, st=2)
    P, Q = WR.rand((70, 4), 10), WR.rand((70, 3), 11)
    a, _ = WR.wgrad_ref(fwd, P, Q)
    b, _ = WR.wgrad_ref(rev, P, Q)
    assert torch.equal(a, b.flip(0))
    idx = WR.dst_index(rev)
    assert idx.unique().numel() == idx.numel() and int(idx[8, 3, 2]) == 3 * 70 + 2 * 19 + 16


# ---------------------------------------------------------------------------------------------- coverage of the table
_TF = ("true", "false")
_TILES = ["2, 2, 2, 2", "2, 1, 2, 2", "1, 1, 1, 4", "1, 1, 4, 1", "1, 1, 2, 2"]  # with_tile's shapes
_TILES_NT = [f"{t}, 1" for t in _TILES] + ["1, 1, 2, 2, 9", "1, 1, 2, 2, 5"]
_FLAGS = ["true, true, true", "true, true, false", "true, false, false", "false, true, false", "false, false, false"]
_HALO = ["1, 3, 1, 1", "3, 3, 1, 2", "1, 5, 1, 1", "1, 5, 2, 1"]  # with_halo's reachable (KR, KW, SQ, DIL)

REACHABLE = (
    [f"wgrad_kernel<{t}, {f}>" for t in _TILES_NT for f in _FLAGS]                                     # launch_wgrad
    # f16: one tap per block (NT = 1); SQ | ONE | neither; with_io
    + [f"wgrad_f16_kernel<{t}, 1, {k}, {io}>" for t in _TILES for k in ("true, false", "false, true", "false, false")
       for io in range(4)]
    # ... and behind an fp32 plan (an fp16 operand converted to a contiguous copy: io 0), its taps grouped
    + [f"wgrad_f16_kernel<1, 1, 2, 2, {nt}, {sq}, false, 0>" for nt in (9, 5) for sq in _TF]
    + [f"wgrad1x1_kernel<{t}, {g}>" for t in _TILES for g in (1, 2)]
    + [f"wgrad1x1_bf6_kernel<{t}>" for t in _TILES] + [f"wgrad1x1_bf6_pf2_kernel<{t}>" for t in _TILES]
    + [f"wgrad_thin_kernel<{mw}, {nc}, {tg}, {sq}, {ph}>" for mw in (1, 2) for nc in (3, 4) for tg in (9, 25 if mw == 1 else 13)
       for sq in (1, 2) for ph in _TF]                                                                 # launch_thin
    + [f"wgrad_halo_kernel<{h}, 1>" for h in _HALO] + [f"wgrad_halo_bf6_kernel<{h}>" for h in _HALO]
    + [f"wgrad_halo_f16_kernel<{h}, {io}, 1>" for h in _HALO for io in range(4)]
    + ["wgrad_halo_bf6_pf2_kernel<3, 1, 1, 2>", "wgrad_halo_bf6_pf2_kernel<5, 1, 1, 2>",
       "wgrad_halo_bf6_pf2_kernel<5, 2, 1, 1>"])
FAMILIES = {"wgrad_kernel", "wgrad_f16_kernel", "wgrad1x1_kernel", "wgrad1x1_bf6_kernel", "wgrad1x1_bf6_pf2_kernel",
            "wgrad_thin_kernel", "wgrad_halo_kernel", "wgrad_halo_f16_kernel", "wgrad_halo_bf6_kernel",
            "wgrad_halo_bf6_pf2_kernel"}


def test_case_table_names_are_the_librarys_and_cover_every_reachable_instantiation():
    L = _L()
    lib = L.load()
    saved = {}
    for k in range(24):
        old = ctypes.c_int(0)
        assert lib.hyres_conv_tuning(k, 1, ctypes.byref(old)) == 0
        saved[k] = old.value
        assert lib.hyres_conv_tuning(k, old.value, None) == 0
    seen = {0: set(), 1: set()}
    try:
        assert len(T.BY_ID) == len(T.CASES) == len(T.KERNELS)
        for c, mode in itertools.product(T.CASES, (0, 1)):
            name, lanes = T.query(L, c, mode)
            assert name == T.kernel_of(c, mode), (c.id, mode, name)
            assert lanes == c.lanes, (c.id, mode, lanes)
            if mode in T.modes_of(c):
                seen[mode].add(name)
    finally:
        for k, v in saved.items():
            assert lib.hyres_conv_tuning(k, v, None) == 0
    for k, v in saved.items():  # T.query restored what it set
        old = ctypes.c_int(0)
        assert lib.hyres_conv_tuning(k, v, ctypes.byref(old)) == 0 and old.value == v, k
    assert len(set(REACHABLE)) == len(REACHABLE) == 35 + 60 + 4 + 10 + 10 + 32 + 8 + 16 + 3
    union = seen[0] | seen[1]
    assert not set(REACHABLE) - union, sorted(set(REACHABLE) - union)
    assert not union - set(REACHABLE), sorted(union - set(REACHABLE))
    assert {n.split("<")[0] for n in union} == FAMILIES
    # each GEMM mode reaches its own families, and both reach the ones key 7 does not move
    native = {"wgrad1x1_kernel", "wgrad_halo_kernel"}
    bf6 = {"wgrad1x1_bf6_kernel", "wgrad1x1_bf6_pf2_kernel", "wgrad_halo_bf6_kernel", "wgrad_halo_bf6_pf2_kernel"}
    assert {n.split("<")[0] for n in seen[0]} == FAMILIES - bf6 - {"wgrad_f16_kernel", "wgrad_halo_f16_kernel"}
    assert {n.split("<")[0] for n in seen[1]} == FAMILIES - native


def test_misaligned_name_query_matches_ideal_when_aligned():
    """hyres_wgrad_kernel_name_at(d, 1, 1, 1) is hyres_wgrad_kernel_name(d) on every case."""
    L = _L()
    for c in T.CASES:
        d = T.make_desc(L, c)
        a, b = ctypes.create_string_buffer(96), ctypes.create_string_buffer(96)
        L.call("hyres_wgrad_kernel_name", ctypes.byref(d), a, 96)
        L.call("hyres_wgrad_kernel_name_at", ctypes.byref(d), 1, 1, 1, b, 96)
        assert a.value == b.value
