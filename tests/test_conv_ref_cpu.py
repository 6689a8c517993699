"""CPU (no GPU): the fp64 convolution reference of tests/conv_ref.py against torch fp64 at 1e-12, and the coverage of
the GPU case table of tests/test_conv_kernels_gpu.py: the names and float4 flags it records are the ones the built
library reports (hyres_conv_kernel_name_at with alignment flags synthesised from each case's offsets, under both values
of tuning key 7), and their union holds every instantiation route(), launch_fwd, launch_tiles and launch_narrow can
produce for the TILES and NARROW families, listed below from those functions.

Instantiations that are compiled or spelled and never selected (they are not in the lists): conv_fwd_b6db_kernel off
the 64x64 tile (choose_gemm asks for it on tile 4 only; launch_fwd falls through to conv_fwd_b6_kernel elsewhere);
conv_fwd_h_kernel<..., 2, ..., IO> with IO = 1 / 3 (fp16 X needs Ci % 32 == 0, refused) ; conv_fwd_kernel<..., 2, ...,
true> (f16_operands is ignored on the scalar-load path).  conv_narrow_kernel / conv_narrow_strip_kernel<CO, S, true>
(fp16 X) are reached by the nar/*-x16 cases but print as <CO, S>.  The narrow kernels always store through the scalar
epilogue, so the float4 flag is not asked of them in both values."""
import ctypes
import itertools

import pytest
import torch

import conv_ref as CR
import test_conv_kernels_gpu as T
from helpers import rel_err

TOL = 1e-12


def _L():
    from hyres_hip import _lib as L
    return L


def _layer(geom):
    c = T.Case("cpu", geom)
    x, w, mask, acc = T.conv_data.__wrapped__(geom, False, False, False, False, False)
    return c, x, w, mask, acc


GEOMS = [T.cv(2, 5, 7, 3, 4, 1), T.cv(2, 5, 7, 3, 4, 1, s=2), T.cv(2, 5, 7, 3, 4, 3), T.cv(3, 6, 9, 5, 2, 3, s=2),
         T.cv(2, 7, 5, 3, 4, 3, d=2), T.cv(1, 9, 11, 2, 3, 3, s=2, p=2, d=2), T.cv(2, 5, 7, 3, 4, 5),
         T.cv(2, 7, 9, 3, 4, 5, s=2), T.cv(2, 4, 6, 3, 2, 3, p=0), ("conv", 2, 5, 8, 3, 4, 3, 6, 1, 2, 1),
         T.cv(2, 5, 7, 3, 4, 3, kind="dgrad"), T.cv(2, 5, 7, 3, 4, 5, kind="dgrad"), T.cv(2, 7, 5, 3, 4, 3, d=2, kind="dgrad"),
         T.cv(2, 6, 8, 3, 4, 5, s=2, kind="dgrad"), T.cv(2, 2, 6, 3, 4, 5, s=2, kind="dgrad"),
         T.cv(1, 10, 14, 2, 3, 3, s=2, kind="dgrad"), ("deconv", 2, 3, 5, 3, 4), ("deconv", 1, 4, 1, 2, 3),
         ("deconv", 3, 1, 1, 4, 2), ("deconv_dgrad", 2, 3, 5, 3, 4), ("deconv_dgrad", 1, 4, 7, 2, 3),
         ("mconv", 2, 5, 7, 3, 4), ("mconv", 1, 4, 4, 2, 3), ("mdgrad", 2, 5, 7, 3, 4), ("mdgrad", 1, 6, 4, 2, 3)]


@pytest.mark.parametrize("geom", GEOMS, ids=[CR.shape_id(g) for g in GEOMS])
def test_geometry_evaluator_on_helper_geometry_and_relayout_matches_torch(geom):
    """conv_ref.geom_eval on each hyres_geom_* helper's output and conv_ref.relayout == F.conv2d / F.conv_transpose2d /
    their autograd input-gradients / the masked conv, also through an ldw wider than ntaps * Ci."""
    L = _L()
    c, x, w, mask, acc = _layer(geom)
    g, prep = T.make_geom(L, c)
    w2 = CR.relayout(g, w, prep[0], mask)
    y, written = CR.geom_eval(g, x, w2)
    assert written.all() and tuple(y.shape) == tuple(acc.shape)
    assert rel_err(y, acc) < TOL
    wide = torch.full((w2.shape[0], w2.shape[1] + 3), float("nan"))
    wide[:, :w2.shape[1]] = w2
    y2, _ = CR.geom_eval(g, x, wide, ldw=w2.shape[1] + 3)
    assert torch.equal(y, y2)
    ysq, _ = CR.geom_eval(g, x, w2, square=True)
    assert rel_err(ysq, CR.torch_acc(T.layer_of(c)[0], x, w, mask, square=True)) < TOL


def test_epilogue_reference_by_hand():
    """Each epilogue kind of conv_ref.epilogue on a 2 x 3 example worked by hand from hyres_hip.h:95-124."""
    acc = torch.tensor([[1.0, -2.0, 3.0], [-4.0, 5.0, -6.0]], dtype=torch.float64)
    bias = torch.tensor([0.5, 0.25, -1.0])
    y, o2 = CR.epilogue(T.BIAS, T.PRELU, acc, bias, None, 0.25)
    assert torch.equal(o2, acc + bias) and torch.equal(y, torch.where(o2 >= 0, o2, 0.25 * o2))
    m = torch.tensor([[1.0, 0.0, -1.0], [2.0, -0.0, 3.0]])
    y, _ = CR.epilogue(T.BIAS, T.RELU_MASK, acc, None, None, None, m, y_old=torch.ones(2, 3))
    assert torch.equal(y, torch.tensor([[2.0, 1.0, 1.0], [-3.0, 1.0, -5.0]], dtype=torch.float64))
    y, _ = CR.epilogue(T.SA_BWD, 0, acc, aux0=torch.tensor([[10.0, 100.0], [20.0, 200.0]]), aux2=torch.tensor([2, 0]))
    assert torch.equal(y, torch.tensor([[11.0, 8.0, 113.0], [216.0, 25.0, 14.0]], dtype=torch.float64))
    y, _ = CR.epilogue(T.ROWSCALE, T.RELU, acc, bias, torch.ones(2, 3), aux1=torch.tensor([2.0, -1.0]))
    assert torch.equal(y, (acc * torch.tensor([[2.0], [-1.0]]) + bias + 1).clamp(min=0))
    n = torch.tensor([[4.0, 9.0, 16.0], [1.0, 4.0, 25.0]])
    x = torch.tensor([[1.0, 2.0, 3.0], [4.0, 5.0, 6.0]])
    y, o2 = CR.epilogue(T.GDN, 0, n - 1, torch.ones(3), aux0=x)
    assert torch.equal(o2, n.double()) and rel_err(y, x.double() / n.double().sqrt()) < TOL
    y, _ = CR.epilogue(T.IGDN_BWD, 0, acc, aux0=x, aux1=m, aux2=n)
    assert rel_err(y, 2 * x.double() * acc + m.double() * n.double().sqrt()) < TOL


# ---------------------------------------------------------------------------------------------- coverage of the table
_TILES = ["2, 2, 2, 2", "2, 1, 2, 2", "1, 1, 4, 1", "1, 2, 2, 2", "1, 1, 2, 2"]  # launch_tiles' five shapes
_SP = ("false", "true")
REACHABLE = (
    [f"conv_fwd_kernel<{t}, {m}, {s}, false>" for t in _TILES for m in (0, 1, 2) for s in _SP]       # fp32 MFMA / MODE 2
    + [f"conv_fwd_kernel<{t}, {m}, {s}, true>" for t in _TILES for m in (0, 1) for s in _SP]         # f16_operands
    + [f"conv_fwd_b6_kernel<{t}, {m}, {s}>" for t in _TILES for m in (0, 1) for s in _SP]            # bf16x6
    + [f"conv_fwd_b6db_kernel<1, 1, 2, 2, {m}, {s}>" for m in (0, 1) for s in _SP]                   # key 20, tile 4
    + [f"conv_fwd_h_kernel<{t}, {m}, {s}, {io}>" for t in _TILES for m in (0, 1) for s in _SP for io in (1, 2, 3)]
    + [f"conv_fwd_h_kernel<{t}, 2, {s}, 2>" for t in _TILES for s in _SP]                            # fp32 image in, fp16 out
    + [f"{k}<{co}, {s}>" for k in ("conv_narrow_kernel", "conv_narrow_strip_kernel") for co in (1, 2, 3, 4)
       for s in (1, 2)])                                                                              # launch_narrow
REDUCES = {"false": {"conv_splitk_reduce4_kernel<false>", "conv_splitk_reduce_kernel<false>"},
           "true": {"conv_splitk_reduce4_kernel<true>", "conv_splitk_reduce_kernel<true>"}}


def test_case_table_names_are_the_librarys_and_cover_every_reachable_instantiation():
    L = _L()
    lib = L.load()
    saved = {}
    for k in range(24):
        old = ctypes.c_int(0)
        assert lib.hyres_conv_tuning(k, 1, ctypes.byref(old)) == 0
        saved[k] = old.value
        assert lib.hyres_conv_tuning(k, old.value, None) == 0
    seen = {}  # base name -> {vec4 values}
    reduces = {}  # split base name -> {reduce kernels}
    try:
        assert len(T.BY_ID) == len(T.CASES) == len(T.KERNELS)
        for c, mode in itertools.product(T.CASES, (0, 1)):
            got = T.query(L, c, mode)
            assert got == T.recorded(c, mode), (c.id, mode, got)
            if mode not in T.modes_of(c):
                continue
            base, _, red = got[0].partition("+")
            seen.setdefault(base, set()).add(got[1])
            if red:
                reduces.setdefault(base, set()).add(red)
                assert c.ws in ("full", "misaligned")
                assert (got[1] == 1) == red.startswith("conv_splitk_reduce4_kernel")
            if c.ws in ("none", "short"):
                assert not red, c.id
            if c.ws == "misaligned" and red:
                assert got[1] == 0 and red.startswith("conv_splitk_reduce_kernel"), c.id
    finally:
        for k, v in saved.items():
            assert lib.hyres_conv_tuning(k, v, None) == 0
    for k, v in saved.items():  # T.query restored what it set
        old = ctypes.c_int(0)
        assert lib.hyres_conv_tuning(k, v, ctypes.byref(old)) == 0 and old.value == v, k
    assert len(set(REACHABLE)) == len(REACHABLE) == 30 + 20 + 20 + 4 + 60 + 10 + 16
    assert not set(REACHABLE) - set(seen), sorted(set(REACHABLE) - set(seen))
    assert not set(seen) - set(REACHABLE), sorted(set(seen) - set(REACHABLE))
    # every tiles instantiation with the float4 and with the scalar epilogue (a split one: the slab store and the reduce)
    one = sorted(n for n, v in seen.items() if not n.startswith("conv_narrow") and v != {0, 1})
    assert not one, one
    # every split instantiation followed by both reduce kernels, of its Y dtype
    split = [n for n in REACHABLE if not n.startswith("conv_narrow") and _is_split(n)]
    assert len(split) == (15 + 10 + 10 + 2 + 30 + 5)
    for n in split:
        y16 = n.startswith("conv_fwd_h_kernel") and n.endswith((", 2>", ", 3>"))
        assert reduces.get(n) == REDUCES["true" if y16 else "false"], (n, reduces.get(n))
    assert not set(reduces) - set(split)


def _is_split(name):
    """The SPLITK template argument of a tiles kernel name (the sixth)."""
    return name[name.index("<") + 1:-1].split(", ")[5] == "true"


def test_ragged_split_cases_have_the_last_split_they_claim():
    """plan_split's arithmetic, restated: the cases named for a ragged last split have nk % cps != 0, one of them a last
    split of a single K chunk; the 4-phase split case has phases shorter than the plan's K range."""
    L = _L()
    lib = L.load()

    def plan(cid):
        c = T.BY_ID[cid]
        with T.tuned(lib, {**dict(c.tune), 7: 1}):
            g, _ = T.make_geom(L, c)
            e = T.make_epi(L, c, g, T.fake_ptrs(c, g))
            ns, _ = T.exact_split_bytes(L, g, e)
        maxtap = max(g.ntap[p] for p in range(g.nphase))
        nk = maxtap * (g.Ci // 32) if g.Ci % 32 == 0 else -(-maxtap * g.Ci // 32)
        cps = [k for k in range(1, nk + 1) if -(-nk // k) == ns][0]  # ceil_div(nk, ns) is the smallest such
        return g, nk, ns, cps

    g, nk, ns, cps = plan("split/k5-minchunks3-last1")
    assert (nk, ns, cps) == (25, 7, 4) and nk - (ns - 1) * cps == 1
    g, nk, ns, cps = plan("split/k3-64-last3")
    assert (nk, ns, cps) == (18, 4, 5) and nk - (ns - 1) * cps == 3
    g, nk, ns, cps = plan("ph/deconv-5x7-split")
    assert g.nphase == 4 and ns > 1 and min(g.ntap[p] for p in range(4)) * (g.Ci // 32) < (ns - 1) * cps
    for cid in ("split/640-full", "split/64to40-short", "ph/mconv-64to64-split", "k/m2-ci40-k3-split"):
        assert plan(cid)[2] > 1, cid


def test_name_query_matches_ideal_when_aligned():
    """hyres_conv_kernel_name_at with aligned operands and the full workspace is hyres_conv_kernel_name with the plan's
    own split flag, on every case without an offset, an odd pitch or a reduced workspace."""
    L = _L()
    lib = L.load()
    n = 0
    for c in T.CASES:
        if c.off or c.ws != "full" or any(p % 4 for _, p in c.pitch):
            continue
        with T.tuned(lib, {**dict(c.tune), 7: 1}):
            g, _ = T.make_geom(L, c)
            e = T.make_epi(L, c, g, T.fake_ptrs(c, g))
            ns, _ = T.exact_split_bytes(L, g, e)
            tile = ctypes.c_int(0)
            L.call("hyres_conv_plan", ctypes.byref(g), ctypes.byref(e), ctypes.byref(tile), None)
            a = ctypes.create_string_buffer(160)
            L.call("hyres_conv_kernel_name", ctypes.byref(g), ctypes.byref(e), int(ns > 1 and tile.value >= 0), a, 160)
        assert T.query(L, c, 1)[0].split("+")[0] == a.value.decode(), c.id
        n += 1
    assert n > 100
