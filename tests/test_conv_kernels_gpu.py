"""Per-kernel fp64 parity of the implicit-GEMM (csrc/conv_gemm.hip) and narrow (csrc/conv.hip) convolution kernels at
ragged shapes.

Every case builds a hyres_conv_geom with the hyres_geom_* helpers (hyres_geom_filter_taps for the checkerboard conv),
re-lays the PyTorch-layout weight on the device with hyres_conv_weight_prep (checked bit for bit against
conv_ref.relayout), calls hyres_conv_forward through ``_lib.call`` and compares with tests/conv_ref.py: torch fp64 on the
CPU from the values the kernel is given, then the epilogue in fp64.  ``CASES`` carries no GPU state, so
tests/test_conv_ref_cpu.py imports it and checks on the CPU that the table reaches every instantiation route(),
launch_fwd, launch_tiles and launch_narrow can produce.  ``KERNELS`` (tests/golden/conv_kernels.json) records per case
the name and the float4-epilogue flag hyres_conv_kernel_name_at reports at the case's real pointer alignments, pitches
and workspace, under the native and the bf16x6 fp32 GEMM (hyres_conv_tuning key 7); the test id carries the name and
the test asserts name and flag before launching, so a case that drifts to another kernel fails instead of testing
something else.  A split-K launch is named "<tiles kernel>+<reduce kernel>".

Storage: y, out2 and the workspace sit inside buffers of the sentinel -777 (exact in fp32 and fp16), the workspace
exactly hyres_conv_workspace_bytes long in mode "full"; the gap columns of a strided y / out2 are sentinels too and every
sentinel must be intact after the call.  Columns of x, res, aux0..2 outside their channel range in an ld-wide row, the
ldw gap of w2 and the guard elements around every input hold NaN: outside the image the kernels read zeros through
out-of-range buffer offsets, so a NaN in a result is a stray read.  No element is left out of a comparison.

Operand rounding the reference follows: with f16_operands or fp16 X / Y on the vector path (conv_fwd_kernel<..., true>,
conv_fwd_h_kernel MODE 0 / 1) X and W2 are rounded to fp16 when staged, so the reference starts from the fp16-rounded
tensors (an fp16 x fp16 product is exact in fp32; only the accumulation and the stored result round); with square_input
those cases draw x from the grid k / 32, |k| <= 32, whose squares are exact in fp16.  The scalar-load path (MODE 2) and
the narrow kernels keep fp32 operands (f16_operands is ignored there).  fp16 storage of y / out2 adds 2^-11 to the bar.

Shapes: B <= 3, so a 128-row tile spans at most 3 images (HqWq = 1, 15, 35 at B = 3; the X resource starts at the
block's first image, the rows of images b0 + 1 and b0 + 2 are the ones an ``a_base`` from image 0 would move).  An M
tail of exactly one row exists at BM 64 (M = 65 = 5 x 13); no product of the allowed sizes is 1 mod 128, the BM 128 tail
cases are 127 rows (M = 255) and 61 rows (M = 189).

Not reachable at test sizes and untested: the 32-bit span guards of hyres_conv_forward (``fits32``: a weight of 2 GB,
three images of 2 GB, an output image of 2^31 elements) and the > 2 GB branches of the buffer-resource ranges.
Compiled-in names that the table cannot show: conv_narrow_kernel / conv_narrow_strip_kernel<CO, S, true> (fp16 X) print
as <CO, S>; the nar/*-x16 cases run them.  x misaligned on a Co <= 4, Ci = 64 / 128 layer: xw16 is false, the narrow
kernels are skipped, the layer is MODE 0 and hyres_conv_forward refuses it (HYRES_E_ALIGN, refusal "narrow-x-misaligned").

Bars (max-norm, helpers.rel_err; ceiling test_parity_gpu.TOL = 1e-4): 1e-5 for every family (BARS), plus 2^-11 where y /
out2 are stored as fp16; the GDN / IGDN epilogue is also checked on the kernel's own arithmetic (y from the device out2)
at 1e-6.  Every test prints its figures before it asserts (``-s``).

Worst error per family on an MI355X (1049 cases, 1693 tests, 5.3 s; the slowest test 0.8 s, the first to load the
library): conv_fwd_kernel 1.8e-6, conv_fwd_b6_kernel 2.2e-6, conv_fwd_b6db_kernel 7.5e-7, conv_fwd_h_kernel 3.0e-7 with an
fp32 Y and 4.2e-4 with an fp16 Y (bar 1e-5 + 4.9e-4), conv_narrow_kernel 2.7e-7, conv_narrow_strip_kernel 1.8e-7 (the
split reduces are part of the tiles launch that names them); y from the device GDN norm 9.0e-8.  All at most 2.5e-6, so
every bar is 1e-5: the K depth is at most 5760 products (640 x 3 x 3) of O(1) terms, accumulated in fp32 from products
that are exact (fp16), fp32-rounded, or bf16x6 (2^-25).  No kernel bug was found.

Mutations (each a scratch copy of the source with one line changed, values or in-bounds reads only, linked with the
other objects and run over CASES; failing tests of 1693). They were made when the whole family was in csrc/conv.hip;
epi_store (1-3) is now in csrc/conv_epilogue.h, conv_fwd_body and the split reduces (4-7) in csrc/conv_gemm.hip.
Mutations 1, 4 and 7 were applied again to that text (shared row stores, one lambda per MFMA flavour): 570, 500 and 1330
failing, the counts below:
1. epi_store subtracts the bias: 570, every scalar-epilogue case with a bias (Co = 42 / 70, odd pitches, pointers one
   element off, every narrow case, the scalar split reduce); no float4 case.
2. epi_store ignores accumulate (fp32 Y): 258, the accumulate cases on the scalar path (epi/*-a*/co42 | ld | ptr,
   nar/*-key13off, split/acc-scalar, split/deconv-misaligned); float4 and fp16-Y accumulate cases pass.
3. epi_store reads the GDN-backward norm with ld0 for ld2: 26, exactly the cases whose aux2 pitch differs from aux0's
   (epi/*gdnbwd*/ld-aux2+1, epi/*igdnbwd*/ld-aux0+1, split/gdnbwd-ld2+1).
4. the last K chunk of a ragged last split dropped: 500, every split whose nk % cps != 0 (the 3x3 Ci = 32 splits 5 + 4,
   split/k5-minchunks3-last1 7 x 4 - 3, split/k3-64-last3, the phases of ph/deconv-5x7-split); fused cases pass.
5. the phase's tap0 omitted from the weight column: 54, the 4-phase cases (ph/deconv-*, ph/dgrad-k*s2-*, their b6/, dt/
   and split/ variants) and nothing single-phase.
6. conv_splitk_reduce_kernel skips the last slab: 339, every split case with the scalar reduce (Co % 4 != 0, an odd pitch,
   a misaligned pointer or workspace); the reduce4 cases pass.
7. a_base computed from image 0 instead of the block's first image: 1330, every tiles case with a block that starts past
   image 0 (M = 70 at BM 64 and up: m/hw35-bm64, m/hw63-*, xcd/*, the epilogue cross); m/hw1, m/hw15 (one block) pass.
"""
import ctypes
import functools
import json
import os
from dataclasses import dataclass, replace

import pytest
import torch

import conv_ref as CR
from helpers import rel_err

CEIL = 1e-4            # test_parity_gpu.TOL
F16_STORE = 2.0 ** -11  # one rounding of a stored fp16 result
SENT = -777.0
PAD = 64
BIAS, GDN, IGDN, GDN_BWD, IGDN_BWD, ROWSCALE, SA_BWD = range(7)
NONE, RELU, PRELU, RELU_MASK = range(4)
KIND_NAME = ["bias", "gdn", "igdn", "gdnbwd", "igdnbwd", "rowscale", "sabwd"]
ACT_NAME = ["", "-relu", "-prelu", "-mask"]
SLOPE = 0.25

# family -> bar: 1e-5, the weight-gradient file's bar for the same arithmetic at the same K depths; every family's worst
# measured error is at most 2.5e-6 (module docstring)
BARS = {"conv_fwd_kernel": 1e-5, "conv_fwd_b6_kernel": 1e-5, "conv_fwd_b6db_kernel": 1e-5, "conv_fwd_h_kernel": 1e-5,
        "conv_narrow_kernel": 1e-5, "conv_narrow_strip_kernel": 1e-5}
WORST = {}


@dataclass(frozen=True)
class Case:
    """geom: ("conv" | "dgrad", B, H, W, Ci, Co, KH, KW, stride, pad, dil) | ("deconv" | "deconv_dgrad", B, H, W, Ci, Co)
    (K = 5, padding 2, as the model's) | ("mconv" | "mdgrad", B, H, W, Ci, Co) (the checkerboard-masked 5x5, padding 2,
    and its input-gradient, on its 12 live taps); (B, H, W, Ci, Co) are the ORIGINAL layer's.
    pitch: ((operand, extra elements per row), ...), off: ((operand, elements past a 256-byte aligned address), ...) with
    operands x, y, w, bias, res, aux0, aux1, aux2, out2.  ws: full | none | short | misaligned."""
    id: str
    geom: tuple
    kind: int = BIAS
    act: int = NONE
    bias: bool = True
    res: bool = False
    out2: bool = False
    acc: bool = False
    sq: bool = False
    f16: int = 0
    io: int = 0
    pitch: tuple = ()
    off: tuple = ()
    ws: str = "full"
    tune: tuple = ()
    only: int = -1  # run under this value of key 7 only (-1: both where the name differs)


def cv(B, H, W, Ci, Co, K, s=1, p=None, d=1, kind="conv"):
    return (kind, B, H, W, Ci, Co, K, K, s, d * (K // 2) if p is None else p, d)


CASES = []


def _add(id, geom, **kw):
    CASES.append(Case(id, geom, **kw))


# ---- M / image raggedness: tiles across images, M tails, tile counts for the XCD remap (all fused: no workspace)
for _h, _w in ((1, 1), (3, 5), (5, 7), (7, 9)):
    _add(f"m/hw{_h * _w}-bm128", cv(3, _h, _w, 32, 64, 3), ws="none", tune=((0, 1),))
    _add(f"m/hw{_h * _w}-bm64", cv(3, _h, _w, 32, 64, 3), ws="none")
    _add(f"m/hw{_h * _w}-bm64-split", cv(3, _h, _w, 32, 64, 3))
_add("m/tail1-bm64", cv(1, 5, 13, 32, 64, 3), ws="none")
_add("m/tail63-bm64", cv(1, 7, 9, 32, 64, 3), ws="none")
_add("m/tail127-bm128", cv(3, 9, 33, 32, 64, 3, s=2), ws="none", tune=((0, 1),))
_add("m/tail61-bm128", cv(3, 7, 9, 32, 64, 5), ws="none", tune=((0, 0),))
_add("xcd/7-tiles", cv(3, 12, 12, 32, 64, 3), ws="none")
_add("xcd/8-tiles", cv(2, 12, 20, 32, 64, 3), ws="none")
_add("xcd/9-tiles", cv(3, 9, 20, 32, 64, 3), ws="none")
_add("xcd/17-tiles", cv(2, 13, 33, 32, 64, 3, p=2), ws="none")
_add("xcd/9x3-tiles", cv(3, 9, 20, 32, 132, 3), ws="none", tune=((0, 4),))
# ---- Co raggedness across BN 32 / 64 / 128: Co % 4 != 0 -> scalar epilogue, Co % 4 == 0 with a BN tail -> float4
for _co in (40, 42, 70, 132, 136):
    for _t, _bn in ((2, 32), (4, 64), (0, 128)):
        _add(f"co/{_co}-bn{_bn}", cv(2, 5, 7, 32, _co, 3), ws="none", tune=((0, _t),), res=True, act=RELU)
# ---- K: taps, dilation, stride; MODE 2 (Ci % 32 != 0: the tap crossing inside a chunk); MODE 1 (square_input)
for _n, _g in (("k1", cv(2, 9, 12, 32, 64, 1)), ("k3", cv(2, 9, 12, 32, 64, 3)), ("k3d2", cv(2, 9, 12, 32, 64, 3, d=2)),
               ("k5", cv(2, 9, 12, 32, 64, 5)), ("k5s2", cv(2, 9, 12, 32, 64, 5, s=2)),
               ("k3s2-96to40", cv(2, 9, 13, 96, 40, 3, s=2)), ("k5s2-odd", cv(3, 7, 13, 32, 40, 5, s=2))):
    _add(f"k/{_n}", _g)
    _add(f"k/{_n}-fused", _g, ws="none")
for _ci, _k in ((1, 3), (3, 3), (5, 3), (3, 5), (5, 5)):
    for _co in (5, 64, 70):
        _add(f"k/m2-ci{_ci}-k{_k}-co{_co}", cv(2, 9, 13, _ci, _co, _k))
for _ci in (40, 70):
    _add(f"k/m2-ci{_ci}-k3", cv(2, 9, 13, _ci, 64, 3), ws="none")
    _add(f"k/m2-ci{_ci}-k3-split", cv(2, 9, 13, _ci, 64, 3))
    _add(f"k/m2-ci{_ci}-k3s2", cv(2, 9, 13, _ci, 42, 3, s=2), ws="none")
    _add(f"k/m2-ci{_ci}-k3d2", cv(2, 9, 13, _ci, 64, 3, d=2), ws="none", pitch=(("x", 1), ("w", 1)),
         off=(("x", 1), ("w", 3)))
    _add(f"k/m2-ci{_ci}-k5s2-split-scalar", cv(2, 9, 13, _ci, 42, 5, s=2))
_add("k/m1-1x1-64", cv(2, 5, 7, 64, 64, 1), sq=True, kind=GDN)
_add("k/m1-1x1-64-igdn-ld", cv(2, 5, 7, 64, 64, 1), sq=True, kind=IGDN, pitch=(("x", 4), ("y", 4), ("aux0", 8)))
_add("k/m1-k3-64", cv(2, 5, 7, 64, 64, 3), sq=True, ws="none")
_add("k/m1-k3-64-split", cv(2, 5, 7, 64, 64, 3), sq=True)
_add("k/m1-1x1-64to96", cv(2, 5, 7, 64, 96, 1), sq=True)
_add("k/m1-k3s2-64to42", cv(2, 5, 7, 64, 42, 3, s=2), sq=True, ws="none")
_add("k/m1-k3-64to42-split", cv(2, 5, 7, 64, 42, 3), sq=True)
# ---- strided / offset operands on the vector path: a read one column past Ci lands on NaN
_LD = cv(2, 5, 7, 64, 40, 3)
_add("ld/x+4", _LD, ws="none", pitch=(("x", 4),))
_add("ld/x+32-xoff4", _LD, ws="none", pitch=(("x", 32),), off=(("x", 4),))
_add("ld/w+4-woff4", _LD, ws="none", pitch=(("w", 4),), off=(("w", 4),))
_add("ld/y+4-yoff4", _LD, ws="none", pitch=(("y", 4),), off=(("y", 4),))
_add("ld/y+1", _LD, ws="none", pitch=(("y", 1),))
_add("ld/yoff1-split", _LD, off=(("y", 1),))
_add("ld/all+4-split", _LD, pitch=(("x", 4), ("w", 8), ("y", 12), ("res", 4)), res=True, act=PRELU)
# ---- phases: deconv forward, stride-2 conv dgrad (odd and even base grids), stride-1 dgrad, deconv dgrad, masked
for _h, _w in ((1, 1), (3, 4), (4, 5), (5, 7), (7, 3)):
    _add(f"ph/deconv-{_h}x{_w}", ("deconv", 2, _h, _w, 32, 40), ws="none")
    _add(f"ph/dgrad-k5s2-{_h}x{_w}", cv(2, 2 * _h, 2 * _w, 40, 32, 5, s=2, kind="dgrad"), ws="none")
    _add(f"ph/dgrad-k3s2-{_h}x{_w}", cv(2, 2 * _h, 2 * _w, 42, 32, 3, s=2, kind="dgrad"), ws="none")
_add("ph/deconv-5x7-split", ("deconv", 2, 5, 7, 64, 40))
_add("ph/deconv-3x4-co70-ld", ("deconv", 3, 3, 4, 32, 70), ws="none", pitch=(("x", 4), ("y", 2)))
_add("ph/dgrad-k5s2-3x4-split", cv(2, 6, 8, 40, 64, 5, s=2, kind="dgrad"))
_add("ph/dgrad-k3s1", cv(2, 5, 7, 40, 32, 3, kind="dgrad"), ws="none")
_add("ph/dgrad-k5s1", cv(2, 5, 7, 42, 32, 5, kind="dgrad"))
_add("ph/dgrad-k3d2", cv(2, 5, 7, 40, 64, 3, d=2, kind="dgrad"), ws="none", act=RELU_MASK)
_add("ph/dgrad-k3s1-to3", cv(2, 5, 7, 3, 32, 3, kind="dgrad"), ws="none")
_add("ph/deconv-dgrad-3x4", ("deconv_dgrad", 2, 3, 4, 40, 32), ws="none")
_add("ph/deconv-dgrad-5x7-split", ("deconv_dgrad", 2, 5, 7, 42, 64), acc=True)
for _ci, _co in ((32, 40), (64, 64), (5, 42)):
    _add(f"ph/mconv-{_ci}to{_co}", ("mconv", 2, 5, 7, _ci, _co), ws="none")
    _add(f"ph/mconv-{_ci}to{_co}-split", ("mconv", 2, 5, 7, _ci, _co))
    if _co % 32 == 0:
        _add(f"ph/mdgrad-{_ci}to{_co}", ("mdgrad", 2, 5, 7, _ci, _co), ws="none")
_add("ph/mdgrad-40to32-split", ("mdgrad", 2, 5, 7, 40, 32))
# ---- split-K: the four workspace modes, ragged last splits, phases, epilogues behind the reduce kernels
_SP = cv(1, 4, 4, 640, 128, 3)
for _ws in ("full", "none", "short", "misaligned"):
    _add(f"split/640-{_ws}", _SP, ws=_ws)
    _add(f"split/64to40-{_ws}", cv(2, 5, 7, 64, 40, 3), ws=_ws, res=True, act=RELU)
_add("split/k5-minchunks3-last1", cv(2, 5, 7, 32, 64, 5), tune=((2, 3),))
_add("split/k5-minchunks3-last1-scalar", cv(2, 5, 7, 32, 42, 5), tune=((2, 3),))
_add("split/k3-64-last3", cv(2, 5, 7, 64, 64, 3))
_add("split/k3-64-blocks16", cv(2, 5, 7, 64, 64, 3), tune=((1, 16), (2, 1)))
_add("split/deconv-misaligned", ("deconv", 2, 3, 4, 64, 40), ws="misaligned", acc=True)
_add("split/deconv-co42", ("deconv", 2, 3, 4, 64, 42), res=True, act=RELU)
_add("split/acc", cv(2, 5, 7, 64, 40, 3), acc=True)
_add("split/acc-scalar", cv(2, 5, 7, 64, 42, 3), acc=True, out2=True)
_add("split/y16", cv(2, 5, 7, 64, 40, 3), io=2, res=True, act=RELU)
_add("split/y16-acc-scalar", cv(2, 5, 7, 64, 42, 3), io=2, acc=True)
_add("split/y16-misaligned", cv(2, 5, 7, 64, 40, 3), io=3, ws="misaligned", out2=True)
_add("split/gdnbwd", cv(2, 5, 7, 64, 40, 3), kind=GDN_BWD)
_add("split/gdnbwd-ld2+1", cv(2, 5, 7, 64, 40, 3), kind=IGDN_BWD, pitch=(("aux2", 1),))
_add("split/sabwd", cv(2, 5, 7, 64, 40, 3), kind=SA_BWD, acc=True)
_add("split/rowscale-co42", cv(2, 5, 7, 64, 42, 3), kind=ROWSCALE, res=True, act=PRELU)
# ---- the epilogue cross on a 3x3 (fused and behind the split reduce) and a 1x1: every kind with every activation it
# accepts, flag variants, on the float4 path and on the scalar path reached three ways
_BIASF = ((False, False, False, False), (True, True, False, False), (True, False, True, True), (False, True, True, True))
EPI = ([(BIAS, a, f) for a in (NONE, RELU, PRELU, RELU_MASK) for f in _BIASF]
       + [(ROWSCALE, a, f[:3] + (False,)) for a in (NONE, RELU, PRELU) for f in _BIASF]
       + [(k, NONE, (True, False, False, a)) for k in (GDN, IGDN) for a in (False, True)]
       + [(k, NONE, (False, False, False, a)) for k in (GDN_BWD, IGDN_BWD, SA_BWD) for a in (False, True)])
_VEC_OPS = {BIAS: ("res", "out2", "aux0", "bias"), ROWSCALE: ("res", "out2", "bias"), GDN: ("aux0", "out2", "bias"),
            IGDN: ("out2", "aux0", "bias"), GDN_BWD: ("aux2", "aux1", "aux0"), IGDN_BWD: ("aux0", "aux2", "aux1"),
            SA_BWD: ()}


def present(c):
    """The epilogue operands a case passes."""
    p = []
    if c.bias and c.kind in (BIAS, ROWSCALE, GDN, IGDN):
        p.append("bias")
    if c.res:
        p.append("res")
    if c.act == RELU_MASK or c.kind in (GDN, IGDN, GDN_BWD, IGDN_BWD, SA_BWD):
        p.append("aux0")
    if c.kind in (GDN_BWD, IGDN_BWD, ROWSCALE):
        p.append("aux1")
    if c.kind in (GDN_BWD, IGDN_BWD, SA_BWD):
        p.append("aux2")
    if c.out2 or c.kind in (GDN, IGDN):
        p.append("out2")
    return p


for _gn, _mk, _wss in (("3x3", lambda co: cv(2, 5, 7, 32, co, 3), ("none", "full")),
                       ("1x1", lambda co: cv(2, 5, 7, 64, co, 1), ("none",))):
    for _kind, _act, (_b, _r, _o, _a) in EPI:
        for _ws in _wss:
            _base = Case("", _mk(40), kind=_kind, act=_act, bias=_b, res=_r, out2=_o, acc=_a, ws=_ws)
            _ops = [o for o in _VEC_OPS[_kind] if o in present(_base) and (o != "bias")]
            _pit = (_ops[0] if _ops else "y")
            _ptr = ([o for o in _VEC_OPS[_kind] if o in present(_base)] or ["y"])[-1]
            _fl = f"{'b' if _b else ''}{'r' if _r else ''}{'o' if _o else ''}{'a' if _a else ''}" or "0"
            _id = f"epi/{_gn}-{KIND_NAME[_kind]}{ACT_NAME[_act]}-{_fl}{'-split' if _ws == 'full' else ''}"
            CASES.append(replace(_base, id=_id + "/v4"))
            CASES.append(replace(_base, id=_id + "/co42", geom=_mk(42)))
            CASES.append(replace(_base, id=_id + f"/ld-{_pit}+1", pitch=((_pit, 1),)))
            CASES.append(replace(_base, id=_id + f"/ptr-{_ptr}+1", off=((_ptr, 1),)))
# ---- dtypes: f16_operands alone; fp16 X / Y on conv_fwd_h_kernel across the kinds it accepts; AUX16; fp16-Y accumulate
_add("dt/f16-k3", cv(2, 5, 7, 64, 40, 3), f16=1, ws="none")
_add("dt/f16-k3-split-co42", cv(2, 5, 7, 64, 42, 3), f16=1, res=True, act=PRELU)
_add("dt/f16-gdn", cv(2, 5, 7, 64, 64, 1), f16=1, sq=True, kind=GDN)
_add("dt/f16-deconv", ("deconv", 2, 3, 4, 64, 40), f16=1, ws="none")
_add("dt/f16-m2-ignored", cv(2, 5, 7, 3, 40, 3), f16=1)
for _io in (1, 2, 3):
    for _co in (40, 42):
        for _kn, _g in (("k1", cv(2, 5, 7, 64, _co, 1)), ("k3", cv(2, 5, 7, 64, _co, 3))):
            _p = f"dt/io{_io}-{_kn}-co{_co}"
            _add(f"{_p}-bias", _g, io=_io, ws="none")
            _add(f"{_p}-relu-res-out2", _g, io=_io, ws="none", act=RELU, res=True, out2=True)
            _add(f"{_p}-prelu-nobias", _g, io=_io, ws="none", act=PRELU, bias=False)
            _add(f"{_p}-mask-acc", _g, io=_io, ws="none", act=RELU_MASK, acc=True)
            _add(f"{_p}-rowscale-res", _g, io=_io, ws="none", kind=ROWSCALE, res=True, act=RELU)
            if _io & 2:
                _add(f"{_p}-gdnbwd", _g, io=_io, ws="none", kind=GDN_BWD)
                _add(f"{_p}-igdnbwd-acc", _g, io=_io, ws="none", kind=IGDN_BWD, acc=True)
            else:
                _add(f"{_p}-sabwd", _g, io=_io, ws="none", kind=SA_BWD)
    _add(f"dt/io{_io}-gdn", cv(2, 5, 7, 64, 64, 1), io=_io, sq=True, kind=GDN)
    _add(f"dt/io{_io}-igdn-ld", cv(2, 5, 7, 64, 64, 1), io=_io, sq=True, kind=IGDN, pitch=(("aux0", 4), ("out2", 8)))
    _add(f"dt/io{_io}-deconv-co42", ("deconv", 2, 3, 4, 64, 42), io=_io, ws="none", res=True)
_add("dt/io2-m2-ci3", cv(2, 9, 13, 3, 64, 3), io=2, act=RELU)
_add("dt/io2-m2-ci5-co42-k5", cv(2, 9, 13, 5, 42, 5), io=2, res=True)
for _co in (40, 42):
    _g = cv(2, 5, 7, 64, _co, 3)
    _add(f"dt/aux16-mask-co{_co}", _g, io=4, ws="none", act=RELU_MASK)
    _add(f"dt/aux16-mask-co{_co}-split-acc", _g, io=4, act=RELU_MASK, acc=True)
    _add(f"dt/aux16-gdnbwd-co{_co}", _g, io=4, ws="none", kind=GDN_BWD)
    _add(f"dt/aux16-igdnbwd-co{_co}-split", _g, io=4, kind=IGDN_BWD, acc=True)
# ---- every tile x MODE x split x epilogue width of every GEMM variant (the coverage the CPU file checks)
for _t in range(5):
    for _ws in ("none", "full"):
        for _co in (136, 70):
            _kw = dict(ws=_ws, tune=((0, _t),), res=True, act=RELU)
            _s = f"t{_t}-{'split' if _ws == 'full' else 'fused'}-co{_co}"
            _add(f"cover/m0-{_s}", cv(2, 5, 7, 64, _co, 3), **_kw)
            _add(f"cover/m1-{_s}", cv(2, 5, 7, 64, _co, 3), sq=True, **_kw)
            _add(f"cover/m2-{_s}", cv(2, 5, 7, 40, _co, 3), **_kw)
            _add(f"cover/f16-m0-{_s}", cv(2, 5, 7, 64, _co, 3), f16=1, **_kw)
            _add(f"cover/f16-m1-{_s}", cv(2, 5, 7, 64, _co, 3), f16=1, sq=True, **_kw)
            for _io in (1, 2, 3):
                _add(f"cover/io{_io}-m0-{_s}", cv(2, 5, 7, 64, _co, 3), io=_io, **_kw)
                _add(f"cover/io{_io}-m1-{_s}", cv(2, 5, 7, 64, _co, 3), io=_io, sq=True, **_kw)
            _add(f"cover/io2-m2-{_s}", cv(2, 5, 7, 40, _co, 3), io=2, **_kw)
# ---- bf16x6: unswizzled LDS rows (key 19 = 0) and the double-buffered 64x64 kernel (key 20 = 1) at the ragged cases
_B6 = ["m/hw1-bm64", "m/hw15-bm64", "m/hw35-bm128", "m/hw63-bm64-split", "m/tail1-bm64", "m/tail127-bm128", "xcd/9-tiles",
       "co/42-bn64", "co/136-bn64", "co/70-bn128", "ph/deconv-5x7", "ph/deconv-5x7-split", "ph/dgrad-k5s2-3x4",
       "ph/dgrad-k3s2-7x3", "split/k5-minchunks3-last1", "split/k5-minchunks3-last1-scalar", "split/deconv-misaligned",
       "k/m1-k3-64", "k/m1-k3-64-split", "k/m1-1x1-64", "k/m1-k3s2-64to42", "k/m1-k3-64to42-split"]
for _c in [c for c in CASES if c.id in _B6]:
    CASES.append(replace(_c, id="b6/sw0-" + _c.id, tune=_c.tune + ((19, 0),), only=1))
    CASES.append(replace(_c, id="b6/db-" + _c.id, tune=tuple(t for t in _c.tune if t[0] != 0) + ((0, 4), (20, 1)), only=1))
assert len([c for c in CASES if c.id.startswith("b6/")]) == 2 * len(_B6)
# ---- narrow (Co <= 4, Ci = 64 / 128): plain and strip, fp16 X, phases, the weight-staging limit
for _co in (1, 2, 3, 4):
    for _ci in (64, 128):
        _add(f"nar/{_ci}to{_co}-k3-strip", cv(2, 5, 8, _ci, _co, 3))
        _add(f"nar/{_ci}to{_co}-k3-w7", cv(2, 5, 7, _ci, _co, 3), res=True, act=RELU)
        _add(f"nar/{_ci}to{_co}-k3-key13off", cv(2, 5, 8, _ci, _co, 3), tune=((13, 0),), acc=True)
        _add(f"nar/{_ci}to{_co}-k3-strip-x16", cv(3, 5, 4, _ci, _co, 3), io=1, out2=True, act=PRELU)
        _add(f"nar/{_ci}to{_co}-k3-w7-x16", cv(3, 3, 7, _ci, _co, 3), io=1)
for _ci in (64, 128):
    _add(f"nar/deconv-{_ci}to3-strip", ("deconv", 2, 3, 4, _ci, 3))
    _add(f"nar/deconv-{_ci}to3-w5", ("deconv", 2, 3, 5, _ci, 3), pitch=(("x", 4), ("y", 1)))
    _add(f"nar/deconv-{_ci}to3-strip-x16", ("deconv", 3, 5, 12, _ci, 3), io=1, act=RELU)
    _add(f"nar/{_ci}to3-k1", cv(3, 7, 12, _ci, 3, 1), pitch=(("x", 8), ("w", 4)), off=(("x", 4), ("y", 1)))
    _add(f"nar/dgrad-3to{_ci}-k3", cv(2, 9, 12, 3, _ci, 3, kind="dgrad"), acc=True)
    _add(f"nar/{_ci}to2-k3d2", cv(2, 9, 12, _ci, 2, 3, d=2))
    _add(f"nar/{_ci}to2-k3s2", cv(2, 9, 12, _ci, 2, 3, s=2))
_add("nar/64to3-k5", cv(2, 5, 8, 64, 3, 5))
_add("nar/128to2-k5", cv(2, 5, 8, 128, 2, 5, s=2))
_add("nar/3x13x20-64to3-two-blocks", cv(3, 13, 20, 64, 3, 3))
_add("nar/3x13x20-64to3-two-blocks-plain", cv(3, 13, 20, 64, 3, 3), tune=((13, 0),))
_add("nar/limit-128to4-k4x4", ("conv", 2, 5, 8, 128, 4, 4, 4, 1, 1, 1))
_add("nar/over-limit-128to4-k3x6-tiles", ("conv", 2, 5, 8, 128, 4, 3, 6, 1, 2, 1), ws="none")
_add("nar/over-limit-128to3-k5-tiles", cv(2, 5, 8, 128, 3, 5))

BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES), [c.id for c in CASES if sum(d.id == c.id for d in CASES) > 1]

# case id -> [name, vec4], or [[name, vec4] native, [name, vec4] bf16x6] where the fp32 GEMM mode changes it: recorded
# from the library's own query by tests/golden/make_conv_kernels.py, checked against the built library on the CPU
with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "conv_kernels.json")) as _f:
    KERNELS = json.load(_f)


def recorded(c, mode):
    k = KERNELS[c.id]
    return tuple(k) if isinstance(k[0], str) else tuple(k[mode])


def modes_of(c):
    if c.only >= 0:
        return (c.only,)
    return (1,) if isinstance(KERNELS[c.id][0], str) else (0, 1)


# ------------------------------------------------------------------------------------------------- host-only pieces
def _L():
    from hyres_hip import _lib as L
    return L


class tuned:
    """hyres_conv_tuning keys set for a block and restored after it."""

    def __init__(self, lib, keys):
        self.lib, self.keys, self.old = lib, dict(keys), {}

    def __enter__(self):
        try:
            for k, v in self.keys.items():
                o = ctypes.c_int(0)
                assert self.lib.hyres_conv_tuning(k, v, ctypes.byref(o)) == 0
                self.old[k] = o.value
        except BaseException:
            self.__exit__()
            raise
        return self

    def __exit__(self, *exc):
        for k, v in self.old.items():
            assert self.lib.hyres_conv_tuning(k, v, None) == 0
        return False


def pitch_of(c, name):
    return dict(c.pitch).get(name, 0)


def off_of(c, name):
    return dict(c.off).get(name, 0)


def layer_of(c):
    """(conv_ref geometry, mask kind): the masked kinds are a 5x5 conv / its input-gradient with the checkerboard mask."""
    if c.geom[0] in ("mconv", "mdgrad"):
        B, H, W, Ci, Co = c.geom[1:]
        return ("conv" if c.geom[0] == "mconv" else "dgrad", B, H, W, Ci, Co, 5, 5, 1, 2, 1), True
    return c.geom, False


def make_geom(L, c):
    """(hyres_conv_geom, weight-prep arguments (mode, Ci, Co, KH, KW, pad)) of a case; host only."""
    g = L.ConvGeom()
    geom, masked = layer_of(c)
    kind, B, H, W, Ci, Co = geom[:6]
    if kind in ("conv", "dgrad"):
        KH, KW, s, p, d = geom[6:]
        gci, gco = (Ci, Co) if kind == "conv" else (Co, Ci)
        # conv: (ldx, ldy) = the input's / output's pitch; dgrad: (ld_dx, ld_dy) = the OUTPUT's / INPUT's pitch
        lda, ldb = (gci + pitch_of(c, "x"), gco + pitch_of(c, "y")) if kind == "conv" else \
                   (gco + pitch_of(c, "y"), gci + pitch_of(c, "x"))
        L.call("hyres_geom_conv2d" if kind == "conv" else "hyres_geom_conv2d_dgrad", ctypes.byref(g), B, H, W, Ci, lda, Co,
               ldb, KH, KW, s, p, d)
        prep = (L.WPREP_CONV if kind == "conv" else L.WPREP_CONV_DGRAD, Ci, Co, KH, KW, p)
        if masked:
            keep = (ctypes.c_ubyte * 25)(*[v for row in CR.checkerboard_keep() for v in row])
            L.call("hyres_geom_filter_taps", ctypes.byref(g), keep, 5)
            assert g.ntaps == 12
    elif kind == "deconv":
        L.call("hyres_geom_deconv2d", ctypes.byref(g), B, H, W, Ci, Ci + pitch_of(c, "x"), Co, Co + pitch_of(c, "y"), 5, 2)
        prep = (L.WPREP_DECONV, Ci, Co, 5, 5, 2)
    else:
        assert kind == "deconv_dgrad"
        L.call("hyres_geom_deconv2d_dgrad", ctypes.byref(g), B, H, W, Ci, Ci + pitch_of(c, "y"), Co, Co + pitch_of(c, "x"),
               5, 2)
        prep = (L.WPREP_DECONV_DGRAD, Ci, Co, 5, 5, 2)
    assert g.ldx == g.Ci + pitch_of(c, "x") and g.ldy == g.Co + pitch_of(c, "y")
    return g, prep


def y16(c):
    return bool(c.io & 2)


def opnd_spec(c, g, name):
    """(columns, pitch, torch dtype) of an epilogue operand / of y: [P][columns] rows of ``pitch`` elements."""
    h = torch.float16
    f = torch.float32
    if name == "bias":
        return g.Co, g.Co, f
    if c.kind == ROWSCALE and name == "aux1":
        return 1, 1 + pitch_of(c, name), f
    if c.kind == SA_BWD and name == "aux0":
        return 2, 2 + pitch_of(c, name), f
    if c.kind == SA_BWD and name == "aux2":
        return 1, 1 + pitch_of(c, name), torch.int32
    half = y16(c) or (c.io == 4 and name in ("aux0", "aux2"))
    return g.Co, g.Co + pitch_of(c, name), h if half else f


def esize(dt):
    return 2 if dt == torch.float16 else 4


def make_epi(L, c, g, ptrs):
    """hyres_epilogue of a case; ptrs: operand name -> address (absent operands are not looked up)."""
    e = L.Epilogue()
    e.kind, e.act, e.accumulate, e.square_input = c.kind, c.act, int(c.acc), int(c.sq)
    e.f16_operands, e.io_f16 = c.f16, c.io
    for name in present(c):
        setattr(e, name, ptrs[name])
        if name != "bias":
            setattr(e, {"res": "ldres", "aux0": "ld0", "aux1": "ld1", "aux2": "ld2", "out2": "ldo2"}[name],
                    opnd_spec(c, g, name)[1])
    if c.act == PRELU:
        e.slope = ptrs["slope"]
    return e


def exact_split_bytes(L, g, e):
    """The slab of the ideal plan: nsplit * nphase * M * Co floats (hyres_conv_plan's nsplit)."""
    ns = ctypes.c_int(0)
    L.call("hyres_conv_plan", ctypes.byref(g), ctypes.byref(e), None, ctypes.byref(ns))
    return ns.value, (ns.value * g.nphase * g.B * g.Hq * g.Wq * g.Co * 4 if ns.value > 1 else 0)


def ws_bytes(L, c, g, e):
    """(bytes passed, floats to allocate, element offset) of the workspace under the case's mode."""
    full = int(L.load().hyres_conv_workspace_bytes(ctypes.byref(g)))
    if c.ws == "none":
        return 0, 0, 0
    if c.ws == "short":
        ns, need = exact_split_bytes(L, g, e)
        assert ns > 1, "a short workspace needs a plan that splits"
        return need - 4, need // 4, 0
    return full, full // 4, int(c.ws == "misaligned")


def fake_ptrs(c, g):
    """Addresses with the case's alignments, for the host-only name query (never dereferenced)."""
    p = {"slope": 0x7000000}
    for i, name in enumerate(("x", "y", "w", "bias", "res", "aux0", "aux1", "aux2", "out2")):
        if name == "x":
            es = 2 if c.io & 1 else 4
        elif name == "w":
            es = 4
        elif name == "y":
            es = 2 if y16(c) else 4
        else:
            es = esize(opnd_spec(c, g, name)[2])
        p[name] = 0x1000000 * (i + 1) + off_of(c, name) * es
    return p


def query(L, c, mode, ptrs=None, ws_ptr=None):
    """(kernel name, vec4) hyres_conv_kernel_name_at reports for the case under GEMM ``mode``; host only."""
    lib = L.load()
    with tuned(lib, {**dict(c.tune), 7: mode}):
        g, _ = make_geom(L, c)
        ptrs = fake_ptrs(c, g) if ptrs is None else ptrs
        e = make_epi(L, c, g, ptrs)
        nbytes, _, woff = ws_bytes(L, c, g, e)
        if ws_ptr is None:
            ws_ptr = 0x9000000 + 4 * woff
        buf = ctypes.create_string_buffer(160)
        v4 = ctypes.c_int(-1)
        L.call("hyres_conv_kernel_name_at", ctypes.byref(g), ctypes.byref(e), ptrs["x"], ptrs["w"],
               g.ntaps * g.Ci + pitch_of(c, "w"), ptrs["y"], None if c.ws == "none" else ws_ptr, nbytes,
               ctypes.byref(v4), buf, len(buf))
    return buf.value.decode(), v4.value


def staged_f16(c, name):
    """X and W2 are rounded to fp16 when staged: the f16 / fp16-IO tiles off the scalar-load path."""
    return name.startswith("conv_fwd_h_kernel") and ", 2, true, 2>" not in name and ", 2, false, 2>" not in name or \
        (name.startswith("conv_fwd_kernel") and name.split("+")[0].endswith(", true>"))


@functools.lru_cache(maxsize=16)
def conv_data(geom_key, sq, pos, x16, f16k, grid):
    """x (as the kernel is given it), w (PyTorch layout, fp32), mask and the fp64 GEMM result of one layer."""
    c = Case("data", geom_key)
    geom, masked = layer_of(c)
    kind, B, H, W, Ci, Co = geom[:6]
    if kind in ("conv", "dgrad"):
        KH, KW, s, p, d = geom[6:]
        Ho, Wo = (H + 2 * p - d * (KH - 1) - 1) // s + 1, (W + 2 * p - d * (KW - 1) - 1) // s + 1
        wshape = (Co, Ci, KH, KW)
        xshape = (B, H, W, Ci) if kind == "conv" else (B, Ho, Wo, Co)
    else:
        wshape = (Ci, Co, 5, 5)
        xshape = (B, H, W, Ci) if kind == "deconv" else (B, 2 * H, 2 * W, Co)
    x = CR.grid32(xshape, 1) if grid else CR.rand(xshape, 1)
    w = CR.rand(wshape, 2, (wshape[2] * wshape[3] * xshape[3] / 4) ** -0.5)
    if pos:
        x, w = x.abs(), w.abs()
    if x16:
        x = x.half()
    mask = None
    if masked:
        mask = torch.tensor(CR.checkerboard_keep(), dtype=torch.float32).expand(wshape).contiguous()
    xr, wr = (x.half(), w.half()) if f16k else (x, w)
    return x, w, mask, CR.torch_acc(geom, xr, wr, mask, square=sq)


def epi_data(c, P, Co):
    """name -> the epilogue operand as the kernel is given it ([P, columns]; bias [Co]); y_old for accumulate."""
    d = {}
    for name in present(c):
        seed = 10 + ("bias", "res", "aux0", "aux1", "aux2", "out2").index(name)
        if name == "out2":
            continue
        if name == "bias":
            v = CR.rand((Co,), seed, 0.5)
            v = 1 + v.abs() if c.kind in (GDN, IGDN) else v
        elif c.kind == SA_BWD and name == "aux2":  # argmax at channel 0, at Co - 1, inside the Co tail, anywhere
            p = torch.arange(P)
            v = torch.stack([torch.zeros(P), torch.full((P,), Co - 1.0), torch.full((P,), float((Co - 1) // 32 * 32 + 1)),
                             (p * 7 % Co).float()])[p % 4, p].to(torch.int32).view(P, 1)
        elif c.kind == SA_BWD:
            v = CR.rand((P, 2), seed)
        elif c.kind == ROWSCALE and name == "aux1":
            v = CR.rand((P, 1), seed)
        elif name == "aux2":  # the GDN norm: bounded away from 0
            v = 1 + CR.rand((P, Co), seed).abs()
        elif name == "aux0" and c.act == RELU_MASK:  # both signs and exact zeros
            v = CR.rand((P, Co), seed)
            v = torch.where(v.abs() < 0.3, torch.zeros(()), v)
        else:
            v = CR.rand((P, Co), seed)
        d[name] = v
    if c.acc:
        d["y_old"] = CR.rand((P, Co), 20)
    return d


# ------------------------------------------------------------------------------------------------------ GPU side
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


class Buf:
    """``n`` elements ``off`` elements past a 256-byte aligned address, between guards of ``fill``."""

    def __init__(self, n, dtype=torch.float32, off=0, fill=SENT):
        self.fill = fill
        if dtype == torch.int32:
            fill = self.fill = -1 if fill != fill else int(fill)  # NaN has no integer: -1 matches no channel
        self.buf = torch.full((PAD + off + n + PAD,), fill, dtype=dtype, device=dev())
        self.v = self.buf[PAD + off:PAD + off + n]
        assert self.buf.data_ptr() % 256 == 0

    @property
    def ptr(self):
        return self.v.data_ptr()

    def _same(self, t):
        return bool(torch.isnan(t).all()) if self.fill != self.fill else bool((t == self.fill).all())

    def untouched(self):
        torch.cuda.synchronize()
        return self._same(self.buf)

    def guards_intact(self):
        torch.cuda.synchronize()
        n0 = self.v.storage_offset()
        return self._same(self.buf[:n0]) and self._same(self.buf[n0 + self.v.numel():])


class Rows:
    """[rows, C] values in rows of ``ld`` elements inside a Buf; every other element is ``fill`` (NaN for inputs, the
    sentinel for outputs)."""

    def __init__(self, rows, C, ld, dtype, off, fill, vals=None):
        assert ld >= C
        self.rows, self.C, self.ld = rows, C, ld
        self.b = Buf((rows - 1) * ld + C, dtype, off, fill)
        if vals is not None:
            self.view()[:] = vals.to(dev()).reshape(rows, C)

    @property
    def ptr(self):
        return self.b.ptr

    def view(self):
        return torch.as_strided(self.b.v, (self.rows, self.C), (self.ld, 1))

    def take(self):
        """The values, after checking that nothing but them was written."""
        torch.cuda.synchronize()
        out = self.view().cpu()
        self.view()[:] = self.b.fill
        assert self.b.untouched(), "a sentinel outside the output was overwritten"
        return out


def _show(name, err, bar):
    print(f"{name}: {err:.3e} (bar {bar:.1e})")
    return err


class Prepared:
    pass


def prepare(c, mode):
    """Device buffers, geometry and epilogue of a case (inside the caller's tuning block)."""
    L = _L()
    S = Prepared()
    S.name, S.vec4 = recorded(c, mode)
    g, prep = make_geom(L, c)
    S.g = g
    f16k = staged_f16(c, S.name)
    pos = c.kind in (GDN, IGDN)
    x, w, mask, acc = conv_data(c.geom, c.sq, pos, bool(c.io & 1), f16k, c.sq and f16k)
    S.acc = acc
    P = g.B * g.Ho * g.Wo
    assert tuple(acc.shape) == (g.B, g.Ho, g.Wo, g.Co)
    # the weight: PyTorch layout -> device re-layout (a pure copy) -> rows of ldw elements, NaN between them
    wd, md = w.to(dev()), (mask.to(dev()) if mask is not None else None)
    rows = prep[2] if prep[0] in (L.WPREP_CONV, L.WPREP_DECONV) else prep[1]
    assert rows == g.Co
    w2 = Buf(rows * g.ntaps * g.Ci, fill=float("nan"))
    L.call("hyres_conv_weight_prep", ctypes.byref(g), wd.data_ptr(), w2.ptr, *prep, md.data_ptr() if mask is not None else None,
           L.stream())
    torch.cuda.synchronize()
    assert w2.guards_intact()
    assert torch.equal(w2.v.cpu().view(rows, -1), CR.relayout(g, w, prep[0], mask)), "hyres_conv_weight_prep is not a copy"
    S.ldw = g.ntaps * g.Ci + pitch_of(c, "w")
    S.w2 = Rows(rows, g.ntaps * g.Ci, S.ldw, torch.float32, off_of(c, "w"), float("nan"), w2.v)
    S.x = Rows(g.B * g.Hi * g.Wi, g.Ci, g.ldx, x.dtype, off_of(c, "x"), float("nan"), x)
    S.data = epi_data(c, P, g.Co)
    ydt = torch.float16 if y16(c) else torch.float32
    S.y = Rows(P, g.Co, g.ldy, ydt, off_of(c, "y"), SENT)
    if c.acc:
        S.data["y_old"] = S.data["y_old"].to(ydt)
        S.y.view()[:] = S.data["y_old"].to(dev())
    S.bufs = {}
    ptrs = {"x": S.x.ptr, "w": S.w2.ptr, "y": S.y.ptr}
    for name in present(c):
        C, ld, dt = opnd_spec(c, g, name)
        if name == "out2":
            S.bufs[name] = Rows(P, C, ld, dt, off_of(c, name), SENT)
        elif name == "bias":
            S.bufs[name] = Rows(1, C, C, dt, off_of(c, name), float("nan"), S.data[name])
        else:
            S.data[name] = S.data[name].to(dt)
            S.bufs[name] = Rows(P, C, ld, dt, off_of(c, name), float("nan"), S.data[name])
        ptrs[name] = S.bufs[name].ptr
    if c.act == PRELU:
        S.slope = Rows(1, 1, 1, torch.float32, 0, float("nan"), torch.tensor([SLOPE]))
        ptrs["slope"] = S.slope.ptr
    S.ptrs = ptrs
    S.e = make_epi(L, c, g, ptrs)
    S.nbytes, nfl, woff = ws_bytes(L, c, g, S.e)
    S.ws = Buf(nfl, off=woff)
    S.ws_ptr = None if c.ws == "none" else S.ws.ptr
    return S


def reference(c, S):
    d = S.data
    P, Co = S.g.B * S.g.Ho * S.g.Wo, S.g.Co
    acc = S.acc.reshape(P, Co)
    sq = (lambda t: t.reshape(P) if t is not None else None)
    aux1 = sq(d.get("aux1")) if c.kind == ROWSCALE else d.get("aux1")
    aux2 = sq(d.get("aux2")) if c.kind == SA_BWD else d.get("aux2")
    return CR.epilogue(c.kind, c.act, acc, d.get("bias"), d.get("res"), SLOPE, d.get("aux0"), aux1, aux2, d.get("y_old"))


def bar_of(c, name):
    bar = BARS[name.split("<")[0]] + (F16_STORE if y16(c) else 0.0)
    assert bar <= CEIL + F16_STORE
    return bar


def run_case(c, mode):
    L = _L()
    lib = L.load()
    with tuned(lib, {**dict(c.tune), 7: mode}):
        S = prepare(c, mode)
        got = query(L, c, mode, S.ptrs, S.ws_ptr if S.ws_ptr is not None else 0)
        assert got == (S.name, S.vec4), (c.id, mode, got, (S.name, S.vec4))
        if c.ws in ("none", "short"):
            assert "+" not in S.name, "without a usable workspace the launch must not split"
        if c.ws == "misaligned" and "+" in S.name:
            assert "+conv_splitk_reduce_kernel" in S.name and S.vec4 == 0
        L.call("hyres_conv_forward", ctypes.byref(S.g), S.x.ptr, S.w2.ptr, S.ldw, S.y.ptr, ctypes.byref(S.e), S.ws_ptr,
               S.nbytes, L.stream())
        torch.cuda.synchronize()
    assert S.ws.guards_intact(), "the workspace was overrun"
    if c.ws == "short":
        assert S.ws.untouched(), "a short workspace must not be used"
    yref, o2ref = reference(c, S)
    y = S.y.take()
    assert S.x.b.guards_intact() and S.w2.b.guards_intact()
    bar = bar_of(c, S.name)
    assert not torch.isnan(y).any(), "NaN in y: a read outside an operand's channel range or rows"
    err = _show(f"{c.id} {S.name} y", rel_err(y, yref), bar)
    err2 = 0.0
    if "out2" in S.bufs:
        o2 = S.bufs["out2"].take()
        assert not torch.isnan(o2).any()
        err2 = _show(f"{c.id} {S.name} out2", rel_err(o2, o2ref), bar)
        if c.kind in (GDN, IGDN) and not y16(c):
            # the few-operation epilogue on the kernel's own arithmetic: y from the device norm
            n, a0 = o2.double(), S.data["aux0"].double()
            own = a0 / n.sqrt() if c.kind == GDN else a0 * n.sqrt()
            if c.acc:
                own = own + S.data["y_old"].double()
            e_own = _show(f"{c.id} {S.name} y | device out2", rel_err(y, own), 1e-6)
            assert e_own < 1e-6
    fam = S.name.split("<")[0]
    WORST[fam] = max(WORST.get(fam, 0.0), err - (F16_STORE if y16(c) else 0.0), err2 - (F16_STORE if y16(c) else 0.0))
    assert err < bar and err2 < bar, (c.id, S.name, err, err2, bar)


def _params(pred):
    out = []
    for c in CASES:
        if pred(c) and c.id in KERNELS:
            for m in modes_of(c):
                out.append(pytest.param(c.id, m, id=f"{c.id}/{'bf16x6' if m else 'native'}/{recorded(c, m)[0]}"))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("cid,mode", _params(lambda c: True))
def test_conv_kernel(cid, mode):
    run_case(BY_ID[cid], mode)


# ------------------------------------------------------------------------------------------------- weight re-layout
@pytest.mark.gpu
@pytest.mark.parametrize("masked", [False, True], ids=["plain", "masked"])
@pytest.mark.parametrize("mode", [0, 1, 2, 3], ids=["conv", "conv-dgrad", "deconv", "deconv-dgrad"])
def test_weight_prep_is_a_copy_in_tap_order(mode, masked):
    """hyres_conv_weight_prep against conv_ref.relayout bit for bit: the four modes, with and without a mask, Ci and Co
    in {3, 5, 64, 96} (the masked conv modes on the checkerboard's 12 taps)."""
    L = _L()
    for Ci in (3, 5, 64, 96):
        for Co in (3, 5, 64, 96):
            g = L.ConvGeom()
            if mode == L.WPREP_CONV:
                L.call("hyres_geom_conv2d", ctypes.byref(g), 1, 4, 4, Ci, Ci, Co, Co, 5, 5, 1, 2, 1)
            elif mode == L.WPREP_CONV_DGRAD:
                L.call("hyres_geom_conv2d_dgrad", ctypes.byref(g), 1, 4, 4, Ci, Ci, Co, Co, 5, 5, 2, 2, 1)
            elif mode == L.WPREP_DECONV:
                L.call("hyres_geom_deconv2d", ctypes.byref(g), 1, 4, 4, Ci, Ci, Co, Co, 5, 2)
            else:
                L.call("hyres_geom_deconv2d_dgrad", ctypes.byref(g), 1, 4, 4, Ci, Ci, Co, Co, 5, 2)
            if masked and mode in (L.WPREP_CONV, L.WPREP_CONV_DGRAD):
                keep = (ctypes.c_ubyte * 25)(*[v for row in CR.checkerboard_keep() for v in row])
                L.call("hyres_geom_filter_taps", ctypes.byref(g), keep, 5)
            wshape = (Co, Ci, 5, 5) if mode in (L.WPREP_CONV, L.WPREP_CONV_DGRAD) else (Ci, Co, 5, 5)
            w = CR.rand(wshape, 30 + mode)
            mask = (CR.rand(wshape, 40) > 0).float() if masked else None
            rows = Co if mode in (L.WPREP_CONV, L.WPREP_DECONV) else Ci
            w2 = Buf(rows * g.ntaps * g.Ci)
            wd, md = w.to(dev()), (mask.to(dev()) if masked else None)
            L.call("hyres_conv_weight_prep", ctypes.byref(g), wd.data_ptr(), w2.ptr, mode, Ci, Co, 5, 5, 2,
                   md.data_ptr() if masked else None, L.stream())
            assert w2.guards_intact()
            assert torch.equal(w2.v.cpu().view(rows, -1), CR.relayout(g, w, mode, mask)), (mode, Ci, Co)


# ------------------------------------------------------------------------------------------------------ refusals
E_SHAPE, E_ALIGN, E_ARG = 1001, 1002, 1003
_R3 = cv(2, 5, 7, 64, 40, 3)
# id -> (case, fields of the epilogue changed after it is built (a string names another operand's pointer), ldw
# change, error code)
REFUSALS = {
    "x-misaligned-ci64": (Case("r", _R3, off=(("x", 1),)), {}, 0, E_ALIGN),
    "narrow-x-misaligned": (Case("r", cv(2, 5, 8, 64, 3, 3), off=(("x", 1),)), {}, 0, E_ALIGN),
    "ci40-four-phases": (Case("r", ("deconv", 2, 3, 4, 40, 64)), {}, 0, E_SHAPE),
    "ci40-square-input": (Case("r", cv(2, 5, 7, 40, 64, 1), sq=True), {}, 0, E_SHAPE),
    "ldw-one-short": (Case("r", _R3), {}, -1, E_SHAPE),
    "gdn-without-aux0": (Case("r", cv(2, 5, 7, 64, 64, 1), sq=True, kind=GDN), {"aux0": None}, 0, E_ARG),
    "gdn-without-out2": (Case("r", cv(2, 5, 7, 64, 64, 1), sq=True, kind=IGDN), {"out2": None}, 0, E_ARG),
    "gdnbwd-without-aux2": (Case("r", _R3, kind=GDN_BWD), {"aux2": None}, 0, E_ARG),
    "prelu-without-slope": (Case("r", _R3, act=PRELU), {"slope": None}, 0, E_ARG),
    "io5": (Case("r", _R3), {"io_f16": 5}, 0, E_ARG),
    "x16-ci3": (Case("r", cv(2, 5, 7, 3, 40, 3)), {"io_f16": 1}, 0, E_ARG),
    "y16-narrow": (Case("r", cv(2, 5, 8, 64, 3, 3)), {"io_f16": 2}, 0, E_ARG),
    "relu-mask-kind-gdn": (Case("r", cv(2, 5, 7, 64, 64, 1), sq=True, kind=GDN), {"act": RELU_MASK}, 0, E_ARG),
    "rowscale-accumulate": (Case("r", _R3, kind=ROWSCALE), {"accumulate": 1}, 0, E_ARG),
    "sabwd-with-res": (Case("r", _R3, kind=SA_BWD), {"res": "aux0", "ldres": 40}, 0, E_ARG),
    "sabwd-y16-on-tiles": (Case("r", _R3, kind=SA_BWD), {"io_f16": 2}, 0, E_ARG),
}


@pytest.mark.gpu
@pytest.mark.parametrize("rid", list(REFUSALS))
def test_conv_refusals_leave_everything_untouched(rid):
    """One per HY_REQUIRE of hyres_conv_forward that small arguments reach (the PReLU-mask refusal has its own test in
    test_bf6_gpu.py; the 32-bit span guards are out of reach, module docstring)."""
    L = _L()
    c, change, dldw, code = REFUSALS[rid]
    g, _ = make_geom(L, c)
    P = g.B * g.Ho * g.Wo
    x = Rows(g.B * g.Hi * g.Wi, g.Ci, g.ldx, torch.float32, off_of(c, "x"), float("nan"),
             CR.rand((g.B * g.Hi * g.Wi, g.Ci), 1))
    w2 = Rows(g.Co, g.ntaps * g.Ci, g.ntaps * g.Ci, torch.float32, 0, float("nan"), CR.rand((g.Co, g.ntaps * g.Ci), 2))
    y = Rows(P, g.Co, g.ldy, torch.float32, 0, SENT)
    bufs, ptrs = {}, {"x": x.ptr, "w": w2.ptr, "y": y.ptr}
    for name in present(c):
        C, ld, dt = opnd_spec(c, g, name)
        bufs[name] = Rows(1 if name == "bias" else P, C, ld, dt, 0, SENT if name == "out2" else 1.0)
        ptrs[name] = bufs[name].ptr
    slope = Rows(1, 1, 1, torch.float32, 0, SLOPE)
    ptrs["slope"] = slope.ptr
    e = make_epi(L, c, g, ptrs)
    for k, v in change.items():
        setattr(e, k, ptrs[v] if isinstance(v, str) else v)
    need = int(L.load().hyres_conv_workspace_bytes(ctypes.byref(g)))
    ws = Buf(need // 4)
    with pytest.raises(L.HipError, match=rf"\({code}\)"):
        L.call("hyres_conv_forward", ctypes.byref(g), x.ptr, w2.ptr, g.ntaps * g.Ci + dldw, y.ptr, ctypes.byref(e), ws.ptr,
               need, L.stream())
    assert y.b.untouched() and ws.untouched()
    assert "out2" not in bufs or bufs["out2"].b.untouched()
