"""Per-kernel fp64 parity of the weight-gradient kernels (csrc/wgrad.hip) at ragged shapes.

Every case builds a hyres_wgrad_desc (the two hyres_wgrad_desc_* helpers, then the fields the case changes), calls
hyres_conv_wgrad (one group: hyres_conv_wgrad_deferred + hyres_wgrad_reduce_jobs) through ``_lib.call`` and compares
with tests/wgrad_ref.py, the fp64 definition, computed from the values the kernel is given (fp16 storage: the fp16
tensors).  The case table ``CASES`` carries no GPU state, so tests/test_wgrad_ref_cpu.py imports it and checks on the
CPU that it reaches every instantiation wgrad_route() can produce.  ``KERNELS`` records, per case, the kernel the
library names for it (hyres_wgrad_kernel_name_at: with the case's real pointer alignments) under the native and the
bf16x6 fp32 GEMM (hyres_conv_tuning key 7); the id carries that name and the test asserts it before launching, so a case
that drifts to another kernel fails instead of testing something else.

Storage: dst, dbias and the workspace sit inside sentinel-filled buffers, the workspace exactly
hyres_wgrad_workspace_bytes long; the gaps of a strided dst are sentinels too and every sentinel must be intact after
the call.  Operand columns outside [0, M) / [0, N) of an ``ld``-wide row, and the guard elements around the operands,
hold NaN.

Bars (max-norm, helpers.rel_err): 1e-5 for every family, fp32 operands under both GEMM modes and fp16 operands alike
(an fp16 x fp16 product is exact in fp32; only the accumulation rounds).  With f16_operands and fp32 storage the f16
kernels round P and Q to fp16 (round to nearest even, as torch's .half()); the bias gradient sums the unrounded P.

The one widened bar: wgrad_f16_kernel's SQ path (GDN gamma gradient) with Q stored fp32.  Its store_q squares Q in fp32
and rounds Q * Q to fp16 at the LDS store, and the compiled kernel does that two ways within one store of four
channels: three by v_pk_mul_f32 + v_cvt_pk_f16_f32 (the product rounded to fp32, then to fp16) and the fourth
(n % 4 == 3) by v_fma_mixlo_f16 (the exact product rounded once).  The two differ by one fp16 ulp where the fp32
rounding lands on an fp16 tie; read back through a one-hot P, 2 of 4096 staged values of f16/gdn64-1x5x13-io0 (pixel 14
channel 27, pixel 41 channel 59) were the once-rounded ones, every other the same under both.  Which lanes get which is
the compiler's choice and both are Q * Q to within fp16 rounding, so the reference rounds the exact square once
(square_to_half) and the bar of such a case is 1e-5 plus what the ties can move: max over outputs of sum_q |P| |once -
twice| over max |dW|, computed from the inputs and the two number formats alone.  That allowance is 1.2e-5 to 5.1e-5
on the 13 such cases (bars 2.2e-5 to 6.1e-5, each asserted below the project's 1e-4, test_parity_gpu.TOL) and exactly 0,
the bar 1e-5, for every other case, the fp16-Q squares included (an fp16 square is exact in fp32).

Worst error per family on an MI355X (547 cases, 3.6 s): wgrad_kernel 7.6e-7, wgrad1x1_kernel 5.2e-7,
wgrad1x1_bf6_kernel 4.6e-7, wgrad1x1_bf6_pf2_kernel 4.5e-7, wgrad_halo_kernel 5.3e-7, wgrad_halo_bf6_kernel 3.5e-7,
wgrad_halo_bf6_pf2_kernel 3.5e-7, wgrad_halo_f16_kernel 1.8e-7, wgrad_thin_kernel 2.5e-7, colsum 2.2e-7,
wgrad_f16_kernel 2.6e-7; its 13 SQ cases with an fp32 Q: 1.3e-7 to 5.12e-5, none more than 2.2e-7 above its own tie
allowance.

Mutations (each built on a scratch copy of csrc/wgrad.hip and run over CASES; failing cases of 518):
1. load_p of wgrad_kernel guarded by Qtot rounded up to a chunk: 170 (NaN from the guard after P: every wgrad_kernel
   case whose pixel count is no multiple of 32, e.g. gen/3x5x7-k3, all of gx/, tile/, flag/, swap/ on wgrad_kernel).
2. wgrad_swapped keeps dw's sign: 32, every swapped case (swap/*, cvt/swap-M3-io*, defer/swap-M3), errors about 1.
3. cvtq_off = cvtp_off: 13, every case that converts both operands (cvt/*-io3*, cvt/gdn64-io3,
   f16late/k3-sq-p16-q16-ld+1).
4. wgrad_bias_reduce_kernel ignores accumulate for the bias: 81, every accumulate case with a bias off the swapped
   path (dbias error 0.05 and up, dW untouched).
5. wgrad_halo_kernel's row bound d.Hq for d.Hqq: 4, the native stride-2 cases halo/3x7x63-k5s2,
   halo/3x5x191-k5s2-pf2-acc, halo/3x3x32-deconv5, halo/3x3x32-deconv5-pf2 (stride 1 has Hq == Hqq).
6. thin_plan's ncol one short: 6.  thin/N3-M64-k3-W263-span265 fails its name (the route changes), and
   thin/N3-M64-k3-pad0 and thin/N4-M128-k3s2-W20 fail by value (0.24, 0.39).  With "same" padding the window's last
   column is the zero column right of the image, so no other thin case can see it; those two were added for it."""
import ctypes
import functools
import json
import os
from dataclasses import dataclass

import numpy as np
import pytest
import torch

import wgrad_ref as WR
from helpers import rel_err

TOL = 1e-5
TOL_WIDE = 1e-4  # test_parity_gpu.TOL: the ceiling of the one family whose bar is widened (module docstring)
SENT = -777.0
PAD = 64

# worst rel_err per kernel family seen by this process (printed figures; the recorded ones are in the docstring)
WORST = {}


@dataclass(frozen=True)
class Case:
    """geom: ("conv", B, H, W, Ci, Co, K, stride, pad, dil) | ("deconv", B, H, W, Ci, Co) (K = 5, pad 2, as the model's)
    | ("gdn", B, H, W, C) | ("rev3", B, H, W, Ci, Co) (a 3x3 with its taps listed in reversed order) | ("convsq", ...)
    (conv's arguments with square_q set: squared multi-tap and M != N descriptors no layer builds).
    ldp / ldq: extra elements per operand row; poff / qoff: elements past a 256-byte aligned address; wsoff: bytes."""
    id: str
    geom: tuple
    ldp: int = 0
    ldq: int = 0
    poff: int = 0
    qoff: int = 0
    wsoff: int = 0
    f16: int = 0        # desc.f16_operands
    io: int = 0         # desc.io_f16
    acc: int = 0
    bias: bool = True
    dst: str = "torch"  # "wide": sm, sn larger than PyTorch's and st = 2
    tune: tuple = ()    # ((key, value), ...) of hyres_conv_tuning
    lanes: int = 16     # of the split reduce, as hyres_wgrad_plan reports it
    deferred: bool = False


def _c(id, *geom, **kw):
    return Case(id, geom, **kw)


CASES = []


def _add(*cases):
    CASES.extend(cases)


# ---- generic kernel: pixel raggedness (rows narrower than a chunk, chunks across images, short last split)
_add(_c("gen/3x5x7-k3", "conv", 3, 5, 7, 64, 64, 3, 1, 1, 1),
     _c("gen/3x5x7-k3-minchunks1", "conv", 3, 5, 7, 64, 64, 3, 1, 1, 1, tune=((4, 1),)),
     _c("gen/1x1x33-k3", "conv", 1, 1, 33, 64, 64, 3, 1, 1, 1),
     _c("gen/2x9x20-k3", "conv", 2, 9, 20, 64, 64, 3, 1, 1, 1),
     _c("gen/2x9x20-k5", "conv", 2, 9, 20, 64, 64, 5, 1, 2, 1),
     _c("gen/2x9x23-k3-short-last-split", "conv", 2, 9, 23, 64, 64, 3, 1, 1, 1),
     _c("gen/2x9x20-k3-nt1", "conv", 2, 9, 20, 64, 64, 3, 1, 1, 1, tune=((5, 1),)),
     _c("gen/2x9x20-k3-acc-nobias", "conv", 2, 9, 20, 64, 64, 3, 1, 1, 1, acc=1, bias=False),
     _c("gen/2x9x20-k3-acc-wide-dst", "conv", 2, 9, 20, 64, 64, 3, 1, 1, 1, acc=1, dst="wide"),
     _c("gen/2x9x20-k3s2", "conv", 2, 9, 20, 64, 64, 3, 2, 1, 1),
     _c("gen/2x9x20-k3d2", "conv", 2, 9, 20, 64, 64, 3, 1, 2, 2),
     _c("gen/2x5x7-deconv5", "deconv", 2, 5, 7, 64, 64))
# ---- generic kernel: every with_tile branch, partial tiles
_add(_c("tile/128x128", "conv", 2, 9, 20, 128, 128, 3, 1, 1, 1),
     _c("tile/M128-1x1s2", "conv", 2, 9, 20, 64, 128, 1, 2, 0, 1),
     _c("tile/M32", "conv", 2, 9, 20, 64, 32, 3, 1, 1, 1),
     _c("tile/N32", "conv", 2, 9, 20, 32, 64, 3, 1, 1, 1),
     _c("tile/fold-N3k3", "conv", 2, 9, 20, 3, 40, 3, 1, 1, 1),
     _c("tile/fold-N5k3", "conv", 2, 9, 20, 5, 40, 3, 1, 1, 1),
     _c("tile/fold-N3k5", "conv", 2, 9, 20, 3, 96, 5, 1, 2, 1),
     _c("tile/fold-N5k5-acc", "conv", 2, 9, 20, 5, 96, 5, 1, 2, 1, acc=1),
     _c("tile/M40xN96", "conv", 2, 9, 20, 96, 40, 3, 1, 1, 1, ldp=4, ldq=8),
     _c("tile/M40xN96-k5", "conv", 2, 9, 20, 96, 40, 5, 1, 2, 1),
     _c("tile/M136xN132", "conv", 2, 9, 20, 132, 136, 3, 1, 1, 1))
# ---- generic kernel: the VP / VQ / SQ flags through M % 4, ld % 4 and a pointer one element off
_add(_c("flag/gdn64", "gdn", 2, 9, 20, 64),
     _c("flag/gdn192-acc", "gdn", 1, 5, 13, 192, acc=1, ldq=4),
     _c("flag/N70", "conv", 2, 9, 20, 70, 64, 3, 1, 1, 1),
     _c("flag/ldq+1", "conv", 2, 9, 20, 64, 64, 3, 1, 1, 1, ldq=1),
     _c("flag/M42", "conv", 2, 9, 20, 64, 42, 3, 1, 1, 1),
     _c("flag/ldp+2", "conv", 2, 9, 20, 64, 64, 3, 1, 1, 1, ldp=2),
     _c("flag/M42xN70", "conv", 2, 9, 20, 70, 42, 3, 1, 1, 1),
     _c("flag/poff1-qoff1", "conv", 2, 9, 20, 64, 64, 3, 1, 1, 1, poff=1, qoff=1),
     _c("flag/1x1-qoff1", "conv", 1, 5, 13, 64, 64, 1, 1, 0, 1, qoff=1),
     _c("flag/1x1-poff1-128", "conv", 1, 5, 13, 64, 128, 1, 1, 0, 1, poff=1),
     _c("flag/thin-poff1", "conv", 2, 9, 20, 3, 64, 3, 1, 1, 1, poff=1),
     _c("flag/thin-ldp+1", "conv", 2, 9, 20, 3, 64, 3, 1, 1, 1, ldp=1))
# ---- generic kernel: every tile shape x every flag combination launch_wgrad has
GEN_TILES = {"2222n1": (132, 136, 3, 1, 1, 1), "2122n1": (64, 128, 1, 2, 0, 1), "1114n1": (64, 32, 3, 1, 1, 1),
             "1141n1": (32, 64, 3, 1, 1, 1), "1122n9": (64, 64, 3, 1, 1, 1), "1122n5": (64, 64, 5, 1, 2, 1),
             "1122n1": (64, 64, 3, 2, 1, 1)}
for _t, _g in GEN_TILES.items():
    _tn = ((5, 1),) if _t == "1122n1" else ()
    _add(_c(f"gx/{_t}-ttf", "conv", 2, 9, 20, *_g, tune=_tn),
         _c(f"gx/{_t}-tff", "conv", 2, 9, 20, *_g, tune=_tn, ldq=1),
         _c(f"gx/{_t}-ftf", "conv", 2, 9, 20, *_g, tune=_tn, ldp=1),
         _c(f"gx/{_t}-fff", "conv", 2, 9, 20, *_g, tune=_tn, ldp=3, ldq=2),
         _c(f"gx/{_t}-ttt", "convsq", 2, 9, 20, *_g, tune=_tn, ldq=4))
# ---- plain 1x1: wgrad1x1_kernel G = 1 / 2, wgrad1x1_bf6_kernel (key 15 = 1), wgrad1x1_bf6_pf2_kernel
for _ci, _co in ((64, 128), (128, 64), (64, 64), (128, 128)):
    _add(_c(f"1x1/1x5x13-{_ci}to{_co}", "conv", 1, 5, 13, _ci, _co, 1, 1, 0, 1),
         _c(f"1x1/1x5x13-{_ci}to{_co}-pf1", "conv", 1, 5, 13, _ci, _co, 1, 1, 0, 1, tune=((15, 1),)))
for _ci, _co in ((64, 32), (32, 64)):
    _add(_c(f"1x1/1x5x13-{_ci}to{_co}", "conv", 1, 5, 13, _ci, _co, 1, 1, 0, 1),
         _c(f"1x1/1x5x13-{_ci}to{_co}-pf1", "conv", 1, 5, 13, _ci, _co, 1, 1, 0, 1, tune=((15, 1),)),
         _c(f"1x1/1x129x128-{_ci}to{_co}", "conv", 1, 129, 128, _ci, _co, 1, 1, 0, 1, acc=1))
_add(_c("1x1/3x11x11-64to64-ld+4-acc", "conv", 3, 11, 11, 64, 64, 1, 1, 0, 1, ldp=4, ldq=4, acc=1),
     _c("1x1/3x11x11-64to64-ld+4-pf1", "conv", 3, 11, 11, 64, 64, 1, 1, 0, 1, ldp=4, ldq=4, tune=((15, 1),)),
     _c("1x1/1x33x1-96to40", "conv", 1, 33, 1, 96, 40, 1, 1, 0, 1, bias=False),
     _c("1x1/1x129x128-64to128", "conv", 1, 129, 128, 64, 128, 1, 1, 0, 1),
     _c("1x1/1x129x128-128to64-ldq+4", "conv", 1, 129, 128, 128, 64, 1, 1, 0, 1, ldq=4, acc=1),
     _c("1x1/1x129x128-128to128", "conv", 1, 129, 128, 128, 128, 1, 1, 0, 1, bias=False),
     _c("1x1/1x129x128-64to64-pf1", "conv", 1, 129, 128, 64, 64, 1, 1, 0, 1, tune=((15, 1),)))
# ---- halo kernels: partial M / N tiles, ldp = M + 4, images shorter than the tap span
for _h, _w in ((3, 32), (3, 96), (5, 32), (5, 96)):
    _add(_c(f"halo/3x{_h}x{_w}-k3", "conv", 3, _h, _w, 100, 36, 3, 1, 1, 1, ldp=4),
         _c(f"halo/3x{_h}x{_w}-k3-pf1", "conv", 3, _h, _w, 100, 36, 3, 1, 1, 1, ldp=4, tune=((16, 1),)),
         _c(f"halo/3x{_h}x{_w}-k3d2", "conv", 3, _h, _w, 100, 36, 3, 1, 2, 2, ldp=4),
         _c(f"halo/3x{_h}x{_w}-k5", "conv", 3, _h, _w, 100, 36, 5, 1, 2, 1, ldp=4),
         _c(f"halo/3x{_h}x{_w}-k5-pf2", "conv", 3, _h, _w, 100, 36, 5, 1, 2, 1, ldp=4, tune=((22, 1),)))
_add(_c("halo/3x7x63-k5s2", "conv", 3, 7, 63, 100, 36, 5, 2, 2, 1, ldp=4),
     _c("halo/3x5x191-k5s2-pf2-acc", "conv", 3, 5, 191, 100, 36, 5, 2, 2, 1, ldp=4, tune=((22, 1),), acc=1),
     _c("halo/3x3x32-deconv5", "deconv", 3, 3, 32, 36, 100, ldp=4),
     _c("halo/3x3x32-deconv5-pf2", "deconv", 3, 3, 32, 36, 100, ldp=4, tune=((22, 1),)),
     _c("halo/3x3x32-k3-acc-wide-dst-nobias", "conv", 3, 3, 32, 100, 36, 3, 1, 1, 1, ldp=4, acc=1, dst="wide",
        bias=False),
     _c("halo/1x40x64-k3-64to64", "conv", 1, 40, 64, 64, 64, 3, 1, 1, 1))
HALO16 = {"k3": ("conv", 3, 3, 32, 100, 36, 3, 1, 1, 1), "k3d2": ("conv", 3, 5, 96, 100, 36, 3, 1, 2, 2),
          "k5": ("conv", 3, 5, 32, 100, 36, 5, 1, 2, 1), "k5s2": ("conv", 3, 7, 63, 100, 36, 5, 2, 2, 1),
          "deconv5": ("deconv", 3, 3, 32, 36, 100)}
for _t, _g in HALO16.items():
    for _io in range(4):
        _add(_c(f"halo16/{_t}-io{_io}", *_g, ldp=4, ldq=4 * (_io >> 1), f16=1, io=_io, acc=_io & 1))
# ---- wgrad_f16_kernel: square_q, one16, multi-tap, every io mask, the tile branches, 64 k + 1 pixels
for _io in range(4):
    _add(_c(f"f16/gdn64-1x5x13-io{_io}", "gdn", 1, 5, 13, 64, f16=1, io=_io),
         _c(f"f16/1x1-1x5x13-io{_io}", "conv", 1, 5, 13, 64, 64, 1, 1, 0, 1, f16=1, io=_io, ldp=4 * (_io & 1)))
_add(_c("f16/gdn192-acc", "gdn", 2, 9, 20, 192, f16=1, acc=1, io=3),
     _c("f16/2x9x20-k3", "conv", 2, 9, 20, 64, 64, 3, 1, 1, 1, f16=1),
     _c("f16/2x9x20-k3-io3-ld+4", "conv", 2, 9, 20, 64, 64, 3, 1, 1, 1, f16=1, io=3, ldp=4, ldq=4),
     _c("f16/3x5x7-k5s2-io2", "conv", 3, 5, 7, 64, 64, 5, 2, 2, 1, f16=1, io=2),
     _c("f16/128x128-k3", "conv", 2, 9, 20, 128, 128, 3, 1, 1, 1, f16=1),
     _c("f16/M128-1x1", "conv", 1, 5, 13, 64, 128, 1, 1, 0, 1, f16=1, io=1),
     _c("f16/M32-k3", "conv", 2, 9, 20, 64, 32, 3, 1, 1, 1, f16=1),
     _c("f16/N32-k3-acc", "conv", 2, 9, 20, 32, 64, 3, 1, 1, 1, f16=1, acc=1),
     _c("f16/M40xN96-k3", "conv", 2, 9, 20, 96, 40, 3, 1, 1, 1, f16=1, io=3),
     _c("f16/2x5x7-deconv5", "deconv", 2, 5, 7, 64, 64, f16=1))
F16_TILES = {"2222": (128, 128), "2122": (64, 128), "1114": (64, 32), "1141": (32, 64), "1122": (96, 40)}
for _t, (_ci, _co) in F16_TILES.items():
    for _io in range(4):
        _add(_c(f"f16x/{_t}-sq-io{_io}", "convsq", 1, 5, 13, _ci, _co, 1, 1, 0, 1, f16=1, io=_io),
             _c(f"f16x/{_t}-one-io{_io}", "conv", 1, 5, 13, _ci, _co, 1, 1, 0, 1, f16=1, io=_io, acc=_io & 1),
             _c(f"f16x/{_t}-1x1s2-io{_io}", "conv", 2, 9, 20, _ci, _co, 1, 2, 0, 1, f16=1, io=_io, ldq=4))
# ---- wgrad_f16_kernel behind a plan made for the fp32 kernels: with f16_operands, an fp16 operand whose ld % 4 != 0
# keeps the plan off the f16 kernel (32-pixel chunks, taps grouped 9 / 5 per block, the fp32 copy reserved), and its
# contiguous fp32 copy then makes the launch descriptor f16-eligible: NT = 9 / 5, 64-pixel chunks counted as 32-pixel
# ones (the upper half of the chunks lies past the last pixel and must contribute zeros)
_add(_c("f16late/k3-p16-ldp+1", "conv", 2, 9, 20, 64, 64, 3, 1, 1, 1, f16=1, io=1, ldp=1),
     _c("f16late/k5-q16-ldq+2-acc", "conv", 2, 9, 20, 64, 64, 5, 1, 2, 1, f16=1, io=2, ldq=2, acc=1),
     _c("f16late/k3-sq-p16-q16-ld+1", "convsq", 2, 9, 20, 64, 64, 3, 1, 1, 1, f16=1, io=3, ldp=1, ldq=1),
     _c("f16late/k5-sq-p16-ldp+3", "convsq", 3, 5, 7, 64, 64, 5, 1, 2, 1, f16=1, io=1, ldp=3),
     _c("f16late/128x128-k3-p16-ldp+1", "conv", 2, 9, 20, 128, 128, 3, 1, 1, 1, f16=1, io=1, ldp=1),
     _c("f16late/1x1-q16-ldq+1", "conv", 1, 5, 13, 64, 64, 1, 1, 0, 1, f16=1, io=2, ldq=1),
     _c("f16late/gdn64-q16-ldq+2", "gdn", 1, 5, 13, 64, f16=1, io=2, ldq=2))
# ---- thin kernel
for _n in (1, 2):
    _add(_c(f"thin/N{_n}-M64-k3", "conv", 2, 9, 20, _n, 64, 3, 1, 1, 1, ldq=4 - _n))
# every instantiation: M / 64 x (3 | 4 channels) x tap groups of 9 | 25 (M = 64) | 13 (M = 128, two groups) x Q stride x
# fp32 | fp16 P
for _m in (64, 128):
    for _n in (3, 4):
        for _k in (3, 5):
            for _s in (1, 2):
                for _io in (0, 1):
                    _add(_c(f"thin/N{_n}-M{_m}-k{_k}s{_s}{'-p16' if _io else ''}", "conv", 2, 9, 21, _n, _m, _k, _s,
                            _k // 2, 1, io=_io, acc=_io))
_add(_c("thin/N3-M128-k3", "conv", 2, 9, 20, 3, 128, 3, 1, 1, 1),
     _c("thin/N3-M64-k5", "conv", 2, 9, 20, 3, 64, 5, 1, 2, 1),
     _c("thin/N3-M128-k5-two-groups", "conv", 2, 9, 20, 3, 128, 5, 1, 2, 1),
     _c("thin/N4-M128-k3s2-acc", "conv", 2, 9, 21, 4, 128, 3, 2, 1, 1, acc=1, ldp=4),
     _c("thin/N3-M64-k3-p16", "conv", 2, 9, 20, 3, 64, 3, 1, 1, 1, io=1),
     _c("thin/N3-M64-k5s2-p16-q16", "conv", 2, 9, 21, 3, 64, 5, 2, 2, 1, io=3),
     _c("thin/N3-M64-k3-q16", "conv", 2, 9, 20, 3, 64, 3, 1, 1, 1, io=2),
     _c("thin/N3-M64-k3-window-off", "conv", 2, 9, 20, 3, 64, 3, 1, 1, 1, tune=((23, 0),)),
     _c("thin/N3-M64-k3-W260", "conv", 1, 2, 260, 3, 64, 3, 1, 1, 1),
     _c("thin/N3-M64-k3-W262-span264", "conv", 1, 2, 262, 3, 64, 3, 1, 1, 1),
     _c("thin/N3-M64-k3-W263-span265", "conv", 1, 2, 263, 3, 64, 3, 1, 1, 1),
     _c("thin/N3-M64-rev3", "rev3", 2, 9, 20, 3, 64),
     # the staged window's last column inside the image (with "same" padding it is the zero column right of it)
     _c("thin/N3-M64-k3-pad0", "conv", 2, 9, 20, 3, 64, 3, 1, 0, 1),
     _c("thin/N4-M128-k3s2-W20", "conv", 2, 9, 20, 4, 128, 3, 2, 1, 1),
     # ... and a padding that is neither 0 nor K / 2
     _c("thin/N3-M64-k5-pad1-p16", "conv", 2, 9, 20, 3, 64, 5, 1, 1, 1, io=1),
     _c("thin/N3-M128-k5-515rows-rpb2", "conv", 1, 515, 4, 3, 128, 5, 1, 2, 1, lanes=4),
     _c("thin/N3-M64-k3-wide-dst-nobias", "conv", 2, 9, 20, 3, 64, 3, 1, 1, 1, dst="wide", bias=False))
# ---- swapped small-M path: negated shifts, hyres_colsum bias after the slab
for _m, _n in ((1, 48), (3, 64), (5, 64), (3, 48)):
    _add(_c(f"swap/M{_m}-N{_n}-k3", "conv", 2, 9, 20, _n, _m, 3, 1, 1, 1),
         _c(f"swap/M{_m}-N{_n}-k3-acc-p16", "conv", 2, 9, 20, _n, _m, 3, 1, 1, 1, acc=1, io=1, ldp=(4 - _m) % 4))
_add(_c("swap/M3-N64-k5", "conv", 2, 9, 20, 64, 3, 5, 1, 2, 1),
     _c("swap/M3-N64-k3-window-off", "conv", 2, 9, 20, 64, 3, 3, 1, 1, 1, tune=((23, 0),)),
     _c("swap/M4-N128-k5-nobias", "conv", 2, 9, 20, 128, 4, 5, 1, 2, 1, bias=False),
     _c("swap/M3-N64-k3-wide-dst", "conv", 2, 9, 20, 64, 3, 3, 1, 1, 1, dst="wide"))
# ---- fp16 operands on the fp32 kernels: half_to_float_2d into the workspace after the slab and the bias partials
for _io in (1, 2, 3):
    _add(_c(f"cvt/gen-k3-io{_io}", "conv", 2, 9, 20, 64, 64, 3, 1, 1, 1, io=_io, ldp=4, ldq=8),
         _c(f"cvt/1x1-io{_io}", "conv", 1, 5, 13, 64, 128, 1, 1, 0, 1, io=_io, ldp=4, ldq=8),
         _c(f"cvt/halo-k3-io{_io}", "conv", 3, 3, 32, 100, 36, 3, 1, 1, 1, io=_io, ldp=4, ldq=8),
         _c(f"cvt/swap-M3-io{_io}", "conv", 2, 9, 20, 64, 3, 3, 1, 1, 1, io=_io, ldp=1, ldq=8))
_add(_c("cvt/1x1-io3-ws+4", "conv", 1, 5, 13, 64, 128, 1, 1, 0, 1, io=3, ldp=4, ldq=8, wsoff=4),
     _c("cvt/gen-k3-io3-ld+1-acc", "conv", 2, 9, 20, 64, 64, 3, 1, 1, 1, io=3, ldp=1, ldq=3, acc=1),
     _c("cvt/gdn64-io3", "gdn", 2, 9, 20, 64, io=3, ldp=4))
# ---- the split reduces: more than 64 splits select 4 / 8 lanes below 65536 / 32768 outputs (reduce_lx)
_RT = ((4, 1), (6, 256))
_add(_c("red/1x40x65-64to64-lanes4", "conv", 1, 40, 65, 64, 64, 1, 1, 0, 1, tune=_RT, lanes=4, acc=1),
     _c("red/1x40x65-192to192-lanes8", "conv", 1, 40, 65, 192, 192, 1, 1, 0, 1, tune=_RT, lanes=8, acc=1),
     _c("red/1x40x65-256to256-lanes16", "conv", 1, 40, 65, 256, 256, 1, 1, 0, 1, tune=_RT, lanes=16, acc=1),
     _c("red/1x40x65-k3-40to36-lanes4-wide-dst", "conv", 1, 40, 65, 40, 36, 3, 1, 1, 1, tune=_RT, lanes=4, dst="wide"),
     _c("red/1x40x65-64to64-lanes4-nobias", "conv", 1, 40, 65, 64, 64, 1, 1, 0, 1, tune=_RT, lanes=4, bias=False))
# ---- deferred GEMM + hyres_wgrad_reduce_jobs
_add(_c("defer/gen-k3-acc", "conv", 2, 9, 20, 64, 64, 3, 1, 1, 1, acc=1, deferred=True),
     _c("defer/1x1", "conv", 1, 5, 13, 64, 128, 1, 1, 0, 1, deferred=True),
     _c("defer/halo-k3-wide-dst", "conv", 3, 3, 32, 100, 36, 3, 1, 1, 1, ldp=4, dst="wide", deferred=True),
     _c("defer/thin-k5s2", "conv", 2, 9, 21, 3, 64, 5, 2, 2, 1, deferred=True),
     _c("defer/swap-M3", "conv", 2, 9, 20, 64, 3, 3, 1, 1, 1, acc=1, deferred=True),
     _c("defer/lanes4", "conv", 1, 40, 65, 64, 64, 1, 1, 0, 1, tune=_RT, lanes=4, acc=1, deferred=True),
     _c("defer/f16-gdn", "gdn", 1, 5, 13, 64, f16=1, io=3, deferred=True))

BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES)

# case id -> kernel name, or [native, bf16x6] where the fp32 GEMM mode changes it: recorded from the library's own name
# query by tests/golden/make_wgrad_kernels.py, checked against the built library on the CPU (test_wgrad_ref_cpu.py)
with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "wgrad_kernels.json")) as _f:
    KERNELS = json.load(_f)


def f16_family(c):
    k = KERNELS[c.id]
    return isinstance(k, str) and "f16" in k


def kernel_of(c, mode):
    k = KERNELS[c.id]
    return k if isinstance(k, str) else k[mode]


def modes_of(c):
    """Both GEMM modes for fp32 arithmetic; the f16-MFMA kernels do not read key 7."""
    return (1,) if f16_family(c) else (0, 1)


def esize(c, which):
    return 2 if c.io & (1 if which == "p" else 2) else 4


def facts(c):
    """(p, q, workspace) 16-byte aligned?"""
    return (int(c.poff * esize(c, "p") % 16 == 0), int(c.qoff * esize(c, "q") % 16 == 0), int(c.wsoff % 16 == 0))


def make_desc(L, c):
    """The case's hyres_wgrad_desc (host only)."""
    d = L.WgradDesc()
    kind, g = c.geom[0], c.geom[1:]
    if kind in ("conv", "rev3", "convsq"):
        B, H, W, Ci, Co, K, s, p, dil = g + (3, 1, 1, 1) if kind == "rev3" else g
        L.call("hyres_wgrad_desc_conv2d", ctypes.byref(d), B, H, W, Ci, Ci + c.ldq, Co, Co + c.ldp, K, K, s, p, dil)
        if kind == "rev3":  # the same taps listed backwards: dst[.. + t] = the gradient of tap 8 - t
            for t in range(9):
                d.dh[t], d.dw[t] = 1 - t // 3, 1 - t % 3
        d.square_q = int(kind == "convsq")
    elif kind == "deconv":
        B, H, W, Ci, Co = g
        L.call("hyres_wgrad_desc_deconv2d", ctypes.byref(d), B, H, W, Ci, Ci + c.ldp, Co, Co + c.ldq, 5, 2)
    else:
        B, H, W, C = g
        L.call("hyres_wgrad_desc_conv2d", ctypes.byref(d), B, H, W, C, C + c.ldq, C, C + c.ldp, 1, 1, 1, 0, 1)
        d.square_q = 1
    if c.dst == "wide":
        d.st = 2
        d.sn = 2 * d.ntaps + 1
        d.sm = d.N * d.sn + 3
    d.accumulate, d.f16_operands, d.io_f16 = c.acc, c.f16, c.io
    return d


class tuned:
    """hyres_conv_tuning keys set for a block and restored after it."""

    def __init__(self, lib, keys):
        self.lib, self.keys, self.old = lib, dict(keys), {}

    def __enter__(self):
        for k, v in self.keys.items():
            o = ctypes.c_int(0)
            assert self.lib.hyres_conv_tuning(k, v, ctypes.byref(o)) == 0
            self.old[k] = o.value
        return self

    def __exit__(self, *exc):
        for k, v in self.old.items():
            assert self.lib.hyres_conv_tuning(k, v, None) == 0
        return False


def query(L, c, mode):
    """(kernel name at the case's alignments, lanes) under GEMM ``mode``; host only."""
    lib = L.load()
    with tuned(lib, {**dict(c.tune), 7: mode}):
        d = make_desc(L, c)
        buf = ctypes.create_string_buffer(96)
        L.call("hyres_wgrad_kernel_name_at", ctypes.byref(d), *facts(c), buf, len(buf))
        lanes = ctypes.c_int(0)
        L.call("hyres_wgrad_plan", ctypes.byref(d), None, None, None, ctypes.byref(lanes))
    return buf.value.decode(), lanes.value


# ------------------------------------------------------------------------------------------------------ GPU side
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def _L():
    from hyres_hip import _lib as L
    return L


class Buf:
    """``n`` elements ``off`` elements past a 256-byte aligned address, between guards of ``fill``."""

    def __init__(self, n, dtype=torch.float32, off=0, fill=SENT):
        self.fill = fill
        self.buf = torch.full((PAD + off + n + PAD,), fill, dtype=dtype, device=dev())
        self.v = self.buf[PAD + off:PAD + off + n]
        assert self.buf.data_ptr() % 256 == 0

    @property
    def ptr(self):
        return self.v.data_ptr()

    def untouched(self):
        torch.cuda.synchronize()
        return bool((self.buf == self.fill).all())

    def guards_intact(self):
        torch.cuda.synchronize()
        n0 = self.v.storage_offset()
        return bool((self.buf[:n0] == self.fill).all()) and bool((self.buf[n0 + self.v.numel():] == self.fill).all())


def operand(vals, ld, off):
    """[rows, C] values in rows of ``ld`` elements; everything else in the buffer NaN."""
    rows, C = vals.shape
    b = Buf(rows * ld, vals.dtype, off, float("nan"))
    b.v.view(rows, ld)[:, :C] = vals.to(dev())
    return b


class Dst:
    """The strided destination inside sentinels; ``take`` returns dW[t][m][n] and checks every other element."""

    def __init__(self, d, prefill=None):
        self.idx = WR.dst_index(d)
        assert self.idx.unique().numel() == self.idx.numel()
        self.b = Buf(int(self.idx.max()) + 1)
        self.idx = self.idx.to(dev())
        if prefill is not None:
            self.b.v[self.idx] = prefill.to(dev())

    def take(self):
        torch.cuda.synchronize()
        out = self.b.v[self.idx].cpu()
        self.b.v[self.idx] = SENT
        assert self.b.untouched(), "a sentinel outside the destination was overwritten"
        return out


def _show(name, err, bar):
    print(f"{name}: {err:.3e} (bar {bar:.1e})")
    return err


@functools.lru_cache(maxsize=8)
def _data(geom, io, f16k, ldp, ldq):
    """P, Q as the kernel is given them and the fp64 reference (dW [t][m][n], dbias [m]) of one geometry."""
    L = _L()
    d = make_desc(L, Case("ref", geom, io=io, ldp=ldp, ldq=ldq))
    P = WR.rand((d.B * d.Hq * d.Wq, d.M), 11)
    Q = WR.rand((d.B * d.Hqq * d.Wqq, d.N), 12)
    if io & 1:
        P = P.half()
    if io & 2:
        Q = Q.half()
    Pr, Qr = P, Q
    dn = WR.Desc(d.B, d.Hq, d.Wq, d.M, d.N, d.Hqq, d.Wqq, d.sq, list(d.dh)[:d.ntaps], list(d.dw)[:d.ntaps],
                 square_q=d.square_q)
    tie = 0.0
    if f16k:  # the f16-MFMA kernels round what they stage (see the module docstring)
        Pr = P.half()
        if d.square_q:
            Qr, twice = square_to_half(Q)
            dn.square_q = 0
            # the most a result can move if every double-rounding tie goes the other way: sum_q |P| |once - twice|
            tie = float(WR.wgrad_ref(dn, Pr.double().abs(), (Qr.double() - twice.double()).abs())[0].max())
        else:
            Qr = Q.half()
    dW, _ = WR.wgrad_ref(dn, Pr, Qr)
    return P, Q, dW, P.double().sum(0), tie


def square_to_half(Q):
    """Q * Q in fp16, (rounded once from the exact square, rounded to fp32 and then to fp16).  numpy converts float64
    to float16 in one rounding (torch's CPU cast goes through fp32); an fp32 x fp32 product is exact in float64."""
    sq = Q.double() * Q.double()
    once = torch.from_numpy(sq.numpy().astype(np.float16))
    return once, sq.float().half()


def run_case(c, mode):
    L = _L()
    lib = L.load()
    name, lanes = query(L, c, mode)
    assert name == kernel_of(c, mode), (c.id, mode, name)
    assert lanes == c.lanes, (c.id, lanes)
    with tuned(lib, {**dict(c.tune), 7: mode}):
        d = make_desc(L, c)
        P, Q, dWr, dbr, tie = _data(c.geom, c.io, "f16" in name, c.ldp, c.ldq)
        p, q = operand(P, d.ldp, c.poff), operand(Q, d.ldq, c.qoff)
        w0 = WR.rand((d.ntaps, d.M, d.N), 13) if c.acc else None
        b0 = WR.rand((d.M,), 14) if c.acc else None
        dst = Dst(d, w0)
        db = Buf(d.M) if c.bias else None
        if c.bias and c.acc:
            db.v.copy_(b0)
        need = int(lib.hyres_wgrad_workspace_bytes(ctypes.byref(d)))
        assert need % 4 == 0 and c.wsoff % 4 == 0
        ws = Buf(need // 4, off=c.wsoff // 4)
        args = (ctypes.byref(d), p.ptr, q.ptr, dst.b.ptr, db.ptr if c.bias else None, ws.ptr, need)
        if c.deferred:
            jobs = (L.WgradJob * 2)()
            nj = ctypes.c_int(0)
            L.call("hyres_conv_wgrad_deferred", *args, jobs, ctypes.byref(nj), L.stream())
            assert nj.value == (1 if (not c.bias or d.M <= 16 and d.ntaps > 1 and d.N > 16) else 2)
            assert jobs[0].lanes == c.lanes
            L.call("hyres_wgrad_reduce_jobs", jobs, nj.value, L.stream())
        else:
            L.call("hyres_conv_wgrad", *args, L.stream())
        assert ws.guards_intact(), "the workspace was overrun"
        got = dst.take()
        ref = dWr + w0.double() if c.acc else dWr
        fam = name.split("<")[0]
        bar = TOL + tie / float(ref.abs().max())  # tie: only wgrad_f16_kernel's SQ path with an fp32 Q has any
        assert bar < TOL_WIDE
        err = _show(f"{c.id} {name} dW", rel_err(got, ref), bar)
        errb = 0.0
        if c.bias:
            assert db.guards_intact()
            torch.cuda.synchronize()
            errb = _show(f"{c.id} {name} dbias", rel_err(db.v.cpu(), dbr + b0.double() if c.acc else dbr), TOL)
        WORST[fam] = max(WORST.get(fam, 0.0), err, errb)
        assert err < bar and errb < TOL, (c.id, name, err, errb, bar)
        return got, (db.v.cpu() if c.bias else None)


def _params(pred):
    out = []
    for c in CASES:
        if pred(c) and c.id in KERNELS:
            for m in modes_of(c):
                out.append(pytest.param(c.id, m, id=f"{c.id}/{'bf16x6' if m else 'native'}/{kernel_of(c, m)}"))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("cid,mode", _params(lambda c: not c.deferred))
def test_wgrad_kernel(cid, mode):
    run_case(BY_ID[cid], mode)


@pytest.mark.gpu
@pytest.mark.parametrize("cid,mode", _params(lambda c: c.deferred))
def test_wgrad_deferred_then_batched_reduce(cid, mode):
    """hyres_conv_wgrad_deferred + hyres_wgrad_reduce_jobs against the reference, and bit for bit against the
    immediate call."""
    c = BY_ID[cid]
    dw, db = run_case(c, mode)
    dw0, db0 = run_case(Case(**{**c.__dict__, "deferred": False}), mode)
    assert torch.equal(dw, dw0)
    assert db is None or torch.equal(db, db0)


# ------------------------------------------------------------------------------------------------------ colsum
COLSUM = [(1001, 64, 64, 0, 0, "colsum_partial_kernel<4, false>"), (1001, 64, 68, 0, 1, "colsum_partial_kernel<4, false>"),
          (1001, 6, 6, 0, 0, "colsum_partial_kernel<1, false>"), (1001, 64, 66, 0, 1, "colsum_partial_kernel<1, false>"),
          (1001, 64, 68, 1, 0, "colsum_partial_kernel<4, true>"), (1001, 6, 7, 1, 1, "colsum_partial_kernel<1, true>"),
          (77, 300, 300, 0, 0, "colsum_partial_kernel<4, false>"), (70000, 8, 8, 0, 1, "colsum_partial_kernel<4, false>"),
          (1, 5, 5, 0, 0, "colsum_partial_kernel<1, false>")]


@pytest.mark.gpu
@pytest.mark.parametrize("P,C,ld,f16,acc,kernel", COLSUM, ids=[f"P{a[0]}xC{a[1]}-ld{a[2]}{'-acc' if a[4] else ''}/{a[5]}"
                                                               for a in COLSUM])
def test_colsum(P, C, ld, f16, acc, kernel):
    """hyres_colsum alone: float4 / scalar, fp32 / fp16, a last block of fewer rows (1001 = 7 x 126 + 119), more
    channel groups than threads (C = 300: 75 groups, one row per 3 thread rows), 512 partial rows (P = 70000)."""
    L = _L()
    lib = L.load()
    assert (C % 4 == 0 and ld % 4 == 0) == ("<4" in kernel) and bool(f16) == ("true" in kernel)
    x = WR.rand((P, C), 21)
    if f16:
        x = x.half()
    xb = operand(x, ld, 0)
    d0 = WR.rand((C,), 22)
    out = Buf(C)
    if acc:
        out.v.copy_(d0)
    need = int(lib.hyres_colsum_workspace_bytes(P, C))
    ws = Buf(need // 4)
    L.call("hyres_colsum", xb.ptr, P, C, ld, out.ptr, acc, ws.ptr, need, f16, L.stream())
    assert ws.guards_intact() and out.guards_intact()
    ref = x.double().sum(0) + (d0.double() if acc else 0.0)
    err = _show(f"colsum {kernel}", rel_err(out.v.cpu(), ref), TOL)
    WORST["colsum_partial_kernel"] = max(WORST.get("colsum_partial_kernel", 0.0), err)
    assert err < TOL


# ------------------------------------------------------------------------------------------------------ refusals
E_SHAPE, E_ALIGN, E_ARG, E_WORKSPACE = 1001, 1002, 1003, 1004
REFUSALS = {
    "workspace-one-byte-short": (_c("r", "conv", 2, 9, 20, 64, 64, 3, 1, 1, 1), "short", E_WORKSPACE),
    "workspace-null": (_c("r", "conv", 2, 9, 20, 64, 64, 3, 1, 1, 1), "nows", E_WORKSPACE),
    "p-null": (_c("r", "conv", 2, 9, 20, 64, 64, 3, 1, 1, 1), "nop", E_ARG),
    "q-null": (_c("r", "conv", 1, 5, 13, 64, 64, 1, 1, 0, 1), "noq", E_ARG),
    "dst-null": (_c("r", "conv", 3, 3, 32, 100, 36, 3, 1, 1, 1), "nodst", E_ARG),
    "halo-p-misaligned": (_c("r", "conv", 3, 3, 32, 100, 36, 3, 1, 1, 1, poff=1), "", E_ALIGN),
    "halo-q-misaligned": (_c("r", "conv", 3, 3, 32, 100, 36, 5, 1, 2, 1, qoff=2), "", E_ALIGN),
    "halo-cvt-workspace-misaligned": (_c("r", "conv", 3, 3, 32, 100, 36, 3, 1, 1, 1, io=3, wsoff=4), "", E_ALIGN),
    "f16-q-misaligned": (_c("r", "conv", 2, 9, 20, 64, 64, 3, 1, 1, 1, f16=1, qoff=1), "", E_ALIGN),
    "f16-p16-misaligned": (_c("r", "conv", 1, 5, 13, 64, 64, 1, 1, 0, 1, f16=1, io=1, poff=4), "", E_ALIGN),
    "square-q-C6": (_c("r", "gdn", 2, 9, 20, 6), "", E_SHAPE),
    "square-q-misaligned": (_c("r", "gdn", 2, 9, 20, 64, qoff=1), "", E_SHAPE),
    "square-q-ldq+1": (_c("r", "gdn", 2, 9, 20, 64, ldq=1), "", E_SHAPE),
}


@pytest.mark.gpu
@pytest.mark.parametrize("rid", list(REFUSALS))
def test_wgrad_refusals_leave_everything_untouched(rid):
    L = _L()
    lib = L.load()
    c, how, code = REFUSALS[rid]
    d = make_desc(L, c)
    P, Q, _, _, _ = _data(c.geom, c.io, False, c.ldp, c.ldq)
    p, q = operand(P, d.ldp, c.poff), operand(Q, d.ldq, c.qoff)
    dst, db = Dst(d), Buf(d.M)
    need = int(lib.hyres_wgrad_workspace_bytes(ctypes.byref(d)))
    ws = Buf(need // 4, off=c.wsoff // 4)
    with pytest.raises(L.HipError, match=rf"\({code}\)"):
        L.call("hyres_conv_wgrad", ctypes.byref(d), None if how == "nop" else p.ptr, None if how == "noq" else q.ptr,
               None if how == "nodst" else dst.b.ptr, db.ptr, None if how == "nows" else ws.ptr,
               need - (how == "short"), L.stream())
    assert dst.b.untouched() and db.untouched() and ws.untouched()


@pytest.mark.gpu
@pytest.mark.parametrize("bad", ["lanes5", "nsplit0", "slab-null", "dst-null", "M0", "jobs-null", "n-negative"])
def test_reduce_jobs_refusals(bad):
    L = _L()
    slab, dst = Buf(2 * 8 * 8), Buf(64)
    j = L.WgradJob(slab.ptr, dst.ptr, 2, 1, 8, 8, 8, 1, 1, 0, 16, 0)
    good = L.WgradJob(slab.ptr, dst.ptr, 2, 1, 8, 8, 8, 1, 1, 0, 16, 0)
    n = 2
    if bad == "lanes5":
        j.lanes = 5
    elif bad == "nsplit0":
        j.nsplit = 0
    elif bad == "slab-null":
        j.slab = None
    elif bad == "dst-null":
        j.dst = None
    elif bad == "M0":
        j.M = 0
    elif bad == "n-negative":
        n = -1
    jobs = (L.WgradJob * 2)(good, j)  # the good job first: nothing may be reduced before the list is validated
    with pytest.raises(L.HipError, match=rf"\({E_ARG}\)"):
        L.call("hyres_wgrad_reduce_jobs", None if bad == "jobs-null" else jobs, n, L.stream())
    assert dst.untouched() and slab.untouched()
