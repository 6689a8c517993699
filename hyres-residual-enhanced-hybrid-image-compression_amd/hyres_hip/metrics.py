"""MS-SSIM and SSIM as HIP kernels (csrc/msssim.hip): pytorch_msssim's ``ms_ssim`` / ``ssim`` at their defaults
(11-tap sigma-1.5 Gaussian, valid filtering, K = (0.01, 0.03), five levels, 2x2 average pooling with padding
``side % 2`` between them), the second figure of every rate-distortion table (src/inference.py, src/utils/metrics.py).

    ms_ssim(x, y, data_range=1.0, size_average=True, weights=None) -> 0-dim tensor, or [B] if not size_average
    ssim(x, y, data_range=1.0, size_average=True)                  -> the same for single-scale SSIM (not clamped)
    per_level(x, y, ...)  -> ([B], [levels, B, C]): the per-image values and the raw per-level means behind them

Tensors on the GPU run the kernels on the current stream: no host sync, no allocation inside the native call, every
sum in a fixed order (the same input gives the same bits; capture-legal). CPU tensors run the pure-host twin of the
same arithmetic (csrc/msssim_core.h).

Differentiable: with grad mode on and an input that requires grad, ``ms_ssim``, ``ssim`` and ``per_level``'s ``out``
carry a gradient (hyres_msssim_bwd: two more kernels per level, gather only, the same bits on every call, capture-legal;
the host twin for CPU tensors), returned in the input's dtype; ``per_level``'s ``means`` never does. The function is
symmetric in its two images, so the gradient towards ``x`` is the native call with the images swapped: two native calls
when both require grad. A channel in which any level's mean is <= 0 contributes 0 to the value and gets a zero gradient
(also under ``ssim``, whose value is not clamped). Double backward is refused. Without grad the code path and the bits
are what they were before the backward existed.
"""
from __future__ import annotations

import ctypes
from typing import Optional, Sequence, Tuple

import torch

from . import _lib as L

DEFAULT_WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)
MAX_LEVELS = 5
WIN = 11


def min_side(levels: int) -> int:
    """min(H, W) must be LARGER than this for ``levels`` levels."""
    return (WIN - 1) * 2 ** (levels - 1)


def _check(x: torch.Tensor, y: torch.Tensor, levels: int, what: str) -> None:
    if not (isinstance(x, torch.Tensor) and isinstance(y, torch.Tensor)):
        raise ValueError(f"{what}: x and y must be tensors")
    if x.dim() != 4 or x.shape != y.shape:
        raise ValueError(f"{what}: x and y must be [B,C,H,W] of one shape (got {tuple(x.shape)}, {tuple(y.shape)})")
    if not (x.is_floating_point() and y.is_floating_point()):
        raise ValueError(f"{what}: floating-point inputs (got {x.dtype}, {y.dtype})")
    if x.device != y.device:
        raise ValueError(f"{what}: x on {x.device}, y on {y.device}")
    if not 1 <= levels <= MAX_LEVELS:
        raise ValueError(f"{what}: 1 to {MAX_LEVELS} level weights (got {levels})")
    B, C, H, W = x.shape
    if B < 1 or C < 1 or B * C > 65535:
        raise ValueError(f"{what}: B, C >= 1 and B * C <= 65535 (got {B}, {C})")
    if min(H, W) <= min_side(levels):
        raise ValueError(f"{what}: min(H, W) must be larger than {min_side(levels)} = (11 - 1) * 2^(levels - 1) "
                         f"for {levels} levels (got {H} x {W})")


def _forward(x, y, w, data_range):
    """x, y: fp32 contiguous, no autograd."""
    B, C, H, W = x.shape
    levels = len(w)
    wts = (ctypes.c_float * levels)(*w)
    out = torch.empty(B, dtype=torch.float32, device=x.device)
    means = torch.empty((levels, B, C), dtype=torch.float32, device=x.device)
    if x.is_cuda:
        from .ops import Workspace
        nws = L.load().hyres_msssim_workspace_bytes(B, C, H, W, levels)
        if nws < 0:
            L.check(1, "hyres_msssim_workspace_bytes")
        ws = Workspace.get(int(nws), x.device, "msssim")
        L.call("hyres_msssim", x.data_ptr(), y.data_ptr(), B, C, H, W, levels, wts, float(data_range), out.data_ptr(),
               means.data_ptr(), ws.data_ptr(), ws.numel(), L.stream())
    else:
        L.call("hyres_msssim_host", x.data_ptr(), y.data_ptr(), B, C, H, W, levels, wts, float(data_range),
               out.data_ptr(), means.data_ptr(), None, 0, ctypes.c_void_p(None))
    return out, means


def _backward(x, y, w, data_range, grad_out):
    """d (sum_b grad_out[b] * out[b]) / d y; swap x and y for the gradient towards x."""
    B, C, H, W = x.shape
    levels = len(w)
    wts = (ctypes.c_float * levels)(*w)
    grad_out = grad_out.to(torch.float32).contiguous()
    grad = torch.empty_like(y)
    if x.is_cuda:
        from .ops import Workspace
        nws = L.load().hyres_msssim_bwd_workspace_bytes(B, C, H, W, levels)
        if nws < 0:
            L.check(1, "hyres_msssim_bwd_workspace_bytes")
        ws = Workspace.get(int(nws), x.device, "msssim_bwd")
        L.call("hyres_msssim_bwd", x.data_ptr(), y.data_ptr(), B, C, H, W, levels, wts, float(data_range),
               grad_out.data_ptr(), grad.data_ptr(), ws.data_ptr(), ws.numel(), L.stream())
    else:
        L.call("hyres_msssim_bwd_host", x.data_ptr(), y.data_ptr(), B, C, H, W, levels, wts, float(data_range),
               grad_out.data_ptr(), grad.data_ptr(), None, 0, ctypes.c_void_p(None))
    return grad


class _MsSsimFn(torch.autograd.Function):
    """(out [B], means [levels, B, C]) of fp32 contiguous x, y; ``raw`` returns mean_c means[0] in place of out
    (``ssim``: the value is not clamped, the gradient is that of the clamped one)."""

    @staticmethod
    def forward(ctx, x, y, w, data_range, raw):
        out, means = _forward(x, y, w, data_range)
        if raw:
            out = means[0].mean(1)
        ctx.save_for_backward(x, y)
        ctx.w, ctx.data_range = w, data_range
        ctx.mark_non_differentiable(means)
        return out, means

    @staticmethod
    def backward(ctx, grad_out, _grad_means):
        if torch.is_grad_enabled():  # create_graph=True
            raise RuntimeError("ms_ssim / ssim: double backward is not supported (the backward ran with create_graph)")
        x, y = ctx.saved_tensors
        gx = _backward(y, x, ctx.w, ctx.data_range, grad_out) if ctx.needs_input_grad[0] else None
        gy = _backward(x, y, ctx.w, ctx.data_range, grad_out) if ctx.needs_input_grad[1] else None
        return gx, gy, None, None, None


def _wants_grad(x, y):
    return torch.is_grad_enabled() and (x.requires_grad or y.requires_grad)


def per_level(x: torch.Tensor, y: torch.Tensor, data_range: float = 1.0, weights: Optional[Sequence[float]] = None,
              what: str = "ms_ssim") -> Tuple[torch.Tensor, torch.Tensor]:
    """(out [B], means [levels, B, C]): means[l] is the spatial mean of cs_map for l < levels - 1 and of ssim_map for
    the last level, before the relu; out[b] = mean_c prod_l relu(means[l, b, c]) ** weights[l]."""
    w = tuple(float(v) for v in (DEFAULT_WEIGHTS if weights is None else weights))
    _check(x, y, len(w), what)
    if _wants_grad(x, y):
        return _MsSsimFn.apply(x.to(torch.float32).contiguous(), y.to(torch.float32).contiguous(), w,
                               float(data_range), False)
    return _forward(x.detach().to(torch.float32).contiguous(), y.detach().to(torch.float32).contiguous(), w,
                    data_range)


def ms_ssim(x: torch.Tensor, y: torch.Tensor, data_range: float = 1.0, size_average: bool = True,
            weights: Optional[Sequence[float]] = None) -> torch.Tensor:
    out, _ = per_level(x, y, data_range, weights)
    return out.mean() if size_average else out


def ssim(x: torch.Tensor, y: torch.Tensor, data_range: float = 1.0, size_average: bool = True) -> torch.Tensor:
    """Single-scale SSIM: the raw mean of ssim_map per channel (pytorch_msssim's nonnegative_ssim=False), averaged
    over channels, and over the batch if ``size_average``."""
    if _wants_grad(x, y):
        _check(x, y, 1, "ssim")
        v, _ = _MsSsimFn.apply(x.to(torch.float32).contiguous(), y.to(torch.float32).contiguous(), (1.0,),
                               float(data_range), True)
        return v.mean() if size_average else v
    _, means = per_level(x, y, data_range, (1.0,), "ssim")
    return means[0].mean() if size_average else means[0].mean(1)
