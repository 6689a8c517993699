"""The yardstick of the MS-SSIM backward tests: autograd through tests/msssim_ref.py's torch-op restatement, in fp64
as the reference gradient and in fp32 to measure the reference's own rounding error. Nothing here touches the code
under test."""
from __future__ import annotations

import functools

import torch

import msssim_ref as R

PARITY = [(s, d) for s in R.SHAPES for d in ("noise", "blur", "const")]
PARITY_IDS = [f"{'x'.join(map(str, s))}-{d}" for s, d in PARITY]
# the smallest legal shapes of one and two levels: one output row and two tiles across; pooled to 11 x 11, one output
REDUCED = [((1, 1, 12, 43), (1.0,)), ((1, 2, 21, 21), (0.4, 0.6))]
FLOOR = 16 * 2.0 ** -24  # times the gradient's scale: a few fp32 roundings of the largest entry


def grad_out(B):
    """Non-uniform over the batch, so that a per-image mix-up shows."""
    return torch.arange(1, B + 1, dtype=torch.float32) / B


def ref_grad(x, y, dtype, weights=R.WEIGHTS):
    """d (sum_b grad_out[b] * ms_ssim_ref(x, y)[b]) / d y by autograd, evaluated in ``dtype``; returned as fp64."""
    yy = y.detach().clone().to(dtype).requires_grad_(True)
    out, _ = R.ms_ssim_ref(x.detach(), yy, dtype, weights=tuple(weights))
    (out * grad_out(x.shape[0]).to(dtype)).sum().backward()
    return yy.grad.double()


def bound(d, s):
    """max|g - g64| <= max(8 * d, 16 * 2^-24 * s): d = max|g32 - g64| of the case, the factor 8 for an equally valid
    fp32 order (the forward's factor), s the scale of the shape's gradients."""
    return max(8 * float(d), FLOOR * float(s))


@functools.lru_cache(maxsize=None)
def case(shape, distortion, weights=R.WEIGHTS):
    """Computed once per case and shared: the inputs, g64, d, and s = max|g64| of the same shape's "noise" case (of
    the case itself for reduced levels)."""
    x, y = R.make_pair(shape, distortion, seed=R.SHAPES.index(shape) if shape in R.SHAPES else 7)
    g64 = ref_grad(x, y, torch.float64, weights)
    d = float((ref_grad(x, y, torch.float32, weights) - g64).abs().max())
    if shape in R.SHAPES and distortion != "noise":
        s = case(shape, "noise", weights)["s"]
    else:
        s = float(g64.abs().max())
    return {"x": x, "y": y, "g64": g64, "d": d, "s": s, "tol": bound(d, s)}


def device_grad(metrics, x, y, weights=None, wrt="y"):
    """The gradient of sum_b grad_out[b] * ms_ssim(x, y)[b] through the code under test, towards ``wrt``."""
    x, y = x.detach().clone(), y.detach().clone()
    leaf = (y if wrt == "y" else x).requires_grad_(True)
    out = metrics.ms_ssim(x, y, size_average=False, weights=weights)
    assert out.requires_grad and out.shape == (x.shape[0],)
    (out * grad_out(x.shape[0]).to(out.device)).sum().backward()
    return leaf.grad


def check(g, ref, what=""):
    """Print the figures, then assert the bound."""
    assert g.dtype == torch.float32 and torch.isfinite(g).all(), what
    err = float((g.detach().cpu().double() - ref["g64"]).abs().max())
    print(f"{what}: max|g64| {float(ref['g64'].abs().max()):.3e} d {ref['d']:.3e} err {err:.3e} (bound {ref['tol']:.3e})")
    assert err <= ref["tol"], (what, err, ref["tol"])
    return err
