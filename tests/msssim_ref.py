"""The yardstick of the MS-SSIM tests: a torch-op restatement of pytorch_msssim's ``ms_ssim`` at its defaults (grouped
F.conv2d + F.avg_pool2d), run in fp64 as the reference and in fp32 to measure the reference's own rounding error, plus
the seeded synthetic inputs and the tolerance derived from the two.  Nothing here touches the code under test."""
from __future__ import annotations

import functools

import torch
import torch.nn.functional as F

WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)
SHAPES = [(2, 3, 161, 161), (2, 3, 163, 245), (1, 3, 176, 208), (1, 1, 192, 224)]
DISTORTIONS = ["noise", "blur", "same", "const", "inverted"]
FLOOR = 16 * 2.0 ** -24


@functools.lru_cache(maxsize=None)
def window(dtype, device="cpu"):
    """g[i] = exp(-(i - 5)^2 / (2 * 1.5^2)), built in fp32 and normalised to sum 1, then cast (kept per dtype and
    device, so a repeated call copies nothing to the device)."""
    c = torch.arange(11, dtype=torch.float32) - 5
    g = torch.exp(-(c ** 2) / (2 * 1.5 ** 2))
    return (g / g.sum()).to(dtype=dtype, device=device)


@functools.lru_cache(maxsize=None)
def _weights(weights, dtype, device):
    return torch.tensor(weights, dtype=dtype, device=device).view(-1, 1, 1)


def _gauss(t, g):
    C = t.shape[1]
    t = F.conv2d(t, g.view(1, 1, -1, 1).repeat(C, 1, 1, 1), groups=C)
    return F.conv2d(t, g.view(1, 1, 1, -1).repeat(C, 1, 1, 1), groups=C)


def level(X, Y, g, L=1.0):
    """(cs[b,c], ssim[b,c]): the spatial means of cs_map and ssim_map."""
    C1, C2 = (0.01 * L) ** 2, (0.03 * L) ** 2
    mu1, mu2 = _gauss(X, g), _gauss(Y, g)
    mu1_sq, mu2_sq, mu12 = mu1 * mu1, mu2 * mu2, mu1 * mu2
    s1 = _gauss(X * X, g) - mu1_sq
    s2 = _gauss(Y * Y, g) - mu2_sq
    s12 = _gauss(X * Y, g) - mu12
    cs_map = (2 * s12 + C2) / (s1 + s2 + C2)
    ssim_map = ((2 * mu12 + C1) / (mu1_sq + mu2_sq + C1)) * cs_map
    return cs_map.flatten(2).mean(-1), ssim_map.flatten(2).mean(-1)


def ms_ssim_ref(X, Y, dtype=torch.float64, L=1.0, weights=WEIGHTS):
    """(per image [B], raw per-level means [levels,B,C]: cs for l < levels - 1, ssim for the last)."""
    X, Y = X.to(dtype), Y.to(dtype)
    g = window(dtype, X.device)
    raw = []
    n = len(weights)
    for l in range(n):
        cs, ss = level(X, Y, g, L)
        raw.append(cs if l < n - 1 else ss)
        if l < n - 1:
            pad = (X.shape[2] % 2, X.shape[3] % 2)
            X = F.avg_pool2d(X, kernel_size=2, stride=2, padding=pad)
            Y = F.avg_pool2d(Y, kernel_size=2, stride=2, padding=pad)
    raw = torch.stack(raw)
    w = _weights(tuple(weights), dtype, X.device)
    return torch.prod(torch.relu(raw) ** w, dim=0).mean(1), raw


def ssim_ref(X, Y, dtype=torch.float64, L=1.0):
    """[B]: the channel mean of the unclamped level-0 ssim mean."""
    X, Y = X.to(dtype), Y.to(dtype)
    return level(X, Y, window(dtype, X.device), L)[1].mean(1)


def smooth_field(shape, seed):
    """A smooth sinusoidal field per channel + 0.1 * Gaussian noise, clamped to [0, 1]."""
    B, C, H, W = shape
    g = torch.Generator().manual_seed(seed)
    yy = torch.arange(H, dtype=torch.float32).view(1, 1, H, 1)
    xx = torch.arange(W, dtype=torch.float32).view(1, 1, 1, W)
    f = torch.rand((2, B, C, 1, 1), generator=g) * 0.08 + 0.02  # radians per pixel
    ph = torch.rand((2, B, C, 1, 1), generator=g) * 6.2831853
    base = 0.5 + 0.25 * torch.sin(f[0] * yy + ph[0]) * torch.cos(f[1] * xx + ph[1])
    return (base + 0.1 * torch.randn(shape, generator=g)).clamp(0, 1)


def make_pair(shape, distortion, seed=0):
    g = torch.Generator().manual_seed(1000 + seed)
    x = smooth_field(shape, seed)
    if distortion == "noise":
        y = (x + 0.05 * torch.randn(shape, generator=g)).clamp(0, 1)
    elif distortion == "blur":
        C = shape[1]
        y = F.conv2d(F.pad(x, (2, 2, 2, 2), mode="replicate"), torch.full((C, 1, 5, 5), 1 / 25.0), groups=C)
    elif distortion == "same":
        y = x.clone()
    elif distortion == "const":
        y = torch.full(shape, 0.5)
    elif distortion == "inverted":
        x = torch.rand(shape, generator=g)
        y = 1 - x
    else:
        raise KeyError(distortion)
    return x.contiguous(), y.contiguous()


def bound(d):
    """|result - fp64 restatement| <= max(8 * d, 16 * 2^-24), d = |fp32 restatement - fp64 restatement|: the factor 8
    covers a different but equally valid fp32 summation order, the floor a few fp32 roundings at 1.0.

    d is one figure per case for ``out`` (the larger of the images') and one per case and level for ``per_level`` (the
    largest over that level's (b, c) entries, which share one map size and so one error scale; the coarse levels'
    maps of a few pixels average far less rounding away than level 0's). It is not taken entry by entry: a single
    entry's fp32 value can land on its fp64 value by chance (seen: 5e-8 beside siblings at 1e-6 .. 3e-6), which says
    nothing about the rounding error of the arithmetic and would make the bound arbitrarily tight."""
    return torch.clamp(8 * d, min=FLOOR)


@functools.lru_cache(maxsize=None)
def case(shape, distortion):
    """Computed once per (shape, distortion) and shared: inputs, the fp64 reference, the bounds."""
    x, y = make_pair(shape, distortion, seed=SHAPES.index(shape))
    out64, raw64 = ms_ssim_ref(x, y, torch.float64)
    out32, raw32 = ms_ssim_ref(x, y, torch.float32)
    d_out = (out32.double() - out64).abs().max().expand_as(out64)
    d_raw = (raw32.double() - raw64).abs().flatten(1).max(1).values.view(-1, 1, 1).expand_as(raw64)
    return {"x": x, "y": y, "out": out64, "raw": raw64, "d_out": d_out, "d_raw": d_raw,
            "tol_out": bound(d_out), "tol_raw": bound(d_raw)}


def check(got_out, got_raw, ref, what=""):
    """Print the figures, then assert out and every per_level entry within the bound of the fp64 restatement."""
    e_out = (got_out.detach().cpu().double() - ref["out"]).abs()
    e_raw = (got_raw.detach().cpu().double() - ref["raw"]).abs()
    print(f"{what}: ref {ref['out'].tolist()} d {ref['d_out'].max():.3e} err {e_out.max():.3e} "
          f"(bound {ref['tol_out'].min():.3e}); per-level d {ref['d_raw'].max():.3e} err {e_raw.max():.3e}")
    assert (e_out <= ref["tol_out"]).all(), (what, e_out.tolist(), ref["tol_out"].tolist())
    assert (e_raw <= ref["tol_raw"]).all(), (what, e_raw.tolist(), ref["tol_raw"].tolist())
    return float(e_out.max()), float(e_raw.max())
