"""The yardstick of the MultiScaleRefine kernel tests: plain fp64 torch on the CPU for bilinear resampling (explicit
1-D weight matrices and their transpose), the SE block, SpatialAttention with its multiply, and the closed form of the
folded SpatialAttention / PReLU backward.  Activations are NHWC, as the kernels store them.  Nothing here touches the
code under test, and the bilinear adjoint shares nothing with the kernels' output-range search."""
from __future__ import annotations

import functools

import torch
import torch.nn.functional as F

# (Hi, Wi), (Ho, Wo), the convention the model reaches the shape with ("size": scale = in / out, "sf": scale = 1 / sf)
# and a scale_factor pair whose floor(in * sf) is the output size (the other convention, for the CPU checks; chosen with
# 1 / sf a short binary fraction, so that convention's scale is the same number in fp32 and fp64)
BILINEAR_SHAPES = [
    ((13, 9), (5, 7), "size", (0.4, 0.8)),
    ((5, 7), (13, 9), "size", (1 / 0.375, 1 / 0.75)),
    ((13, 10), (6, 5), "sf", (0.5, 0.5)),     # an odd height under scale_factor=0.5: scale 2, Hi != 2 * Ho
    ((16, 12), (8, 6), "sf", (0.5, 0.5)),     # exact 2x
    ((16, 12), (4, 3), "sf", (0.25, 0.25)),   # exact 4x
    ((16, 12), (8, 3), "sf", (0.5, 0.25)),    # 2 vertically, 4 horizontally
    ((1, 1), (3, 3), "size", (3.0, 3.0)),
    ((3, 3), (1, 1), "size", (0.5, 0.5)),
]
# hyres_bilinear_bwd_prelu's up-samples
PRELU_UP_SHAPES = [((6, 7), (13, 15), "size", (1 / 0.4375, 1 / 0.453125)), ((8, 5), (16, 10), "sf", (2.0, 2.0))]


def shape_id(s):
    (hi, wi), (ho, wo), conv, _ = s
    return f"{hi}x{wi}-{ho}x{wo}-{conv}"


def scales_of(s, conv=None):
    """torch's source-index scales (scale_h, scale_w) of a shape entry under a call convention."""
    (hi, wi), (ho, wo), own, sf = s
    conv = conv or own
    if conv == "size":
        return hi / ho, wi / wo
    return 1.0 / sf[0], 1.0 / sf[1]


def rand(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(shape, generator=g) * 2 - 1) * scale


# ---------------------------------------------------------------------------------------------------- bilinear
@functools.lru_cache(maxsize=None)
def weight_matrix(n_in, n_out, scale):
    """[n_out, n_in] fp64 matrix of one axis of F.interpolate(mode="bilinear", align_corners=False).  The source index
    max(scale * (o + 0.5) - 0.5, 0), its clamps and the two weights are fp32 (torch's
    area_pixel_compute_source_index on fp32 data); the weights are widened to fp64 afterwards."""
    o = torch.arange(n_out, dtype=torch.float32)
    s = torch.tensor(scale, dtype=torch.float32)
    src = torch.clamp(s * (o + 0.5) - 0.5, min=0.0)
    assert src.dtype == torch.float32
    i0 = torch.clamp(src.to(torch.int64), max=n_in - 1)
    i1 = i0 + (i0 < n_in - 1).to(torch.int64)
    l1 = src - i0.to(torch.float32)
    l0 = 1.0 - l1
    m = torch.zeros(n_out, n_in, dtype=torch.float64)
    r = torch.arange(n_out)
    m.index_put_((r, i0), l0.double(), accumulate=True)
    m.index_put_((r, i1), l1.double(), accumulate=True)
    return m


def bilinear_ref(x, Ho, Wo, scale_h, scale_w):
    """x [B, Hi, Wi, C] -> [B, Ho, Wo, C], fp64 sums."""
    mh = weight_matrix(x.shape[1], Ho, float(scale_h))
    mw = weight_matrix(x.shape[2], Wo, float(scale_w))
    return torch.einsum("oh,pw,bhwc->bopc", mh, mw, x.double())


def bilinear_bwd_ref(gy, Hi, Wi, scale_h, scale_w):
    """The adjoint: gy [B, Ho, Wo, C] -> [B, Hi, Wi, C] through the transposes of the same two matrices."""
    mh = weight_matrix(Hi, gy.shape[1], float(scale_h))
    mw = weight_matrix(Wi, gy.shape[2], float(scale_w))
    return torch.einsum("ho,wp,bopc->bhwc", mh.t(), mw.t(), gy.double())


def prelu_bwd_ref(pre, g, slope):
    """PReLU backward on a given pre-activation (torch's rule: pre > 0 passes, everything else takes the slope):
    (g_in, d slope)."""
    pre, g = pre.double(), g.double()
    pos = pre > 0
    return torch.where(pos, g, float(slope) * g), (pre * g)[~pos].sum()


# ---------------------------------------------------------------------------------------------------- SE block
def se_ref(x, w1, w2):
    """SEBlock on x [B, HW, C]: (y, pooled, hidden, gate), fp64; the backward is autograd."""
    pooled = x.mean(1)
    hidden = F.relu(F.linear(pooled, w1))
    gate = torch.sigmoid(F.linear(hidden, w2))
    return x * gate[:, None, :], pooled, hidden, gate


# ---------------------------------------------------------------------------------------------------- SpatialAttention
def first_argmax(x):
    """The first maximal index over the last axis, computed without torch.max's own tie rule."""
    C = x.shape[-1]
    m = x.max(-1, keepdim=True)[0]
    idx = torch.arange(C, dtype=torch.int64).expand(x.shape)
    return torch.where(x == m, idx, torch.full_like(idx, C)).min(-1)[0]


def sa_ref(x, w):
    """SpatialAttention with its multiply on x [B, H, W, C], w [1, 2, 7, 7]: (y, attn [B, H, W], pooled2 [B, H, W, 2],
    argmax [B, H, W]), fp64.  The channel max is torch's x.max(1) on the CPU (NCHW view), whose index autograd routes
    the max's gradient to."""
    xc = x.permute(0, 3, 1, 2)
    mean = xc.mean(1, keepdim=True)
    mx, idx = xc.max(1, keepdim=True)
    pooled = torch.cat([mean, mx], 1)
    attn = torch.sigmoid(F.conv2d(pooled, w, None, padding=3))
    y = (xc * attn).permute(0, 2, 3, 1)
    return y, attn[:, 0], pooled.permute(0, 2, 3, 1), idx[:, 0]


def sa_map_bwd_ref(glogit, pooled2, w):
    """Backward of the 7x7 (2 -> 1) conv at the attention logit: (g pooled2 [B, H, W, 2], g w), fp64 autograd."""
    p = pooled2.double().permute(0, 3, 1, 2).clone().requires_grad_()
    wr = w.double().clone().requires_grad_()
    F.conv2d(p, wr, None, padding=3).backward(glogit.double()[:, None])
    return p.grad.permute(0, 2, 3, 1), wr.grad


def tie_input(shape, seed):
    """Inputs with ties in the channel max: relu(round(2 x) / 2) (values 0, 0.5, 1), every 5th pixel all zeros, every
    7th pixel's maximum duplicated in the last channel."""
    x = torch.relu(torch.round(2 * rand(shape, seed)) / 2)
    f = x.view(-1, shape[-1])
    f[0::5] = 0.0
    f[3::7, -1] = f[3::7].max(-1)[0]
    return x


# ---------------------------------------------------------------------------------------------------- SA fold
def sa_fold_bwd_ref(pre, gy, attn, bias, slope):
    """Backward of h = PReLU(pre), pre = attn[p] * z[p] + bias, attn = sigmoid(logit), in closed form on pre [P, C],
    gy [P, C], attn [P]: gs = d z, glogit = d logit, d bias, d slope."""
    pre, gy, attn, bias = pre.double(), gy.double(), attn.double(), bias.double()
    pos = pre > 0
    gp = torch.where(pos, gy, float(slope) * gy)
    gs = attn[:, None] * gp
    glogit = (1.0 - attn) * (gp * (pre - bias)).sum(1)      # attn (1 - attn) sum gp z, with attn z = pre - bias
    return gs, glogit, gp.sum(0), (pre * gy)[~pos].sum()
