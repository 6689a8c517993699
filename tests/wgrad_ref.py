"""A plain fp64 reference of the weight gradient of include/hyres_hip.h, written from its definition:

    dW[t][m][n] = sum_q P[q][m] * Q[shift_t(q)][n],   q over (B, Hq, Wq),
    shift_t(q) = (b, i * sq + dh[t], j * sq + dw[t]), the term zero outside (Hqq, Wqq),
    Q -> Q * Q with square_q, dbias[m] = sum_q P[q][m], written at dst[m * sm + n * sn + t * st].

It takes the descriptor's fields (any object with hyres_wgrad_desc's attribute names: the ctypes struct or ``Desc``
below), not a conv signature, so conv, transposed conv, the GDN gamma gradient and arbitrary tap lists are one function.
One zero-padded gather per tap and an einsum in float64: no tiles, no splits.  The operands are promoted as they are
given, so a caller that stores fp16 passes the fp16 tensors."""
from types import SimpleNamespace

import torch


def Desc(B, Hq, Wq, M, N, Hqq, Wqq, sq, dh, dw, sm=None, sn=None, st=1, square_q=0):
    """A descriptor by hand (PyTorch's [M][N][taps] destination unless the strides are given)."""
    nt = len(dh)
    assert len(dw) == nt
    return SimpleNamespace(B=B, Hq=Hq, Wq=Wq, M=M, N=N, Hqq=Hqq, Wqq=Wqq, sq=sq, ntaps=nt, dh=list(dh), dw=list(dw),
                           sm=N * nt if sm is None else sm, sn=nt if sn is None else sn, st=st, square_q=square_q)


def rand(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def wgrad_ref(d, P, Q):
    """P: [B * Hq * Wq, M], Q: [B * Hqq * Wqq, N] -> (dW [ntaps, M, N], dbias [M]) in float64."""
    p = P.double().reshape(d.B, d.Hq, d.Wq, d.M)
    q = Q.double().reshape(d.B, d.Hqq, d.Wqq, d.N)
    if d.square_q:
        q = q * q
    dh, dw = [d.dh[t] for t in range(d.ntaps)], [d.dw[t] for t in range(d.ntaps)]
    # pad Q so that every i * sq + dh, j * sq + dw is an index
    top, left = max(0, -min(dh)), max(0, -min(dw))
    bot = max(0, (d.Hq - 1) * d.sq + max(dh) - (d.Hqq - 1))
    right = max(0, (d.Wq - 1) * d.sq + max(dw) - (d.Wqq - 1))
    qp = torch.zeros(d.B, d.Hqq + top + bot, d.Wqq + left + right, d.N, dtype=torch.float64)
    qp[:, top:top + d.Hqq, left:left + d.Wqq] = q
    out = torch.empty(d.ntaps, d.M, d.N, dtype=torch.float64)
    for t in range(d.ntaps):
        h0, w0 = top + dh[t], left + dw[t]
        g = qp[:, h0:h0 + (d.Hq - 1) * d.sq + 1:d.sq, w0:w0 + (d.Wq - 1) * d.sq + 1:d.sq]
        out[t] = torch.einsum("bijm,bijn->mn", p, g)
    return out, p.sum((0, 1, 2))


def dst_index(d):
    """The flat destination index of every dW[t][m][n], as a [ntaps, M, N] LongTensor."""
    t = torch.arange(d.ntaps).view(-1, 1, 1)
    m = torch.arange(d.M).view(1, -1, 1)
    n = torch.arange(d.N).view(1, 1, -1)
    return m * d.sm + n * d.sn + t * d.st
