"""A plain fp64 reference of hyres_conv_forward, written from include/hyres_hip.h and with no GPU state:

  * ``torch_acc``: the convolution itself by torch fp64 on the CPU, from the values the kernel is given: F.conv2d,
    F.conv_transpose2d(stride=2, padding=2, output_padding=1), torch.autograd.grad of those for the two input-gradient
    geometries, the masked weight for the checkerboard conv, x * x for square_input;
  * ``geom_eval``: the geometry-level definition, literally the formula of hyres_hip.h:40-42 applied to the fields of a
    hyres_conv_geom (the ctypes struct or any object with its attribute names) and a re-laid-out w2 of any ``ldw``. It
    serves what no torch op expresses and, on the CPU, checks the hyres_geom_* helpers and ``relayout`` against torch;
  * ``relayout``: the reference of hyres_conv_weight_prep from g.kh / g.kw;
  * ``epilogue``: the seven epilogue kinds, the four activations, res, out2 and accumulate (hyres_hip.h:95-124).

Activations are NHWC ([B, H, W, C]), weights in the PyTorch layout.  Operands are promoted as they are given, so a
caller that stores or stages fp16 passes the fp16-rounded tensors."""
import torch
import torch.nn.functional as F

EPI_BIAS, EPI_GDN, EPI_IGDN, EPI_GDN_BWD, EPI_IGDN_BWD, EPI_ROWSCALE, EPI_SA_BWD = range(7)
ACT_NONE, ACT_RELU, ACT_PRELU, ACT_RELU_MASK = range(4)
WPREP_CONV, WPREP_CONV_DGRAD, WPREP_DECONV, WPREP_DECONV_DGRAD = range(4)


def rand(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def grid32(shape, seed):
    """Values k / 32, |k| <= 32: x and x * x are both exact in fp16."""
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-32, 33, shape, generator=g).float() / 32


def shape_id(geom):
    return f"{geom[0]}-" + "x".join(str(v) for v in geom[1:])


def checkerboard_keep(K=5):
    """CheckboardMaskedConv2d's live taps (models/layers/checkerboard.py:49-50): kh + kw odd, 12 of 25."""
    return [[(kh + kw) % 2 for kw in range(K)] for kh in range(K)]


def _nchw(x):
    return x.permute(0, 3, 1, 2)


def _nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous()


def torch_acc(geom, x, w, mask=None, square=False):
    """The GEMM result [B, Ho, Wo, Co] (no bias) of a case geometry in fp64.  geom: ("conv" | "dgrad", B, H, W, Ci, Co, KH,
    KW, stride, pad, dil) | ("deconv" | "deconv_dgrad", B, H, W, Ci, Co) (K = 5, stride 2, padding 2, output_padding 1),
    (B, H, W, Ci, Co) those of the ORIGINAL layer; x is the kernel's input (the layer's input, or dY for the gradients),
    w the layer's PyTorch-layout weight."""
    kind = geom[0]
    x, w = x.double(), w.double()
    if mask is not None:
        w = w * mask.double()
    if square:
        x = x * x
    if kind == "conv":
        s, p, d = geom[8:11]
        return _nhwc(F.conv2d(_nchw(x), w, None, stride=s, padding=p, dilation=d))
    if kind == "deconv":
        return _nhwc(F.conv_transpose2d(_nchw(x), w, None, stride=2, padding=2, output_padding=1))
    B, H, W, Ci = geom[1:5]
    xin = torch.zeros(B, Ci, H, W, dtype=torch.float64, requires_grad=True)
    if kind == "dgrad":
        s, p, d = geom[8:11]
        y = F.conv2d(xin, w, None, stride=s, padding=p, dilation=d)
    else:
        assert kind == "deconv_dgrad"
        y = F.conv_transpose2d(xin, w, None, stride=2, padding=2, output_padding=1)
    assert tuple(y.shape) == tuple(_nchw(x).shape), (y.shape, x.shape)
    (gx,) = torch.autograd.grad(y, xin, _nchw(x))
    return _nhwc(gx)


def relayout(g, w, mode, mask=None):
    """hyres_conv_weight_prep's result [rows, ntaps * cols] from g.kh / g.kw (a pure copy: same dtype as w)."""
    if mask is not None:
        w = w * mask
    rows = []
    for t in range(g.ntaps):
        wt = w[:, :, g.kh[t], g.kw[t]]  # Conv2d: [Co][Ci]; ConvTranspose2d: [Ci][Co]
        rows.append(wt if mode in (WPREP_CONV, WPREP_DECONV_DGRAD) else wt.t())
    return torch.stack(rows, 1).reshape(rows[0].shape[0], -1).contiguous()


def geom_eval(g, x, w2, ldw=None, square=False):
    """Y[b, i*osh+oph[p], j*osw+opw[p], co] = sum over taps t of phase p and ci < Ci of
    X[b, i*ish + dh[t], j*isw + dw[t], ci] * W2[co*ldw + t*Ci + ci], zero outside X.  x: [B, Hi, Wi, Ci]; w2: [rows >= Co,
    ldw] (or flat).  Returns (Y [B, Ho, Wo, Co] float64, written [Ho, Wo] bool: the pixels some phase produces)."""
    ldw = g.ntaps * g.Ci if ldw is None else ldw
    x = x.double().reshape(g.B, g.Hi, g.Wi, g.Ci)
    if square:
        x = x * x
    w2 = w2.double().reshape(-1, ldw)[:g.Co]
    dh, dw = [g.dh[t] for t in range(g.ntaps)], [g.dw[t] for t in range(g.ntaps)]
    top, left = max(0, -min(dh)), max(0, -min(dw))
    bot = max(0, (g.Hq - 1) * g.ish + max(dh) - (g.Hi - 1))
    right = max(0, (g.Wq - 1) * g.isw + max(dw) - (g.Wi - 1))
    xp = torch.zeros(g.B, g.Hi + top + bot, g.Wi + left + right, g.Ci, dtype=torch.float64)
    xp[:, top:top + g.Hi, left:left + g.Wi] = x
    y = torch.zeros(g.B, g.Ho, g.Wo, g.Co, dtype=torch.float64)
    written = torch.zeros(g.Ho, g.Wo, dtype=torch.bool)
    for p in range(g.nphase):
        acc = torch.zeros(g.B, g.Hq, g.Wq, g.Co, dtype=torch.float64)
        for t in range(g.tap0[p], g.tap0[p] + g.ntap[p]):
            h0, w0 = top + dh[t], left + dw[t]
            xs = xp[:, h0:h0 + (g.Hq - 1) * g.ish + 1:g.ish, w0:w0 + (g.Wq - 1) * g.isw + 1:g.isw]
            acc += torch.einsum("bijc,oc->bijo", xs, w2[:, t * g.Ci:(t + 1) * g.Ci])
        hs = slice(g.oph[p], g.oph[p] + (g.Hq - 1) * g.osh + 1, g.osh)
        ws = slice(g.opw[p], g.opw[p] + (g.Wq - 1) * g.osw + 1, g.osw)
        assert not written[hs, ws].any(), "two phases write one pixel"
        y[:, hs, ws] = acc
        written[hs, ws] = True
    return y, written


def epilogue(kind, act, acc, bias=None, res=None, slope=None, aux0=None, aux1=None, aux2=None, y_old=None):
    """(y, out2) in fp64 from the GEMM result acc [..., Co]; out2 is None where the kind writes none.  Operands are
    [..., Co] except ROWSCALE's aux1 [...] (one scale per pixel) and SA_BWD's aux0 [..., 2] / aux2 [...] (argmax, integer);
    y_old: the destination's previous content, added last (accumulate)."""
    v = acc.double()
    d = (lambda t: None if t is None else t.double())
    bias, res, aux0, aux1 = d(bias), d(res), d(aux0), d(aux1)
    out2 = None
    if kind in (EPI_BIAS, EPI_ROWSCALE):
        if kind == EPI_ROWSCALE:
            v = v * aux1.unsqueeze(-1)
        if bias is not None:
            v = v + bias
        if res is not None:
            v = v + res
        out2 = v
        if act == ACT_RELU:
            v = v.clamp(min=0)
        elif act == ACT_PRELU:
            v = torch.where(v >= 0, v, float(slope) * v)
        elif act == ACT_RELU_MASK:
            v = torch.where(aux0 > 0, v, torch.zeros_like(v))
    elif kind in (EPI_GDN, EPI_IGDN):
        n = v + bias if bias is not None else v
        out2 = n
        v = aux0 / n.sqrt() if kind == EPI_GDN else aux0 * n.sqrt()
    elif kind in (EPI_GDN_BWD, EPI_IGDN_BWD):
        n = aux2.double()
        v = 2.0 * aux0 * v + (aux1 / n.sqrt() if kind == EPI_GDN_BWD else aux1 * n.sqrt())
    elif kind == EPI_SA_BWD:
        co = torch.arange(v.shape[-1])
        v = v + aux0[..., 0:1] + torch.where(co == aux2.long().unsqueeze(-1), aux0[..., 1:2], torch.zeros(()).double())
    else:
        raise ValueError(kind)
    if y_old is not None:
        v = v + y_old.double()
    return v, out2
