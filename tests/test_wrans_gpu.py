"""GPU: the device rANS coder (csrc/wrans.hip) against its pure-host twin on the cases of tests/test_wrans_cpu.py, and
the model's compress / decompress with ``device_coder`` against the host coder. Integer work: every comparison is
equality."""
import numpy as np
import pytest
import torch

from helpers import build_model
from test_wrans_cpu import ESC_HI, NAMES, _case, host_decode, host_encode, tables

pytestmark = pytest.mark.gpu


def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def batch_of(c):
    """B = 3 strings of the case's shape and different byte lengths: the case itself, one with further escapes, one
    without any (same indexes and means)."""
    own = c["own"]
    more, none = dict(c), dict(c)
    more["sym"], none["sym"] = c["sym"].copy(), c["sym"].copy()
    cdf, lengths, offsets, _ = tables()
    if len(own):
        more["sym"][own[::3]] = ESC_HI
        ci = c["idx"][own]
        none["sym"][own] = np.clip(c["sym"][own], offsets[ci], offsets[ci] + lengths[ci] - 3)
    return [c, more, none]


def device_tables(D):
    cdf, lengths, offsets, _ = tables()
    return [torch.from_numpy(a).to(D) for a in (cdf, lengths, offsets)]


def table_args(t):
    return t[0].data_ptr(), t[0].shape[1], t[1].data_ptr(), t[2].data_ptr(), t[0].shape[0]


def device_encode(batch, D, t):
    from hyres_hip import _lib as L
    c = batch[0]
    B, shape = len(batch), (c["C"], c["H"], c["W"], c["parity"])
    sym = torch.from_numpy(np.stack([b["sym"] for b in batch])).to(D)
    idx = torch.from_numpy(np.stack([b["idx"] for b in batch])).to(D)
    lib = L.load()
    cap = B * lib.hyres_wrans_max_string_bytes(*shape)
    out = torch.zeros(cap, dtype=torch.uint8, device=D)
    offs = torch.full((B + 1,), -1, dtype=torch.int64, device=D)
    ws = torch.empty(lib.hyres_wrans_workspace_bytes(B, *shape), dtype=torch.uint8, device=D)
    L.call("hyres_wrans_encode", sym.data_ptr(), idx.data_ptr(), B, *shape, *table_args(t), out.data_ptr(), cap,
           offs.data_ptr(), 0, ws.data_ptr(), ws.numel(), L.stream())
    o = offs.cpu().tolist()
    data = out.cpu().numpy().tobytes()
    assert o[0] == 0 and o[-1] <= cap
    return [data[o[b]:o[b + 1]] for b in range(B)]


def device_decode(batch, strings, D, t):
    from hyres_hip import _lib as L
    c = batch[0]
    B, shape = len(batch), (c["C"], c["H"], c["W"], c["parity"])
    idx = torch.from_numpy(np.stack([b["idx"] for b in batch])).to(D)
    params = torch.from_numpy(np.stack([b["means"] for b in batch])).to(D)  # [B, H*W, 2C]
    offs = torch.tensor(np.cumsum([0] + [len(s) for s in strings]), dtype=torch.int64, device=D)
    buf = torch.from_numpy(np.frombuffer(b"".join(strings), dtype=np.uint8).copy()).to(D)
    out = torch.full((B, c["sym"].size), -12345, dtype=torch.int32, device=D)
    L.call("hyres_wrans_decode", buf.data_ptr(), offs.data_ptr(), idx.data_ptr(), B, *shape, *table_args(t),
           params.data_ptr(), 2 * c["C"], c["C"], out.data_ptr(), L.stream())
    return out, params


@pytest.mark.parametrize("name", NAMES)
def test_device_coder_equals_host_twin(name):
    D = dev()
    t = device_tables(D)
    batch = batch_of(_case(name))
    want = [host_encode(b) for b in batch]
    if len(batch[0]["own"]) > 2:
        assert len({len(s) for s in want}) == 3  # three different lengths in one call
    got = device_encode(batch, D, t)
    assert [len(s) for s in got] == [len(s) for s in want]
    assert got == want
    assert device_encode(batch, D, t) == got  # again: the same bytes
    # device decode of the host twin's bytes (= the device's), with the unowned fill
    out, params = device_decode(batch, want, D, t)
    c = batch[0]
    C, H, W = c["C"], c["H"], c["W"]
    for b, cb in enumerate(batch):
        assert np.array_equal(out[b].cpu().numpy(), cb["sym"]), b
        assert np.array_equal(host_decode(cb, got[b]), cb["sym"]), b  # host twin decodes the device's bytes
    if c["parity"] >= 0:
        means = params[:, :, C:].reshape(len(batch), H, W, C).permute(0, 3, 1, 2)  # [B, C, H, W]
        fill = torch.round(0.0 - means).to(torch.int32).reshape(len(batch), -1)
        hh, ww = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
        unowned = (((hh + ww) % 2) != c["parity"]).expand(C, H, W).reshape(-1).to(D)
        assert torch.equal(out[:, unowned], fill[:, unowned])


def _x(shape, seed):
    return torch.rand(shape, generator=torch.Generator().manual_seed(seed))


@pytest.fixture(scope="module")
def net():
    n, _ = build_model()
    n = n.to(dev()).eval()
    assert n.update(force=True)
    return n


@pytest.mark.parametrize("shape", [(2, 3, 64, 64), (1, 3, 64, 192)])
@pytest.mark.parametrize("literal", [False, True])
def test_model_round_trip_equals_host_coder(net, shape, literal):
    """decompress(compress(x)) with the device coder is torch.equal to the host coder's, under both settings of
    decode_in_compress; the device coder's strings are HRW1, the host coder's are not."""
    D = dev()
    rm = net.residual_model
    x = _x(shape, 3).to(D)
    res = {}
    rm.decode_in_compress = literal
    try:
        for coder in (False, True):
            rm.device_coder = coder
            with torch.no_grad():
                c = net.compress(x)
                d = net.decompress(c)
            torch.cuda.synchronize()
            res[coder] = (c, d)
    finally:
        rm.device_coder = False
        rm.decode_in_compress = False
    (ch, dh), (cd, dd) = res[False], res[True]
    assert torch.equal(dd["x_hat"], dh["x_hat"])
    assert cd["shape"] == ch["shape"]
    flat = lambda s: s[0][0] + s[0][1] + s[1]  # noqa: E731
    assert len(flat(cd["strings"])) == 3 * shape[0]
    assert all(isinstance(s, bytes) and s[:4] == b"HRW1" for s in flat(cd["strings"]))
    assert not any(s[:4] == b"HRW1" for s in flat(ch["strings"]))
    print("bytes host", sum(map(len, flat(ch["strings"]))), "device", sum(map(len, flat(cd["strings"]))))


def test_literal_and_default_compress_write_the_same_strings(net):
    rm = net.residual_model
    x = _x((2, 3, 64, 64), 5).to(dev())
    rm.device_coder = True
    try:
        with torch.no_grad():
            a = net.compress(x)["strings"]
            rm.decode_in_compress = True
            b = net.compress(x)["strings"]
    finally:
        rm.device_coder = False
        rm.decode_in_compress = False
    assert a == b


def test_host_format_and_truncated_strings_are_refused(net):
    rm = net.residual_model
    x = _x((2, 3, 64, 64), 3).to(dev())
    with torch.no_grad():
        host = net.compress(x)
        rm.device_coder = True
        try:
            good = net.compress(x)
            with pytest.raises(ValueError, match="magic"):
                net.decompress(host)
            with pytest.raises(ValueError, match="magic"):
                rm.decompress(host["strings"], host["shape"])
            cut = dict(good)
            (a, na), z = good["strings"]
            cut["strings"] = [[a, [na[0], na[1][:-4]]], z]
            with pytest.raises(ValueError, match="byte count"):
                net.decompress(cut)
        finally:
            rm.device_coder = False


def test_decompress_queues_without_a_host_wait(net):
    """residual_model.decompress with the device coder under torch's sync debug mode "error": one pinned upload, the
    decode launches between the conv launches, no device-to-host copy and no wait up to the caller's own read of
    x_hat. (One call before it fills the weight, table and workspace caches.)"""
    rm = net.residual_model
    x = _x((2, 3, 64, 64), 7).to(dev())
    rm.device_coder = True
    try:
        with torch.no_grad():
            c = net.compress(x)
            want = rm.decompress(c["strings"], c["shape"])["x_hat"].cpu()
            torch.cuda.synchronize()
            torch.cuda.set_sync_debug_mode("error")
            try:
                out = rm.decompress(c["strings"], c["shape"])
            finally:
                torch.cuda.set_sync_debug_mode("default")
        assert torch.equal(out["x_hat"].cpu(), want)  # the caller's read
    finally:
        rm.device_coder = False
