"""GPU: the segmented device rANS format HRW2 (one wave per segment) against its pure-host twin on the cases of
tests/test_wrans_cpu.py, chained encode calls, and the model's compress / decompress with ``coder_segment_rows`` against
the host coder. Integer work: every comparison is equality. Nothing damaged is decoded on the GPU: damaged strings are
the job of scripts/wrans2_host_check.cpp and tests/test_wrans2_cpu.py."""
import struct

import numpy as np
import pytest
import torch

from helpers import build_model
from test_wrans2_cpu import host_decode2, host_encode2
from test_wrans_cpu import NAMES, _case
from test_wrans_gpu import _x, batch_of, dev, device_tables, table_args

pytestmark = pytest.mark.gpu


def device_encode2(batches, R, D, t):
    """One hyres_wrans2_encode call per batch, chained into one buffer and one offset table; the strings per batch."""
    from hyres_hip import _lib as L
    lib = L.load()
    shapes = [(b[0]["C"], b[0]["H"], b[0]["W"], b[0]["parity"]) for b in batches]
    cap = sum(len(b) * lib.hyres_wrans2_max_string_bytes(*s, R) for b, s in zip(batches, shapes))
    out = torch.zeros(cap, dtype=torch.uint8, device=D)
    nstr = sum(len(b) for b in batches)
    offs = torch.full((nstr + 1,), -1, dtype=torch.int64, device=D)
    done = 0
    for j, (batch, shape) in enumerate(zip(batches, shapes)):
        B = len(batch)
        sym = torch.from_numpy(np.stack([b["sym"] for b in batch])).to(D)
        idx = torch.from_numpy(np.stack([b["idx"] for b in batch])).to(D)
        ws = torch.empty(lib.hyres_wrans2_workspace_bytes(B, *shape, R), dtype=torch.uint8, device=D)
        L.call("hyres_wrans2_encode", sym.data_ptr(), idx.data_ptr(), B, *shape, *table_args(t), R, out.data_ptr(), cap,
               offs.data_ptr() + 8 * done, int(j > 0), ws.data_ptr(), ws.numel(), L.stream())
        done += B
    o = offs.cpu().tolist()
    data = out.cpu().numpy().tobytes()
    assert o[0] == 0 and o[-1] <= cap and o == sorted(o)
    strings = [data[o[k]:o[k + 1]] for k in range(nstr)]
    res, k = [], 0
    for b in batches:
        res.append(strings[k:k + len(b)])
        k += len(b)
    return res


def device_decode2(batch, strings, R, D, t):
    from hyres_hip import _lib as L
    c = batch[0]
    B, shape = len(batch), (c["C"], c["H"], c["W"], c["parity"])
    idx = torch.from_numpy(np.stack([b["idx"] for b in batch])).to(D)
    params = torch.from_numpy(np.stack([b["means"] for b in batch])).to(D)  # [B, H*W, 2C]
    offs = torch.tensor(np.cumsum([0] + [len(s) for s in strings]), dtype=torch.int64, device=D)
    buf = torch.from_numpy(np.frombuffer(b"".join(strings), dtype=np.uint8).copy()).to(D)
    out = torch.full((B, c["sym"].size), -12345, dtype=torch.int32, device=D)
    L.call("hyres_wrans2_decode", buf.data_ptr(), offs.data_ptr(), idx.data_ptr(), B, *shape, R, *table_args(t),
           params.data_ptr(), 2 * c["C"], c["C"], out.data_ptr(), L.stream())
    return out, params


@pytest.mark.parametrize("R", [1, 3, 64])
@pytest.mark.parametrize("name", NAMES)
def test_device_coder_equals_host_twin(name, R):
    D = dev()
    t = device_tables(D)
    batch = batch_of(_case(name))
    want = [host_encode2(b, R) for b in batch]
    if len(batch[0]["own"]) > 2:
        assert len({len(s) for s in want}) == 3  # three different lengths in one call
    got = device_encode2([batch], R, D, t)[0]
    assert [len(s) for s in got] == [len(s) for s in want]
    assert got == want
    assert device_encode2([batch], R, D, t)[0] == got  # again: the same bytes
    out, params = device_decode2(batch, got, R, D, t)
    c = batch[0]
    C, H, W = c["C"], c["H"], c["W"]
    for b, cb in enumerate(batch):
        assert np.array_equal(out[b].cpu().numpy(), cb["sym"]), b
        assert np.array_equal(host_decode2(cb, got[b]), cb["sym"]), b  # host twin decodes the device's bytes
    if c["parity"] >= 0:
        means = params[:, :, C:].reshape(len(batch), H, W, C).permute(0, 3, 1, 2)  # [B, C, H, W]
        fill = torch.round(0.0 - means).to(torch.int32).reshape(len(batch), -1)
        hh, ww = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
        unowned = (((hh + ww) % 2) != c["parity"]).expand(C, H, W).reshape(-1).to(D)
        assert torch.equal(out[:, unowned], fill[:, unowned])


def test_chained_calls_fill_one_buffer_and_one_offset_table():
    """chain = 0 then chain = 1, with the offset pointer moved on by the first call's B: the strings of both calls lie
    one after the other (device_encode2 checks offs[0] == 0 and that the table ascends) and equal the host twin's."""
    D = dev()
    t = device_tables(D)
    first, second = batch_of(_case("n4097_esc_row")), batch_of(_case("ckbd_anchor"))[:2]
    got = device_encode2([first, second], 3, D, t)
    assert got[0] == [host_encode2(b, 3) for b in first]
    assert got[1] == [host_encode2(b, 3) for b in second]


@pytest.fixture(scope="module")
def net():
    n, _ = build_model()
    n = n.to(dev()).eval()
    assert n.update(force=True)
    return n


SHAPES = [(2, 3, 64, 64), (1, 3, 64, 192)]
_cache = {}


def run(net, shape, coder, R=0, literal=False):
    """compress and decompress of the seeded input of ``shape`` under one setting; computed once and shared."""
    key = (shape, coder, R, literal)
    if key not in _cache:
        rm = net.residual_model
        x = _x(shape, 3).to(dev())
        rm.device_coder, rm.coder_segment_rows, rm.decode_in_compress = coder, R, literal
        try:
            with torch.no_grad():
                c = net.compress(x)
                d = net.decompress(c)
            torch.cuda.synchronize()
        finally:
            rm.device_coder, rm.coder_segment_rows, rm.decode_in_compress = False, 0, False
        _cache[key] = (c, d)
    return _cache[key]


def flat(s):
    return s[0][0] + s[0][1] + s[1]


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("R", [5, 8])
@pytest.mark.parametrize("literal", [False, True])
def test_model_round_trip_equals_host_coder(net, shape, R, literal):
    """decompress(compress(x)) with HRW2 is torch.equal to the host coder's, under both settings of decode_in_compress
    (which write the same strings); every string is HRW2 with the R asked for and the segment count its symbols give
    (at 64 x 64 the latent is 192 x 8 x 8, so a y pass is 96 rows: 20 segments for R = 5, the last of one row, and 12
    for R = 8; z is 128 x 2 x 2, 8 rows: 2 ragged segments for R = 5, one for R = 8)."""
    ch, dh = run(net, shape, False)
    cd, dd = run(net, shape, True, R, literal)
    assert torch.equal(dd["x_hat"], dh["x_hat"])
    assert cd["shape"] == ch["shape"]
    strings = flat(cd["strings"])
    assert len(strings) == 3 * shape[0]
    assert all(isinstance(s, bytes) and s[:4] == b"HRW2" for s in strings)
    for s in strings:
        n, r, S = struct.unpack_from("<3I", s, 4)
        assert r == R and S == max(1, -(-n // (64 * R)))
    if shape == (2, 3, 64, 64):
        (a, na), z = cd["strings"]
        assert [struct.unpack_from("<3I", s, 4)[::2] for s in (a[0], na[1], z[0])] == \
            [(6144, -(-96 // R)), (6144, -(-96 // R)), (512, -(-8 // R))]
    assert cd["strings"] == run(net, shape, True, R, not literal)[0]["strings"]
    print("bytes host", sum(map(len, flat(ch["strings"]))), "HRW2", sum(map(len, strings)))


@pytest.mark.parametrize("shape", SHAPES)
def test_hrw1_strings_still_decode_with_segment_rows_set(net, shape):
    """The format comes from each string's magic: HRW1 strings (written with the switch unset) give the same x_hat
    when ``coder_segment_rows`` is set at decompress."""
    rm = net.residual_model
    c1, _ = run(net, shape, True, 0)
    assert all(s[:4] == b"HRW1" for s in flat(c1["strings"]))
    rm.device_coder, rm.coder_segment_rows = True, 5
    try:
        with torch.no_grad():
            d = net.decompress(c1)
        torch.cuda.synchronize()
    finally:
        rm.device_coder, rm.coder_segment_rows = False, 0
    assert torch.equal(d["x_hat"], run(net, shape, False)[1]["x_hat"])


def test_host_format_strings_are_refused_before_any_launch(net):
    rm = net.residual_model
    host, _ = run(net, SHAPES[0], False)
    rm.device_coder, rm.coder_segment_rows = True, 5
    try:
        with pytest.raises(ValueError, match="magic"):
            net.decompress(host)
    finally:
        rm.device_coder, rm.coder_segment_rows = False, 0


def test_decompress_queues_without_a_host_wait(net):
    """residual_model.decompress of HRW2 strings under torch's sync debug mode "error": one pinned upload, the decode
    launches between the conv launches, no device-to-host copy and no wait up to the caller's own read of x_hat. (One
    call before it fills the weight, table and workspace caches.)"""
    rm = net.residual_model
    c, _ = run(net, SHAPES[0], True, 5)
    rm.device_coder, rm.coder_segment_rows = True, 5
    try:
        with torch.no_grad():
            want = rm.decompress(c["strings"], c["shape"])["x_hat"].cpu()
            torch.cuda.synchronize()
            torch.cuda.set_sync_debug_mode("error")
            try:
                out = rm.decompress(c["strings"], c["shape"])
            finally:
                torch.cuda.set_sync_debug_mode("default")
        assert torch.equal(out["x_hat"].cpu(), want)  # the caller's read
    finally:
        rm.device_coder, rm.coder_segment_rows = False, 0
