"""CPU: the segmented device-coder format HRW2. The pure-host twins of the kernels (hyres_wrans2_encode_host /
_decode_host) against the Python restatement tests/wrans2_ref.py, the per-segment equality with HRW1 that defines the
format, the string-size bound, hyres_wrans2_validate, and the model's ``coder_segment_rows`` switch. No GPU call is
made."""
import ctypes
import functools
import struct

import numpy as np
import pytest

import wrans2_ref
import wrans_ref
from test_wrans_cpu import NAMES, _case, coded, ref_tables, table_args, tables
from test_wrans_cpu import host_encode as host_encode1

ROWS = [1, 2, 3, 64, 1 << 21]
CASES = [(name, R) for name in NAMES for R in ROWS]


def host_encode2(c, R):
    from hyres_hip import _lib as L
    lib = L.load()
    ln = ctypes.c_longlong(0)
    args = (c["sym"].ctypes.data, c["idx"].ctypes.data, c["C"], c["H"], c["W"], c["parity"], *table_args(), R)
    L.check(lib.hyres_wrans2_encode_host(*args, None, 0, ctypes.byref(ln)), "size query")
    buf = np.zeros(ln.value, np.uint8)
    L.check(lib.hyres_wrans2_encode_host(*args, buf.ctypes.data, buf.size, ctypes.byref(ln)), "encode_host")
    assert ln.value == buf.size
    return buf.tobytes()


def host_decode2(c, data):
    from hyres_hip import _lib as L
    out = np.full(c["sym"].size, -12345, np.int32)
    L.check(L.load().hyres_wrans2_decode_host(data, len(data), c["idx"].ctypes.data, c["C"], c["H"], c["W"],
                                              c["parity"], *table_args(), c["means"].ctypes.data, 2 * c["C"], c["C"],
                                              out.ctypes.data), "decode_host")
    return out


@functools.lru_cache(maxsize=None)
def ref_encode2(name, R):
    """The restatement's string of a case: computed once, shared by the tests."""
    sym, idx = coded(_case(name))
    return wrans2_ref.encode(sym, idx, *ref_tables(), R)


def validate2(data, shape):
    """(return code, message, R) of hyres_wrans2_validate."""
    from hyres_hip import _lib as L
    lib = L.load()
    rows = ctypes.c_int(-1)
    r = lib.hyres_wrans2_validate(data, len(data), *shape, ctypes.byref(rows))
    return r, lib.hyres_last_error_string().decode(), rows.value


def shape_of(c):
    return c["C"], c["H"], c["W"], c["parity"]


def test_segment_counts_of_the_cases():
    from hyres_hip import _lib as L
    lib = L.load()
    for name, R in CASES:
        c = _case(name)
        n = len(c["own"])
        S = lib.hyres_wrans2_segments(*shape_of(c), R)
        assert S == wrans2_ref.segments(n, R) == max(1, -(-n // (64 * R)))
        assert lib.hyres_wrans2_max_string_bytes(*shape_of(c), R) == 16 + 520 * S + 8 * n
    assert wrans2_ref.segments(65, 1) == 2 and len(wrans2_ref.seg_range(65, 1, 1)) == 1  # a last segment of 1 symbol
    assert wrans2_ref.segments(4097, 1) == 65
    assert wrans2_ref.segments(0, 1) == 1  # n0_no_owned_position
    c = _case("n4097_esc_row")
    _, _, _, directory, segs = wrans2_ref.parse2(ref_encode2("n4097_esc_row", 1))
    assert len(segs[3][1]) == 64 and directory[3][0] - directory[2][0] == 64  # row 3: a segment made of escapes
    assert lib.hyres_wrans2_segments(*shape_of(c), 0) == -1 and lib.hyres_wrans2_segments(1, 1, 1, 2, 1) == -1
    assert lib.hyres_wrans2_max_string_bytes(*shape_of(c), 0) == -1


@pytest.mark.parametrize("name,R", CASES)
def test_host_twin_equals_restatement_and_round_trips(name, R):
    c = _case(name)
    sym, idx = coded(c)
    data = host_encode2(c, R)
    assert data == ref_encode2(name, R)
    assert data[:4] == b"HRW2"
    n, r, S, directory, segs = wrans2_ref.parse2(data)
    assert (n, r, S) == (len(sym), R, wrans2_ref.segments(len(sym), R))
    assert len(data) == 16 + 8 * S + 512 * S + 4 * (directory[-1][0] + directory[-1][1])
    assert len(data) <= 16 + 520 * S + 8 * n
    assert directory[-1][0] >= c["n_esc_min"]
    assert wrans2_ref.decode(data, idx, *ref_tables()) == sym
    assert np.array_equal(host_decode2(c, data), c["sym"])  # owned from the stream, the rest round(0 - mean)
    assert validate2(data, shape_of(c))[::2] == (0, R)


@pytest.mark.parametrize("name,R", CASES)
def test_every_segment_equals_the_hrw1_string_of_its_symbols(name, R):
    """The defining property: states, escapes and payload of segment s are those of the HRW1 string of the segment's
    symbols alone; with one segment the body after the header and directory is the HRW1 host twin's body."""
    c = _case(name)
    sym, idx = coded(c)
    data = host_encode2(c, R)
    n, _, S, _, segs = wrans2_ref.parse2(data)
    for s in range(S):
        k = wrans2_ref.seg_range(n, R, s)
        alone = wrans_ref.encode(sym[k.start:k.stop], idx[k.start:k.stop], *ref_tables())
        n_s, states, esc, words = wrans_ref.parse(alone)
        assert n_s == len(k) and (states, esc, words) == segs[s], s
        assert states[n_s:] == [1 << 31] * max(64 - n_s, 0)  # a lane that coded nothing in its segment
        assert wrans2_ref.hrw1_of_segment(n_s, segs[s]) == alone
    if S == 1:
        assert data[16 + 8:] == host_encode1(c)[16:]


@pytest.mark.parametrize("name,R", CASES)
def test_string_size_is_within_the_rans64_bound_per_segment(name, R):
    """8 * (512 S + 4 words) <= ideal_bits + S * 64 * 64 + n * 4.5e-5: HRW1's bound (tests/test_wrans_cpu.py) once per
    segment, since every segment flushes its own 64 states. Header, directory and escapes are side information.
    Checked on the restatement and on the library."""
    c = _case(name)
    sym, idx = coded(c)
    ideal = wrans_ref.ideal_bits(sym, idx, *ref_tables())
    for data in (ref_encode2(name, R), host_encode2(c, R)):
        n, _, S, directory, _ = wrans2_ref.parse2(data)
        bound = ideal + S * 64 * 64 + n * 4.5e-5
        bits = 8 * (512 * S + 4 * directory[-1][1])
        print(name, R, "S", S, "bits", bits, "ideal", ideal, "bound", bound)
        assert bits <= bound


def patched(data, word, value):
    return data[:4 * word] + struct.pack("<I", value) + data[4 * word + 4:]


def test_validate_rejects_damaged_and_foreign_strings():
    from hyres_hip import _lib as L
    lib = L.load()
    c = _case("n4097_esc_row")
    shape = shape_of(c)
    good = host_encode2(c, 3)
    n, R, S, directory, _ = wrans2_ref.parse2(good)
    assert (n, R, S) == (4097, 3, 22)
    assert validate2(good, shape)[::2] == (0, 3)

    def refused(data, word, shp=shape):
        r, msg, _ = validate2(data, shp)
        assert r == 1003 and word in msg, (r, msg)

    refused(host_encode1(c), "magic")  # an HRW1 string
    cdf, lengths, offsets, _ = tables()
    ln = ctypes.c_longlong(0)
    buf = np.zeros(8 * c["sym"].size + 64, np.uint8)
    L.check(lib.hyres_rans_encode_with_indexes(c["sym"].ctypes.data, c["idx"].ctypes.data, c["sym"].size,
                                               cdf.ctypes.data, cdf.shape[1], lengths.ctypes.data,
                                               offsets.ctypes.data, 64, buf.ctypes.data, buf.size, ctypes.byref(ln)),
            "host coder")
    host_format = buf[:ln.value].tobytes()
    refused(host_format, "magic")  # the host coder's string of the same symbols (compressai's format)
    refused(host_format[:2], "magic")
    refused(patched(good, 2, 0), "segment")          # R = 0
    refused(patched(good, 2, 4), "segment")          # another R: S no longer follows from n and R
    refused(patched(good, 3, S + 1), "segment")      # S patched
    refused(patched(good, 3, 0), "segment")
    # a directory entry past its segment's size: segment 3 holds 192 symbols
    refused(patched(good, 4 + 2 * 3, directory[2][0] + 193), "segment")
    refused(patched(good, 4 + 2 * 3 + 1, directory[2][1] + 193), "segment")
    refused(patched(good, 4 + 2 * 5, directory[4][0] - 1), "segment")  # a directory that decreases
    refused(good[:-4], "byte count")
    refused(good[:16 + 8 * S], "byte count")
    refused(good + b"\0\0\0\0", "byte count")
    refused(good, "symbol count", (1, 1, 4096, -1))
    refused(good, "symbol count", (1, 1, 4097, 0))  # the same latent under a checkerboard parity
    # the order of the checks: magic, symbol count, segments, directory, byte count
    refused(patched(good, 2, 0), "symbol count", (1, 1, 4096, -1))
    refused(patched(good, 2, 0)[:-4], "segment")
    refused(patched(good, 4 + 2 * 3, directory[2][0] + 193)[:-4], "segment")
    # the HRW1 entry point keeps refusing an HRW2 string
    assert lib.hyres_wrans_validate(good, len(good), *shape) == 1003
    assert "magic" in lib.hyres_last_error_string().decode()
    # the host decoder refuses a damaged string before it reads a symbol
    out = np.zeros(c["sym"].size, np.int32)
    bad = patched(good, 4 + 2 * 3, directory[2][0] + 193)
    assert lib.hyres_wrans2_decode_host(bad, len(bad), c["idx"].ctypes.data, *shape, *table_args(), None, 0, 0,
                                        out.ctypes.data) == 1003


def test_bad_arguments_are_refused_before_any_launch():
    """No GPU here: a launch would fail differently."""
    from hyres_hip import _lib as L
    lib = L.load()
    one = np.zeros(64, np.int64)
    p = one.ctypes.data  # a non-NULL host address: a refused call never dereferences it
    assert lib.hyres_wrans2_workspace_bytes(0, 1, 1, 1, -1, 1) == -1
    assert lib.hyres_wrans2_workspace_bytes(1, 1, 1, 1, -1, 0) == -1
    assert lib.hyres_wrans2_workspace_bytes(1, 1, 1, 64, -1, 1) == 16 + 16 + 4 * (128 + 2 * 64)
    assert lib.hyres_wrans2_encode(None, None, 1, 1, 1, 1, -1, *table_args(), 1, None, 0, None, 0, None, 0,
                                   None) == 1003  # NULLs
    assert lib.hyres_wrans2_encode(p, None, 1, 1, 1, 1, -1, *table_args(), 0, p, 0, p, 0, p, 1 << 20, None) == 1003
    assert "seg_rows" in lib.hyres_last_error_string().decode()
    a = (p + 15) & ~15
    r = lib.hyres_wrans2_encode(a, None, 1, 1, 1, 64, -1, *table_args(), 1, a, 0, a, 0, a, 8, None)
    assert r != 0 and "workspace" in lib.hyres_last_error_string().decode()
    assert lib.hyres_wrans2_decode(None, None, None, 1, 1, 1, 1, 0, 1, *table_args(), None, 0, 0, None, None) == 1003
    assert lib.hyres_wrans2_decode(p, p, None, 1, 1, 1, 1, -1, 0, *table_args(), None, 0, 0, p, None) == 1003
    assert "seg_rows" in lib.hyres_last_error_string().decode()
    ln = ctypes.c_longlong(0)
    assert lib.hyres_wrans2_encode_host(p, None, 1, 1, 1, -1, *table_args(), -3, None, 0, ctypes.byref(ln)) == 1003


def test_environment_switch_and_argument_wins(monkeypatch):
    from models import LightWeightCheckerboard
    from hyres_hip import entropy_coding as EC
    monkeypatch.delenv("HYRES_WRANS_SEGMENT_ROWS", raising=False)
    monkeypatch.delenv("HYRES_ENTROPY_CODER", raising=False)
    assert EC.segment_rows() == 0  # HRW1, as before
    net = LightWeightCheckerboard(N=8, M=8)
    assert net.coder_segment_rows == 0 and net.device_coder is False
    monkeypatch.setenv("HYRES_WRANS_SEGMENT_ROWS", "0")
    assert LightWeightCheckerboard(N=8, M=8).coder_segment_rows == 0
    monkeypatch.setenv("HYRES_WRANS_SEGMENT_ROWS", "512")
    net = LightWeightCheckerboard(N=8, M=8, device_coder=True)
    assert net.coder_segment_rows == 512 and net.device_coder is True
    assert LightWeightCheckerboard(N=8, M=8, coder_segment_rows=7).coder_segment_rows == 7  # the argument wins
    assert LightWeightCheckerboard(N=8, M=8, coder_segment_rows=0).coder_segment_rows == 0
    for bad in ("x", "-1", "1.5"):
        monkeypatch.setenv("HYRES_WRANS_SEGMENT_ROWS", bad)
        with pytest.raises(ValueError, match="HYRES_WRANS_SEGMENT_ROWS"):
            LightWeightCheckerboard(N=8, M=8)
        assert LightWeightCheckerboard(N=8, M=8, coder_segment_rows=3).coder_segment_rows == 3  # not looked up
    for bad in (-1, "x", 1.5):
        with pytest.raises(ValueError, match="coder_segment_rows"):
            LightWeightCheckerboard(N=8, M=8, coder_segment_rows=bad)


def test_cpu_model_keeps_the_host_coder(monkeypatch):
    """A model on the CPU with device_coder=True and coder_segment_rows set still routes compress / decompress to the
    host coder's path (which ends in the library's "no CPU fallback" error, as with the switch unset)."""
    import torch
    from models import LightWeightCheckerboard
    net = LightWeightCheckerboard(N=8, M=8, device_coder=True, coder_segment_rows=5).eval()
    assert net.coder_segment_rows == 5
    assert not net.on_device_coder(next(net.parameters()).device)

    def boom(*a, **k):
        raise AssertionError("the device coder was entered on a CPU model")
    monkeypatch.setattr(net, "_compress_device", boom)
    monkeypatch.setattr(net, "_decompress_device", boom)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        net.compress(torch.zeros(1, 3, 32, 32))


def test_group_format_is_read_from_the_strings():
    """DeviceDecoder's host check: a group of HRW1 strings is format 0, of HRW2 strings its R; a group that mixes
    formats or R, and a string of neither format, are refused before anything is launched."""
    from hyres_hip import entropy_coding as EC
    c = _case("ckbd_anchor")
    shape = shape_of(c)
    h1, a3, a64 = host_encode1(c), host_encode2(c, 3), host_encode2(c, 64)
    assert EC.wrans_group_format([h1, h1], *shape) == 0
    assert EC.wrans_group_format([a3, a3], *shape) == 3
    assert EC.wrans_group_format([a64], *shape) == 64
    for mixed in ([h1, a3], [a3, a64]):
        with pytest.raises(ValueError, match="mix"):
            EC.wrans_group_format(mixed, *shape)
    with pytest.raises(ValueError, match="magic"):
        EC.wrans_group_format([b"\x01\x02\x03\x04" * 200], *shape)
    with pytest.raises(ValueError, match="byte count"):
        EC.wrans_group_format([a3[:-4]], *shape)
