"""CPU: the device coder's string format HRW1. The pure-host twins of the kernels (hyres_wrans_encode_host /
_decode_host, built from csrc/wrans_core.h) against the Python restatement tests/wrans_ref.py, the string-size bound,
hyres_wrans_validate, and the model's ``device_coder`` switch. No GPU call is made."""
import ctypes
import functools

import numpy as np
import pytest

import wrans_ref

ESC_HI, ESC_LO = 5000, -777


@functools.lru_cache(maxsize=None)
def tables():
    """The 64-level Gaussian tables of test_rans_roundtrip_and_bitstream_matches_restatement, as int32 arrays."""
    from oracle.entropy_coding import gc_tables
    scales = np.exp(np.linspace(np.log(0.11), np.log(256), 64))
    cdf, lengths, offsets = gc_tables(scales.astype(np.float32))
    return (np.ascontiguousarray(cdf, np.int32), np.ascontiguousarray(lengths, np.int32),
            np.ascontiguousarray(offsets, np.int32), scales)


def make_case(name, C, H, W, parity, seed, esc=(), esc_rows=(), edge=()):
    """A latent [C, H, W] as the symbol kernels leave it: ``idx`` random CDF rows, ``sym`` Gaussian at the row's
    scale on the positions the parity owns and round(0 - mean) elsewhere. ``esc``: coded-symbol numbers that get an
    out-of-range value (5000 / -777 alternating); ``esc_rows``: rows of 64 coded symbols made wholly of them; ``edge``:
    coded symbols set to offset + max_value, the first value past the CDF's range."""
    cdf, lengths, offsets, scales = tables()
    rng = np.random.default_rng(seed)
    chw = C * H * W
    idx = rng.integers(0, 64, chw).astype(np.int32)
    means = rng.normal(0, 3, (H * W, 2 * C)).astype(np.float32)  # NHWC params [scales(C) | means(C)] of one image
    own = np.array(wrans_ref.owned(C, H, W, parity), dtype=np.int64)
    mean_chw = means[:, C:].T.reshape(chw)
    sym = np.rint(np.float32(0) - mean_chw).astype(np.int32)
    sym[own] = np.round(rng.normal(0, 1, len(own)) * scales[idx[own]]).astype(np.int32)
    ks = sorted(set(esc) | {k for r in esc_rows for k in range(64 * r, 64 * r + 64)})
    for j, k in enumerate(ks):
        idx[own[k]] = k % 32  # a scale below 6: -777 is outside its CDF too (the widest CDFs reach past it)
        sym[own[k]] = ESC_HI if j % 2 == 0 else ESC_LO
    for k in edge:
        sym[own[k]] = offsets[idx[own[k]]] + lengths[idx[own[k]]] - 2
    return {"name": name, "C": C, "H": H, "W": W, "parity": parity, "sym": sym, "idx": idx, "means": means,
            "own": own, "n_esc_min": len(ks) + len(edge)}


@functools.lru_cache(maxsize=None)
def cases():
    out = [make_case("n1", 1, 1, 1, -1, 1),
           make_case("n63", 1, 1, 63, -1, 2, esc=(0, 62)),
           make_case("n64_esc_lane63_last_row", 1, 1, 64, -1, 3, esc=(0, 63)),
           make_case("n65_edge", 1, 1, 65, -1, 4, esc=(64,), edge=(10,)),
           make_case("n4097_esc_row", 1, 1, 4097, -1, 5, esc=(4095, 4096, 100, 1000), esc_rows=(3,)),
           make_case("n128_esc_lane63_last_row", 2, 1, 64, -1, 9, esc=(127, 64)),
           make_case("ckbd_all", 3, 5, 7, -1, 6, esc=(7,)),
           make_case("ckbd_anchor", 3, 5, 7, 0, 7, esc=(3, 53)),
           make_case("ckbd_non_anchor", 3, 5, 7, 1, 8, esc=(0, 50)),
           make_case("n0_no_owned_position", 2, 1, 1, 1, 10)]
    return tuple(out)


def table_args():
    cdf, lengths, offsets, _ = tables()
    return cdf.ctypes.data, cdf.shape[1], lengths.ctypes.data, offsets.ctypes.data, cdf.shape[0]


def host_encode(c):
    from hyres_hip import _lib as L
    lib = L.load()
    ln = ctypes.c_longlong(0)
    args = (c["sym"].ctypes.data, c["idx"].ctypes.data, c["C"], c["H"], c["W"], c["parity"], *table_args())
    L.check(lib.hyres_wrans_encode_host(*args, None, 0, ctypes.byref(ln)), "size query")
    buf = np.zeros(ln.value, np.uint8)
    L.check(lib.hyres_wrans_encode_host(*args, buf.ctypes.data, buf.size, ctypes.byref(ln)), "encode_host")
    assert ln.value == buf.size
    return buf.tobytes()


def host_decode(c, data):
    from hyres_hip import _lib as L
    out = np.full(c["sym"].size, -12345, np.int32)
    L.check(L.load().hyres_wrans_decode_host(data, len(data), c["idx"].ctypes.data, c["C"], c["H"], c["W"],
                                             c["parity"], *table_args(), c["means"].ctypes.data, 2 * c["C"], c["C"],
                                             out.ctypes.data), "decode_host")
    return out


def coded(c):
    return c["sym"][c["own"]].tolist(), c["idx"][c["own"]].tolist()


def ref_tables():
    cdf, lengths, offsets, _ = tables()
    return cdf, lengths.tolist(), offsets.tolist()


def _case(name):
    return next(c for c in cases() if c["name"] == name)


NAMES = ["n1", "n63", "n64_esc_lane63_last_row", "n65_edge", "n4097_esc_row", "n128_esc_lane63_last_row", "ckbd_all",
         "ckbd_anchor", "ckbd_non_anchor", "n0_no_owned_position"]


def test_case_list_covers_the_sizes_and_the_checkerboard():
    assert [c["name"] for c in cases()] == NAMES
    ns = {len(c["own"]) for c in cases()}
    assert {0, 1, 63, 64, 65, 4097} <= ns
    assert [len(_case(n)["own"]) for n in ("ckbd_all", "ckbd_anchor", "ckbd_non_anchor")] == [105, 54, 51]  # odd W
    from hyres_hip import _lib as L
    for c in cases():
        assert L.load().hyres_wrans_count(c["C"], c["H"], c["W"], c["parity"]) == len(c["own"])


@pytest.mark.parametrize("name", NAMES)
def test_host_twin_equals_restatement_and_round_trips(name):
    c = _case(name)
    sym, idx = coded(c)
    data = host_encode(c)
    ref = wrans_ref.encode(sym, idx, *ref_tables())
    assert data == ref
    assert data[:4] == b"HRW1"
    n, states, esc, words = wrans_ref.parse(data)
    assert n == len(sym) and len(esc) >= c["n_esc_min"]
    assert states[n:] == [1 << 31] * max(64 - n, 0)  # a lane that coded nothing
    assert wrans_ref.decode(data, idx, *ref_tables()) == sym
    assert np.array_equal(host_decode(c, data), c["sym"])  # owned from the stream, the rest round(0 - mean)
    from hyres_hip import _lib as L
    assert L.load().hyres_wrans_validate(data, len(data), c["C"], c["H"], c["W"], c["parity"]) == 0


def test_escapes_are_raw_values_in_coded_order_and_max_value_escapes():
    c = _case("n65_edge")
    sym, idx = coded(c)
    _, lengths, offsets = ref_tables()
    edge = offsets[idx[10]] + lengths[idx[10]] - 2
    assert sym[10] == edge  # v == max_value: the first value that has no slot of its own
    _, _, esc, _ = wrans_ref.parse(host_encode(c))
    in_range = [0 <= s - offsets[i] < lengths[i] - 2 for s, i in zip(sym, idx)]
    assert esc == [s for s, ok in zip(sym, in_range) if not ok]
    assert edge in esc and ESC_HI in esc
    c = _case("n4097_esc_row")
    sym, idx = coded(c)
    _, _, esc, _ = wrans_ref.parse(host_encode(c))
    row3 = sym[192:256]
    assert set(row3) == {ESC_HI, ESC_LO} and sym[4095] in (ESC_HI, ESC_LO) and sym[4096] in (ESC_HI, ESC_LO)
    assert len(esc) >= 68


@pytest.mark.parametrize("name", NAMES)
def test_string_size_is_within_the_rans64_bound(name):
    """8 * (states + payload bytes) <= ideal_bits + 64 * 64 + n * 4.5e-5: one 64-bit flush per lane, and per step a
    relative loss <= 2^-15 (state >= 2^31, freq <= 2^16), i.e. log2(1 + 2^-15) < 4.5e-5 bits. The escape values are
    side information outside the bound. Checked on the restatement and on the library."""
    c = _case(name)
    sym, idx = coded(c)
    ideal = wrans_ref.ideal_bits(sym, idx, *ref_tables())
    bound = ideal + 64 * 64 + len(sym) * 4.5e-5
    for data in (wrans_ref.encode(sym, idx, *ref_tables()), host_encode(c)):
        _, states, _, words = wrans_ref.parse(data)
        bits = 8 * (8 * len(states) + 4 * len(words))
        print(name, "bits", bits, "ideal", ideal, "bound", bound)
        assert bits <= bound


def test_validate_rejects_damaged_and_foreign_strings():
    from hyres_hip import _lib as L
    lib = L.load()
    c = _case("n4097_esc_row")
    good = host_encode(c)
    shape = (c["C"], c["H"], c["W"], c["parity"])

    def rc(data, shp=shape):
        r = lib.hyres_wrans_validate(data, len(data), *shp)
        return r, lib.hyres_last_error_string().decode()

    assert rc(good)[0] == 0
    r, msg = rc(b"HRW2" + good[4:])
    assert r == 1003 and "magic" in msg
    # the host coder's string of the same symbols (compressai's format)
    cdf, lengths, offsets, _ = tables()
    ln = ctypes.c_longlong(0)
    buf = np.zeros(8 * c["sym"].size + 64, np.uint8)
    L.check(lib.hyres_rans_encode_with_indexes(c["sym"].ctypes.data, c["idx"].ctypes.data, c["sym"].size,
                                               cdf.ctypes.data, cdf.shape[1], lengths.ctypes.data,
                                               offsets.ctypes.data, 64, buf.ctypes.data, buf.size, ctypes.byref(ln)),
            "host coder")
    host_format = buf[:ln.value].tobytes()
    assert len(host_format) > 528
    r, msg = rc(host_format)
    assert r == 1003 and "magic" in msg
    assert rc(host_format[:64])[0] == 1003  # a short one
    r, msg = rc(good[:-4])
    assert r == 1003 and "byte count" in msg
    r, msg = rc(good, (1, 1, 4096, -1))
    assert r == 1003 and "symbol count" in msg
    assert rc(good, (1, 1, 4097, 0))[0] == 1003  # the same latent under a checkerboard parity
    # the host decoder refuses them too, before it reads a symbol
    out = np.zeros(c["sym"].size, np.int32)
    assert lib.hyres_wrans_decode_host(host_format, len(host_format), c["idx"].ctypes.data, *shape, *table_args(), None,
                                       0, 0, out.ctypes.data) == 1003
    # bad arguments are refused before any launch (no GPU here: a launch would fail differently)
    assert lib.hyres_wrans_workspace_bytes(0, 1, 1, 1, -1) == -1 and lib.hyres_wrans_count(1, 1, 1, 2) == -1
    assert lib.hyres_wrans_encode(None, None, 1, 1, 1, 1, -1, *table_args(), None, 0, None, 0, None, 0, None) == 1003
    assert lib.hyres_wrans_decode(None, None, None, 1, 1, 1, 1, 0, *table_args(), None, 0, 0, None, None) == 1003


def test_environment_switch_and_argument_wins(monkeypatch):
    from models import LightWeightCheckerboard
    from hyres_hip import entropy_coding as EC
    monkeypatch.delenv("HYRES_ENTROPY_CODER", raising=False)
    assert EC.coder_from_env() is False
    assert LightWeightCheckerboard(N=8, M=8).device_coder is False
    monkeypatch.setenv("HYRES_ENTROPY_CODER", "device")
    assert LightWeightCheckerboard(N=8, M=8).device_coder is True
    assert LightWeightCheckerboard(N=8, M=8, device_coder=False).device_coder is False
    monkeypatch.setenv("HYRES_ENTROPY_CODER", "host")
    assert LightWeightCheckerboard(N=8, M=8).device_coder is False
    assert LightWeightCheckerboard(N=8, M=8, device_coder=True).device_coder is True
    monkeypatch.setenv("HYRES_ENTROPY_CODER", "gpu")
    with pytest.raises(ValueError, match="HYRES_ENTROPY_CODER"):
        LightWeightCheckerboard(N=8, M=8)
    assert LightWeightCheckerboard(N=8, M=8, device_coder=True).device_coder is True  # the argument is not looked up


def test_cpu_model_keeps_the_host_coder(monkeypatch):
    """A model on the CPU with device_coder=True routes compress / decompress to the host coder's path, never to the
    device coder's (as the JPEG switch does for CPU tensors). The host path's own symbol kernels need the GPU, so on a
    CPU model it ends in the library's "no CPU fallback" error, exactly as it does with device_coder=False; the strings
    of the host coder it would call are compressai's format (no HRW1 magic)."""
    import torch
    from models import LightWeightCheckerboard
    from hyres_hip import entropy_coding as EC
    net = LightWeightCheckerboard(N=8, M=8, device_coder=True).eval()
    assert not net.on_device_coder(next(net.parameters()).device)
    assert net.on_device_coder(torch.device("cuda", 0))

    def boom(*a, **k):
        raise AssertionError("the device coder was entered on a CPU model")
    monkeypatch.setattr(net, "_compress_device", boom)
    monkeypatch.setattr(net, "_decompress_device", boom)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        net.compress(torch.zeros(1, 3, 32, 32))
    gc = net.gaussian_conditional
    net.update(force=True)
    c = _case("ckbd_all")
    s = EC._encode(gc, c["sym"], c["idx"])  # what the host path calls per image
    assert s[:4] != EC.WRANS_MAGIC and len(s) % 4 == 0
    assert np.array_equal(EC._decode(gc, s, c["idx"]), c["sym"])
