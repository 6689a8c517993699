"""CPU: the weight-gradient launcher's routing as its host-only queries report it (hyres_wgrad_kernel_name,
hyres_wgrad_plan, hyres_wgrad_workspace_bytes) against tests/golden/wgrad_routing.json, recorded by
tests/golden/make_wgrad_routing.py (the file's layout is described there) over 1x1 / 3x3 / 5x5 / deconv descriptors,
GDN gamma gradients, every dtype mode and each hyres_conv_tuning key the routing reads. The GPU tests name the kernel
a case is meant to reach through these queries, and the split plan fixes the summation order, so the built library
must reproduce the file exactly."""
import ctypes
import itertools
import json
import os

from conftest import REPO


def _expand(sec):
    if "geoms" in sec:
        return sec["geoms"]
    x = sec["ld_extra"]
    return [[B, S, S, ci, ci + x, co, co, K, K, stride, (K // 2) * dil, dil]
            for ci, co, (K, stride, dil), S, B in itertools.product(sec["cin"], sec["cout"], sec["conv"], sec["hw"],
                                                                   sec["batch"])]


def _query(lib, d):
    buf = ctypes.create_string_buffer(96)
    assert lib.hyres_wgrad_kernel_name(ctypes.byref(d), buf, len(buf)) == 0
    v = [ctypes.c_int(-9) for _ in range(4)]
    assert lib.hyres_wgrad_plan(ctypes.byref(d), *[ctypes.byref(x) for x in v]) == 0
    return [buf.value.decode()] + [x.value for x in v], lib.hyres_wgrad_workspace_bytes(ctypes.byref(d))


def test_wgrad_routing_reproduces_the_recorded_grid():
    from hyres_hip import _lib as L
    lib = L.load()
    with open(os.path.join(REPO, "tests", "golden", "wgrad_routing.json")) as f:
        fx = json.load(f)
    base = {int(k): v for k, v in fx["base"].items()}
    saved = {}
    for k, v in base.items():  # the recorded defaults, whatever the environment tuned at load
        old = ctypes.c_int(0)
        assert lib.hyres_conv_tuning(k, v, ctypes.byref(old)) == 0
        saved[k] = old.value
    wrong, cases, seen = [], 0, set()
    try:
        for sec in fx["sections"]:
            tune = fx["tunings"][sec["tuning"]]
            if tune:
                assert lib.hyres_conv_tuning(tune[0], tune[1], None) == 0
            try:
                want = iter(sec["cases"])
                for args in _expand(sec):
                    for di in sec["dtypes"]:
                        d = L.WgradDesc()
                        assert getattr(lib, sec["fn"])(ctypes.byref(d), *args) == 0, args
                        d.square_q = sec["square_q"]
                        d.f16_operands, d.io_f16 = fx["dtypes"][di]
                        res, ws = next(want), next(want)
                        name, *plan = fx["results"][res]
                        got = _query(lib, d)
                        cases += 1
                        seen.add(got[0][0].split("<")[0])
                        if got != ([fx["names"][name]] + plan, ws):
                            wrong.append((args, sec["square_q"], fx["dtypes"][di], tune, got, fx["names"][name], plan, ws))
                assert next(want, None) is None
            finally:
                if tune:
                    assert lib.hyres_conv_tuning(tune[0], base[tune[0]], None) == 0
    finally:
        for k, v in saved.items():
            assert lib.hyres_conv_tuning(k, v, None) == 0
    assert cases > 5000 and len(seen) == 10, (cases, sorted(seen))
    assert not wrong, (len(wrong), wrong[:5])
