"""CPU: the conv launcher's routing as its host-only queries report it (hyres_conv_kernel_name, hyres_conv_plan,
hyres_conv_workspace_bytes) against tests/golden/conv_routing.json, recorded by tests/golden/make_conv_routing.py
(the file's layout is described there) over 1x1 / 3x3 / 5x5 / deconv geometries and their input-gradients, the
epilogue cross under every dtype mode, and each hyres_conv_tuning key the routing reads. Python picks epilogue folds
from these names and bench.py prices kernels by them, so the built library must reproduce the file exactly."""
import ctypes
import json
import os

from conftest import REPO


def _query(lib, g, e):
    names = []
    for split in (0, 1):
        buf = ctypes.create_string_buffer(96)
        assert lib.hyres_conv_kernel_name(ctypes.byref(g), ctypes.byref(e), split, buf, len(buf)) == 0
        names.append(buf.value.decode())
    tile, ns = ctypes.c_int(-9), ctypes.c_int(-9)
    assert lib.hyres_conv_plan(ctypes.byref(g), ctypes.byref(e), ctypes.byref(tile), ctypes.byref(ns)) == 0
    return names[0], names[1], tile.value, ns.value


def test_conv_routing_reproduces_the_recorded_grid():
    from hyres_hip import _lib as L
    lib = L.load()
    with open(os.path.join(REPO, "tests", "golden", "conv_routing.json")) as f:
        fx = json.load(f)
    base = {int(k): v for k, v in fx["base"].items()}
    saved = {}
    for k, v in base.items():  # the recorded defaults, whatever the environment tuned at load
        old = ctypes.c_int(0)
        assert lib.hyres_conv_tuning(k, v, ctypes.byref(old)) == 0
        saved[k] = old.value
    wrong, cases, seen = [], 0, set()
    try:
        for gi, ti, ws, si, ri in fx["groups"]:
            spec = fx["geoms"][gi]
            g = L.ConvGeom()
            assert getattr(lib, fx["fns"][spec[0]])(ctypes.byref(g), *spec[1:]) == 0, spec
            tune = fx["tunings"][ti]
            if tune:
                assert lib.hyres_conv_tuning(tune[0], tune[1], None) == 0
            try:
                got_ws = lib.hyres_conv_workspace_bytes(ctypes.byref(g))
                if got_ws != ws:
                    wrong.append((spec, tune, "workspace", got_ws, ws))
                assert len(fx["episets"][si]) == len(fx["rows"][ri])
                for (ei, di), res in zip(fx["episets"][si], fx["rows"][ri]):
                    n0, n1, tile, ns = fx["results"][res]
                    e = L.Epilogue()
                    for k, v in fx["epis"][ei].items():
                        setattr(e, k, g.Co if v == "Co" else v)
                    e.f16_operands, e.io_f16 = fx["dtypes"][di]
                    got = _query(lib, g, e)
                    want = (fx["names"][n0], fx["names"][n1], tile, ns)
                    cases += 1
                    seen.add(got[0].split("<")[0])
                    if got != want:
                        wrong.append((spec, tune, fx["epis"][ei], fx["dtypes"][di], got, want))
            finally:
                if tune:
                    assert lib.hyres_conv_tuning(tune[0], base[tune[0]], None) == 0
    finally:
        for k, v in saved.items():
            assert lib.hyres_conv_tuning(k, v, None) == 0
    assert cases > 10000 and len(seen) >= 13, (cases, sorted(seen))
    assert not wrong, (len(wrong), wrong[:5])
