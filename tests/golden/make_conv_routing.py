"""Generator of conv_routing.json: what the conv launcher's host-only queries answer over a grid of geometries,
epilogues and tunings (hyres_conv_kernel_name for split = 0 / 1, hyres_conv_plan's (tile, nsplit),
hyres_conv_workspace_bytes). tests/test_conv_routing_cpu.py asserts that the built library reproduces the file, so
run this on the commit whose routing is the reference (the parent of a dispatch refactor), never to make a test pass:

    python tests/golden/make_conv_routing.py [--lib path/to/libhyres_hip.so]

File layout (every table is indexed by the ones below it, which keeps the file small):
    fns      [geometry function, ...]
    geoms    [[fn, its integer arguments...], ...]
    epis     [{hyres_epilogue field: value}, ...]   (without the dtype fields; pointer fields: a dummy non-zero integer
                                                     where the operand exists; the pitch "Co": the geometry's Co)
    dtypes   [[f16_operands, io_f16], ...]
    episets  [[[epi, dtype], ...], ...]             (the epilogues one group asks about, in order)
    tunings  [null | [key, value], ...]             (one hyres_conv_tuning key off its default at a time)
    base     {key: the value every touched key has while another tuning is recorded}
    names    [kernel name, ...]
    results  [[name split=0, name split=1, tile, nsplit], ...]
    rows     [[result, ...], ...]                   (the answers to one episet, in its order)
    groups   [[geom, tuning, workspace bytes, episet, row], ...]
"""
import argparse
import ctypes
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(REPO, "hyres-residual-enhanced-hybrid-image-compression_amd"))

PTR = 0x1000  # the host queries only test pointers for null
DTYPES = [(0, 0), (1, 0), (1, 3), (1, 1), (0, 2)]  # (f16_operands, io_f16)
THIN = [0, 2]  # ... and the two of them (by index) asked where the cross product is thinned
REQUIRED = ["conv_narrow_kernel", "conv_narrow_strip_kernel", "conv3x3_wres_bf6_kernel", "conv3x3_wres_f16_kernel",
            "conv3x3_halo_f16_kernel", "conv1x1_stream_b6_kernel", "conv1x1_stream_kernel", "conv1x1_stream_hf_kernel",
            "conv1x1_stream_h_kernel", "conv_fwd_kernel", "conv_fwd_b6_kernel", "conv_fwd_b6db_kernel",
            "conv_fwd_h_kernel"]


def geometries():
    """(all, representative): every geometry gets a few epilogues, the representative ones the full epilogue cross
    and, with fewer epilogues, every tuning."""
    conv, dgrad = "hyres_geom_conv2d", "hyres_geom_conv2d_dgrad"
    allg, rep = [], []

    def both(B, H, W, Ci, Co, K, stride, pad, dil):
        Ho = (H + 2 * pad - dil * (K - 1) - 1) // stride + 1
        Wo = (W + 2 * pad - dil * (K - 1) - 1) // stride + 1
        a = [conv, B, H, W, Ci, Ci, Co, Co, K, K, stride, pad, dil]
        # the input-gradient: hyres_geom_conv2d_dgrad takes the forward conv's shapes (dx is H x W x Ci)
        b = [dgrad, B, H, W, Ci, Ci, Co, Co, K, K, stride, pad, dil]
        assert Ho > 0 and Wo > 0
        allg.extend([a, b])
        return a, b

    ch = [64, 96, 128, 192]
    pairs = [(ci, co) for ci in ch for co in ch] + [(512, 384), (640, 512), (96, 192)]
    for ci, co in pairs:
        for B, S in [(16, 16), (16, 32), (16, 64), (16, 128), (16, 256), (5, 117)]:
            both(B, S, S, ci, co, 1, 1, 0, 1)
    for ci in [3, 64, 96, 128]:
        for co in [3, 4, 32, 64, 96, 128, 192]:
            for dil in [1, 2]:
                for W in [32, 48, 64, 128]:
                    both(16, W, W, ci, co, 3, 1, dil, dil)
    for co in [128, 192]:
        for S in [128, 64]:
            both(16, S, S, 128, co, 5, 2, 2, 1)
    for ci, co, S in [(128, 128, 32), (192, 128, 16), (128, 3, 64)]:
        for fn in ("hyres_geom_deconv2d", "hyres_geom_deconv2d_dgrad"):
            allg.append([fn, 16, S, S, ci, ci, co, co, 5, 2])
    for B, S, ci, co, K, stride, dil in [
            (16, 128, 64, 64, 1, 1, 1), (16, 128, 64, 128, 1, 1, 1), (16, 128, 128, 128, 1, 1, 1),
            (16, 32, 96, 192, 1, 1, 1), (16, 128, 192, 64, 1, 1, 1), (16, 128, 64, 192, 1, 1, 1),
            (16, 64, 64, 64, 3, 1, 1), (16, 128, 64, 128, 3, 1, 2), (16, 32, 96, 96, 3, 1, 1),
            (16, 64, 64, 3, 3, 1, 1), (16, 64, 3, 64, 3, 1, 1), (16, 128, 128, 128, 5, 2, 1)]:
        rep.append([conv, B, S, S, ci, ci, co, co, K, K, stride, (K // 2) * dil, dil])
    return allg, rep


def epilogues():
    """(few, medium, full) epilogue sets, before the dtype cross; the pitch "Co" stands for the geometry's Co."""
    Co = "Co"
    res = {"res": PTR, "ldres": Co}
    mask = {"act": 3, "aux0": PTR, "ld0": Co}
    bias = {"kind": 0, "bias": PTR}
    full = []
    for act in (0, 1, 2, 3):
        for r in (0, 1):
            for acc in (0, 1):
                for o2 in (0, 1):
                    for sq in (0, 1):
                        e = dict(bias, act=act, accumulate=acc, square_input=sq)
                        if act == 2:
                            e["slope"] = PTR
                        if act == 3:
                            e.update(mask)
                        if r:
                            e.update(res)
                        if o2:
                            e.update(out2=PTR, ldo2=Co)
                        full.append(e)
    prelu_mask = dict(bias, act=4, aux0=PTR, ld0=Co, aux1=PTR, ld1=1, aux2=PTR, ld2=2048, slope=PTR)
    rowscale = [dict(kind=5, act=a, bias=PTR, slope=PTR, aux1=PTR, ld1=1, out2=PTR, ldo2=Co) for a in (0, 1, 2)]
    sab = dict(kind=6, aux0=PTR, ld0=2, aux2=PTR)
    sa_bwd = [sab, dict(sab, accumulate=1),
              dict(sab, act=4, aux1=PTR, ld1=64, slope=PTR, res=PTR, ldres=1, out2=PTR, ldo2=2048)]
    full += [prelu_mask] + rowscale + sa_bwd
    few = [bias, dict(bias, **mask, **res), prelu_mask]
    medium = few + [dict(bias, act=1, **res), rowscale[2], sa_bwd[0], sa_bwd[2]]
    return few, medium, full


def tunings():
    t = [[0, v] for v in range(5)] + [[k, 0] for k in (7, 8, 9, 10, 11, 13, 14, 17, 18, 21)]
    return t + [[12, v] for v in (1, 2, 3)] + [[20, 1], [20, -1]]


class Recorder:
    def __init__(self, L):
        self.L, self.lib = L, L.load()
        self.tables = {k: [] for k in ("fns", "geoms", "epis", "episets", "names", "results", "rows")}
        self._index = {k: {} for k in self.tables}

    def _intern(self, table, item):
        key = json.dumps(item, sort_keys=True)
        index = self._index[table]
        if key not in index:
            index[key] = len(self.tables[table])
            self.tables[table].append(item)
        return index[key]

    def geom(self, spec):
        g = self.L.ConvGeom()
        rc = getattr(self.lib, spec[0])(ctypes.byref(g), *spec[1:])
        assert rc == 0, (spec, self.lib.hyres_last_error_string())
        return g

    def epi(self, fields, g):
        e = self.L.Epilogue()
        for k, v in fields.items():
            setattr(e, k, g.Co if v == "Co" else v)
        return e

    def group(self, gspec, especs):
        """especs: [(epilogue fields, index into DTYPES), ...]"""
        g = self.geom(gspec)
        episet, row = [], []
        for fields, d in especs:
            e = self.epi(dict(fields, f16_operands=DTYPES[d][0], io_f16=DTYPES[d][1]), g)
            names = []
            for split in (0, 1):
                buf = ctypes.create_string_buffer(96)
                assert self.lib.hyres_conv_kernel_name(ctypes.byref(g), ctypes.byref(e), split, buf, len(buf)) == 0
                names.append(self._intern("names", buf.value.decode()))
            tile, ns = ctypes.c_int(-9), ctypes.c_int(-9)
            assert self.lib.hyres_conv_plan(ctypes.byref(g), ctypes.byref(e), ctypes.byref(tile), ctypes.byref(ns)) == 0
            episet.append([self._intern("epis", fields), d])
            row.append(self._intern("results", [names[0], names[1], tile.value, ns.value]))
        ws = self.lib.hyres_conv_workspace_bytes(ctypes.byref(g))
        gi = self._intern("geoms", [self._intern("fns", gspec[0])] + gspec[1:])
        return [gi, 0, ws, self._intern("episets", episet), self._intern("rows", row)]


def with_dtypes(especs, dtypes=range(len(DTYPES))):
    return [(e, d) for e in especs for d in dtypes]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=None, help="library to record (default: the in-tree build)")
    ap.add_argument("--out", default=os.path.join(HERE, "conv_routing.json"))
    args = ap.parse_args()
    from hyres_hip import _lib as L
    if args.lib:
        L.load(args.lib)
    rec = Recorder(L)
    lib = rec.lib
    tun = tunings()
    keys = sorted({k for k, _ in tun})
    base = {}
    for k in keys:
        old = ctypes.c_int(0)
        assert lib.hyres_conv_tuning(k, 0, ctypes.byref(old)) == 0
        assert lib.hyres_conv_tuning(k, old.value, None) == 0
        base[k] = old.value
    allg, rep = geometries()
    groups = []
    for gspec in allg:
        few = epilogues()[0]
        three = gspec[0].startswith("hyres_geom_conv2d") and gspec[8] == 3
        groups.append(rec.group(gspec, with_dtypes(few[:1]) + with_dtypes(few[1:2], THIN) + ([(few[2], 0)] if three else [])))
    for gspec in rep:
        groups.append(rec.group(gspec, with_dtypes(epilogues()[2])))
    table = [None]
    for ti, (k, v) in enumerate(tun, start=1):
        table.append([k, v])
        assert lib.hyres_conv_tuning(k, v, None) == 0
        try:
            for gspec in rep:
                grp = rec.group(gspec, with_dtypes(epilogues()[1], THIN))
                grp[1] = ti
                groups.append(grp)
        finally:
            assert lib.hyres_conv_tuning(k, base[k], None) == 0
    names = rec.tables["names"]
    missing = [r for r in REQUIRED if not any(n == r or n.startswith(r + "<") for n in names)]
    if missing:
        sys.exit(f"not written: no recorded case runs {missing}")
    out = dict(rec.tables, dtypes=DTYPES, tunings=table, base={str(k): v for k, v in base.items()}, groups=groups)
    with open(args.out, "w") as f:
        json.dump(out, f, separators=(",", ":"))
        f.write("\n")
    n = sum(len(rec.tables["rows"][g[4]]) for g in groups)
    print(f"{args.out}: {len(groups)} groups, {n} cases, {len(names)} kernel names, {os.path.getsize(args.out)} bytes")


if __name__ == "__main__":
    main()
