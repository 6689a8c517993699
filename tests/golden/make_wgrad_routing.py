"""Generator of wgrad_routing.json: what the weight-gradient launcher's host-only queries answer over a grid of
descriptors, dtype modes and tunings (hyres_wgrad_kernel_name, hyres_wgrad_plan's (nsplit, blocks, threads, lanes),
hyres_wgrad_workspace_bytes). tests/test_wgrad_routing_cpu.py asserts that the built library reproduces the file, so
run this on the commit whose routing is the reference (the parent of a dispatch refactor), never to make a test pass:

    python tests/golden/make_wgrad_routing.py [--lib path/to/libhyres_hip.so]

File layout (the descriptors are not listed: a section names the axes it crosses, expand() below enumerates them):
    dtypes    [[f16_operands, io_f16], ...]
    tunings   [null | [key, value], ...]            (one hyres_conv_tuning key off its default at a time)
    base      {key: the value every touched key has while another tuning is recorded}
    names     [kernel name, ...]
    results   [[name, nsplit, blocks, threads, lanes], ...]
    sections  [{"fn": descriptor function, "tuning": index, "square_q": 0 | 1, "dtypes": [index, ...],
                either "geoms": [[the function's integer arguments...], ...]
                or     "cin", "cout", "conv" ([[K, stride, dilation], ...]), "hw", "batch", "ld_extra": the cross, in
                       this nesting order, of hyres_wgrad_desc_conv2d(B, HW, HW, Ci, Ci + ld_extra, Co, Co, K, K,
                       stride, (K // 2) * dilation, dilation),
                "cases": [result, workspace bytes, result, workspace bytes, ...]}, ...]
                                                    (one pair per descriptor and dtype, the dtypes innermost)
"""
import argparse
import ctypes
import itertools
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(REPO, "hyres-residual-enhanced-hybrid-image-compression_amd"))

DTYPES = [(0, 0), (1, 0), (1, 1), (1, 2), (1, 3), (0, 1), (0, 2), (0, 3)]  # (f16_operands, io_f16)
ALL_DT = list(range(len(DTYPES)))
CH = [3, 4, 5, 16, 32, 48, 64, 96, 128, 192, 512]
CONV = [[1, 1, 1], [1, 2, 1], [3, 1, 1], [3, 1, 2], [3, 2, 1], [3, 2, 2], [5, 1, 1], [5, 2, 1]]  # K, stride, dilation
HW = [12, 16, 32, 48, 64, 128, 256]
TUNINGS = [[3, 1024], [4, 2], [5, 1], [6, 128], [7, 0], [15, 1], [16, 1], [22, 1], [23, 0]]
REQUIRED = ["wgrad_kernel", "wgrad_f16_kernel", "wgrad1x1_kernel", "wgrad1x1_bf6_kernel", "wgrad1x1_bf6_pf2_kernel",
            "wgrad_thin_kernel", "wgrad_halo_kernel", "wgrad_halo_f16_kernel", "wgrad_halo_bf6_kernel",
            "wgrad_halo_bf6_pf2_kernel"]
CONV2D, DECONV2D = "hyres_wgrad_desc_conv2d", "hyres_wgrad_desc_deconv2d"


def sections():
    def cross(tuning=0, square_q=0, dtypes=ALL_DT, cin=CH, cout=CH, conv=CONV, hw=HW, batch=(2, 16), ld_extra=0):
        return dict(fn=CONV2D, tuning=tuning, square_q=square_q, dtypes=list(dtypes), cin=list(cin), cout=list(cout),
                    conv=list(conv), hw=list(hw), batch=list(batch), ld_extra=ld_extra)

    one = [c for c in CONV if c[0] == 1]
    per_k = [[1, 1, 1], [3, 1, 1], [5, 1, 1]]
    rep = [3, 64, 128]
    # the full cross of the axes is 13552 descriptors x 8 dtype modes: thinned so that the file stays reviewable, every
    # value of every axis still meeting every kernel size and stride
    out = [
        cross(hw=[32, 128], batch=[16], dtypes=[0]),                              # every channel pair, fp32
        cross(cin=[3, 16, 64, 192], cout=[3, 16, 64, 192], dtypes=[0]),           # every grid and batch, fp32
        cross(cin=[3, 32, 64, 128], cout=[3, 32, 64, 128], hw=[64], batch=[16]),  # every dtype mode
        cross(square_q=1, cin=[32, 64, 128, 192], cout=[32, 64, 128, 192], conv=one, hw=[32], batch=[16],
              dtypes=[0, 1, 4, 6]),                                               # GDN gamma gradients
        cross(cin=[64], cout=[64, 128], conv=per_k, hw=[64], batch=[16], ld_extra=4),   # ldx > Ci, once per K
        cross(cin=[64], cout=[64, 128], conv=per_k, hw=[64], batch=[16], ld_extra=2),   # ... and ldx % 4 != 0
        dict(fn=DECONV2D, tuning=0, square_q=0, dtypes=ALL_DT,
             geoms=[[16, S, S, ci, ci, co, co, 5, 2] for ci, co, S in [(128, 128, 32), (192, 128, 16), (128, 3, 64)]]),
    ]
    for ti in range(1, len(TUNINGS) + 1):
        out.append(cross(tuning=ti, cin=rep, cout=rep, hw=[128], batch=[16], dtypes=[0, 1]))
    return out


def expand(section):
    """The descriptor-function argument lists of a section, in the order of its cases."""
    if "geoms" in section:
        return [list(g) for g in section["geoms"]]
    x = section["ld_extra"]
    return [[B, S, S, ci, ci + x, co, co, K, K, stride, (K // 2) * dil, dil]
            for ci, co, (K, stride, dil), S, B in itertools.product(section["cin"], section["cout"], section["conv"],
                                                                   section["hw"], section["batch"])]


def descriptor(L, lib, section, args, dtype):
    d = L.WgradDesc()
    assert getattr(lib, section["fn"])(ctypes.byref(d), *args) == 0, (section["fn"], args)
    d.square_q = section["square_q"]
    d.f16_operands, d.io_f16 = dtype
    return d


def query(lib, d):
    """((name, nsplit, blocks, threads, lanes), workspace bytes) of a descriptor."""
    buf = ctypes.create_string_buffer(96)
    assert lib.hyres_wgrad_kernel_name(ctypes.byref(d), buf, len(buf)) == 0
    v = [ctypes.c_int(-9) for _ in range(4)]
    assert lib.hyres_wgrad_plan(ctypes.byref(d), *[ctypes.byref(x) for x in v]) == 0
    return (buf.value.decode(), *[x.value for x in v]), lib.hyres_wgrad_workspace_bytes(ctypes.byref(d))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=None, help="library to record (default: the in-tree build)")
    ap.add_argument("--out", default=os.path.join(HERE, "wgrad_routing.json"))
    args = ap.parse_args()
    from hyres_hip import _lib as L
    lib = L.load(args.lib) if args.lib else L.load()
    base = {}
    for k in sorted({k for k, _ in TUNINGS}):
        old = ctypes.c_int(0)
        assert lib.hyres_conv_tuning(k, 0, ctypes.byref(old)) == 0
        assert lib.hyres_conv_tuning(k, old.value, None) == 0
        base[k] = old.value
    assert all(base[k] != v for k, v in TUNINGS), base
    tunings = [None] + TUNINGS
    names, results, index = [], [], {}

    def intern(table, item):
        key = (id(table), json.dumps(item))
        if key not in index:
            index[key] = len(table)
            table.append(item)
        return index[key]

    secs, ncases = sections(), 0
    for sec in secs:
        tune = tunings[sec["tuning"]]
        if tune:
            assert lib.hyres_conv_tuning(tune[0], tune[1], None) == 0
        try:
            cases = []
            for a in expand(sec):
                for di in sec["dtypes"]:
                    res, ws = query(lib, descriptor(L, lib, sec, a, DTYPES[di]))
                    cases += [intern(results, [intern(names, res[0])] + list(res[1:])), ws]
            sec["cases"] = cases
            ncases += len(cases) // 2
        finally:
            if tune:
                assert lib.hyres_conv_tuning(tune[0], base[tune[0]], None) == 0
    missing = [r for r in REQUIRED if not any(n.startswith(r + "<") for n in names)]
    if missing:
        sys.exit(f"not written: no recorded case runs {missing}")
    out = dict(dtypes=DTYPES, tunings=tunings, base={str(k): v for k, v in base.items()}, names=names, results=results,
               sections=secs)
    with open(args.out, "w") as f:
        json.dump(out, f, separators=(",", ":"))
        f.write("\n")
    print(f"{args.out}: {len(secs)} sections, {ncases} cases, {len(names)} kernel names, {os.path.getsize(args.out)} bytes")


if __name__ == "__main__":
    main()
