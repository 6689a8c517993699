"""Compare two builds of libhyres_hip.so kernel by kernel (host tools only, no GPU): threads, LDS, scratch, allocated
VGPRs, SGPRs and whether the instruction streams are equal. The check a refactor of device code runs against the
parent commit's build.

    python scripts/kernel_diff.py parent.so new.so [--renamed OLD=NEW ...] [--only names.json] [--json out.json]

--renamed maps a kernel's demangled name in the parent to its name in the new build (a merged or re-templated kernel);
a kernel only one build has is reported under "only_parent" / "only_new". --only names.json (a JSON object keyed by
kernel name, such as tests/golden/refine_kernels.json) lists those kernels row by row and sums the others up under
"rest_of_library".
"""
from __future__ import annotations

import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kernel_meta  # noqa: E402

FIELDS = ("threads", "lds", "scratch", "alloc", "sgpr")


def load(so: str) -> dict[str, dict]:
    ks = kernel_meta.kernels(so)
    dis = kernel_meta.disassembly(so)
    names = kernel_meta.demangle([k["name"] for k in ks])
    out = {}
    for k, n in zip(ks, names):
        short = n.replace("hyres::", "").replace("void ", "").split("(")[0]
        out[short] = {**{f: k[f] for f in FIELDS}, "isa": dis.get(k["name"], [])}
    return out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("parent")
    ap.add_argument("new")
    ap.add_argument("--renamed", nargs="*", default=[])
    ap.add_argument("--only", default=None)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    old, new = load(a.parent), load(a.new)
    for pair in a.renamed:
        o, n = pair.split("=", 1)
        if o in old:
            old[n + " (was " + o + ")"] = old.pop(o)
            new[n + " (was " + o + ")"] = new[n]  # several parent kernels may map to one new kernel
    mapped = {n.split(" (was ")[0] for n in new if " (was " in n}
    rows = {}
    for n in sorted(set(old) & set(new)):
        p, q = old[n], new[n]
        rows[n] = {"parent": {f: p[f] for f in FIELDS}, "new": {f: q[f] for f in FIELDS},
                   "meta_equal": all(p[f] == q[f] for f in FIELDS), "isa_equal": p["isa"] == q["isa"]}
    res = {"command": "scripts/kernel_diff.py " + " ".join(
               [os.path.basename(a.parent), os.path.basename(a.new)] + (["--renamed"] + [repr(r) for r in a.renamed]
                                                                        if a.renamed else [])
               + (["--only", a.only] if a.only else [])),
           "fields": "threads = the launch bound in the metadata (1024: none); alloc = allocated VGPRs",
           "kernels": rows, "only_parent": sorted(set(old) - set(new)),
           "only_new": sorted(set(new) - set(old) - mapped),
           "meta_differs": sorted(n for n, r in rows.items() if not r["meta_equal"]),
           "lds_scratch_or_vgpr_allocation_differs": sorted(
               n for n, r in rows.items() if any(r["parent"][f] != r["new"][f] for f in ("lds", "scratch", "alloc"))),
           "isa_differs": sorted(n for n, r in rows.items() if not r["isa_equal"])}
    if a.only:
        with open(a.only) as f:
            keep = set(json.load(f))
        rest = {n: r for n, r in rows.items() if n.split(" (was ")[0] not in keep}
        res["kernels"] = {n: r for n, r in rows.items() if n not in rest}
        res["rest_of_library"] = {"kernels": len(rest),
                                  "all_identical": all(r["meta_equal"] and r["isa_equal"] for r in rest.values())}
    for key in ("only_parent", "only_new", "meta_differs", "lds_scratch_or_vgpr_allocation_differs", "isa_differs"):
        print(f"{key}: {len(res[key])}")
        for n in res[key]:
            r = rows.get(n)
            print("   ", n, "" if r is None else f"{r['parent']} -> {r['new']}")
    print(f"{len(rows)} kernels in both, {sum(r['isa_equal'] for r in rows.values())} instruction-equal")
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
