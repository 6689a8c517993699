"""Records tests/golden/wgrad_kernels.json: for every case of tests/test_wgrad_kernels_gpu.py the kernel the built
library names for it (hyres_wgrad_kernel_name_at, at the case's pointer alignments) as a string, or as
[native, bf16x6] where hyres_conv_tuning key 7 changes it.  Host only; run it after a deliberate routing change and
review the diff:

    python tests/golden/make_wgrad_kernels.py
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "wgrad_kernels.json")
sys.path[:0] = [os.path.join(REPO, "tests"), os.path.join(REPO, "hyres-residual-enhanced-hybrid-image-compression_amd"),
                REPO]

if __name__ == "__main__":
    if not os.path.exists(OUT):  # the test module reads the file at import
        with open(OUT, "w") as f:
            f.write("{}\n")
    import test_wgrad_kernels_gpu as T
    from hyres_hip import _lib as L
    names = {}
    for c in T.CASES:
        n0, n1 = T.query(L, c, 0)[0], T.query(L, c, 1)[0]
        names[c.id] = n0 if n0 == n1 else [n0, n1]
    with open(OUT, "w") as f:
        f.write("{\n" + ",\n".join(f" {json.dumps(k)}: {json.dumps(v)}" for k, v in names.items()) + "\n}\n")
    print(f"{len(names)} cases -> {OUT}")
