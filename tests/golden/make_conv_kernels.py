"""Records tests/golden/conv_kernels.json: for every case of tests/test_conv_kernels_gpu.py the kernel name and the
float4-epilogue flag the built library reports (hyres_conv_kernel_name_at, at the case's pointer alignments, pitches
and workspace mode) as [name, vec4], or as [[name, vec4] native, [name, vec4] bf16x6] where hyres_conv_tuning key 7
changes it.  Host only; run it after a deliberate routing change and review the diff:

    python tests/golden/make_conv_kernels.py
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "conv_kernels.json")
sys.path[:0] = [os.path.join(REPO, "tests"), os.path.join(REPO, "hyres-residual-enhanced-hybrid-image-compression_amd"),
                REPO]

if __name__ == "__main__":
    if not os.path.exists(OUT):  # the test module reads the file at import
        with open(OUT, "w") as f:
            f.write("{}\n")
    import test_conv_kernels_gpu as T
    from hyres_hip import _lib as L
    names = {}
    for c in T.CASES:
        n0, n1 = list(T.query(L, c, 0)), list(T.query(L, c, 1))
        names[c.id] = n0 if n0 == n1 else [n0, n1]
    with open(OUT, "w") as f:
        f.write("{\n" + ",\n".join(f" {json.dumps(k)}: {json.dumps(v)}" for k, v in names.items()) + "\n}\n")
    print(f"{len(names)} cases -> {OUT}")
