"""Records tests/golden/ref_nn.json, tests/golden/ref_nn_neartie.json, tests/golden/ref_nn_exact.json and
tests/golden/ref_nn_prune.json:
what the compiled reference kd-tree (oracle/_ref/libref_nn.so, `make -C oracle ref` where the reference
checkout is present) answers for the inputs of tests/test_oracle_golden.py's kd-tree tests, for every
case of tests/helpers/neartie_cases.py, for the chunk and near-tie cases of
tests/helpers/exact_cases.py, and for the tie rows (the two nearest code vectors within 1e-12
relative) of the tie-bearing cases of tests/helpers/prune_cases.py, as fingerprints of its index arrays beside those of the codebooks it
was given.  Run from the repository root after a change of those inputs:

    python tests/helpers/record_ref_nn.py
"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))   # tests/: conftest, the test module

import numpy as np   # noqa: E402

import test_oracle_golden as t   # noqa: E402
from helpers import exact_cases as ex   # noqa: E402
from helpers import neartie_cases as nt   # noqa: E402
from helpers import prune_cases as pc   # noqa: E402

WHAT = ("sha-256[:16] of the compiled reference kd-tree's indices (A, little-endian u32) for the codebook "
        "with fingerprint C (float64), over every row of the case's training set")
WHAT_TIES = WHAT.replace("every row", "the tie rows (the two nearest code vectors within 1e-12 relative)")


def record(C, X):
    ref = t._ref_nn(C, X)
    if ref is None:
        sys.exit("oracle/_ref/libref_nn.so is not built: make -C oracle ref")
    return {"C": t.sha(np.ascontiguousarray(C, np.float64)), "A": t.sha(ref.astype("<u4"))}


def record_prune():
    prune = {"what": WHAT_TIES, "cases": {}}
    for c in pc.CASES:
        if not c["has_ties"]:
            continue
        X, C, _ = pc.inputs(c)
        d1, d2, _, _ = nt.top_two(X, C)
        prune["cases"][pc.key(c)] = record(C, X[(d2 - d1) <= pc.TIE_REL * d1])
    with open(os.path.join(t.GOLDEN, "ref_nn_prune.json"), "w") as f:
        json.dump(prune, f, indent=1)
        f.write("\n")


def main():
    out = {"what": WHAT,
           "tie_heavy": {str(K): record(C, X) for K, C, X in t.tie_heavy_codebooks()}, "levels": {}}
    for case in t.LEVEL_CASES:
        X, splits, _ = t.level_case(case)
        out["levels"][case] = [record(Cs, X) for Cs in splits]
    with open(os.path.join(t.GOLDEN, "ref_nn.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    near = {"what": WHAT, "cases": {}}
    for c in nt.CASES:
        X, C = nt.inputs(c)
        near["cases"][nt.key(c)] = record(C, X)
    with open(os.path.join(t.GOLDEN, "ref_nn_neartie.json"), "w") as f:
        json.dump(near, f, indent=1)
        f.write("\n")
    exact = {"what": WHAT, "cases": {}}
    for c in ex.CHUNK_CASES + ex.NEARTIE_CASES:
        X, C = ex.inputs(c)[:2]
        exact["cases"][ex.key(c)] = record(C, X)
    with open(os.path.join(t.GOLDEN, "ref_nn_exact.json"), "w") as f:
        json.dump(exact, f, indent=1)
        f.write("\n")
    record_prune()


if __name__ == "__main__":
    main()
