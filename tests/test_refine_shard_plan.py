"""The row cuts of tests/test_gpu_refine_sharded.py attack qvq_refine's stop rule: a rank that
decided on the rows it holds would stop before the others.  The reference loop
(tests/helpers/refine_ref.py's steps over the oracle), run here on the CPU with the changed rows
counted per shard, holds the figures that claim rests on."""
import json
import os

from conftest import GOLDEN
from helpers import refine_ref as ref
from oracle import oracle


def moved_rows(name):
    """Per iteration of the reference loop on case `name`, to the fixed point: which rows changed
    their code vector."""
    S, b, bits = ref.CASES[name]
    _, X = ref.case_vectors(S, b)
    C, A, _ = ref.lbg_start(X, bits)
    out = []
    for _ in range(100):
        A_t = oracle.kdtree_nn(C, X)
        C = oracle.centroids(X, A_t, 1 << bits, sum_mode=1)
        out.append(A_t != A)
        A = A_t
        if not out[-1].any():
            break
    return out


def shard_counts(moved, cuts):
    """The rows changed within each shard (row cuts), per iteration."""
    return [[int(m[lo:hi].sum()) for lo, hi in zip(cuts[:-1], cuts[1:])] for m in moved]


def test_cuts_make_a_local_stop_rule_stop_early():
    with open(os.path.join(GOLDEN, "refine_trace.json")) as f:
        trace = json.load(f)["s128_b2_6"]
    N = trace["n"]
    moved = moved_rows("s128_b2_6")
    assert N == 4096 and moved[0].size == N
    thirds = shard_counts(moved, [N * r // 3 for r in range(4)])
    assert [sum(c) for c in thirds] == trace["changed"] and len(thirds) == 35
    # iteration 15 (index 14): rank 0 sees no change while 14 rows move elsewhere
    assert thirds[14][0] == 0 and sum(thirds[14]) == 14
    # rank 0 is at rest from iteration 25 on, rank 1 from 28 on; all ranks only at 35
    assert thirds[23][0] != 0 and all(c[0] == 0 for c in thirds[24:])
    assert thirds[26][1] != 0 and all(c[1] == 0 for c in thirds[27:])
    assert [i + 1 for i, c in enumerate(thirds) if sum(c) == 0] == [35]
    # seven rows on rank 0: 5 of them move once, then none, 33 iterations before the end
    seven = shard_counts(moved, [0, 7, N])
    assert [sum(c) for c in seven] == trace["changed"]
    assert seven[0][0] == 5 and all(c[0] == 0 for c in seven[1:])
    # equal halves: the sums over the shards are the global counts (the all-reduced u64)
    halves = shard_counts(moved, [0, N // 2, N])
    assert [sum(c) for c in halves] == trace["changed"]
