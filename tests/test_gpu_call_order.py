"""Calls in the orders that abandon a level with work pending: a refine that stops at max_iters,
one that stops early on eps and drops the search in flight, a quantize after each, then assign,
update and a warm-started refine, all on the session's context.  Every result must equal, bit for
bit, what a fresh context gives that ran only the calls the result depends on.  (Parity with the
oracle is the business of the other GPU tests.)"""
import numpy as np
import pytest

import quant_amd
from oracle import oracle

pytestmark = pytest.mark.gpu


def tie_rows(bw, rows, zeroed):
    """test_lbg_zero_rows_and_empty_cells' construction: more code vectors than distinct rows, so
    empty cells give zero code vectors whose split copies coincide, and the zero rows tie."""
    rng = np.random.default_rng(11)
    X, _ = oracle.tile(oracle.gen_image(64), 64, 64, bw, bw)
    X = X[:rows].copy()
    X[rng.choice(rows, zeroed, replace=False)] = 0.0
    return X


def same_lbg(got, want):
    return np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[2] == want[2]


def same_refine(got, want):
    return same_lbg(got, want) and got[3] == want[3]


# D = 12: the fused search, the ties go with the reduce.  D = 48, K = 256 > 200 rows: the wide
# search with a separate sums pass, the ties' moves applied to the finished sums.
@pytest.mark.parametrize("bw,rows,zeroed,bits", [(2, 300, 120, 9), (4, 200, 80, 8)])
def test_call_order(engine, bw, rows, zeroed, bits):
    X = tie_rows(bw, rows, zeroed)
    K = 1 << bits
    assert X.shape[1] == 3 * bw * bw

    engine.set_vectors(X)
    r1 = engine.lbg(bits)
    assert sum(engine.timings()["host_ties"]) > 0   # the tie paths ran
    r2 = engine.refine(max_iters=2, eps=0.0)        # MAXIT, nothing in flight at the end
    r3 = engine.refine(max_iters=40, eps=0.5)       # stops on eps, drops the search in flight
    r4 = engine.lbg(bits)
    C = r4[0]
    A5 = engine.assign(C)
    u6 = engine.update(A5, K)
    r7 = engine.refine(K=K, C=C, max_iters=1, fresh=True)
    r8 = engine.lbg(bits)
    assert r2[3]["stop"] == quant_amd.STOP_MAXIT and r2[3]["iters"] == 2
    assert r3[3]["stop"] == quant_amd.STOP_EPS and r3[3]["iters"] < 40

    with quant_amd.Engine(0) as ref:   # lbg, then step 2's refine, then step 3's on top of it
        ref.set_vectors(X)
        w1 = ref.lbg(bits)
        assert sum(ref.timings()["host_ties"]) > 0
        w2 = ref.refine(max_iters=2, eps=0.0)
        w3 = ref.refine(max_iters=40, eps=0.5)
    assert same_lbg(r1, w1)
    assert same_refine(r2, w2)
    assert same_refine(r3, w3)
    assert same_lbg(r4, w1)
    assert same_lbg(r8, w1)
    assert same_lbg(r4, r1) and same_lbg(r8, r1)

    with quant_amd.Engine(0) as ref:   # steps 5-7 depend on the codebook alone
        ref.set_vectors(X)
        assert np.array_equal(A5, ref.assign(C))
        w6 = ref.update(A5, K)
        assert np.array_equal(u6[0], w6[0]) and np.array_equal(u6[1], w6[1])
        assert same_refine(r7, ref.refine(K=K, C=C, max_iters=1, fresh=True))
