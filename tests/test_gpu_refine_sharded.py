"""qvq_refine on a communicator (include/qvq.h): the rows split over 2 or 3
rank processes that share GPU 0 through the host communicator (tests/helpers/refine_rank_worker.py),
and a one-rank RCCL communicator in-process.  Every rank must return what one rank returns over all
the rows -- codebook, distortion and traces bit for bit, its own rows' indices -- which in turn is
the reference loop of tests/helpers/refine_ref.py (indices and codebook bit for bit, distortions
within 1e-9 relative, as tests/test_gpu_refine.py).  The cuts are those whose local changed counts
would stop a rank early (tests/test_refine_shard_plan.py)."""
import functools
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import quant_amd
from conftest import GOLDEN
from helpers import refine_ref as ref
from oracle import oracle

pytestmark = pytest.mark.gpu
QVQ_EINVAL, QVQ_ESTATE = 1, 6
WORKER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers", "refine_rank_worker.py")
with open(os.path.join(GOLDEN, "refine_trace.json")) as _f:
    TRACE = json.load(_f)

HALVES = ["0/2", "1/2", "2/2"]
THIRDS = ["0/3", "1/3", "2/3", "3/3"]
SEVEN = ["=0", "=7", "1/1"]


def run_ranks(world, plan, cuts, tmp, env=None, limit=150):
    """world rank processes sharing GPU 0 through the host communicator; returns each rank's
    results.  A rank that fails ends the others at once; the group is bounded by `limit` seconds."""
    rdv = str(tmp / "rendezvous")
    outs = [str(tmp / ("rank%d.npz" % r)) for r in range(world)]
    penv = dict(os.environ, **(env or {}))
    procs = [subprocess.Popen([sys.executable, WORKER, str(r), str(world), rdv, plan, outs[r], *cuts], env=penv)
             for r in range(world)]
    deadline = time.time() + limit
    try:
        while any(p.poll() is None for p in procs):
            if any(p.poll() not in (None, 0) for p in procs) or time.time() > deadline:
                break
            time.sleep(0.05)
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
                p.wait()
    codes = [p.returncode for p in procs]
    assert codes == [0] * world, codes
    res = [dict(np.load(o)) for o in outs]
    for r in res:
        assert r["info"][0] == world and r["info"][2] == 2   # host communicator, world ranks
    return res


@pytest.fixture(scope="module")
def halves(tmp_path_factory):
    return run_ranks(2, "fix_s128_b2_6,k512,state", HALVES, tmp_path_factory.mktemp("halves"))


@pytest.fixture(scope="module")
def thirds(tmp_path_factory):
    return run_ranks(3, "fix_s128_b2_6,fix_s64_b2_4,fix_s96_b4_5,eps,fresh0,fresh3,warm", THIRDS,
                     tmp_path_factory.mktemp("thirds"))


@pytest.fixture(scope="module")
def seven(tmp_path_factory):
    return run_ranks(2, "fix_s128_b2_6", SEVEN, tmp_path_factory.mktemp("seven"))


@pytest.fixture(scope="module")
def disagree(tmp_path_factory):
    return run_ranks(3, "disagree", THIRDS, tmp_path_factory.mktemp("disagree"), env={"QVQ_TIMEOUT_S": "20"})


@functools.lru_cache(maxsize=None)
def vectors(name, seed=0x5EED):
    S, b, bits = ref.CASES[name] if name in ref.CASES else (256, 2, 9)
    return ref.case_vectors(S, b, seed) + (S, b, bits)


@functools.lru_cache(maxsize=None)
def oracle_run(name, max_iters=100, eps=0.0, fresh=False):
    """The reference loop from the case's lbg start."""
    _, X, _, _, bits = vectors(name)
    return ref.refine(X, *ref.lbg_start(X, bits), max_iters=max_iters, eps=eps, fresh=fresh)


@functools.lru_cache(maxsize=None)
def warm_vectors():
    return ref.case_vectors(128, 2, seed=0xBEEF)


def lbg_on(engine, name):
    rgb, _, S, b, bits = vectors(name)
    engine.set_images(rgb, 1, S, S, b, b, quant_amd.SCALED)
    return engine.lbg(bits)


def got_of(r, key):
    """A rank's results of step `key` as Engine.refine returns them."""
    return (r[key + "_C"], r[key + "_A"], float(r[key + "_d"][0]),
            {"iters": int(r[key + "_iters"][0]), "stop": int(r[key + "_stop"][0]),
             "changed": [int(x) for x in r[key + "_changed"]], "distortion": [float(x) for x in r[key + "_trace"]]})


def same_as_one_rank(res, key, one, want):
    """Every rank's run `key` against the one-rank engine's run `one` (codebook, distortion and
    traces bit for bit, the ranks' indices concatenated) and the reference loop's `want` (indices
    and codebook bit for bit, distortions within 1e-9 relative)."""
    C1, A1, d1, info1 = one
    C_r, A_r, d_r, info_r = want
    for r in res:
        C, _, d, info = got_of(r, key)
        assert info["iters"] == info1["iters"] == info_r["iters"]
        assert info["stop"] == info1["stop"] == info_r["stop"]
        assert info["changed"] == info1["changed"] == info_r["changed"]
        assert np.array_equal(C, C_r), "codebook differs from the reference loop"
        assert np.array_equal(C, C1), "codebook differs from the one-rank engine"
        assert info["distortion"] == info1["distortion"] and d == d1, "distortion differs from the one-rank engine"
        print(key, "distortion", d, "reference", d_r)
        np.testing.assert_allclose(info["distortion"], info_r["distortion"], rtol=1e-9, atol=0)
        assert abs(d - d_r) <= 1e-9 * abs(d_r)
    A = np.concatenate([r[key + "_A"] for r in res])
    assert np.array_equal(A, A_r), "indices differ from the reference loop"
    assert np.array_equal(A, A1), "indices differ from the one-rank engine"


def budget(res, key, K, D, fresh=False):
    """Case 8: at most iters + 3 collectives in the call -- the entry vote, the histogram, one per
    iteration, one more with fresh -- of which exactly the iterations' (and the fresh tail's) carry
    a level's sums."""
    for r in res:
        calls, iters = [int(c) for c in r[key + "_calls"]], int(r[key + "_iters"][0])
        print(key, "collectives", calls)
        assert len(calls) <= iters + 3
        assert sum(c >= 2 * K * D + K for c in calls) == iters + (1 if fresh else 0)


def fixed_point(engine, res, name):
    lbg_on(engine, name)
    one = engine.refine(max_iters=40, eps=0.0)
    for r in res:
        _, _, _, info = got_of(r, "fix_" + name)
        assert info["iters"] == TRACE[name]["iters"] and info["stop"] == quant_amd.STOP_FIXED
        assert info["changed"] == TRACE[name]["changed"]
    same_as_one_rank(res, "fix_" + name, one, oracle_run(name))
    budget(res, "fix_" + name, *one[0].shape)


@pytest.mark.timeout(300)
@pytest.mark.parametrize("cut", ["halves", "thirds", "seven"])
def test_fixed_point_s128(engine, request, cut):
    """Case 1: 35 iterations to the fixed point on every rank, under cuts whose local changed
    counts reach 0 at iterations 15, 25 and 28 (thirds) and 2 (seven rows)."""
    res = request.getfixturevalue(cut)
    assert [int(r["fix_s128_b2_6_iters"][0]) for r in res] == [35] * len(res)
    fixed_point(engine, res, "s128_b2_6")


@pytest.mark.timeout(300)
@pytest.mark.parametrize("name", ["s64_b2_4", "s96_b4_5"])
def test_fixed_point_other_searches(engine, thirds, name):
    """Case 2: the small-K scan (12 iterations) and the counting-sort sums (D = 48, 9 iterations)."""
    fixed_point(engine, thirds, name)


@pytest.mark.timeout(300)
def test_eps_stop(engine, thirds):
    lbg_on(engine, "s128_b2_6")
    one = engine.refine(max_iters=40, eps=0.01)
    for r in thirds:
        assert int(r["eps_iters"][0]) == 5 and int(r["eps_stop"][0]) == quant_amd.STOP_EPS
    same_as_one_rank(thirds, "eps", one, oracle_run("s128_b2_6", 40, 0.01))
    budget(thirds, "eps", *one[0].shape)


@pytest.mark.timeout(300)
def test_fresh(engine, thirds):
    _, X, _, _, bits = vectors("s128_b2_6")
    C0, _, _ = ref.lbg_start(X, bits)
    lbg_on(engine, "s128_b2_6")
    one = engine.refine(max_iters=0, fresh=True)
    A_ref = oracle.kdtree_nn(C0, X)
    direct = ref.distortion(X, C0, A_ref)
    for r in thirds:
        C, _, d, info = got_of(r, "fresh0")
        assert info["iters"] == 0 and info["changed"] == []
        assert np.array_equal(C, C0) and np.array_equal(C, r["fresh0_lbg_C"])
        print("fresh distortion", d, "direct", direct)
        assert abs(d - direct) <= 1e-9 * direct and d == one[2]
    assert np.array_equal(np.concatenate([r["fresh0_A"] for r in thirds]), A_ref)
    budget(thirds, "fresh0", *C0.shape, fresh=True)
    lbg_on(engine, "s128_b2_6")
    one = engine.refine(max_iters=3, eps=0.0, fresh=True)
    same_as_one_rank(thirds, "fresh3", one, oracle_run("s128_b2_6", 3, 0.0, True))
    budget(thirds, "fresh3", *C0.shape, fresh=True)


@pytest.mark.timeout(300)
def test_warm_start(engine, thirds):
    C_fix = oracle_run("s128_b2_6")[0]
    rgb, X = warm_vectors()
    engine.set_images(rgb, 1, 128, 128, 2, 2, quant_amd.SCALED)
    one = engine.refine(C=C_fix, max_iters=4, eps=0.0)
    for r in thirds:
        assert int(r["warm_changed"][0]) == X.shape[0]   # the rows of every rank
    same_as_one_rank(thirds, "warm", one, ref.refine(X, C_fix, max_iters=4, eps=0.0))
    budget(thirds, "warm", *C_fix.shape)


@pytest.mark.timeout(300)
def test_pruned_search_k512(engine, halves):
    rgb, X, S, b, bits = vectors("k512")
    engine.set_images(rgb, 1, S, S, b, b, quant_amd.SCALED)
    engine.lbg(bits)
    one = engine.refine(max_iters=3, eps=0.0)
    same_as_one_rank(halves, "k512", one, ref.refine(X, *ref.lbg_start(X, bits), max_iters=3, eps=0.0))
    budget(halves, "k512", *one[0].shape)


@pytest.mark.timeout(300)
def test_state_rules(engine, halves):
    """A later lbg gives what it gave before; two refines in a row equal one longer refine."""
    C1, A1, d1 = lbg_on(engine, "s64_b2_4")
    for r in halves:
        for key in ("state_lbg1", "state_lbg2"):
            assert np.array_equal(r[key + "_C"], C1) and float(r[key + "_d"][0]) == d1
    for key in ("state_lbg1", "state_lbg2"):
        assert np.array_equal(np.concatenate([r[key + "_A"] for r in halves]), A1)
    same_as_one_rank(halves, "state_r40", engine.refine(max_iters=40, eps=0.0), oracle_run("s64_b2_4"))
    for r in halves:
        C5, A5, d5, i5 = got_of(r, "state_r5")
        C3, A3, d3, i3 = got_of(r, "state_r2r3")
        i2 = got_of(r, "state_r2")[3]
        assert i2["iters"] == 2 and i3["iters"] == 3 and i5["iters"] == 5
        assert np.array_equal(C3, C5) and np.array_equal(A3, A5) and d3 == d5
        assert i2["changed"] + i3["changed"] == i5["changed"]
        assert i2["distortion"] + i3["distortion"] == i5["distortion"]
    lbg_on(engine, "s64_b2_4")
    same_as_one_rank(halves, "state_r5", engine.refine(max_iters=5, eps=0.0), oracle_run("s64_b2_4", 5, 0.0))


@pytest.mark.timeout(300)
def test_disagreement_ends_every_rank_at_once(engine, disagree):
    """Case 9: a rank with other arguments, then a rank without a state to continue from.  Every
    rank returns within seconds (the ranks' waits are bounded by 20 s here: none ran into it), and
    the contexts still work."""
    for rank, r in enumerate(disagree):
        st, secs = r["dis_iters"]
        print("rank", rank, "different max_iters:", st, "%.3f s" % secs)
        assert st == QVQ_EINVAL and secs < 10
        st, secs = r["dis_state"]
        print("rank", rank, "rank 1 without state:", st, "%.3f s" % secs)
        assert st == (QVQ_ESTATE if rank == 1 else QVQ_EINVAL) and secs < 10
    lbg_on(engine, "s64_b2_4")
    same_as_one_rank(disagree, "dis_after", engine.refine(max_iters=40, eps=0.0), oracle_run("s64_b2_4"))


def test_one_rank_rccl_communicator(engine):
    """Case 10: the ncclAllReduce path, one rank in-process: bit-equal to the engine without a
    communicator to the fixed point, with fresh indices and from a warm start."""
    rgb, _, S, b, bits = vectors("s128_b2_6")
    rgb_w, _ = warm_vectors()
    C_fix = oracle_run("s128_b2_6")[0]

    def runs(eng):
        out = []
        eng.set_images(rgb, 1, S, S, b, b, quant_amd.SCALED)
        eng.lbg(bits)
        out.append(eng.refine(max_iters=40, eps=0.0))
        eng.lbg(bits)
        out.append(eng.refine(max_iters=0, fresh=True))
        eng.lbg(bits)
        out.append(eng.refine(max_iters=3, eps=0.0, fresh=True))
        eng.set_images(rgb_w, 1, 128, 128, 2, 2, quant_amd.SCALED)
        out.append(eng.refine(C=C_fix, max_iters=4, eps=0.0))
        return out

    want = runs(engine)
    with quant_amd.Engine(0) as eng:
        eng.comm_init(1, 0, quant_amd.Engine.comm_unique_id())
        got = runs(eng)
    assert want[0][3]["iters"] == 35 and want[3][3]["changed"][0] == 4096
    for (C, A, d, info), (C1, A1, d1, info1) in zip(got, want):
        assert info == info1 and d == d1
        assert np.array_equal(C, C1) and np.array_equal(A, A1)
