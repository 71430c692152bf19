"""Codebooks past each kernel's LDS capacity (tests/helpers/largek_cases.py): the unfused and
unstaged MFMA searches, the tiled VALU search, the chunked and global-memory rechecks, the sums in
several passes, trees too large for the device build or for kd_resolve's LDS -- against the CPU
oracle, bit for bit.  tests/test_largek_plan.py holds each case to the path it is there for.

References: oracle.kdtree_nn (the reference's kd-tree answer, src/Quantizer.cpp:24-32) for
qvq_assign, oracle.centroids(sum_mode=1) and np.bincount for qvq_update, reference_lbg for qvq_lbg,
tests/helpers/refine_ref.py for qvq_refine."""
import functools

import numpy as np
import pytest

import quant_amd
from helpers import largek_cases as lk
from helpers import refine_ref as ref
from oracle import oracle
from test_gpu_parity import _check_against_oracle

pytestmark = pytest.mark.gpu


def _id(c):
    return "%dx%d-K%d" % (c["bw"], c["bh"], c["K"])


# -- (a) qvq_assign ------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _vectors(bw, bh):
    X = lk.assign_vectors(bw, bh)
    X.setflags(write=False)
    return X


@functools.lru_cache(maxsize=None)
def _assign_case(bw, bh, K):
    """(rows, codebook, the reference's indices), computed once per case."""
    X = _vectors(bw, bh)
    C = lk.codebook(X, K, seed=K + 10 * bw + bh)
    want = oracle.kdtree_nn(C, X)
    C.setflags(write=False)
    want.setflags(write=False)
    return X, C, want


def _assign_and_check(engine, C, want):
    A = engine.assign(C)
    t = engine.timings()
    np.testing.assert_array_equal(A, want)
    assert t["flagged"][0] > 0        # the split pairs: the recheck ran
    assert t["host_ties"][0] > 0      # the duplicate code vectors: the tie path ran


@pytest.mark.parametrize("kd", ["default", "host"])
@pytest.mark.parametrize("case", lk.ASSIGN_CASES, ids=_id)
def test_assign(engine, monkeypatch, case, kd):
    """The default search of every case; ties by the default path (the device's kd_resolve, or the
    host where the tree image and a wave's K distances do not fit the LDS, K = 16385) and by the
    host (QVQ_KDTREE=host)."""
    monkeypatch.delenv("QVQ_SEARCH", raising=False)
    if kd == "host":
        monkeypatch.setenv("QVQ_KDTREE", "host")
    else:
        monkeypatch.delenv("QVQ_KDTREE", raising=False)
    X, C, want = _assign_case(case["bw"], case["bh"], case["K"])
    engine.set_vectors(X)
    _assign_and_check(engine, C, want)


@pytest.mark.parametrize("kd", ["default", "host"])
@pytest.mark.parametrize("case", [c for c in lk.ASSIGN_CASES if c["valu"] is not None], ids=_id)
def test_assign_valu_search(engine, monkeypatch, case, kd):
    """The tiled VALU search at every other width (QVQ_SEARCH=valu)."""
    monkeypatch.setenv("QVQ_SEARCH", "valu")
    if kd == "host":
        monkeypatch.setenv("QVQ_KDTREE", "host")
    else:
        monkeypatch.delenv("QVQ_KDTREE", raising=False)
    X, C, want = _assign_case(case["bw"], case["bh"], case["K"])
    engine.set_vectors(X)
    _assign_and_check(engine, C, want)


# -- (b) qvq_update ------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _update_vectors(bw, bh):
    rgb, S, X = lk.update_vectors(bw, bh)
    X.setflags(write=False)
    return rgb, S, X


@pytest.mark.parametrize("kind", ["uniform", "blocky", "last"])
@pytest.mark.parametrize("case", lk.UPDATE_CASES, ids=_id)
def test_update(engine, case, kind):
    bw, bh, K = case["bw"], case["bh"], case["K"]
    rgb, S, X = _update_vectors(bw, bh)
    A = lk.assignments(len(X), K, seed=K + bw)[kind]
    engine.set_images(rgb, 1, S, S, bw, bh, quant_amd.SCALED)
    C, cnt = engine.update(A, K)
    np.testing.assert_array_equal(cnt, np.bincount(A, minlength=K))
    np.testing.assert_array_equal(C, oracle.centroids(X, A, K, sum_mode=1))


# -- (c) qvq_lbg ---------------------------------------------------------------------------------
def _lbg(engine, c, bits=None):
    cs = oracle.NORMAL if c["cs"] == "normal" else oracle.SCALED
    return _check_against_oracle(engine, lk.noise(c["S"]), c["S"], c["S"], c["bw"], c["bh"], bits or c["bits"], cs=cs)


@pytest.mark.parametrize("case", lk.LBG_CASES, ids=lambda c: c["name"])
def test_lbg(engine, monkeypatch, case):
    monkeypatch.delenv("QVQ_SEARCH", raising=False)
    monkeypatch.delenv("QVQ_KDTREE", raising=False)
    _lbg(engine, case)
    if case["name"] == "2x2_n13":
        # a smaller quantize on the same context: nothing of the large levels' buffers or of their
        # tile order (perm_k) may leak into it
        _lbg(engine, case, bits=10)


# -- (d) qvq_refine above the pruned range -------------------------------------------------------
def test_refine_k8192(engine, monkeypatch):
    """K = 8192 at D = 12: refine's iterations on the VALU search, the chunked recheck and the
    counting-sort sums, against the loop through qvq_assign / qvq_update and the reference loop."""
    monkeypatch.delenv("QVQ_SEARCH", raising=False)
    monkeypatch.delenv("QVQ_KDTREE", raising=False)
    c = next(c for c in lk.LBG_CASES if c["name"] == "2x2_n13")
    S, bits = c["S"], c["bits"]
    rgb = lk.noise(S)
    X, _ = oracle.tile(rgb, S, S, 2, 2)
    engine.set_images(rgb, 1, S, S, 2, 2, quant_amd.SCALED)
    C, _, _ = engine.lbg(bits)
    K = C.shape[0]
    for _ in range(3):
        A = engine.assign(C)
        C, _ = engine.update(A, K)
    engine.lbg(bits)
    C_r, A_r, d_r, info = engine.refine(max_iters=3, eps=0.0)
    assert np.array_equal(A_r, A) and np.array_equal(C_r, C)
    _, _, d_w, want = ref.refine(X, *ref.lbg_start(X, bits), max_iters=3, eps=0.0)
    assert info["iters"] == want["iters"] and info["stop"] == want["stop"]
    assert info["changed"] == want["changed"]
    print("distortion trace", info["distortion"], "reference", want["distortion"])
    np.testing.assert_allclose(info["distortion"], want["distortion"], rtol=1e-9, atol=0)
    assert abs(d_r - d_w) <= 1e-9 * abs(d_w)
