"""The D = 12 MFMA search's epilogue (k_mf32.hip): the fp32 recompute of a winning unit that holds
padding positions, and flagged rows collected in a workgroup's LDS list before they reach the global
one (mfma_util.hpp flag_list_add).  Neither may move an index, a flag or a sum.

Indices: oracle.kdtree_nn (the reference's kd-tree answer, src/Quantizer.cpp:24-32).  Flags: the
engine exposes the number of flagged rows per search (timings()["flagged"]); it must be the number the
build before the LDS list flagged on the same input (tests/golden/search_epilogue_parent.json,
recorded with that build by tests/helpers/search_epilogue_cases.py), and the indices, which the
flagged rows' recheck decides, the oracle's.  The short qvq_lbg's codebook and distortion must be that
build's bit for bit (search_epilogue_parent_codebook.npy), its indices the oracle's."""
import functools

import numpy as np
import pytest

import quant_amd
from conftest import reference_lbg
from helpers import neartie_cases as nt
from helpers import search_epilogue_cases as se
from oracle import oracle

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def default_paths(monkeypatch):
    monkeypatch.delenv("QVQ_SEARCH", raising=False)
    monkeypatch.delenv("QVQ_KDTREE", raising=False)


@functools.lru_cache(maxsize=None)
def _want(key):
    X, C = se.assign_case(key)
    want = oracle.kdtree_nn(C, X)
    want.setflags(write=False)
    return want


def _assign(engine, key):
    X, C = se.assign_case(key)
    engine.set_vectors(X)
    A = engine.assign(C)
    flagged = engine.timings()["flagged"][0]
    want = _want(key)
    bad = np.flatnonzero(A != want)
    print(key, "flagged", flagged, "parent", se.golden()[0]["assign_flagged"][key], "rows that differ", len(bad))
    assert len(bad) == 0, (bad[:10], A[bad[:10]], want[bad[:10]])
    assert flagged == se.golden()[0]["assign_flagged"][key]
    return X, C, A, flagged


@pytest.mark.parametrize("cs", list(se.COLOUR))
@pytest.mark.parametrize("K", se.KS)
def test_assign_indices(engine, K, cs):
    """Codebooks whose last tile is full (64 ... 1024) or partly padding (70, 300, 1000), 4- and
    8-code-vector units, a ragged last chunk."""
    X, _, _, flagged = _assign(engine, "idx-K%d-%s" % (K, cs))
    assert len(X) % 64 != 0 and flagged > 0


@pytest.mark.parametrize("cs", list(se.COLOUR))
@pytest.mark.parametrize("K", se.LAST_KS)
def test_rows_on_last_real_code_vector(engine, K, cs):
    """Rows at distance 0 from the last real code vector of every partly padded unit: the padding
    beside it is the only other candidate at its positions."""
    key = "last-K%d-%s" % (K, cs)
    X, C = se.assign_case(key)
    units = [[p for p in u if p < K] for u in se.last_tile_units(K)]
    targets = [u[-1] for u in units if 0 < len(u) < se.unit_size(K)]
    on = [int(np.sum((X == C[p]).all(axis=1))) for p in targets]
    assert targets and min(on) >= 100, (targets, on)
    _assign(engine, key)


@pytest.mark.parametrize("cs", list(se.COLOUR))
@pytest.mark.parametrize("K", se.ONE_KS)
def test_best_unit_with_one_real_code_vector(engine, K, cs):
    """Rows whose nearest code vector is alone in its unit (the rest of it padding): the unit's
    runner-up is the padding's distance, which must not become the row's second distance."""
    key = "one-K%d-%s" % (K, cs)
    X, C = se.assign_case(key)
    assert [p for p in se.last_tile_units(K)[0] if p < K] == [K - 1]
    want = _want(key)
    assert np.sum(want == K - 1) >= 50     # on it, or one table step away in one component
    _assign(engine, key)


@pytest.mark.parametrize("K", (300, 1000))
@pytest.mark.parametrize("cs", list(se.COLOUR))
def test_pruned_indices(engine, K, cs):
    """The same through qvq_refine's searches, which run in the pruned tile order (K >= 256): padding
    positions behind a permuted last tile.  fresh with no iteration: the unfused search (the fp32
    table in LDS); one iteration: the fused one (K = 1000: the fp32 table in HBM)."""
    plan = quant_amd.host_plan(12, K, se.N_ROWS)
    assert plan["search"] == quant_amd.PLAN_SEARCH_MF32 and plan["prune"] == 1
    X = se.image_rows(cs)
    C = se.refine_start(X, K, cs, seed=K)
    want = oracle.kdtree_nn(C, X)
    engine.set_vectors(X)
    C_r, A, _, info = engine.refine(K, C=C, max_iters=0, fresh=True)
    assert info["iters"] == 0 and np.array_equal(C_r, C)
    np.testing.assert_array_equal(A, want)
    C_r, A, _, info = engine.refine(K, C=C, max_iters=1, eps=0.0)
    assert info["iters"] == 1
    np.testing.assert_array_equal(A, want)
    np.testing.assert_array_equal(C_r, oracle.centroids(X, want, K, sum_mode=1))


@pytest.mark.parametrize("K", se.FLAG_KS)
def test_flag_list_overflows(engine, K):
    """Nearly every row a near tie: each workgroup's 1024 rows (the last one's 512) hold more rows
    that any rigorous search must flag (two code vectors within 1e-9 relative) than its LDS list."""
    key = "flat-K%d-scaled" % K
    X, C = se.assign_case(key)
    rows, inv = np.unique(X, axis=0, return_inverse=True)
    tight = (nt.rel_gap(rows, C) < 1e-9)[inv.ravel()]
    per_wg = [int(tight[i:i + se.WG_ROWS].sum()) for i in range(0, len(X), se.WG_ROWS)]
    assert min(per_wg) > se.FLAG_CAP, per_wg
    _, _, _, flagged = _assign(engine, key)
    assert flagged >= int(tight.sum())


@pytest.mark.parametrize("K", se.FLAG_KS)
def test_flag_list_holds_noise(engine, K):
    """Noise rows against a noise codebook with K / 32 pairs 1e-12 apart: the rows nearest to a pair
    must be flagged, and all the flagged rows together are fewer than one workgroup's list holds."""
    key = "noise-K%d-scaled" % K
    paired = int(np.sum(_want(key) < K // 16))
    assert paired >= 50
    _, _, _, flagged = _assign(engine, key)
    assert paired <= flagged < se.FLAG_CAP


def test_lbg_bit_identical_to_parent(engine):
    """Ten levels on a 128 x 128 image: every K from 64 to 1024 with its own variant (fused; pruned
    from K = 256; the fp32 table in LDS up to K = 512)."""
    g, C_parent = se.golden()
    rgb = oracle.gen_image(se.LBG_SIDE)
    engine.set_images(rgb, 1, se.LBG_SIDE, se.LBG_SIDE, 2, 2, quant_amd.SCALED)
    C, A, d = engine.lbg(se.LBG_BITS)
    flagged = [int(v) for v in engine.timings()["flagged"]]
    print("distortion", float(d).hex(), "parent", g["lbg_distortion_hex"], "flagged", flagged, "parent", g["lbg_flagged"])
    assert C.tobytes() == C_parent.tobytes()
    assert float(d).hex() == g["lbg_distortion_hex"]
    # the pruned levels' tile order (prune_order: a bucket's code vectors in arrival order) and with it
    # their count of flagged rows moves by a few rows from run to run, in the parent as well (C3:
    # 8,315 .. 8,343 at K = 256); the unpruned levels' counts repeat
    unpruned = sum(1 for lvl in range(se.LBG_BITS) if (2 << lvl) < 256)
    assert flagged[:unpruned] == g["lbg_flagged"][:unpruned]
    X, _ = oracle.tile(rgb, se.LBG_SIDE, se.LBG_SIDE, 2, 2)
    np.testing.assert_array_equal(A, reference_lbg(X, se.LBG_BITS)[1])
