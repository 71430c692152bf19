"""The pruned searches where their projection bound is tight (tests/helpers/prune_cases.py,
DESIGN.md 6.6): station codebooks whose answers lie along the all-ones direction from their rows,
so that ||x - c||^2 >= sx^2 (sum w - q_c)^2 / D holds with equality and a window a few per cent
too narrow loses rows -- with no flag, and nothing downstream to repair them.  Through qvq_refine
from the caller's codebook: the unfused pruned search (max_iters = 0, fresh indices) and the fused
one (one iteration), the D = 12 MFMA search, the wide search with and without image geometry, and
the chunked recheck's pruned sweep.  tests/test_prune_plan.py holds every case to its plan and to
the numpy model of the rule (tests/helpers/prune_ref.py) on the CPU.

Reference: oracle.kdtree_nn (the reference's kd-tree answer, src/Quantizer.cpp:24-32) for the
indices, oracle.centroids(sum_mode=1) for the refined codebook, the closed form over long-double
cell sums for the distortion."""
import functools

import numpy as np
import pytest

import quant_amd
from conftest import reference_lbg
from helpers import neartie_cases as nt
from helpers import prune_cases as pc
from helpers import prune_ref as pr
from oracle import oracle
from test_gpu_neartie import _closed_form

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _case(k):
    """(rows, codebook, the reference's indices, the relative gap of every row), once per case."""
    c = next(c for c in pc.CASES if pc.key(c) == k)
    X, C, _ = pc.inputs(c)
    want = oracle.kdtree_nn(C, X)
    gap = nt.rel_gap(X, C)
    want.setflags(write=False)
    gap.setflags(write=False)
    return X, C, want, gap


def _load(engine, case):
    X = pc.inputs(case)[0]
    if case["geometry"]:
        xs, ys = case["geometry"]
        engine.set_images(pc.raster(case), 1, xs, ys, 4, 4,
                          quant_amd.SCALED if case["cs"] == "scaled" else quant_amd.NORMAL)
        assert engine.n == len(X) and engine.dim == X.shape[1]
    else:
        engine.set_vectors(X)


def _explain(engine, case, A, want):
    """The failing rows: index, the two nearest code vectors, their projections and the row's
    sum w, the tile the model puts the answer in, the model's window for the row's chunk, and
    whether the unpruned search (qvq_assign) agrees with the oracle on that row -- which tells a
    failure of the bound from a failure of the search."""
    X, C, _, gap = _case(pc.key(case))
    cs = pc.COLOUR[case["cs"]]
    bad = np.flatnonzero(A != want)
    t = engine.timings()
    lines = ["%s: %d of %d rows differ; flagged %d, kd-tree rows %d"
             % (pc.key(case), len(bad), len(A), t["flagged"][0], t["host_ties"][0])]
    res = pr.search(X, C, cs, case["kind"], case["cpr"], margin=True)
    tile = pr.tile_of(res.perm)
    q = pr.projections(C, cs)
    plain = engine.assign(C)
    _, _, i1, i2 = nt.top_two(X[bad[:12]], C)
    for j, r in enumerate(bad[:12]):
        lines.append("row %d (chunk %d, row %d of it): got %d, reference %d; nearest two %d (q %.2f), %d (q %.2f), "
                     "relative gap %.3e; sum w %d; model: answer in tile %d, first tile %d, window %d..%d of %d "
                     "tiles; unpruned search %s"
                     % (r, r // 64, r % 64, A[r], want[r], i1[j], q[i1[j]], i2[j], q[i2[j]], float(gap[r]),
                        res.qw[r], tile[want[r]], res.first[r], res.window[r, 0], res.window[r, 1], res.tiles,
                        "agrees with the reference" if plain[r] == want[r] else "gives %d" % plain[r]))
    return "\n".join(lines)


@pytest.mark.parametrize("case", pc.CASES, ids=pc.key)
def test_refine_fresh(engine, monkeypatch, case):
    """The indices of the caller's codebook through the unfused pruned search."""
    monkeypatch.delenv("QVQ_SEARCH", raising=False)
    monkeypatch.delenv("QVQ_KDTREE", raising=False)
    X, C, want, gap = _case(pc.key(case))
    _load(engine, case)
    C_r, A, d, info = engine.refine(case["K"], C=C, max_iters=0, fresh=True)
    assert info["iters"] == 0 and np.array_equal(C_r, C)
    assert np.array_equal(A, want), _explain(engine, case, A, want)
    d_w = _closed_form(X, C, want)
    print("distortion", d, "closed form", d_w)
    assert abs(d - d_w) <= 1e-9 * d_w
    if case["has_ties"]:
        # fp32 cannot separate two distances within 1e-9 relative: both lie in far tiles on
        # opposite sides of the row, and a window that holds only one of them raises no flag.
        # qvq_refine reports no flag count (qvq_get_timings covers qvq_lbg and qvq_assign), so the
        # pruned search's flags show in its indices: the reference's rule picks the lo vector on
        # some tie rows and the hi vector on others (tests/test_prune_plan.py), which no search
        # that skips the flag reproduces.  The count itself is asserted on qvq_assign's report.
        close = int(np.sum(gap < 1e-9))
        A2 = engine.assign(C)
        t = engine.timings()
        print("flagged", t["flagged"][0], "rows within 1e-9:", close, "kd-tree rows", t["host_ties"][0])
        assert np.array_equal(A2, want)
        assert close > 0 and t["flagged"][0] >= close


@pytest.mark.parametrize("case", pc.CASES, ids=pc.key)
def test_refine_one_step(engine, monkeypatch, case):
    """One iteration from the caller's codebook: the pruned search with the sums riding in it
    where the plan fuses, every row new."""
    monkeypatch.delenv("QVQ_SEARCH", raising=False)
    monkeypatch.delenv("QVQ_KDTREE", raising=False)
    X, C, want, _ = _case(pc.key(case))
    _load(engine, case)
    C_r, A, _, info = engine.refine(case["K"], C=C, max_iters=1, eps=0.0)
    assert info["iters"] == 1 and info["changed"] == [len(X)]
    assert np.array_equal(A, want), _explain(engine, case, A, want)
    assert np.array_equal(C_r, oracle.centroids(X, want, case["K"], sum_mode=1))


@pytest.mark.parametrize("image", pc.LBG_IMAGES, ids=lambda i: i["name"])
def test_lbg_levels(engine, image):
    """qvq_lbg's own pruned levels (split codebooks up to 1.2 vmax, which no caller can hand to
    qvq_refine) on the images the model finds sharpest: as tests/test_gpu_prune.py asserts."""
    rgb, S, b = pc.lbg_raster(image), image["S"], image["block"]
    X, _ = oracle.tile(rgb, S, S, b, b)
    C_e, A_k, d_k, _ = reference_lbg(X, image["bits"])
    engine.set_images(rgb, 1, S, S, b, b, quant_amd.SCALED)
    C, A, d = engine.lbg(image["bits"])
    np.testing.assert_array_equal(A, A_k)
    np.testing.assert_array_equal(C, C_e)
    assert abs(d - d_k) <= 1e-9 * abs(d_k)
