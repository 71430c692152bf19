"""Near-tie rows on every search and recheck path (tests/helpers/neartie_cases.py):
codebooks of code vector pairs whose distances to a row differ by 1e-17 ... 1e-3 relative, against
the CPU oracle bit for bit.  In that band an fp32 threshold that is too small loses a row, the
recheck's fp64 summation order decides the index, and the reference's kd-tree answer is not always
the fp64 argmin.  tests/test_neartie_plan.py holds each case to its path, the band to its coverage
and the oracle to the compiled reference's recorded answers.

Reference: oracle.kdtree_nn (the reference's kd-tree answer, src/Quantizer.cpp:24-32) for the
indices, oracle.centroids(sum_mode=1) for the refined codebook, the closed form over long-double
cell sums for the distortion."""
import functools

import numpy as np
import pytest

import quant_amd
from helpers import neartie_cases as nt
from oracle import oracle

pytestmark = pytest.mark.gpu
QVQ_OK, QVQ_EINVAL = 0, 1
REFINE_CASES = [c for c in nt.CASES if c["refine"]]


@functools.lru_cache(maxsize=None)
def _case(k):
    """(rows, codebook, the reference's indices, the relative gap of every row), once per case."""
    c = next(c for c in nt.CASES if nt.key(c) == k)
    X, C = nt.inputs(c)
    want = oracle.kdtree_nn(C, X)
    gap = nt.rel_gap(X, C)
    want.setflags(write=False)
    gap.setflags(write=False)
    return X, C, want, gap


def _knobs(monkeypatch, search, kd):
    for name, value in (("QVQ_SEARCH", search), ("QVQ_KDTREE", kd)):
        if value in (None, "default"):
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, value)


def _explain(X, C, A, want, gap, t):
    """The failing rows: index, the two nearest code vectors, the relative gap, and the stage that
    owed the row its index (the kd walk below 1e-12 relative, the recheck above), beside the
    call's counts of flagged rows and kd-tree rows."""
    bad = np.flatnonzero(A != want)
    _, _, i1, i2 = nt.top_two(X[bad[:20]], C)
    lines = ["%d of %d rows differ; flagged %d, kd-tree rows %d" % (len(bad), len(A), t["flagged"][0], t["host_ties"][0])]
    for j, r in enumerate(bad[:20]):
        stage = "kd walk" if gap[r] <= 1e-12 else "flag + recheck"
        lines.append("row %d: got %d, reference %d; nearest two %d, %d; relative gap %.3e (%s)"
                     % (r, A[r], want[r], i1[j], i2[j], float(gap[r]), stage))
    return "\n".join(lines)


def _assign_and_check(engine, case):
    X, C, want, gap = _case(nt.key(case))
    engine.set_vectors(X)
    A = engine.assign(C)
    t = engine.timings()
    assert np.array_equal(A, want), _explain(X, C, A, want, gap, t)
    # fp32 cannot separate two distances within 1e-9 relative: a rigorous search flags those rows
    close = int(np.sum(gap < 1e-9))
    print("flagged", t["flagged"][0], "rows within 1e-9:", close, "kd-tree rows", t["host_ties"][0])
    assert close > 0 and t["flagged"][0] >= close
    assert t["host_ties"][0] > 0


@pytest.mark.parametrize("kd", ["default", "host"])
@pytest.mark.parametrize("case", nt.CASES, ids=nt.key)
def test_assign(engine, monkeypatch, case, kd):
    """The default search and recheck of every case; ties by the default path and by the host."""
    _knobs(monkeypatch, None, kd)
    _assign_and_check(engine, case)


@pytest.mark.parametrize("kd", ["default", "host"])
@pytest.mark.parametrize("case", [c for c in nt.CASES if c["K"] > 32], ids=nt.key)
def test_assign_valu(engine, monkeypatch, case, kd):
    """The same under QVQ_SEARCH=valu: valu_coeffs' bounds at every width of the table."""
    _knobs(monkeypatch, "valu", kd)
    _assign_and_check(engine, case)


def _closed_form(X, C, A):
    """The distortion from the cells' sums: (sum |x|^2 - 2 sum_k c_k . S_k + sum_k n_k |c_k|^2) / (N D)."""
    K = C.shape[0]
    Xl, Cl = X.astype(np.longdouble), C.astype(np.longdouble)
    S = np.zeros(C.shape, np.longdouble)
    np.add.at(S, A.astype(np.int64), Xl)
    n = np.bincount(A, minlength=K).astype(np.longdouble)
    return float(((Xl * Xl).sum() - 2 * (Cl * S).sum() + (n * (Cl * Cl).sum(axis=1)).sum()) / X.size)


@pytest.mark.parametrize("case", REFINE_CASES, ids=nt.key)
def test_refine_fresh(engine, monkeypatch, case):
    """The indices of the caller's codebook through qvq_refine's pruned / fused searches."""
    _knobs(monkeypatch, None, None)
    X, C, want, gap = _case(nt.key(case))
    engine.set_vectors(X)
    C_r, A, d, info = engine.refine(case["K"], C=C, max_iters=0, fresh=True)
    assert info["iters"] == 0 and np.array_equal(C_r, C)
    assert np.array_equal(A, want), _explain(X, C, A, want, gap, engine.timings())
    d_w = _closed_form(X, C, want)
    print("distortion", d, "closed form", d_w)
    assert abs(d - d_w) <= 1e-9 * d_w


@pytest.mark.parametrize("case", REFINE_CASES, ids=nt.key)
def test_refine_one_step(engine, monkeypatch, case):
    """One iteration from the caller's codebook: every row is new, and the hundreds of rows the
    recheck and the kd walk move go through the fused sums' correction slabs."""
    _knobs(monkeypatch, None, None)
    X, C, want, gap = _case(nt.key(case))
    engine.set_vectors(X)
    C_r, A, _, info = engine.refine(case["K"], C=C, max_iters=1, eps=0.0)
    assert info["iters"] == 1 and info["changed"] == [len(X)]
    assert np.array_equal(A, want), _explain(X, C, A, want, gap, engine.timings())
    assert np.array_equal(C_r, oracle.centroids(X, want, case["K"], sum_mode=1))


def _raw_assign(engine, C, A):
    C = np.ascontiguousarray(C, np.float64)
    return quant_amd.lib().qvq_assign(engine._h, quant_amd._p(C), C.shape[0], quant_amd._p(A))


@pytest.mark.parametrize("cs", ["scaled", "normal"])
def test_assign_rejects_out_of_range(engine, monkeypatch, cs):
    """qvq_assign on a byte-path training set refuses a codebook with a component outside
    [min(1.2 vmin, 0.8 vmin), max(1.2 vmax, 0.8 vmax)], NaN included (the range the near-tie
    thresholds are worked out for), and writes nothing; the range's own end and exact mode pass."""
    _knobs(monkeypatch, None, None)
    X, C, _, _ = _case("D12-K100-%s-near" % cs)
    lut = oracle.lut(nt.COLOUR[cs])
    vmin, vmax = lut.min(), lut.max()
    engine.set_vectors(X)
    for row in (0, len(C) - 1):
        for bad in (2 * vmax, 1.2 * vmin - 1, np.nan, np.inf):
            Cb = C.copy()
            Cb[row, 5] = bad
            A = np.full(len(X), 0xA5A5A5A5, np.uint32)
            assert _raw_assign(engine, Cb, A) == QVQ_EINVAL, (row, bad)
            assert (A == 0xA5A5A5A5).all(), "assign written on a refused codebook"
            with pytest.raises(quant_amd.QVQError) as e:
                engine.assign(Cb)
            assert e.value.status == QVQ_EINVAL
        Cb = C.copy()
        Cb[row, 5] = 1.2 * vmax          # the end of the range itself
        np.testing.assert_array_equal(engine.assign(Cb), oracle.kdtree_nn(Cb, X))
    # exact mode runs no fp32 search: any codebook, as tests/test_gpu_exact.py test_single_steps
    rng = np.random.default_rng(11)
    Xe, Ce = rng.normal(size=(4000, 12)), rng.normal(size=(37, 12)) * 3
    engine.set_vectors(Xe)
    np.testing.assert_array_equal(engine.assign(Ce), oracle.kdtree_nn(Ce, Xe))
