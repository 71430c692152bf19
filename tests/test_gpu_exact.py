"""Exact mode (VERDICT r02 missing #2): the AbstractQuantizer path accepts any training set, as the
reference's `quantize(const std::vector<Vector>&, n, eps)` does (include/Quantizer.hpp:10-16).
Values that are not byte images of a colour space -- random doubles, CIE1931-like values, other
dimensions -- go through qvq_set_vectors' exact mode: fp64 search in nanoflann's order with
kd-tree ties (src/Quantizer.cpp:24-32), Kahan sums of each cell's rows in ascending order times
fl(1/n) (src/Quantizer.cpp:46-87).  The bar is bit-identity with the oracle's Kahan rule
(oracle.lbg(sum_mode=0), the reference's arithmetic): indices AND codebook; the distortion (an
OpenMP reduction in the reference, order-dependent in its last bits) within 1e-12 relative.
Byte-image data can be forced through the same mode (exact=True) and then also matches the
reference's Kahan codebook bit for bit, where the fast path's exact sums are within 1 ulp."""
import numpy as np
import pytest

from oracle import oracle

pytestmark = pytest.mark.gpu


def _check(engine, X, bits, exact=False):
    C_r, A_r, d_r = oracle.lbg(X, bits, sum_mode=0)
    engine.set_vectors(X, exact=exact)
    C, A, d = engine.lbg(bits)
    np.testing.assert_array_equal(A, A_r)
    np.testing.assert_array_equal(C, C_r)
    assert abs(d - d_r) <= 1e-12 * abs(d_r)
    return C, A


@pytest.mark.parametrize("D,N,bits", [(12, 6000, 7), (3, 5000, 6), (48, 1500, 5), (1, 777, 4), (20, 333, 9)])
def test_random_fp64_data(engine, D, N, bits):
    rng = np.random.default_rng(D * 1000 + N)
    X = rng.normal(size=(N, D)) * rng.uniform(0.1, 10, size=D) + rng.uniform(-5, 5, size=D)
    _check(engine, X, bits)


def test_cie_like_values(engine):
    """The reference's CIE1931 map (src/ColorSpace.cpp:30-38) applied to every pixel of the 2x2
    blocks: values off the 2^-60 grid, so only the exact mode can take them."""
    X, _ = oracle.tile(oracle.gen_image(64, 0x5EED), 64, 64, 2, 2, cs=oracle.NORMAL)   # signed chars
    p = X.reshape(-1, 3)
    xyz = np.stack([(p[:, 0] * 0.490 + p[:, 1] * 0.310 + p[:, 2] * 0.200) / 0.17697,
                    (p[:, 0] * 0.17697 + p[:, 1] * 0.81240 + p[:, 2] * 0.01063) / 0.17697,
                    (p[:, 0] * 0 + p[:, 1] * 0.01 + p[:, 2] * 0.99) / 0.17697], axis=1)
    _check(engine, xyz.reshape(-1, 12), 8)


def test_duplicates_and_ties(engine):
    """Repeated rows, repeated code vectors (zero rows split to equal code vectors) and exact
    distance ties: the kd-tree's first-visited rule decides, as in the reference."""
    rng = np.random.default_rng(5)
    base = rng.integers(0, 4, size=(40, 6)).astype(np.float64) * 0.25
    X = np.concatenate([base[rng.integers(0, 40, size=3000)], np.zeros((200, 6))])
    _check(engine, X, 7)


def test_byte_data_forced_exact_matches_kahan_bits(engine):
    """beans-like byte data through the exact mode: the Kahan codebook bit for bit (the fast path
    agrees with it to <= 1 ulp and on every index)."""
    X, _ = oracle.tile(oracle.gen_image(128, 0x5EED), 128, 128, 2, 2)
    C_e, A_e = _check(engine, X, 8, exact=True)
    engine.set_vectors(X)
    C_f, A_f, _ = engine.lbg(8)
    np.testing.assert_array_equal(A_f, A_e)
    np.testing.assert_allclose(C_f, C_e, rtol=4e-16, atol=0)


def test_single_steps(engine):
    """qvq_assign / qvq_update in exact mode: the oracle's kd-tree answer and Kahan centroids."""
    rng = np.random.default_rng(11)
    X = rng.normal(size=(4000, 12))
    C = rng.normal(size=(37, 12))
    engine.set_vectors(X)
    A = engine.assign(C)
    np.testing.assert_array_equal(A, oracle.kdtree_nn(C, X))
    C2, cnt = engine.update(A, 37)
    np.testing.assert_array_equal(C2, oracle.centroids(X, A, 37, sum_mode=0))
    np.testing.assert_array_equal(cnt, np.bincount(A, minlength=37))


def test_lbg_quantizer_plugin_generic(engine):
    """getQuantizer(LBG).quantize on arbitrary vectors (the drop-in's generic callers)."""
    import quant_amd
    rng = np.random.default_rng(2)
    X = rng.uniform(-1, 1, size=(2000, 4))
    C, A, d = quant_amd.getQuantizer(quant_amd.Quantizers.LBG).quantize(X, 5, 1e-6)
    C_r, A_r, d_r = oracle.lbg(X, 5, sum_mode=0)
    np.testing.assert_array_equal(A, A_r)
    np.testing.assert_array_equal(C, C_r)


# ---------------------------------------------------------------------------------------------
# Exact mode at its chunk, tile and grid edges.  The cases, and what each is there
# for, are in tests/helpers/exact_cases.py; tests/test_exact_plan.py holds them to the engine's
# dispatch (quant_amd.host_exact_plan) and to their own claims on the CPU.
# ---------------------------------------------------------------------------------------------
import math  # noqa: E402

from conftest import reference_lbg  # noqa: E402
from helpers import exact_cases as ex  # noqa: E402
from helpers import shape_cases as sc  # noqa: E402


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _explain_assign(engine, case, X, C, A, A_ref):
    """The first wrong row of an assignment: its best two fp64 distances, the chunks they and the
    two answers lie in, and the rows the engine sent to the host kd-tree."""
    kc = case["plan"]["kc"]
    row = int(np.flatnonzero(A != A_ref)[0])
    d = ex.sqdist(X[row:row + 1], C)[0]
    o = np.argsort(d, kind="stable")[:2]
    return ("%s: %d rows differ; row %d: engine %d (chunk %d, d = %.17g), oracle %d (chunk %d, d = %.17g); best two "
            "d1 = %.17g at %d (chunk %d), d2 = %.17g at %d (chunk %d), (d2 - d1) / d1 = %.3g; kc = %d; host_ties = %d"
            % (case["key"], int(np.sum(A != A_ref)), row, A[row], A[row] // kc, d[A[row]] if A[row] < len(C) else -1.0,
               A_ref[row], A_ref[row] // kc, d[A_ref[row]], d[o[0]], o[0], o[0] // kc, d[o[1]], o[1], o[1] // kc,
               (d[o[1]] - d[o[0]]) / d[o[0]] if d[o[0]] else np.inf, kc, engine.timings()["host_ties"][0]))


@pytest.mark.parametrize("case", ex.CHUNK_CASES + ex.NEARTIE_CASES, ids=ex.key)
def test_assign_at_chunk_edges_and_near_ties(engine, case):
    """qvq_assign with K at and around the multiples of the LDS chunk, on every instantiation of the
    search, and with pairs of code vectors on both sides of tie_rel, the nearer one at the higher
    index and in a later chunk: the indices are oracle.kdtree_nn's.  The near-tie cases go in
    through qvq_set_vectors' fallback, the chunk cases through qvq_set_vectors_exact."""
    X, C = ex.inputs(case)[:2]
    A_ref = ex.oracle_nn(case)
    engine.set_vectors(X, exact=case["key"].startswith("chunk-"))
    A = engine.assign(C)
    if not np.array_equal(A, A_ref):
        msg = _explain_assign(engine, case, X, C, A, A_ref)
        print(msg)
        pytest.fail(msg)


@pytest.mark.parametrize("case", ex.CHAIN_CASES, ids=ex.key)
def test_update_at_tile_edges(engine, case):
    """qvq_update with one cell of every size around the chains' unroll width and tile, on data
    whose sums show a plain sum, a reversed one and a compensation restarted per tile: the codebook
    is oracle.centroids(sum_mode=0) as bits."""
    X, A = ex.inputs(case)
    engine.set_vectors(X, exact=True)
    C, cnt = engine.update(A, case["K"])
    C_r = oracle.centroids(X, A, case["K"], sum_mode=0)
    bad = np.argwhere(_bits(C) != _bits(C_r))
    sizes = np.bincount(A, minlength=case["K"])
    assert len(bad) == 0, "%s: %d components differ, first in the cell of %d rows (T = %d): %r != %r" % (
        case["key"], len(bad), sizes[bad[0][0]], case["plan"]["tile_rows"], C[tuple(bad[0])], C_r[tuple(bad[0])])
    np.testing.assert_array_equal(cnt, sizes)


def _check_ref(engine, X, bits, ref, d_abs=None):
    """_check against a reference computed once (ex.oracle_lbg): indices equal, codebook equal as
    bits, distortion within 1e-12 relative (d_abs: absolutely, where it can be 0)."""
    C_r, A_r, d_r = ref
    engine.set_vectors(X, exact=True)
    C, A, d = engine.lbg(bits)
    np.testing.assert_array_equal(A, A_r)
    assert np.array_equal(_bits(C), _bits(C_r)), "%d codebook components differ" % int(np.sum(_bits(C) != _bits(C_r)))
    print("distortion %.17g, oracle %.17g" % (d, d_r))
    assert abs(d - d_r) <= (d_abs if d_abs is not None else 1e-12 * abs(d_r))
    return C, A, d


@pytest.mark.parametrize("case", ex.ROW_CASES + ex.MEAN_CASES, ids=ex.key)
def test_lbg_ragged_rows_and_mean_chain(engine, case):
    """qvq_lbg on 1 ... 1025 rows with more code vectors than rows up to N = 257 (empty cells,
    their zero code vectors and the ties those make), and on N at the mean chain's tile edges, to
    the mean itself (bits = 0) and its split (bits = 1)."""
    X = ex.inputs(case)
    # N <= 3: every row can end alone in its cell, distortion 0: absolute, on the scale of the data
    d_abs = 1e-12 * float(np.mean(X * X)) if case["N"] <= 3 else None
    _check_ref(engine, X, case["bits"], ex.oracle_lbg(case), d_abs)


def test_lbg_past_every_grid_cap(engine):
    """2^21 + 257 rows: the search, the row-number fill and the distortion each take their
    grid-stride loop more than once.  The distortion against math.fsum over the oracle's cells: the
    engine adds at most 9 rows per thread, 8 tree steps and 1024 partials in sequence, under
    1100 * 2^-53 = 1.2e-13 relative, so 1e-12 has margin."""
    case = ex.STRIDE_CASE
    X = ex.inputs(case)
    C_r, A_r, _ = ex.oracle_lbg(case)
    e = X - C_r[A_r]
    d_fsum = math.fsum((e * e).ravel()) / (float(case["N"]) * case["D"])
    _check_ref(engine, X, case["bits"], (C_r, A_r, d_fsum))


def test_lbg_scaled_by_powers_of_two(engine):
    """The rows times 2^100 and 2^-100: every operation of the mode scales exactly, so the indices
    are the unscaled run's and the codebook is the unscaled one times the factor, bit for bit."""
    case = ex.SCALE_CASE
    X = ex.inputs(case)
    C1, A1, _ = _check_ref(engine, X, case["bits"], ex.oracle_lbg(case))
    for s in ex.SCALES:
        C, A, _ = _check_ref(engine, X * s, case["bits"], ex.oracle_lbg(case, s))
        np.testing.assert_array_equal(A, A1)
        assert np.array_equal(_bits(C), _bits(C1 * s))


def test_lifecycle_exact_byte_exact(engine):
    """One context through exact -> byte -> exact training sets: everything is reallocated at each
    switch while the chains' offset table and the tie scratch only ever grow; every step against
    the oracle."""
    rng = np.random.default_rng(2024)
    X1 = ex.gaussian_rows(3000, 12, 2024)

    def step(X, K):
        C = X[rng.choice(len(X), K)] + rng.normal(size=(K, X.shape[1])) * 0.3
        A = engine.assign(C)
        np.testing.assert_array_equal(A, oracle.kdtree_nn(C, X))
        C2, cnt = engine.update(A, K)
        assert np.array_equal(_bits(C2), _bits(oracle.centroids(X, A, K, sum_mode=0)))
        np.testing.assert_array_equal(cnt, np.bincount(A, minlength=K))
        return C, A

    engine.set_vectors(X1, exact=True)
    C37, A37 = step(X1, 37)                      # 1. the whole-codebook path
    step(X1, 1400)                               # 2. three chunks; the offset table grows
    step(X1, 5)                                  # 3. and is kept
    Xb = sc.vectors(1777, 12, 5)                 # 4. a byte training set of another N
    C_e, A_k, d_k, _ = reference_lbg(Xb, 6)
    engine.set_vectors(Xb)
    C, A, d = engine.lbg(6)
    np.testing.assert_array_equal(A, A_k)
    np.testing.assert_array_equal(C, C_e)
    assert abs(d - d_k) <= 1e-9 * abs(d_k)
    base = rng.normal(size=(6, 48))              # 5. every row an exact tie: the tie scratch grows
    X5 = base[rng.integers(0, 6, 700)]
    C5 = np.concatenate([base, base[::-1]])
    engine.set_vectors(X5, exact=True)
    A = engine.assign(C5)
    assert engine.timings()["host_ties"][0] == 700
    np.testing.assert_array_equal(A, oracle.kdtree_nn(C5, X5))
    C_r, A_r, d_r = oracle.lbg(X5, 4, sum_mode=0)
    C, A, d = engine.lbg(4)
    np.testing.assert_array_equal(A, A_r)
    assert np.array_equal(_bits(C), _bits(C_r))
    _check(engine, X1, 5, exact=True)            # 6. the first set again
    np.testing.assert_array_equal(engine.assign(C37), A37)
