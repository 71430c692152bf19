"""Every row width and ragged row counts (tests/helpers/shape_cases.py) against the CPU oracle, bit
for bit: all sixteen Dp instantiations of the hot kernels, 0-3 pad bytes, every wide_ks, the three
bodies of mean_sums_kernel; N = 1 ... 8257 on either side of every chunk, group and block size the
kernels cut the rows by; rasters that do not divide into their blocks.  tests/test_shape_plan.py
holds each case to the path it is there for.

References: oracle.kdtree_nn for qvq_assign, oracle.centroids(sum_mode=1) and np.bincount for
qvq_update, oracle.centroids(sum_mode=0) as bits for qvq_update_kahan, reference_lbg for qvq_lbg,
tests/helpers/refine_ref.py for qvq_refine."""
import functools

import numpy as np
import pytest

import quant_amd
from conftest import reference_lbg
from helpers import largek_cases as lk
from helpers import refine_ref as ref
from helpers import shape_cases as sc
from oracle import oracle
from test_gpu_kahan import _cuts
from test_gpu_parity import KAHAN_RTOL

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def default_paths(monkeypatch):
    monkeypatch.delenv("QVQ_SEARCH", raising=False)
    monkeypatch.delenv("QVQ_KDTREE", raising=False)


# -- inputs and the oracle's answers, computed once --------------------------------------------
def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


@functools.lru_cache(maxsize=None)
def _rows(D, N):
    return _frozen(sc.rows(D, N))


@functools.lru_cache(maxsize=None)
def _assign_ref(D, N, K):
    X = _rows(D, N)
    C = sc.codebook(X, K, seed=K + 7 * D)
    return _frozen(C, oracle.kdtree_nn(C, X))


@functools.lru_cache(maxsize=None)
def _lbg_ref(D, N, bits):
    C_e, A_k, d_k, C_k = reference_lbg(_rows(D, N), bits)
    _frozen(C_e, A_k, C_k)
    return C_e, A_k, d_k, C_k


@functools.lru_cache(maxsize=None)
def _refine_ref(D, N, bits):
    X = _rows(D, N)
    return ref.refine(X, *ref.lbg_start(X, bits), max_iters=4, eps=0.0)


def _distortion_bound(X, d_k):
    """tests/test_gpu_kahan.py _check: the closed-form distortion is exact to ~1e-16 of the mean
    square value (cancellation); d_k is exactly 0 where every row has a code vector of its own."""
    return 1e-9 * abs(d_k) + 1e-14 * float(np.mean(X * X))


def _same_as_reference_lbg(X, want, got):
    """test_gpu_parity._check_against_oracle for rows instead of a raster."""
    C_e, A_k, d_k, C_k = want
    C, A, d = got
    assert A.shape == A_k.shape
    np.testing.assert_array_equal(A, A_k)          # reference rule (Kahan centroid bits)
    np.testing.assert_array_equal(C, C_e)          # engine centroid rule on those cells, bit-exact
    assert np.max(np.abs(C - C_k) / np.maximum(np.abs(C_k), 1e-300)) <= KAHAN_RTOL
    print("distortion", d, "reference", d_k)
    assert abs(d - d_k) <= _distortion_bound(X, d_k)


def _check_rows_against_oracle(engine, D, N, bits):
    """qvq_lbg to 0 bits first: its codebook is the mean, mean_sums_kernel's sums over every row
    and nothing else (at the deeper levels a wrong mean shows only where it moves an index)."""
    X = _rows(D, N)
    engine.set_vectors(X)
    _same_as_reference_lbg(X, _lbg_ref(D, N, 0), engine.lbg(0))
    got = engine.lbg(bits)
    _same_as_reference_lbg(X, _lbg_ref(D, N, bits), got)
    return got


# -- the five operations on one training set ---------------------------------------------------
def _assign(engine, monkeypatch, D, N, K, valu=False, host_ties=False):
    X = _rows(D, N)
    C, want = _assign_ref(D, N, K)
    with monkeypatch.context() as m:
        if valu:
            m.setenv("QVQ_SEARCH", "valu")
        if host_ties:
            m.setenv("QVQ_KDTREE", "host")
        engine.set_vectors(X)
        A = engine.assign(C)
        t = engine.timings()
    np.testing.assert_array_equal(A, want, err_msg="D=%d N=%d K=%d valu=%d host=%d" % (D, N, K, valu, host_ties))
    if N >= 64:                           # below that a case need not contain a tie
        assert t["flagged"][0] > 0        # the split pairs: the recheck ran
        assert t["host_ties"][0] > 0      # the duplicate code vectors: the tie path ran


def _update(engine, D, N, K, kind):
    X = _rows(D, N)
    A = lk.assignments(N, K, seed=K + D)[kind]
    engine.set_vectors(X)
    C, cnt = engine.update(A, K)
    np.testing.assert_array_equal(cnt, np.bincount(A, minlength=K))
    np.testing.assert_array_equal(C, oracle.centroids(X, A, K, sum_mode=1))


def _kahan(engine, D, N, bits):
    """qvq_update_kahan on the final assignment of the case's lbg run, whole and cut into ranks."""
    X = _rows(D, N)
    K = 1 << bits
    A = _lbg_ref(D, N, bits)[1]
    want = oracle.centroids(X, A, K, sum_mode=0).view(np.uint64)
    engine.set_vectors(X)
    np.testing.assert_array_equal(engine.update_kahan(A, K).view(np.uint64), want)
    rng = np.random.default_rng(131 * N + D)
    for pieces in (2, 3, 5):
        cuts = _cuts(N, rng, pieces)
        C = engine.update_kahan_split(A, K, cuts)
        np.testing.assert_array_equal(C.view(np.uint64), want, err_msg="cuts %s" % cuts.tolist())


def _refine(engine, D, N, bits, rtol_only):
    """Four iterations with eps = 0 after lbg(bits): the reference loop's run, and the same
    codebook and indices as the loop through qvq_assign / qvq_update."""
    X = _rows(D, N)
    K = 1 << bits
    engine.set_vectors(X)
    engine.lbg(bits)
    C_r, A_r, d_r, info = engine.refine(max_iters=4, eps=0.0)
    C_w, A_w, d_w, want = _refine_ref(D, N, bits)
    assert info["iters"] == want["iters"] and info["stop"] == want["stop"]
    assert info["changed"] == want["changed"]
    assert np.array_equal(A_r, A_w) and np.array_equal(C_r, C_w)
    print("distortion trace", info["distortion"], "reference", want["distortion"])
    if rtol_only:
        np.testing.assert_allclose(info["distortion"], want["distortion"], rtol=1e-9, atol=0)
        assert abs(d_r - d_w) <= 1e-9 * abs(d_w)
    else:       # N <= K: the reference's distortion is exactly 0, the closed form cancels to ~1e-16 of mean(X^2)
        for d, w in zip(info["distortion"] + [d_r], want["distortion"] + [d_w]):
            assert abs(d - w) <= _distortion_bound(X, w)
    C, _, _ = engine.lbg(bits)
    A = None
    for _ in range(info["iters"]):
        A = engine.assign(C)
        C, _ = engine.update(A, K)
    assert np.array_equal(A_r, A) and np.array_equal(C_r, C)


# -- (a) widths ----------------------------------------------------------------------------------
WIDTH = {c["D"]: c for c in sc.WIDTH_CASES}
WIDTH_ASSIGN = [(c["D"], K) for c in sc.WIDTH_CASES for K, _ in c["assign"]]
WIDTH_UPDATE = [(c["D"], K) for c in sc.WIDTH_CASES for K, _ in c["update"]]
WIDTH_LBG = [(c["D"], c["bits"]) for c in sc.WIDTH_CASES] + [(c["D"], c["deep"]["bits"]) for c in sc.WIDTH_CASES
                                                              if c["deep"]]


def _dk(p):
    return "%d-%d" % p


@pytest.mark.parametrize("D,K", WIDTH_ASSIGN, ids=[_dk(p) for p in WIDTH_ASSIGN])
def test_width_assign(engine, monkeypatch, D, K):
    """The default search: VALU below K = 128, the wide MFMA search with the codebook resident
    (K % 32 != 0, and the last resident K) and streamed (the first such K)."""
    _assign(engine, monkeypatch, D, WIDTH[D]["N"], K)
    if K == WIDTH[D]["host_tie_k"]:
        _assign(engine, monkeypatch, D, WIDTH[D]["N"], K, host_ties=True)


@pytest.mark.parametrize("D,K", WIDTH_ASSIGN, ids=[_dk(p) for p in WIDTH_ASSIGN])
def test_width_assign_valu(engine, monkeypatch, D, K):
    _assign(engine, monkeypatch, D, WIDTH[D]["N"], K, valu=True)


@pytest.mark.parametrize("kind", ["uniform", "blocky", "last"])
@pytest.mark.parametrize("D,K", WIDTH_UPDATE, ids=[_dk(p) for p in WIDTH_UPDATE])
def test_width_update(engine, D, K, kind):
    _update(engine, D, WIDTH[D]["N"], K, kind)


@pytest.mark.parametrize("D,bits", WIDTH_LBG, ids=["%d-n%d" % p for p in WIDTH_LBG])
def test_width_lbg(engine, D, bits):
    """bits 8: the VALU and the resident wide search, every level's sums and finalize, the mean;
    the deeper runs end on a streamed, pruned level (rows without image geometry)."""
    _check_rows_against_oracle(engine, D, WIDTH[D]["N"], bits)


@pytest.mark.parametrize("D", sc.WIDTHS)
def test_width_kahan(engine, D):
    _kahan(engine, D, WIDTH[D]["N"], WIDTH[D]["bits"])


@pytest.mark.parametrize("D", sc.REFINE_WIDTHS)
def test_width_refine(engine, D):
    _refine(engine, D, WIDTH[D]["N"], 7, rtol_only=True)


# -- (b) row counts ------------------------------------------------------------------------------
ROWS = [(c["D"], c["N"]) for c in sc.ROW_CASES]
ROW = {(c["D"], c["N"]): c for c in sc.ROW_CASES}
ROW_IDS = ["d%d-n%d" % p for p in ROWS]


@pytest.mark.parametrize("D,N", ROWS, ids=ROW_IDS)
def test_rows_assign(engine, monkeypatch, D, N):
    for K, _ in ROW[(D, N)]["assign"]:
        _assign(engine, monkeypatch, D, N, K)
    _assign(engine, monkeypatch, D, N, ROW[(D, N)]["assign"][1][0], host_ties=True)


@pytest.mark.parametrize("D,N", ROWS, ids=ROW_IDS)
def test_rows_assign_valu(engine, monkeypatch, D, N):
    for K, _ in ROW[(D, N)]["assign"]:
        _assign(engine, monkeypatch, D, N, K, valu=True)


@pytest.mark.parametrize("D,N", ROWS, ids=ROW_IDS)
def test_rows_update(engine, D, N):
    for K, _ in ROW[(D, N)]["update"]:
        for kind in ("uniform", "blocky", "last"):
            _update(engine, D, N, K, kind)


@pytest.mark.parametrize("D,N", ROWS, ids=ROW_IDS)
def test_rows_lbg(engine, D, N):
    """After a run on another N of the same width (alloc_training frees and reallocates), twice in
    a row, and once more after the same rows are set again (alloc_training keeps every buffer): no
    run may see a tail row, a sum or a counter of the one before."""
    bits, other = ROW[(D, N)]["bits"], sc.row_partner(N)
    _check_rows_against_oracle(engine, D, other, ROW[(D, other)]["bits"])
    C, A, d = _check_rows_against_oracle(engine, D, N, bits)
    for again in (engine.lbg(bits), _check_rows_against_oracle(engine, D, N, bits)):
        assert np.array_equal(again[0], C) and np.array_equal(again[1], A) and again[2] == d


@pytest.mark.parametrize("D,N", ROWS, ids=ROW_IDS)
def test_rows_kahan(engine, D, N):
    _kahan(engine, D, N, ROW[(D, N)]["bits"])


@pytest.mark.parametrize("D,N", ROWS, ids=ROW_IDS)
def test_rows_refine(engine, D, N):
    _refine(engine, D, N, min(7, ROW[(D, N)]["bits"]), rtol_only=False)


@pytest.mark.parametrize("N", sc.ROW_NS)
def test_rows_fresh(engine, N):
    """refine(max_iters=0, fresh=True) after lbg: the indices of lbg's codebook, as qvq_assign
    gives them, and their distortion."""
    X = _rows(12, N)
    bits = ROW[(12, N)]["bits"]
    engine.set_vectors(X)
    C_l, _, _ = engine.lbg(bits)
    C, A, d, info = engine.refine(max_iters=0, fresh=True)
    assert info["iters"] == 0 and info["changed"] == [] and np.array_equal(C, C_l)
    np.testing.assert_array_equal(A, oracle.kdtree_nn(C_l, X))
    np.testing.assert_array_equal(A, engine.assign(C_l))
    direct = ref.distortion(X, C_l, A)
    print("fresh distortion", d, "direct", direct)
    assert abs(d - direct) <= _distortion_bound(X, direct)


# -- (c) rasters ---------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _raster_case(name):
    c = next(c for c in sc.RASTER_CASES if c["name"] == name)
    rgb, X = sc.raster_rows(c)
    return c, _frozen(rgb), _frozen(X), reference_lbg(X, c["bits"])


@pytest.mark.parametrize("name", [c["name"] for c in sc.RASTER_CASES])
def test_raster_lbg(engine, name):
    c, rgb, X, want = _raster_case(name)
    cs = quant_amd.NORMAL if c["cs"] == "normal" else quant_amd.SCALED
    engine.set_images(rgb, c["n_images"], c["xs"], c["ys"], c["bw"], c["bh"], cs)
    assert engine.n == X.shape[0] and engine.dim == X.shape[1]
    _same_as_reference_lbg(X, reference_lbg(X, 0), engine.lbg(0))      # the mean alone
    _same_as_reference_lbg(X, want, engine.lbg(c["bits"]))


def test_raster_unaligned_device_pointer(engine):
    """qvq_set_images_device at an odd address: tile22_kernel's dword loads are out, tile_kernel
    takes the raster and gives the same rows."""
    import torch
    c, rgb, X, want = _raster_case(sc.UNALIGNED_RASTER)
    engine.set_images(rgb, c["n_images"], c["xs"], c["ys"], c["bw"], c["bh"], quant_amd.SCALED)
    aligned = engine.lbg(c["bits"])
    buf = torch.zeros(rgb.size + 1, dtype=torch.uint8, device="cuda")
    buf[1:] = torch.from_numpy(np.array(rgb)).to("cuda")
    torch.cuda.synchronize()
    assert buf.data_ptr() % 4 == 0
    engine.set_vectors(_rows(12, 64))      # another training set in between: the rows are tiled again
    engine.set_images_device(buf.data_ptr() + 1, c["n_images"], c["xs"], c["ys"], c["bw"], c["bh"], quant_amd.SCALED)
    got = engine.lbg(c["bits"])
    _same_as_reference_lbg(X, want, got)
    assert np.array_equal(got[0], aligned[0]) and np.array_equal(got[1], aligned[1]) and got[2] == aligned[2]
