"""QVQ_REFINE_RESEED (include/qvq.h) on the device against the restatement of
tests/helpers/reseed_ref.py: indices, codebook, changed and reseeded counts bit for bit, iters and
stop equal, the distortion and its trace within 1e-9 relative (the closed form against the direct
sum, the tolerance of tests/test_gpu_refine.py)."""
import ctypes
import functools
import json
import os
import subprocess

import numpy as np
import pytest

import quant_amd
from conftest import GOLDEN, ROOT
from helpers import refine_ref
from helpers import reseed_ref as ref
from oracle import oracle

pytestmark = pytest.mark.gpu
QUANT = os.path.join(ROOT, "quant_amd", "lib", "quant")
QVQ_EINVAL, QVQ_EUNSUPPORTED, QVQ_ESTATE = 1, 5, 6
with open(os.path.join(GOLDEN, "refine_reseed_trace.json")) as _f:
    TRACE = json.load(_f)


def same_run(got, want):
    C, A, d, info = got
    C_r, A_r, d_r, info_r = want
    print("reseeded", info["reseeded"], "reference", info_r["reseeded"])
    print("distortion trace", info["distortion"], "reference", info_r["distortion"])
    assert info["iters"] == info_r["iters"] and info["stop"] == info_r["stop"]
    assert info["changed"] == info_r["changed"]
    assert info["reseeded"] == info_r["reseeded"]
    assert np.array_equal(A, A_r), "indices differ from the restatement"
    assert np.array_equal(C, C_r), "codebook differs from the restatement"
    np.testing.assert_allclose(info["distortion"], info_r["distortion"], rtol=1e-9, atol=0)
    assert abs(d - d_r) <= 1e-9 * abs(d_r)


def lbg_on(engine, name):
    S, b, bits, cs = ref.CASES[name]
    engine.set_images(oracle.gen_image(S), 1, S, S, b, b, cs)
    return engine.lbg(bits)


@functools.lru_cache(maxsize=None)
def table_rows(n, dim, cs, seed):
    """n rows of byte-image values, drawn from a narrow band of the table (so that cells hold
    many rows) with a few rows anywhere."""
    rng = np.random.default_rng(seed)
    tab = np.sort(quant_amd.colorspace_values(cs))
    idx = rng.integers(96, 160, (n, dim))
    wide = rng.random(n) < 0.1
    idx[wide] = rng.integers(0, 256, (int(wide.sum()), dim))
    return np.ascontiguousarray(tab[idx])


def duplicate_start(X, K, distinct):
    """K code vectors: `distinct` different rows of X, the others copies of the first."""
    _, first = np.unique(X, axis=0, return_index=True)
    rows = X[np.sort(first)[:distinct]]   # (the first `distinct` distinct rows, in row order)
    assert len(rows) == distinct
    C = np.repeat(rows[0][None, :], K, axis=0)
    C[:distinct] = rows
    return np.ascontiguousarray(C)


@pytest.mark.parametrize("name", ["s128_b2_6_scaled",    # D = 12, K = 64: the MFMA search with fused sums; 4 seeds
                                  "s96_b4_5_scaled",     # D = 48: the counting-sort sums; 1 seed
                                  "s128_b2_10_scaled",   # K = 1024: the pruned search; [438, 5] seeds
                                  "s128_b2_10_normal"])  # NORMAL: [269, 4] seeds
def test_cases_against_restatement(engine, name):
    w = TRACE[name]
    lbg_on(engine, name)
    got = engine.refine(max_iters=w["max_iters"], eps=0.0, reseed=True)
    want = ref.run_case(name, w["max_iters"])[2]
    assert got[3]["reseeded"] == w["reseeded"] and sum(w["reseeded"]) > 0
    assert got[3]["iters"] == w["iters"] and got[3]["stop"] == w["stop"] and got[3]["changed"] == w["changed"]
    same_run(got, want)
    assert ref.empty_cells(got[1], got[0].shape[0]) == w["empty_last"] == 0


@pytest.mark.parametrize("name", ["s64_b2_4_scaled", "s64_b2_4_normal", "s128_b2_6_normal"])
def test_without_empties_the_flag_changes_nothing(engine, name):
    lbg_on(engine, name)
    C0, A0, d0, i0 = engine.refine(max_iters=40, eps=0.0)
    assert i0["reseeded"] == [0] * i0["iters"]
    lbg_on(engine, name)
    C1, A1, d1, i1 = engine.refine(max_iters=40, eps=0.0, reseed=True)
    assert i1["reseeded"] == [0] * i1["iters"] == TRACE[name]["reseeded"]
    assert np.array_equal(C0, C1) and np.array_equal(A0, A1) and d0 == d1
    assert i0 == i1   # iters, stop, changed and the distortion trace, bit for bit
    same_run((C1, A1, d1, i1), ref.run_case(name)[2])


def test_small_k_scan_duplicate_warm_start(engine):
    S, b, bits, cs = ref.CASES["s64_b2_4_scaled"]
    X, (C0, _, _), _ = ref.run_case("s64_b2_4_scaled")
    C_start = C0.copy()
    C_start[10:] = C_start[0]
    want = ref.refine(X, C_start, cs, max_iters=6, eps=0.0)
    assert want[3]["reseeded"][0] == 6 and not any(want[3]["reseeded"][1:])
    engine.set_images(oracle.gen_image(S), 1, S, S, b, b, cs)
    same_run(engine.refine(C=C_start, max_iters=6, eps=0.0, reseed=True), want)


def test_no_donor(engine):
    """7 identical rows, 4 copies of the row as the codebook: one cell of E = 0, three empty ones."""
    # (NORMAL: integers, so that the closed-form distortion of the one cell is exactly 0)
    row = np.sort(quant_amd.colorspace_values(quant_amd.NORMAL))[np.arange(12) * 7 + 3]
    X = np.repeat(row[None, :], 7, axis=0)
    C_start = np.repeat(row[None, :], 4, axis=0)
    engine.set_vectors(X)
    C, A, d, info = engine.refine(C=C_start, max_iters=10, eps=0.0, reseed=True)
    assert info["reseeded"] == [0, 0] and info["iters"] == 2 and info["stop"] == quant_amd.STOP_FIXED
    assert info["changed"] == [7, 0]
    assert ref.empty_cells(A, 4) == 3 and d == 0.0
    same_run((C, A, d, info), ref.refine(X, C_start, ref.NORMAL, max_iters=10, eps=0.0))


@pytest.mark.parametrize("dim,cs", [(1, ref.SCALED), (3, ref.NORMAL), (5, ref.SCALED), (13, ref.NORMAL),
                                    (64, ref.SCALED)])
def test_widths(engine, dim, cs):
    """Pad widths 3, 1, 3, 3 and 0; the widest row."""
    X = table_rows(600, dim, cs, 100 + dim)
    C_start = duplicate_start(X, 8, 3)
    want = ref.refine(X, C_start, cs, max_iters=4, eps=0.0)
    assert want[3]["reseeded"][0] > 0
    engine.set_vectors(X)
    assert engine.training_info()["colorspace"] == cs
    same_run(engine.refine(C=C_start, max_iters=4, eps=0.0, reseed=True), want)


def test_one_row(engine):
    """N = 1: an empty cell and no donor (NORMAL: integers, the distortion is exactly 0)."""
    X = np.array([[5.0, -100.0, 77.0]])
    C_start = np.repeat(X, 2, axis=0)
    engine.set_vectors(X)
    got = engine.refine(C=C_start, max_iters=4, eps=0.0, reseed=True)
    assert got[3]["reseeded"] == [0, 0] and got[3]["stop"] == quant_amd.STOP_FIXED
    same_run(got, ref.refine(X, C_start, ref.NORMAL, max_iters=4, eps=0.0))


@pytest.mark.parametrize("delta", [-1, 0, 1])
def test_row_counts_around_the_block(engine, delta):
    n = quant_amd.host_reseed_grid()["block"] + delta
    X = table_rows(n, 3, ref.SCALED, 7 + delta)
    C_start = duplicate_start(X, 8, 3)
    want = ref.refine(X, C_start, ref.SCALED, max_iters=3, eps=0.0)
    assert want[3]["reseeded"][0] > 0
    engine.set_vectors(X)
    same_run(engine.refine(C=C_start, max_iters=3, eps=0.0, reseed=True), want)


def test_second_trip_of_the_grid_stride_loop_decides_a_far_row(engine):
    g = quant_amd.host_reseed_grid()
    first = g["block"] * g["blocks"]
    n, cs = first + 257, ref.NORMAL
    X = table_rows(n, 3, cs, 99).copy()
    tab = np.sort(quant_amd.colorspace_values(cs))
    X[X == tab[0]] = tab[1]        # the extreme value: in the loop's second trip only
    X[first + 100] = tab[0]
    C_start = duplicate_start(X, 16, 3)
    # the restatement's first selection: the row past block * blocks is a seed
    A1 = oracle.kdtree_nn(C_start, X)
    C1 = oracle.centroids(X, A1, 16, sum_mode=1)
    E, cnt, far = ref.cell_stats(ref.row_errors(X, C1, A1, cs), A1, 16)
    empties, donors = ref.select(E, cnt)
    assert len(empties) == len(donors) >= 3 and any(far[d] == first + 100 for d in donors)
    engine.set_vectors(X)
    got = engine.refine(C=C_start, max_iters=1, eps=0.0, reseed=True)   # iteration 1's codebook holds its seeds
    assert any(np.array_equal(c, X[first + 100]) for c in got[0])
    same_run(got, ref.refine(X, C_start, cs, max_iters=1, eps=0.0))
    same_run(engine.refine(C=C_start, max_iters=2, eps=0.0, reseed=True), ref.refine(X, C_start, cs, max_iters=2, eps=0.0))


def test_past_the_lds_capacities(engine):
    """K = 5000: the rows pass without LDS cells (a wave's lanes reduced per cell), and more than
    2048 donors, which the select sorts in global memory."""
    cs, K = ref.SCALED, 5000
    X = table_rows(40000, 3, cs, 4242)
    C_start = duplicate_start(X, K, 4000)
    A1 = oracle.kdtree_nn(C_start, X)
    C1 = oracle.centroids(X, A1, K, sum_mode=1)
    E, cnt, _ = ref.cell_stats(ref.row_errors(X, C1, A1, cs), A1, K)
    donors = int(((cnt >= 2) & (E > 0)).sum())
    print("donors", donors, "empties", int((cnt == 0).sum()))
    assert donors > 2048 and int((cnt == 0).sum()) >= 900
    want = ref.refine(X, C_start, cs, max_iters=2, eps=0.0)
    assert want[3]["reseeded"][0] >= 900
    engine.set_vectors(X)
    same_run(engine.refine(C=C_start, max_iters=2, eps=0.0, reseed=True), want)


def test_fresh_with_reseed(engine):
    X, start, _ = ref.run_case("s128_b2_6_scaled")
    lbg_on(engine, "s128_b2_6_scaled")
    C, A, d, info = engine.refine(max_iters=3, eps=0.0, fresh=True, reseed=True)
    assert info["reseeded"] == [4, 0, 0]
    A_star = oracle.kdtree_nn(C, X)
    assert np.array_equal(A, A_star)
    direct = ref.distortion(X, C, A_star)
    print("fresh distortion", d, "direct", direct)
    assert abs(d - direct) <= 1e-9 * direct
    same_run((C, A, d, info), ref.refine(X, start[0], ref.SCALED, start[1], start[2], max_iters=3, eps=0.0, fresh=True))


def test_continue_and_repeat(engine):
    _, _, (C_w, A_w, d_w, info_w) = ref.run_case("s128_b2_6_scaled")
    C_l, A_l, d_l = lbg_on(engine, "s128_b2_6_scaled")
    C1, _, _, i1 = engine.refine(max_iters=1, eps=0.0, reseed=True)
    assert i1["reseeded"] == [4] and i1["stop"] == quant_amd.STOP_MAXIT
    assert engine.refine_reseeds() == [4]
    C, A, d, info = engine.refine(max_iters=100, eps=0.0, reseed=True)   # from the seeded state
    assert info["iters"] == info_w["iters"] - 1 and info["stop"] == quant_amd.STOP_FIXED
    assert info["changed"] == info_w["changed"][1:] and info["reseeded"] == info_w["reseeded"][1:]
    assert np.array_equal(C, C_w) and np.array_equal(A, A_w) and abs(d - d_w) <= 1e-9 * d_w
    S, b, bits, cs = ref.CASES["s128_b2_6_scaled"]
    C2, A2, d2 = engine.lbg(bits)   # lbg again: what it gave before
    assert np.array_equal(C2, C_l) and np.array_equal(A2, A_l) and d2 == d_l


def test_errors():
    import torch   # noqa: F401  (opens the device before the engine does)
    S, b, bits, cs = ref.CASES["s64_b2_4_scaled"]
    L = quant_amd.lib()
    with quant_amd.Engine(0) as eng:
        n = ctypes.c_uint32()
        assert L.qvq_get_refine_reseeds(eng._h, None, 0, ctypes.byref(n)) == QVQ_ESTATE   # before any refine
        eng.set_images(oracle.gen_image(S), 1, S, S, b, b, cs)
        eng.lbg(bits)
        info = np.zeros(2, np.uint32)
        st = L.qvq_refine(eng._h, 1 << bits, None, 2, 0.0, 4, None, None, None, None, None,
                          info.ctypes.data_as(ctypes.c_void_p))
        assert st == QVQ_EINVAL                                                             # flag bit 4
        st = L.qvq_refine(eng._h, 1 << bits, None, 2, 0.0, 6, None, None, None, None, None, None)
        assert st == QVQ_EINVAL
        eng.comm_init_host(1, 0, lambda arr: None)   # one rank: the sum is the array itself
        eng.lbg(bits)
        with pytest.raises(quant_amd.QVQError) as e:
            eng.refine(max_iters=2, eps=0.0, reseed=True)
        assert e.value.status == QVQ_EUNSUPPORTED
        assert eng.refine(max_iters=2, eps=0.0)[3]["reseeded"] == [0, 0]   # without the flag: as before


def test_cli_and_quantizer_class(tmp_path):
    S, b, bits, cs = ref.CASES["s128_b2_6_scaled"]
    X, _, (C_w, A_w, _, info_w) = ref.run_case("s128_b2_6_scaled")
    assert info_w["iters"] < 40
    C, A, _ = quant_amd.LBGQuantizer(refine_iters=40, reseed=True).quantize(X, bits, 0.0)
    assert np.array_equal(C, C_w) and np.array_equal(A, A_w)
    ppm, out = tmp_path / "in.ppm", tmp_path / "out.quant"
    with open(ppm, "wb") as f:
        f.write(b"P6\n%d %d\n255\n" % (S, S))
        f.write(oracle.gen_image(S).tobytes())
    r = subprocess.run([QUANT, str(ppm), "-o", str(out), "-n", str(bits), "-e", "0", "--refine", "40", "--reseed"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    cb = oracle.codebook_bytes(C_w)
    assert open(out, "rb").read() == oracle.quant_file_bytes(cb, A_w, bits, oracle.SCALED, S, S, b, b)
    # and it is not the plain refinement's file
    _, start, _ = ref.run_case("s128_b2_6_scaled")
    C_p, A_p, _, _ = refine_ref.refine(X, *start, max_iters=40, eps=0.0)
    assert not np.array_equal(C_p, C_w)
