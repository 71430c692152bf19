"""qvq_kmeans_par without a GPU: the sampling test's host helper (quant_amd/csrc/kmeans_par_rule.hpp
through qvq_host_kmeans_par_join) against Python ints, the restatement (tests/helpers/kmeans_par_ref.py)
against an independent brute force and a committed trace, the case table's claims measured on the
restatement, its sizes held to qvq_host_kmeans_par_plan, the plan's invariants and limits, the C++
factory and the CLI's argument rules."""
import json
import os
import subprocess

import numpy as np
import pytest

import quant_amd
from conftest import GOLDEN, ROOT
from helpers import kmeans_par_cases as cases
from helpers import kmeans_par_ref as ref

LIB = os.path.join(ROOT, "quant_amd", "lib")
QUANT = os.path.join(LIB, "quant")
TRACE = os.path.join(GOLDEN, "kmeans_par_trace.json")
TRACE_CASES = ("few_distinct", "near_tie", "join_boundary", "truncate", "dim5")
M64 = (1 << 64) - 1


# -- the rule helper --------------------------------------------------------------------------
def python_join(seed, r, row, phi, ell, m):
    key = ref.mix((seed + r) & M64)
    return (ref.mix((key + row) & M64) * phi) >> 64 < ell * m


def test_join_against_python_ints():
    rng = np.random.default_rng(3)
    phis = [0, 1, 2, 255, (1 << 32) - 1, 1 << 32, (1 << 32) + 1, (1 << 39) - 1, 1 << 39, (1 << 54) - 1, M64]
    ms = [0, 1, 2, 4161600, (1 << 22) - 1]
    ells = [0, 1, 4, 64, 1 << 16, 1 << 17]
    seeds = [0, 1, M64, M64 - 3, 0x123456789ABCDEF0] + [int(x) for x in rng.integers(0, 1 << 63, 6)]
    seen = set()
    for seed in seeds:
        for r in (1, 2, 16):
            for row in (0, 1, 4194303, (1 << 32) - 2):
                for phi in phis:
                    for m in ms:
                        for ell in ells:
                            want = python_join(seed, r, row, phi, ell, m)
                            assert quant_amd.host_kmeans_par_join(seed, r, row, phi, ell, m) == want
                            seen.add(want)
                            if m == 0 or ell == 0:
                                assert not want   # strict: a row on a candidate never joins
    assert seen == {False, True}
    for _ in range(3000):
        seed, row = int(rng.integers(0, 1 << 63)), int(rng.integers(0, 1 << 32))
        phi, m, ell = int(rng.integers(1, 1 << 54)), int(rng.integers(0, 1 << 22)), int(rng.integers(1, (1 << 17) + 1))
        r = int(rng.integers(1, 17))
        assert quant_amd.host_kmeans_par_join(seed, r, row, phi, ell, m) == python_join(seed, r, row, phi, ell, m)
    # the key wraps: seed + r past 2^64
    assert quant_amd.host_kmeans_par_join(M64, 1, 7, 1000, 4, 100) == python_join(M64, 1, 7, 1000, 4, 100)


def test_join_on_the_strict_edge():
    """mulhi = ell m - 1 joins, mulhi = ell m does not: phi chosen so that mulhi lands on both."""
    hits, phi, ell = {0: 0, 1: 0}, 1 << 20, 4
    for seed in range(400):
        v = (ref.mix((ref.mix((seed + 1) & M64) + 5) & M64) * phi) >> 64   # mulhi of row 5 in round 1
        if v >= ell and v % ell == 0:   # ell m = mulhi: not below
            assert not quant_amd.host_kmeans_par_join(seed, 1, 5, phi, ell, v // ell)
            hits[0] += 1
        if (v + 1) % ell == 0:   # mulhi = ell m - 1
            assert quant_amd.host_kmeans_par_join(seed, 1, 5, phi, ell, (v + 1) // ell)
            hits[1] += 1
    assert hits[0] > 20 and hits[1] > 20


def test_join_rejects_bad_arguments():
    for args in ((0, 0, 0, 1, 1, 1), (0, 17, 0, 1, 1, 1), (0, 1, 0, 1, (1 << 17) + 1, 1), (0, 1, 0, 1, 1, 1 << 22)):
        with pytest.raises(quant_amd.QVQError):
            quant_amd.host_kmeans_par_join(*args)


def test_vector_mulhi_against_python_ints():
    rng = np.random.default_rng(4)
    u = rng.integers(0, 1 << 63, 500).astype(np.uint64) * np.uint64(2) + np.uint64(1)
    for phi in (1, (1 << 32) - 1, 1 << 32, (1 << 54) - 1, M64):
        assert [int(x) for x in ref.mulhi_array(u, phi)] == [(int(x) * phi) >> 64 for x in u]
    assert [int(x) for x in ref.mix_array(np.arange(4, dtype=np.uint64))] == [ref.mix(i) for i in range(4)]


# -- the restatement --------------------------------------------------------------------------
@pytest.mark.parametrize("n,dim,K,seed,kw", [(1, 1, 1, 0, {}), (2, 3, 2, 1, {}), (200, 3, 8, 2, {}),
                                              (150, 5, 6, 3, dict(rounds=3, ell=10, round_cap=4)),
                                              (60, 1, 10, 4, dict(rounds=2)), (50, 2, 64, 5, dict(rounds=1, ell=1)),
                                              (64, 1, 6, 6, dict(ell=64)), (90, 2, 5, 7, dict(rounds=16, ell=2))])
def test_restatement_against_brute_force(n, dim, K, seed, kw):
    hi = 4 if dim == 1 and n == 64 else 256
    u = np.random.default_rng(100 + seed).integers(0, hi, (n, dim))
    a = ref.kmeans_par(u, K, seed, **kw)
    rows, cand, wt, placed, pot, truncated = ref.brute_force(u, K, seed, **kw)
    M, info = a["info"]["candidates"], a["info"]
    assert info["placed"] == placed and list(a["rows"][:placed]) == rows and np.all(a["rows"][placed:] == ref.NO_ROW)
    assert M == len(cand) and list(a["cand_rows"][:M]) == cand and np.all(a["cand_rows"][M:] == ref.NO_ROW)
    assert list(a["cand_weights"][:M]) == wt and not a["cand_weights"][M:].any() and sum(wt) == n
    assert info["potential"][:len(pot)] == pot and not any(info["potential"][len(pot):])
    assert info["truncated"] == truncated and len(pot) == info["rounds_run"] + 1
    assert sum(info["round_candidates"]) == M - 1
    assert len(a["cand_rows"]) == ref.options(K, **kw)[3]


def test_candidate_zero_is_kmeanspps_first_seed():
    from helpers import kmeanspp_ref
    u = cases.rows("dim5")
    for seed in (0, 1, 99):
        assert ref.kmeans_par(u, 4, seed)["cand_rows"][0] == kmeanspp_ref.kmeanspp(u, 4, seed)[0][0]


def jsonable(name):
    out, c = cases.trace(name), cases.table()[name]
    M = out["info"]["candidates"]
    return {"K": c["K"], "seed": c["seed"], "opts": c["opts"], "shape": list(cases.rows(name).shape),
            "rows": [int(x) for x in out["rows"]], "cand_rows": [int(x) for x in out["cand_rows"][:M]],
            "cand_weights": [int(x) for x in out["cand_weights"][:M]], "info": out["info"],
            "reduction": [int(x) for x in out["reduction"]]}


def test_committed_trace():
    """Results recorded from the restatement: a change of the rule's text or of a case's rows shows here."""
    want = json.load(open(TRACE))
    assert sorted(want) == sorted(TRACE_CASES)
    for name in TRACE_CASES:
        assert jsonable(name) == want[name], name


# -- the table and its claims -----------------------------------------------------------------
def test_names_match_the_table():
    assert tuple(cases.table()) == cases.NAMES and len(set(cases.NAMES)) == len(cases.NAMES)


def test_gpu_cases_are_small():
    for name in cases.names():
        c = cases.table()[name]
        r, ell, _, mc = ref.options(c["K"], **c["opts"])
        if name not in ("k300", "chunk_minus", "chunk_exact", "chunk_plus", "same_round_twins"):
            assert c["K"] <= 64 and ell <= 64, name
        assert cases.plan(len(cases.rows(name)), cases.rows(name).shape[1], c["K"], **c["opts"])["max_candidates"] == mc


def test_claims_degenerate():
    for name in ("one_row", "all_equal"):
        i = cases.trace(name)["info"]
        assert i["potential"][0] == 0 and i["rounds_run"] == 0 and i["candidates"] == 1 and i["placed"] == 1
        assert cases.table()[name]["K"] > 1 and cases.trace(name)["cand_weights"][0] == len(cases.rows(name))
    i = cases.trace("few_distinct")["info"]
    assert len(np.unique(cases.rows("few_distinct"), axis=0)) == 3 and i["placed"] == 3 < cases.table()["few_distinct"]["K"]
    assert i["rounds_run"] < 5   # phi reaches 0 and the rounds end early
    assert i["potential"][i["rounds_run"]] == 0
    out, c = cases.trace("k_gt_m"), cases.table()["k_gt_m"]
    assert c["K"] == 64 and c["opts"]["rounds"] == 1 and c["opts"]["ell"] == 1
    assert 1 < out["info"]["candidates"] < 64 and out["info"]["placed"] <= out["info"]["candidates"]
    assert out["reduction"][-1] == 0   # stopped by T = 0


def test_claims_truncate():
    out, c = cases.trace("truncate"), cases.table()["truncate"]
    assert c["opts"]["ell"] == 64 and c["opts"]["round_cap"] == 8
    assert out["info"]["truncated"] == 5   # every round
    for tr in out["trace"]:
        assert len(tr["joined"]) > 8 and list(tr["kept"]) == sorted(tr["joined"])[:8]
        assert list(tr["kept"]) != sorted(tr["joined"])[-8:]


def test_claims_twins():
    out = cases.trace("same_round_twins")
    u, M = cases.rows("same_round_twins"), out["info"]["candidates"]
    assert np.array_equal(u[:256], u[256:]) and cases.table()["same_round_twins"]["opts"]["ell"] == len(u)
    zero = [c for c in range(M) if out["cand_weights"][c] == 0]
    assert len(zero) >= 1 and not set(zero) & set(out["picks"])
    # a weight-0 candidate is the later of two equal rows that joined in one round
    cr = out["cand_rows"]
    for c in zero:
        assert int(cr[c]) - 256 in [int(x) for x in cr[:c]]
    assert int(out["cand_weights"].sum()) == len(u)


def test_claims_near_tie():
    out, u = cases.trace("near_tie"), cases.rows("near_tie")
    assert u.shape[1] == 1 and list(out["cand_rows"][:3]) == [int(out["cand_rows"][0]), 100, 100 + cases.TIE_BAND + 1]
    band = np.flatnonzero(u[:, 0] == 120)
    assert len(band) >= 16
    wP, wQ = (u[band, 0] - u[100, 0]) ** 2, (u[band, 0] - u[-1, 0]) ** 2
    assert np.array_equal(wP, wQ) and np.all(wP < out["trace"][0]["m_before"][band])   # a tie that moves the rows
    assert np.all(out["near"][band] == 1)   # the lower index
    assert out["cand_weights"][1] == len(band) + 1 and out["cand_weights"][2] == 1


def test_claims_join_boundary():
    """Found by the bounded search of kmeans_par_cases._boundary_seed: the case pins the strict <."""
    tr = cases.trace("join_boundary")["trace"][0]
    assert cases.boundary_hits(tr) == (True, True)
    below = np.flatnonzero((tr["rhs"] > 0) & (tr["lhs"] + np.uint64(1) == tr["rhs"]))
    on = np.flatnonzero((tr["rhs"] > 0) & (tr["lhs"] == tr["rhs"]))
    assert set(below) <= set(tr["joined"]) and not set(on) & set(tr["joined"])


def test_claims_past_32_bits():
    out, u = cases.trace("phi_past_32_bits"), cases.rows("phi_past_32_bits")
    assert u.shape == (4096, 64) and set(np.unique(u)) == {0, 255}
    tr = out["trace"][0]
    assert tr["phi"] > 1 << 32 and out["info"]["potential"][0] == tr["phi"]
    # phi kept in 32 bits samples other rows
    lhs32 = ref.join_values(cases.table()["phi_past_32_bits"]["seed"], 1, len(u), tr["phi"] & 0xFFFFFFFF)
    assert not np.array_equal(np.flatnonzero(lhs32 < tr["rhs"]), tr["joined"])
    out = cases.trace("reduction_past_32_bits")
    assert out["reduction"][0] > 1 << 32 and out["max_product"][0] > 1 << 32
    u, seed = cases.rows("reduction_past_32_bits"), cases.table()["reduction_past_32_bits"]["seed"]
    assert u.shape[1] == 64 and cases.truncated_pick(out, u, seed) != out["picks"][1]


def test_claims_chunk_edges():
    C = cases.chunk()
    for name, n in (("chunk_minus", C - 1), ("chunk_exact", C), ("chunk_plus", C + 1)):
        out = cases.trace(name)
        assert out["info"]["round_candidates"][:2] == [n, n] and out["info"]["truncated"] == 2, name
        # the last candidate of a trip is some row's nearest: skipping it shows in the weights
        base = 1
        for r in range(2):
            for last in {min(C, n) - 1, n - 1}:
                assert out["cand_weights"][base + last] >= 1
            base += n
    assert cases.trace("k300")["info"]["round_candidates"][0] > C   # several trips without truncation


def test_claims_lds_edge():
    a, b = cases.table()["lds_in"], cases.table()["lds_out"]
    n, dim = cases.rows("lds_in").shape
    assert dim == 64 and b["opts"]["round_cap"] == a["opts"]["round_cap"] + 1
    pa, pb = cases.plan(n, dim, a["K"], **a["opts"]), cases.plan(n, dim, b["K"], **b["opts"])
    assert pa["codes_lds"] == 1 and pb["codes_lds"] == 0 and pa["gw_lds"] == pb["gw_lds"] == 1
    assert pa["lds_bytes"] <= 160 * 1024 < 256 + (8 + 64) * ((pb["lds_bytes"] - 256) // 8)   # the next block of slots does not fit
    assert cases.trace("lds_in")["info"]["candidates"] > 16   # the reduction has candidates to choose among
    c = cases.table()["gw_global"]
    p = cases.plan(len(cases.rows("gw_global")), cases.rows("gw_global").shape[1], c["K"], **c["opts"])
    assert p["gw_lds"] == 0 and p["codes_lds"] == 0 and p["lds_bytes"] < 1024


def test_claims_seeds_and_rounds():
    assert cases.trace("k1")["info"]["placed"] == 1 and cases.table()["k1"]["K"] == 1
    for name, K in (("k37", 37), ("k300", 300)):
        out = cases.trace(name)
        assert out["info"]["placed"] == K == cases.table()[name]["K"] and K & (K - 1)
        assert len(set(out["rows"].tolist())) == K
    assert cases.trace("rounds1")["info"]["rounds_run"] == 1 and cases.trace("rounds16")["info"]["rounds_run"] == 16
    assert all(cases.trace("rounds16")["info"]["round_candidates"])
    pot = cases.trace("rounds16")["info"]["potential"]
    assert all(a >= b for a, b in zip(pot, pot[1:])) and pot[16] > 0


def test_claims_widths():
    pads = set()
    for dim in cases.WIDTHS:
        u = cases.rows("dim%d" % dim)
        assert u.shape[1] == dim and cases.trace("dim%d" % dim)["info"]["placed"] == 16
        pads.add(-dim % 4)
    assert pads == {0, 1, 2, 3}
    for name, pad in (("pad_valued_scaled", 0), ("pad_valued_normal", 128)):
        u = cases.rows(name)
        assert 0.3 < np.mean(u == pad) < 0.5 and cases.table()[name]["cs"] == (ref.SCALED if pad == 0 else ref.NORMAL)


# -- the table's edges, held to the plan ------------------------------------------------------
def test_plan():
    p = quant_amd.host_kmeans_par_plan(1, 1, 1)
    B, S = p["block"], p["segments_cap"]
    assert (p["segments"], p["seg_rows"]) == (1, B) and B % 64 == 0 and p["chunk"] <= 1024 and p["reduce_block"] == 1024
    assert (p["rounds"], p["ell"], p["round_cap"], p["max_candidates"]) == (5, 1, 66, 331)
    for n in (1, B - 1, B, B + 1, 2 * B, 2 * B + 1, S * B - 1, S * B, S * B + 1, 4194304, 16777216, (1 << 32) - 1):
        q = quant_amd.host_kmeans_par_plan(n, 12, 64)
        k = quant_amd.host_kmeanspp_plan(n)
        assert (q["block"], q["segments"], q["seg_rows"], q["segments_cap"]) == (k["block"], k["segments"], k["seg_rows"], S)
        assert q["seg_rows"] % B == 0 and q["seg_rows"] >= B and 1 <= q["segments"] <= S
        assert (q["segments"] - 1) * q["seg_rows"] < n <= q["segments"] * q["seg_rows"]
    assert quant_amd.host_kmeans_par_plan(S * B, 3, 4)["seg_rows"] == B
    assert quant_amd.host_kmeans_par_plan(S * B + 1, 3, 4)["seg_rows"] == 2 * B
    for K, rounds, ell, cap in ((64, 0, 0, 0), (1024, 0, 0, 0), (4096, 0, 0, 0), (16, 16, 1 << 17, 65535), (300, 3, 7, 1)):
        for dim in (1, 12, 48, 64):
            q = quant_amd.host_kmeans_par_plan(4096, dim, K, rounds, ell, cap)
            assert (q["rounds"], q["ell"], q["round_cap"], q["max_candidates"]) == ref.options(K, rounds, ell, cap)
            Dp = (dim + 3) & ~3
            slots = -(-q["max_candidates"] // 1024) * 1024
            need = 256 + 8 * slots + slots * Dp
            assert q["gw_lds"] == (256 + 8 * slots <= 160 * 1024) and q["codes_lds"] == (need <= 160 * 1024)
            assert q["lds_bytes"] == 256 + (8 * slots if q["gw_lds"] else 0) + (need - 256 - 8 * slots if q["codes_lds"] else 0)
            assert q["lds_bytes"] <= 160 * 1024


def test_limits():
    """The QVQ_EINVAL list, where no device is needed: the plan applies the entry point's own check."""
    ok = quant_amd.host_kmeans_par_plan
    ok(100, 3, 1 << 16, 1, 1, 1), ok(100, 3, 4, 16, 1 << 17, 65535)
    assert ok(100, 3, 4, 16, 1, 65535)["max_candidates"] == 1 + 16 * 65535 <= 1 << 20
    for K, rounds, ell, cap in ((0, 0, 0, 0), ((1 << 16) + 1, 0, 0, 0), (4, 17, 0, 0), (4, 0, (1 << 17) + 1, 0),
                                (4, 16, 0, 65536), (4, 1, 0, 1 << 20), (1 << 16, 16, 0, 0), (4, 5, 1 << 17, 0)):
        with pytest.raises(quant_amd.QVQError) as e:
            ok(100, 3, K, rounds, ell, cap)
        assert e.value.status == 1
    for n, dim in ((0, 3), (1 << 32, 3), (10, 0), (10, 65)):
        with pytest.raises(quant_amd.QVQError):
            ok(n, dim, 4)
    L = quant_amd.lib()
    assert L.qvq_kmeans_par(None, 4, 0, None, None, None, None, None, None) == 1
    assert "qvq_kmeans_par" in quant_amd.EXPORTED


def test_row_counts_lie_on_the_plans_edges():
    B, S = cases.block(), cases.cap()
    n = {name: len(cases.rows(name)) for name in cases.names() if name.startswith("rows_")}
    assert (n["rows_block_minus"], n["rows_block"], n["rows_block_plus"]) == (B - 1, B, B + 1)
    seg = quant_amd.host_kmeans_par_plan(n["rows_segs"], 3, 4)["seg_rows"]
    assert (n["rows_segs_minus"], n["rows_segs"], n["rows_segs_plus"]) == (2 * seg - 1, 2 * seg, 2 * seg + 1)
    assert [quant_amd.host_kmeans_par_plan(n[k], 3, 4)["segments"] for k in ("rows_block", "rows_block_plus", "rows_segs", "rows_segs_plus")] == [1, 2, 2, 3]
    assert (n["rows_cap_minus"], n["rows_cap"], n["rows_cap_plus"]) == (S * B - 1, S * B, S * B + 1)
    assert quant_amd.host_kmeans_par_plan(n["rows_cap"], 3, 4)["seg_rows"] == B
    assert quant_amd.host_kmeans_par_plan(n["rows_cap_plus"], 3, 4)["seg_rows"] > B   # the first count at which seg_rows grows
    for name in n:
        c = cases.table()[name]
        assert c["K"] == 4 and ref.options(4, **c["opts"])[1] == 4 and cases.rows(name).shape[1] == 3
    # the big sets' candidates come from many segments
    p = quant_amd.host_kmeans_par_plan(n["rows_cap_plus"], 3, 4)
    out = cases.trace("rows_cap_plus")
    assert len(set(int(r) // p["seg_rows"] for r in out["cand_rows"][:out["info"]["candidates"]])) >= 8


# -- the C++ factory and the CLI --------------------------------------------------------------
def test_cpp_factory(tmp_path):
    if not os.path.exists(os.path.join(LIB, "libquant_amd.so")):
        pytest.fail("libquant_amd.so not built (run __graft_entry__.build())")
    exe = str(tmp_path / "test_kmeans_par_api")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "test_kmeans_par_api.cpp"), "-L" + LIB, "-lquant_amd", "-lqvq",
                    "-Wl,-rpath," + LIB, "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def run_quant(tmp_path, *args):
    if not os.path.exists(QUANT):
        pytest.fail("quant CLI not built (run __graft_entry__.build())")
    ppm = tmp_path / "in.ppm"
    with open(ppm, "wb") as f:
        f.write(b"P6\n2 2\n255\n" + bytes(range(12)))
    return subprocess.run([QUANT, str(ppm), "-o", str(tmp_path / "out.quant"), *args], capture_output=True, text=True)


@pytest.mark.parametrize("q", ["1", "2"])
def test_cli_kmeans_par_needs_lbg(tmp_path, q):
    r = run_quant(tmp_path, "--init", "kmeans-par", "-q", q)
    assert r.returncode == 2 and "'--init kmeans-par' needs the LBG quantizer" in r.stderr


@pytest.mark.parametrize("extra", [[], ["--refine", "3"], ["--reseed"]])
def test_cli_kmeans_par_excludes_lloyd(tmp_path, extra):
    r = run_quant(tmp_path, "--init", "kmeans-par", "--lloyd", "2", *extra)
    assert r.returncode == 2 and "'--init kmeans-par' cannot be combined with '--lloyd'" in r.stderr


def test_cli_kmeans_par_reseed_needs_refine(tmp_path):
    r = run_quant(tmp_path, "--init", "kmeans-par", "--reseed")
    assert r.returncode == 2 and "'--reseed' needs" in r.stderr


@pytest.mark.parametrize("args", [["--init", "kmeans_par"], ["--init=kmeans||"], ["--init", "kmeans-par", "--seed", "-1"]])
def test_cli_bad_values(tmp_path, args):
    r = run_quant(tmp_path, *args)
    assert r.returncode == 2, r.stderr


def test_cli_help():
    h = subprocess.run([QUANT, "--help"], capture_output=True, text=True).stdout
    assert "--init arg (=split)" in h and "kmeans++" in h and "kmeans-par" in h and "--seed arg (=0)" in h
