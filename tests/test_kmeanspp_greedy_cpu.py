"""qvq_kmeanspp_greedy without a GPU: the trial count's host helper (qvq_host_kmpp_trials), the
restatement (tests/helpers/kmeanspp_greedy_ref.py) against an independent brute force, against
qvq_kmeanspp's restatement at L = 1 and against a committed trace, the case table's claims measured
on the restatement, its sizes held to qvq_host_kmeanspp_plan, the recorded quality claim, the C++
factory and the CLI's argument rules."""
import json
import os
import subprocess

import numpy as np
import pytest

import quant_amd
from conftest import GOLDEN, ROOT
from helpers import kmeanspp_cases
from helpers import kmeanspp_greedy_cases as cases
from helpers import kmeanspp_greedy_ref as ref
from oracle import oracle

LIB = os.path.join(ROOT, "quant_amd", "lib")
QUANT = os.path.join(LIB, "quant")
TRACE = os.path.join(GOLDEN, "kmeanspp_greedy_trace.json")
TRACE_CASES = ("two_rows", "stop", "same_row", "mirror_tie", "boundary_later_trial", "width_6")


# -- the trial count --------------------------------------------------------------------------
def test_trials_at_every_power_of_two():
    assert quant_amd.host_kmpp_trials(1) == 2 and quant_amd.host_kmpp_trials(1024) == 9
    assert quant_amd.host_kmpp_trials(1 << 20) == 16
    for e in range(21):
        for K in (2 ** e - 1, 2 ** e, 2 ** e + 1):
            if not 1 <= K <= 1 << 20:
                continue
            lg = e - 1 if K < 2 ** e else e
            assert quant_amd.host_kmpp_trials(K) == ref.trials(K) == 2 + 7 * lg // 10, K
            for L in (1, 2, 15, 16):
                assert quant_amd.host_kmpp_trials(K, L) == ref.trials(K, L) == L
    assert max(quant_amd.host_kmpp_trials(K) for K in (1, 1 << 19, 1 << 20)) == 16   # the default never exceeds the cap


@pytest.mark.parametrize("K,trials", [(0, 0), (0, 3), ((1 << 20) + 1, 0), ((1 << 20) + 1, 16), (1, 17), (1 << 20, 17),
                                      (5, 0xFFFFFFFF), (0xFFFFFFFF, 1), (-1, 0), (4, -1)])
def test_trials_limits(K, trials):
    with pytest.raises(quant_amd.QVQError):
        quant_amd.host_kmpp_trials(K, trials)
    with pytest.raises(ValueError):
        ref.trials(K, trials)


def test_trial_streams():
    """Trial l draws from seed + l 2^32, wrapping; l = 0 is qvq_kmeanspp's own stream."""
    M = ref.MASK
    assert ref.trial_seed(5, 0) == 5 and ref.trial_seed(5, 3) == 5 + (3 << 32)
    assert ref.trial_seed(M, 1) == (1 << 32) - 1 and ref.trial_seed(M - (15 << 32) + 1, 15) == 0
    for seed, l, j, T in ((0, 1, 1, 1000), (M, 15, 7, 1 << 40), (123456789, 9, 4095, (1 << 54) - 1)):
        want = (ref.mix((seed + (l << 32) + j) & M) * T) >> 64
        assert ref.draw(ref.trial_seed(seed, l), j, T) == want == quant_amd.host_kmpp_draw(ref.trial_seed(seed, l), j, T)


# -- the restatement --------------------------------------------------------------------------
@pytest.mark.parametrize("n,dim,K,seed,hi,L", [(1, 1, 1, 0, 256, 16), (2, 3, 2, 1, 256, 16), (40, 3, 7, 2, 256, 3),
                                               (64, 1, 6, 3, 4, 4), (64, 1, 9, 11, 3, 2), (30, 5, 30, 4, 256, 2),
                                               (9, 2, 12, 5, 2, 16), (120, 12, 10, 6, 256, 5), (40, 1, 5, 7, 6, 1)])
def test_restatement_against_brute_force(n, dim, K, seed, hi, L):
    u = np.random.default_rng(100 + seed).integers(0, hi, (n, dim))
    r = ref.kmeanspp_greedy(u, K, seed, L)
    b_rows, b_pot, b_placed, b_trial, b_trows, b_tpot = ref.brute_force(u, K, seed, L)
    assert r["placed"] == b_placed and r["trials"] == L
    assert [int(x) for x in r["rows"][:b_placed]] == b_rows and np.all(r["rows"][b_placed:] == ref.NO_ROW)
    assert [int(x) for x in r["potential"][:b_placed]] == b_pot and np.all(r["potential"][b_placed:] == 0)
    assert [int(x) for x in r["trial"][:b_placed]] == b_trial and np.all(r["trial"][b_placed:] == ref.NO_TRIAL)
    for j in range(K):
        n_l = 0 if j >= b_placed else 1 if j == 0 else L
        if n_l:
            assert [int(x) for x in r["trial_rows"][j, :n_l]] == b_trows[j]
            assert [int(x) for x in r["trial_potential"][j, :n_l]] == b_tpot[j]
        assert np.all(r["trial_rows"][j, n_l:] == ref.NO_ROW) and np.all(r["trial_potential"][j, n_l:] == 0)


@pytest.mark.parametrize("name", kmeanspp_cases.names())
def test_one_trial_is_kmeanspp(name):
    c = kmeanspp_cases.table()[name]
    rows, pot, placed, _ = kmeanspp_cases.trace(name)
    r = ref.kmeanspp_greedy(kmeanspp_cases.rows(name), c["K"], c["seed"], 1)
    assert r["placed"] == placed and np.array_equal(r["rows"], rows) and np.array_equal(r["potential"], pot)
    assert np.all(r["trial"][:placed] == 0) and np.array_equal(r["trial_rows"][:, 0], rows)
    assert np.array_equal(r["trial_potential"][:, 0], pot) and np.all(r["trial_rows"][:, 1:] == ref.NO_ROW)


def test_restatement_against_the_committed_trace():
    with open(TRACE) as f:
        golden = json.load(f)
    assert sorted(golden) == sorted(TRACE_CASES)
    for name in TRACE_CASES:
        r, g = cases.result(name), golden[name]
        L = g["trials"]
        assert r["trials"] == L and r["placed"] == g["placed"], name
        for k in ("rows", "potential", "trial"):
            assert [int(x) for x in r[k]] == g[k], (name, k)
        for k in ("trial_rows", "trial_potential"):
            assert [[int(x) for x in row[:L]] for row in r[k]] == g[k], (name, k)


# -- the table's claims -----------------------------------------------------------------------
def test_names_are_the_tables():
    assert tuple(cases.table()) == cases.NAMES


def test_claims_degenerate_sets():
    for name, n in (("one_row", 1), ("two_rows", 2), ("three_rows_n", 3)):
        r, c = cases.result(name), cases.table()[name]
        assert len(cases.rows(name)) == n == c["K"] == r["placed"] and r["trials"] == c["trials"] == 16
        assert sorted(r["rows"].tolist()) == list(range(n)) and r["potential"][-1] == 0
    r = cases.result("two_rows")   # every trial of round 1 draws the one row left
    assert len(set(r["trial_rows"][1].tolist())) == 1 and r["trial"][1] == 0
    r = cases.result("stop")
    u = cases.rows("stop")
    assert r["placed"] == 3 and len(np.unique(u, axis=0)) == 3 and cases.table()["stop"]["K"] == 8
    assert r["potential"][0] > r["potential"][1] > 0 and np.all(r["potential"][2:] == 0)   # T = 0 before round 3
    assert np.all(r["rows"][3:] == ref.NO_ROW) and np.all(r["trial"][3:] == ref.NO_TRIAL)
    assert np.all(r["trial_rows"][3:] == ref.NO_ROW) and np.all(r["trial_potential"][3:] == 0)
    r, c = cases.result("more_seeds_than_rows"), cases.table()["more_seeds_than_rows"]
    assert c["K"] > len(cases.rows("more_seeds_than_rows")) == r["placed"] == 5 and sorted(r["rows"][:5].tolist()) == list(range(5))
    assert c["trials"] == 0 and r["trials"] == 4   # the default of K = 9


def test_claims_same_row():
    r = cases.result("same_row")
    hits = cases.same_row_rounds(r)
    assert hits
    for j, lo, hi in hits:
        rec = r["trace"][j - 1]
        assert lo < hi and rec["c"][lo] == rec["c"][hi] and rec["P"][lo] == rec["P"][hi] == min(rec["P"])
        assert r["trial"][j] == lo and rec["t"][lo] != rec["t"][hi]


def test_claims_mirror_tie():
    r, u = cases.result("mirror_tie"), cases.rows("mirror_tie")
    assert u.shape[1] == 1 and sorted((254 - u[:, 0]).tolist()) == sorted(u[:, 0].tolist())   # the set is its mirror image
    assert u[r["rows"][0], 0] == 127   # the first seed is the centre, so m is symmetric
    hits = cases.tie_rounds(r)
    assert hits
    for j, lo, hi in hits:
        rec = r["trace"][j - 1]
        a, b = rec["c"][lo], rec["c"][hi]
        assert a != b and u[a, 0] + u[b, 0] == 254 and rec["P"][lo] == rec["P"][hi] == min(rec["P"])
        assert r["trial"][j] == lo < hi and r["rows"][j] == a


def test_claims_winning_trials():
    r = cases.result("last_trial")
    L = r["trials"]
    assert L == 5 and (L - 1) in r["trial"][1:].tolist()
    for name in ("last_trial", "trials_2", "trials_9", "trials_16", "k300"):
        r = cases.result(name)
        won = r["trial"][1:r["placed"]]
        assert np.any(won != 0) and won.max() < r["trials"], name   # a round not won by l = 0
        for j in range(1, r["placed"]):   # the winner has the smallest P, the lowest l among equals
            P = r["trial_potential"][j, :r["trials"]]
            assert r["trial"][j] == int(np.argmin(P)) and r["potential"][j] == P.min()
            assert r["rows"][j] == r["trial_rows"][j, r["trial"][j]]
    assert [cases.result("trials_%d" % L)["trials"] for L in (1, 2, 9, 16)] == [1, 2, 9, 16]
    assert len({cases.rows("trials_%d" % L).tobytes() for L in (1, 2, 9, 16)}) == 1   # one set
    # more trials never see a higher potential after round 1 (the same first seed and first draw)
    p1 = [int(cases.result("trials_%d" % L)["potential"][1]) for L in (1, 2, 9, 16)]
    assert p1 == sorted(p1, reverse=True) and p1[0] > p1[-1]


def test_claims_strict_boundary_on_a_later_trial():
    r, u = cases.result("boundary_later_trial"), cases.rows("boundary_later_trial")
    assert u.shape == (64, 1) and u.min() == 0 and u.max() == 3
    hits = cases.boundary_rounds(r)
    assert hits and all(l > 0 for _, l in hits)
    for j, l in hits:   # >= in place of > would take the zero-weight row before
        assert r["trace"][j - 1]["c"][l] > 0


def test_claims_past_32_bits():
    r, u = cases.result("past_32_bits"), cases.rows("past_32_bits")
    assert u.shape == (20000, 64) and set(np.unique(u)) == {0, 128, 255}
    rec = r["trace"][0]
    assert rec["T"] > 1 << 32 and min(rec["P"]) > 1 << 32 and len(set(rec["c"])) > 1
    assert r["placed"] == 3 and r["potential"][2] == 0


def test_claims_widths_cover_every_padded_width():
    assert sorted((d + 3) // 4 for d in cases.WIDTH_DIMS) == list(range(1, 17))
    assert {(-d) % 4 for d in cases.WIDTH_DIMS} == {0, 1, 2, 3}
    seen = set()
    for d in cases.WIDTH_DIMS:
        name = "width_%d" % d
        c, u = cases.table()[name], cases.rows(name)
        pad = 0 if c["cs"] == ref.SCALED else 128
        assert u.shape[1] == d and c["trials"] >= 2 and (u == pad).mean() > 0.3 and (u != pad).mean() > 0.3
        assert cases.result(name)["placed"] == c["K"]
        seen.add(c["cs"])
    assert seen == {ref.NORMAL, ref.SCALED}


def test_claims_many_seeds():
    for name in ("k300", "k300_d48"):
        r = cases.result(name)
        assert cases.table()[name]["trials"] == 0 and r["trials"] == 7 == quant_amd.host_kmpp_trials(300)
        assert r["placed"] == 300 and len(set(r["rows"].tolist())) == 300
        assert np.all(np.diff(r["potential"].astype(np.int64)) <= 0) and r["potential"][-1] > 0


# -- the table's edges, held to the plan ------------------------------------------------------
def test_row_counts_lie_on_the_plans_edges():
    B, S = cases.block(), cases.cap()
    n = {name: len(cases.rows(name)) for name in cases.names() if name.startswith("rows_")}
    assert (n["rows_block_minus"], n["rows_block"], n["rows_block_plus"]) == (B - 1, B, B + 1)
    assert quant_amd.host_kmeanspp_plan(n["rows_block"])["segments"] == 1
    assert quant_amd.host_kmeanspp_plan(n["rows_block_plus"])["segments"] == 2
    for name, segs in (("rows_segs_minus", 2), ("rows_segs_plus", 3)):
        p = quant_amd.host_kmeanspp_plan(n[name])
        assert p["segments"] == segs and n[name] in (2 * p["seg_rows"] - 1, 2 * p["seg_rows"] + 1)
        assert cases.edge_draws(n[name], cases.result(name)), name
    p = quant_amd.host_kmeanspp_plan(n["rows_cap_minus"])
    assert n["rows_cap_minus"] == S * B - 1 and (p["seg_rows"], p["segments"]) == (B, S)
    p = quant_amd.host_kmeanspp_plan(n["rows_cap_plus"])
    assert n["rows_cap_plus"] == S * B + 1 and p["seg_rows"] == 2 * B
    p = quant_amd.host_kmeanspp_plan(n["rows_select_wide"])
    assert p["seg_rows"] > 1024 and p["segments"] > 1024   # both scans of the select take two items a lane
    sr = -(-p["seg_rows"] // 1024)   # rows a lane of the row scan takes: a candidate that is not the first of its lane's run
    r = cases.result("rows_select_wide")
    assert sr == 2 and any(int(c) % p["seg_rows"] % sr for c in r["trial_rows"][1:, :r["trials"]].ravel())
    for name in n:
        assert cases.table()[name]["K"] <= 4 and cases.result(name)["placed"] == cases.table()[name]["K"]
    for name in ("rows_cap_minus", "rows_cap_plus", "rows_select_wide"):   # the candidates spread over the segments
        r = cases.result(name)
        sr = quant_amd.host_kmeanspp_plan(n[name])["seg_rows"]
        assert len(set(int(c) // sr for c in r["trial_rows"][1:, :r["trials"]].ravel())) >= 4


# -- the quality claim ------------------------------------------------------------------------
def test_default_trials_lower_the_potential():
    """gen_image(96) in 2x2 blocks (2304 rows of 12), K = 64, seeds 0 .. 5: the mean final potential
    at the default L = 6 against L = 1.  Measured on the restatement: 25 745 185.17 against
    32 873 625.33 (-21.7 %), the default lower for 6 of the 6 seeds."""
    rgb = oracle.gen_image(96)
    X, _ = oracle.tile(rgb, 96, 96, 2, 2)
    u = ref.ordinals_from_values(X, ref.SCALED)
    assert u.shape == (2304, 12) and ref.trials(64) == 6
    one = [int(ref.kmeanspp_greedy(u, 64, s, 1)["potential"][-1]) for s in range(6)]
    default = [int(ref.kmeanspp_greedy(u, 64, s, 0)["potential"][-1]) for s in range(6)]
    print("L = 1:", one, np.mean(one), "default:", default, np.mean(default))
    assert np.mean(default) < np.mean(one)
    assert one == [31335573, 32718754, 35697895, 31713292, 32730065, 33046173]
    assert default == [25314686, 25955672, 25842428, 25191921, 26183747, 25982657]


# -- the C++ factory and the CLI --------------------------------------------------------------
def test_cpp_factory(tmp_path):
    if not os.path.exists(os.path.join(LIB, "libquant_amd.so")):
        pytest.fail("libquant_amd.so not built (run __graft_entry__.build())")
    exe = str(tmp_path / "test_kmeanspp_greedy_api")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "test_kmeanspp_greedy_api.cpp"), "-L" + LIB, "-lquant_amd", "-lqvq",
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


@pytest.mark.parametrize("extra", [[], ["--init", "split"], ["--init", "kmeans-par"], ["--refine", "3"], ["--lloyd", "2"],
                                   ["-q", "1"]])
def test_cli_trials_needs_kmeanspp(tmp_path, extra):
    r = run_quant(tmp_path, "--trials", "3", *extra)
    assert r.returncode == 2 and "'--trials' needs '--init kmeans++'" in r.stderr


@pytest.mark.parametrize("val", ["17", "-1", "+3", "3x", "", "1.5", "99999999999"])
def test_cli_bad_trials(tmp_path, val):
    r = run_quant(tmp_path, "--init", "kmeans++", "--trials", val)
    assert r.returncode == 2, r.stderr


def test_cli_trials_value_missing(tmp_path):
    r = run_quant(tmp_path, "--init", "kmeans++", "--trials")
    assert r.returncode == 2 and "missing" in r.stderr


def test_cli_trials_keeps_the_other_rules(tmp_path):
    r = run_quant(tmp_path, "--init", "kmeans++", "--trials", "0", "--lloyd", "2")
    assert r.returncode == 2 and "cannot be combined with '--lloyd'" in r.stderr
    r = run_quant(tmp_path, "--init", "kmeans++", "--trials=16", "--reseed")
    assert r.returncode == 2 and "'--reseed' needs" in r.stderr
    r = run_quant(tmp_path, "--init", "kmeans++", "--trials", "2", "-q", "1")
    assert r.returncode == 2 and "LBG quantizer" in r.stderr


def test_cli_help():
    h = subprocess.run([QUANT, "--help"], capture_output=True, text=True).stdout
    assert "--trials arg" in h and "0 .. 16" in h and "--init kmeans++" in h
