"""qvq_kmeanspp without a GPU: the rule's host helpers (quant_amd/csrc/kmeanspp_rule.hpp through
qvq_host_kmpp_draw / _weight) against Python ints and numpy, the restatement
(tests/helpers/kmeanspp_ref.py) against an independent brute force and a committed trace, the case
table's claims measured on the restatement, its sizes held to qvq_host_kmeanspp_plan, the C++
factory and the CLI's argument rules."""
import json
import os
import subprocess

import numpy as np
import pytest

import quant_amd
from conftest import GOLDEN, ROOT
from helpers import kmeanspp_cases as cases
from helpers import kmeanspp_ref as ref

LIB = os.path.join(ROOT, "quant_amd", "lib")
QUANT = os.path.join(LIB, "quant")
TRACE = os.path.join(GOLDEN, "kmeanspp_trace.json")
TRACE_CASES = ("two_rows", "three_rows", "boundary_0", "dim5")
M64 = (1 << 64) - 1


# -- the rule helpers -------------------------------------------------------------------------
def test_mix_known_values():
    # splitmix64's first outputs from state 0 (Vigna's reference stream): mix(0), mix(gamma)
    assert ref.mix(0) == 0xE220A8397B1DCDAF
    assert ref.mix(0x9E3779B97F4A7C15) == 0x6E789E6AA1B965F4


def test_draw_against_python_ints():
    rng = np.random.default_rng(3)
    Ts = [1, 2, 3, 255, (1 << 32) - 1, 1 << 32, (1 << 32) + 1, (1 << 54) - 1, M64]
    seeds = [0, 1, M64, M64 - 3, 0x123456789ABCDEF0] + [int(x) for x in rng.integers(0, 1 << 63, 20)]
    for seed in seeds:
        for j in (0, 1, 2, 5, 4095, (1 << 20) - 1):
            for T in Ts:
                want = (ref.mix((seed + j) & M64) * T) >> 64
                assert ref.draw(seed, j, T) == want
                assert quant_amd.host_kmpp_draw(seed, j, T) == want
                assert 0 <= want < T
    assert quant_amd.host_kmpp_draw(5, 9, 1) == 0
    # seed + j wraps: (2^64 - 1) + 1 is 0
    assert quant_amd.host_kmpp_draw(M64, 1, 1 << 40) == quant_amd.host_kmpp_draw(0, 0, 1 << 40) == ref.draw(M64, 1, 1 << 40)
    assert quant_amd.host_kmpp_draw(M64 - 3, 5, 999) == ref.draw(1, 0, 999)
    with pytest.raises(quant_amd.QVQError):
        quant_amd.host_kmpp_draw(0, 0, 0)


def test_draw_is_spread():
    """The draws of one seed cover [0, T) without an obvious hole: 4096 draws into 16 bins."""
    h = np.bincount([ref.draw(77, j, 16) for j in range(4096)], minlength=16)
    assert h.min() > 180 and h.max() < 340   # 256 expected, sigma 15.5


@pytest.mark.parametrize("dim", list(range(1, 65)))
def test_weight_against_numpy(dim):
    rng = np.random.default_rng(dim)
    Dp = (dim + 3) & ~3
    for cs, pad in ((ref.NORMAL, 128), (ref.SCALED, 0)):
        u = np.full((6, Dp), pad, np.int64)
        u[:, :dim] = rng.integers(0, 256, (6, dim))
        u[0, :dim], u[1, :dim] = 0, 255   # the extremes: 255^2 on every real component
        codes = ref.codes_from_ordinals(u)
        for a in range(6):
            for b in range(6):
                want = int(((u[a] - u[b]) ** 2).sum())
                assert quant_amd.host_kmpp_weight(codes[a], codes[b]) == want
        assert quant_amd.host_kmpp_weight(codes[0], codes[1]) == dim * 255 * 255


def test_weight_rejects_bad_widths():
    for n in (0, 3, 5, 68):
        with pytest.raises(quant_amd.QVQError):
            quant_amd.host_kmpp_weight(np.zeros(n, np.uint8), np.zeros(n, np.uint8))


# -- the restatement --------------------------------------------------------------------------
@pytest.mark.parametrize("n,dim,K,seed,hi", [(1, 1, 1, 0, 256), (2, 3, 2, 1, 256), (40, 3, 7, 2, 256), (64, 1, 6, 3, 4),
                                             (64, 1, 9, 11, 3), (30, 5, 30, 4, 256), (9, 2, 12, 5, 2), (120, 12, 10, 6, 256)])
def test_restatement_against_brute_force(n, dim, K, seed, hi):
    u = np.random.default_rng(100 + seed).integers(0, hi, (n, dim))
    rows, pot, placed, _ = ref.kmeanspp(u, K, seed)
    b_rows, b_pot, b_placed = ref.brute_force(u, K, seed)
    assert placed == b_placed
    assert [int(r) for r in rows[:placed]] == b_rows and np.all(rows[placed:] == ref.NO_ROW)
    assert [int(p) for p in pot[:len(b_pot)]] == b_pot and np.all(pot[len(b_pot):] == 0)


def test_restatement_against_the_committed_trace():
    with open(TRACE) as f:
        golden = json.load(f)
    assert sorted(golden) == sorted(TRACE_CASES)
    for name in TRACE_CASES:
        rows, pot, placed, _ = cases.trace(name)
        g = golden[name]
        assert [int(r) for r in rows] == g["rows"] and [int(p) for p in pot] == g["potential"] and placed == g["placed"], name


# -- the table's claims -----------------------------------------------------------------------
def test_names_are_the_tables():
    assert tuple(cases.table()) == cases.NAMES


def test_claims_degenerate_sets():
    rows, pot, placed, _ = cases.trace("one_row")
    assert (list(rows), list(pot), placed) == ([0], [0], 1)
    rows, pot, placed, _ = cases.trace("two_rows")
    assert sorted(rows) == [0, 1] and pot[1] == 0 and pot[0] > 0 and placed == 2
    rows, pot, placed, _ = cases.trace("all_equal")
    assert placed == 1 and np.all(rows[1:] == ref.NO_ROW) and np.all(pot == 0)
    rows, pot, placed, _ = cases.trace("three_rows")
    u = cases.rows("three_rows")
    assert placed == 3 and len(np.unique(u, axis=0)) == 3 and cases.table()["three_rows"]["K"] == 8
    assert pot[0] > pot[1] > 0 and np.all(pot[2:] == 0) and np.all(rows[3:] == ref.NO_ROW)
    assert len({tuple(u[r]) for r in rows[:3]}) == 3
    rows, pot, placed, _ = cases.trace("more_seeds_than_rows")
    c = cases.table()["more_seeds_than_rows"]
    assert c["K"] > len(cases.rows("more_seeds_than_rows")) == placed == 5 and sorted(rows[:5]) == list(range(5))


def test_claims_widths_cover_every_pad_remainder():
    dims = sorted(cases.rows(n).shape[1] for n in cases.names() if n.startswith("dim"))
    assert dims == [1, 3, 5, 12, 13, 48, 63, 64]
    assert {(-d) % 4 for d in dims} == {0, 1, 3} and {((d + 3) // 4) for d in dims} >= {1, 2, 3, 4, 12, 16}
    for name in cases.names():
        if name.startswith(("dim", "pad_valued")):
            assert cases.table()[name]["cs"] == ref.NORMAL or name == "pad_valued_scaled"
            assert cases.trace(name)[2] == cases.table()[name]["K"]
    for name, pad in (("pad_valued_scaled", 0), ("pad_valued_normal", 128)):
        u = cases.rows(name)
        assert u.shape[1] % 4 and (u == pad).mean() > 0.3 and (u != pad).mean() > 0.3


def test_claims_strict_boundary():
    names = [n for n in cases.names() if n.startswith("boundary_")]
    assert len(names) == 3
    for name in names:
        u = cases.rows(name)
        assert u.shape == (64, 1) and u.min() == 0 and u.max() == 3
        tr = cases.trace(name)[3]
        hits = [d for d in tr if d["boundary"] and d["zero_before"]]
        assert len(hits) >= 2, name
        # >= in place of > would take an earlier row in each of those draws
        for d in hits:
            assert d["s"] > 0


def test_claims_past_32_bits():
    rows, pot, placed, tr = cases.trace("past_32_bits")
    u = cases.rows("past_32_bits")
    assert u.shape == (8257, 64) and set(np.unique(u)) == {0, 255}
    assert int(pot[0]) > 1 << 32 and tr[0]["T"] > 1 << 32 and tr[0]["t"] > 1 << 32
    assert placed == 2 and pot[1] == 0
    # a total kept in 32 bits, or a 32-bit mulhi, draws another row
    T32 = tr[0]["T"] & 0xFFFFFFFF
    m = ref.weights(u, int(rows[0]))
    assert int(np.searchsorted(np.cumsum(m), ref.draw(cases.table()["past_32_bits"]["seed"], 1, T32), side="right")) != tr[0]["s"]


def test_claims_many_seeds():
    for name, K in (("k4096", 4096), ("k300", 300), ("k300_d48", 300)):
        rows, pot, placed, _ = cases.trace(name)
        assert placed == K == cases.table()[name]["K"] and len(set(rows.tolist())) == K
        assert np.all(np.diff(pot.astype(np.int64)) <= 0) and pot[-1] > 0
    assert 300 & 299


# -- the table's edges, held to the plan ------------------------------------------------------
def test_plan():
    p = quant_amd.host_kmeanspp_plan(1)
    B, S = p["block"], p["segments_cap"]
    assert (p["segments"], p["seg_rows"]) == (1, B) and B % 64 == 0
    for n in (1, B - 1, B, B + 1, 2 * B, 2 * B + 1, S * B - 1, S * B, S * B + 1, 4194304, 16777216, (1 << 32) - 1):
        q = quant_amd.host_kmeanspp_plan(n)
        assert q["block"] == B and q["segments_cap"] == S
        assert q["seg_rows"] % B == 0 and q["seg_rows"] >= B and 1 <= q["segments"] <= S
        assert (q["segments"] - 1) * q["seg_rows"] < n <= q["segments"] * q["seg_rows"]   # every segment holds a row
        assert q["seg_rows"] == B or (q["seg_rows"] - B) * S < n   # no larger than the cap demands
    assert quant_amd.host_kmeanspp_plan(S * B)["seg_rows"] == B
    assert quant_amd.host_kmeanspp_plan(S * B + 1)["seg_rows"] == 2 * B
    for bad in (0, 1 << 32):
        with pytest.raises(quant_amd.QVQError):
            quant_amd.host_kmeanspp_plan(bad)


def test_row_counts_lie_on_the_plans_edges():
    B, S = cases.block(), cases.cap()
    n = {name: len(cases.rows(name)) for name in cases.names() if name.startswith("rows_")}
    assert (n["rows_block_minus"], n["rows_block"], n["rows_block_plus"]) == (B - 1, B, B + 1)
    assert quant_amd.host_kmeanspp_plan(n["rows_block"])["segments"] == 1
    assert quant_amd.host_kmeanspp_plan(n["rows_block_plus"])["segments"] == 2
    for name, segs in (("rows_segs_minus", 2), ("rows_segs_plus", 3)):
        p = quant_amd.host_kmeanspp_plan(n[name])
        assert p["segments"] == segs and n[name] in (2 * p["seg_rows"] - 1, 2 * p["seg_rows"] + 1)
        # the draws take the last row of a segment and the first of the next
        drawn = set(int(r) for r in cases.trace(name)[0][1:])
        last = {k * p["seg_rows"] - 1 for k in range(1, segs)}
        first = {k * p["seg_rows"] for k in range(1, segs) if k * p["seg_rows"] < n[name]}
        assert drawn & last and drawn & first, name
    p = quant_amd.host_kmeanspp_plan(n["rows_cap_plus"])
    assert n["rows_cap_plus"] == S * B + 1 and p["seg_rows"] > B and cases.table()["rows_cap_plus"]["K"] == 8
    assert cases.rows("rows_cap_plus").shape[1] == 3
    segs = set(int(r) // p["seg_rows"] for r in cases.trace("rows_cap_plus")[0])
    assert len(segs) >= 4   # the draws spread over the segments
    p = quant_amd.host_kmeanspp_plan(n["rows_select_wide"])
    assert p["seg_rows"] > 1024 and p["segments"] > 1024   # both scans of the select take two items a lane


# -- the C++ factory and the CLI --------------------------------------------------------------
def test_cpp_factory(tmp_path):
    if not os.path.exists(os.path.join(LIB, "libquant_amd.so")):
        pytest.fail("libquant_amd.so not built (run __graft_entry__.build())")
    exe = str(tmp_path / "test_kmeanspp_api")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "test_kmeanspp_api.cpp"), "-L" + LIB, "-lquant_amd", "-lqvq",
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
def test_cli_kmeanspp_needs_lbg(tmp_path, q):
    r = run_quant(tmp_path, "--init", "kmeans++", "-q", q)
    assert r.returncode == 2 and "LBG quantizer" in r.stderr


@pytest.mark.parametrize("extra", [[], ["--refine", "3"], ["--reseed"]])
def test_cli_kmeanspp_excludes_lloyd(tmp_path, extra):
    r = run_quant(tmp_path, "--init", "kmeans++", "--lloyd", "2", *extra)
    assert r.returncode == 2 and "cannot be combined with '--lloyd'" in r.stderr


def test_cli_kmeanspp_reseed_needs_refine(tmp_path):
    r = run_quant(tmp_path, "--init", "kmeans++", "--reseed")
    assert r.returncode == 2 and "'--reseed' needs" in r.stderr


@pytest.mark.parametrize("args", [["--init", "lbg"], ["--init=kmeans"], ["--seed", "-1"], ["--seed", "7x"], ["--seed", ""],
                                  ["--seed", "18446744073709551616"], ["--init"]])
def test_cli_bad_values(tmp_path, args):
    r = run_quant(tmp_path, *args)
    assert r.returncode == 2, r.stderr


def test_cli_help():
    h = subprocess.run([QUANT, "--help"], capture_output=True, text=True).stdout
    assert "--init arg (=split)" in h and "kmeans++" in h and "--seed arg (=0)" in h
