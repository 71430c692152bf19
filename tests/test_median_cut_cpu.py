"""qvq_median_cut without a GPU: the rule's host helpers (quant_amd/csrc/median_cut_rule.hpp through
qvq_host_median_cut_axis / _select) against the numpy restatement, the case table's claims measured
on the restatement, its sizes held to qvq_host_median_cut_plan, the C++ factory and the CLI's
argument rules."""
import os
import subprocess

import numpy as np
import pytest

import quant_amd
from conftest import ROOT
from helpers import median_cut_cases as cases
from helpers import median_cut_ref as ref

LIB = os.path.join(ROOT, "quant_amd", "lib")
QUANT = os.path.join(LIB, "quant")


# -- the rule helpers -------------------------------------------------------------------------
def test_select_random_histograms():
    rng = np.random.default_rng(1)
    for i in range(400):
        lo, hi = sorted(rng.choice(256, 2, replace=False))
        h = np.zeros(256, np.uint32)
        top = int(rng.choice([1, 2, 5, 1000, 1 << 24]))
        h[lo:hi + 1] = rng.integers(0, top + 1, hi - lo + 1) * (rng.random(hi - lo + 1) < rng.choice([0.2, 1.0]))
        h[lo] = max(h[lo], 1)
        h[hi] = max(h[hi], 1)
        n = int(h.sum())
        t, _ = ref.select(h, int(lo), int(hi), n)
        assert quant_amd.host_median_cut_select(h, lo, hi, n) == t
        assert lo <= t < hi


@pytest.mark.parametrize("vals,t,ties", [([1, 2, 2, 3], 1, 2),             # even n, the minimum twice: the lowest
                                          ([1, 1, 2, 3, 3], 1, 2),          # odd n, the minimum twice
                                          ([4, 4, 9, 13], 4, 1),            # at lo
                                          ([0, 0, 0, 5], 0, 1),             # one split, every v: lo
                                          ([0, 4, 4, 5, 5, 5], 4, 1),       # at hi - 1
                                          ([0, 255], 0, 1),                 # the widest range, one split
                                          ([0] + [255] * 9, 0, 1),          # the upper child holds nearly all
                                          ([0] * 9 + [255], 0, 1),
                                          ([7, 8], 7, 1)])                  # range 1: the only choice
def test_select_crafted(vals, t, ties):
    h = np.bincount(vals, minlength=256).astype(np.uint32)
    lo, hi = min(vals), max(vals)
    assert ref.select(h, lo, hi, len(vals)) == (t, ties)
    assert quant_amd.host_median_cut_select(h, lo, hi) == t


def test_select_counts_past_32_bits():
    h = np.zeros(256, np.uint32)
    h[10], h[11], h[200] = 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF   # n = 3 (2^32 - 1): 2 cum - n needs 64 bits
    assert quant_amd.host_median_cut_select(h, 10, 200, 3 * 0xFFFFFFFF) == ref.select(h, 10, 200, 3 * 0xFFFFFFFF)[0] == 10
    h[10] = 1
    assert quant_amd.host_median_cut_select(h, 10, 200, int(h.astype(np.uint64).sum())) == 11


def test_select_rejects_bad_ranges():
    h = np.ones(256, np.uint32)
    for lo, hi in [(5, 5), (6, 5), (0, 256)]:
        with pytest.raises(quant_amd.QVQError) as e:
            quant_amd.host_median_cut_select(h, lo, hi)
        assert e.value.status == 1


def test_axis():
    rng = np.random.default_rng(2)
    for dim in (1, 3, 5, 12, 48, 64):
        for _ in range(50):
            lo = rng.integers(0, 256, dim)
            hi = lo + rng.integers(0, 4, dim)   # small ranges: equal maxima are common
            hi = np.minimum(hi, 255)
            assert quant_amd.host_median_cut_axis(lo, hi) == ref.axis_of(lo, hi)[0]
    # equal ranges in several dims: the lowest
    assert quant_amd.host_median_cut_axis([0, 10, 20, 30], [5, 15, 25, 35]) == 0
    assert quant_amd.host_median_cut_axis([0, 10, 20, 30], [4, 15, 25, 35]) == 1
    assert quant_amd.host_median_cut_axis([3, 0, 7], [3, 9, 16]) == 1
    assert quant_amd.host_median_cut_axis([3, 3], [3, 3]) == 0              # range 0 everywhere
    assert quant_amd.host_median_cut_axis([0xFFFFFFFF] * 3, [0] * 3) == 0   # an empty box's reset ranges


def test_ordinals_follow_the_values():
    for cs in (ref.NORMAL, ref.SCALED):
        tab = quant_amd.colorspace_values(cs)
        u = ref.ordinals_from_codes(np.arange(256, dtype=np.uint8))
        assert np.array_equal(np.argsort(tab, kind="stable"), np.argsort(u, kind="stable"))
        assert np.array_equal(ref.values(u, cs), tab)
        assert np.array_equal(ref.ordinals_from_values(tab, cs), u)
        assert np.array_equal(ref.codes_from_ordinals(u), np.arange(256, dtype=np.uint8))
    assert ref.ordinals_from_codes(np.uint8([0x7F]))[0] == 255 and ref.ordinals_from_codes(np.uint8([0x80]))[0] == 0


# -- the table's claims, on the restatement ---------------------------------------------------
def trace_of(name):
    return cases.trace(name)


def test_claims_degenerate_sets():
    assert trace_of("one_row")[1] == [0, 0, 0]
    A, cuts, _ = trace_of("two_rows")
    assert cuts == [1, 0, 0] and sorted(A) == [0, 1]
    A, cuts, _ = trace_of("all_equal")
    assert cuts == [0, 0, 0, 0] and not A.any()
    assert trace_of("bits0")[1] == [] and not trace_of("bits0")[0].any()
    A, cuts, trace = trace_of("more_boxes_than_rows")
    assert len(A) == 5 and len(np.unique(A)) == 5 and any(b["n"] == 0 for b in trace[-1])
    assert any(b["n"] == 1 and not b["cut"] for b in trace[-1])   # a single row is not cut


def test_claims_signed_bytes():
    for name in ("signed_bytes", "signed_bytes_normal"):
        u = cases.rows(name)
        _, _, trace = trace_of(name)
        top = trace[0][0]
        assert top["axis"] == 1 and top["lo"] == 0 and top["hi"] == 255
        codes = ref.codes_from_ordinals(u[:, 1])
        assert 0x7F in codes and 0x80 in codes and 0x00 in codes and 0xFF in codes
        # raw-byte order cuts elsewhere: the rows above t differ
        raw = codes.astype(np.int64)
        t_raw, _ = ref.select(np.bincount(raw, minlength=256), int(raw.min()), int(raw.max()), len(raw))
        assert not np.array_equal(raw > t_raw, u[:, 1] > top["t"])


@pytest.mark.parametrize("name", ["axis_tie_d3", "axis_tie_d12"])
def test_claims_axis_tie(name):
    top = trace_of(name)[2][0][0]
    r = top["ranges"]
    assert r[0] == r[-1] == max(r) and top["axis"] == 0 and r.count(max(r)) == 2


def test_claims_balance_and_position():
    even, odd = trace_of("balance_tie_even")[2][0][0], trace_of("balance_tie_odd")[2][0][0]
    assert even["n"] % 2 == 0 and even["ties"] == 2 and odd["n"] % 2 == 1 and odd["ties"] == 2
    at_lo = trace_of("cut_at_lo")[2][0][0]
    assert at_lo["t"] == at_lo["lo"] and at_lo["ties"] == 1
    at_hi = trace_of("cut_at_hi_minus_1")[2][0][0]
    assert at_hi["t"] == at_hi["hi"] - 1 and at_hi["ties"] == 1 and at_hi["hi"] - at_hi["lo"] > 1
    A, _, trace = trace_of("row_at_t")
    top = trace[0][0]
    u = cases.rows("row_at_t")
    assert top["at_t"] == 3 and not A[u[:, top["axis"]] == top["t"]].any()   # the rows at t stay low
    assert A[u[:, top["axis"]] > top["t"]].all()


def test_claims_box_populations():
    A, cuts, _ = trace_of("one_box_per_row")
    assert len(A) == 64 and np.array_equal(np.sort(A), np.arange(64)) and cuts == [1, 2, 4, 8, 16, 32]
    A, cuts, _ = trace_of("skewed")
    n = np.bincount(A, minlength=8)
    assert cuts == [1, 0, 0] and sorted(n)[-2:] == [1, len(A) - 1]
    assert (len(A) - 1) & (len(A) - 2) == 0   # the big box holds a power of two: its centroid is exact


def test_claims_widths_cover_every_pad_class():
    dims = sorted(cases.rows(n).shape[1] for n in cases.CASES if n.startswith("dim"))
    assert dims == [1, 3, 5, 12, 48, 64]
    assert {(-d) % 4 for d in dims} == {0, 1, 3} and {d % 16 == 0 for d in dims} == {True, False}
    for name in cases.CASES:
        if name.startswith("dim"):
            assert all(b["cut"] for b in trace_of(name)[2][-1])   # every level really cuts


# -- the table's edges, held to the plan ------------------------------------------------------
def test_plan_matches_the_tables_constants():
    p = quant_amd.host_median_cut_plan(12, 1, 1000)
    assert (p["block"], p["range_cap"], p["hist_cap"], p["lds_words"]) == (cases.BLOCK, cases.CAP, cases.CAP,
                                                                          cases.LDS_WORDS)
    assert p["range_groups"] == p["hist_groups"] == 1
    assert p["full_hist"] == 0
    assert p["range_grid"] == p["hist_grid"] == 4
    assert quant_amd.host_median_cut_plan(12, 1, 1)["range_grid"] == 1
    assert quant_amd.host_median_cut_plan(12, 1, 10 ** 9)["range_grid"] == cases.CAP
    for bad in [(0, 1, 5), (65, 1, 5), (12, 0, 5), (12, 1, 0), (12, 1 << 20, 5), (12, 3, 5)]:
        with pytest.raises(quant_amd.QVQError):
            quant_amd.host_median_cut_plan(*bad)


def test_row_counts_lie_on_both_sides_of_block_and_cap():
    p = quant_amd.host_median_cut_plan(3, 1, 1000)
    ns = sorted(len(cases.rows(n)) for n in cases.CASES if n.startswith("rows_"))
    for edge in (p["block"], p["block"] * p["range_cap"], p["block"] * p["hist_cap"]):
        assert edge - 1 in ns and edge in ns and any(n > edge for n in ns)
    # the case past the cap takes the loop's second trip, the one at it does not
    over = len(cases.rows("rows_cap_plus"))
    assert over > p["block"] * p["range_cap"] >= len(cases.rows("rows_cap"))
    assert quant_amd.host_median_cut_plan(3, 1, over)["range_grid"] == p["range_cap"]


# case -> the groups (0: global memory) its last level's ranges pass and histogram pass must take
EDGES = {
    "hist_one_group": (1, 1), "hist_two_groups": (1, 2),
    "range_one_group_d12": (1, 16), "range_two_groups_d12": (2, 0), "range_four_groups_d12": (4, 0),
    "range_groups_last_d12": (16, 0), "range_global_first_d12": (0, 0), "range_global_second_d12": (0, 0),
    "range_one_group_d48": (1, 4), "range_two_groups_d48": (2, 8), "range_groups_last_d48": (16, 0),
    "range_global_first_d48": (0, 0), "range_global_second_d48": (0, 0),
    "range_groups_last_d64": (16, 0), "range_global_first_d64": (0, 0),
    "range_one_group_d3": (1, 0), "range_two_groups_d3": (2, 0),
}


def last_level_plan(name):
    u, bits = cases.rows(name), cases.CASES[name][3]
    return quant_amd.host_median_cut_plan(u.shape[1], 1 << (bits - 1), len(u)), u.shape[1], 1 << (bits - 1)


def test_box_counts_lie_on_both_sides_of_every_boundary():
    assert sorted(EDGES) == sorted(n for n in cases.CASES if n.startswith(("hist_", "range_")))
    for name, (rg, hg) in EDGES.items():
        p, dim, boxes = last_level_plan(name)
        assert (p["range_groups"], p["hist_groups"]) == (rg, hg), name
        assert p["range_lds"] == (rg > 0) and p["hist_lds"] == (hg > 0)
        if rg:
            assert p["range_groups"] * p["range_group_boxes"] == boxes
            assert 2 * p["range_group_boxes"] * dim <= p["lds_words"] and rg <= cases.MAX_GROUPS
            assert p["range_cap"] == cases.CAP // rg
        if hg:
            assert p["hist_groups"] * p["hist_group_boxes"] == boxes and 256 * p["hist_group_boxes"] <= p["lds_words"]
        # each boundary is a boundary: one level less or more changes the variant as the names say
        half, twice = (quant_amd.host_median_cut_plan(dim, b, 5000) for b in (max(boxes // 2, 1), 2 * boxes))
        if "one_group" in name and name.startswith("range"):
            assert half["range_groups"] == 1 and twice["range_groups"] == 2
        if "groups_last" in name:
            assert twice["range_groups"] == 0 and twice["range_lds"] == 0
        if "global_first" in name:
            assert half["range_groups"] == cases.MAX_GROUPS
        if "global_second" in name:
            assert half["range_groups"] == 0
    one, two = last_level_plan("hist_one_group")[0], last_level_plan("hist_two_groups")[0]
    assert one["hist_group_boxes"] == 32 and two["hist_group_boxes"] == 32
    assert quant_amd.host_median_cut_plan(12, 512, 5000)["hist_groups"] == cases.MAX_GROUPS
    assert quant_amd.host_median_cut_plan(12, 1024, 5000)["hist_lds"] == 0
    # every edge case's last level cuts boxes (a level without rows to cut would run no atomics)
    for name in EDGES:
        assert cases.trace(name)[1][-1] >= 200 or cases.trace(name)[1][-1] >= last_level_plan(name)[2] // 2, name
    # a group's blocks see rows of other groups: the rows of one block (consecutive rows) spread over groups
    A = cases.trace("range_two_groups_d12")[0]
    assert len(np.unique(A[:256] // 1024)) == 2


# -- the C++ factory and the CLI --------------------------------------------------------------
def test_cpp_factory(tmp_path):
    if not os.path.exists(os.path.join(LIB, "libquant_amd.so")):
        pytest.fail("libquant_amd.so not built (run __graft_entry__.build())")
    exe = str(tmp_path / "test_median_cut_api")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "test_median_cut_api.cpp"), "-L" + LIB, "-lquant_amd", "-lqvq",
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
@pytest.mark.parametrize("extra", [["--refine", "3"], ["--fresh"], ["--reseed", "--refine", "3"]])
def test_cli_refine_flags_still_need_lbg(tmp_path, q, extra):
    r = run_quant(tmp_path, "-q", q, *extra)
    assert r.returncode == 2 and "LBG quantizer" in r.stderr


@pytest.mark.parametrize("q", ["1", "2"])
def test_cli_median_cut_has_no_exact_mode(tmp_path, q):
    r = run_quant(tmp_path, "-q", q, "-c", "2")
    assert r.returncode == 3 and "median cut has no exact mode" in r.stderr


def test_cli_abc_and_help(tmp_path):
    r = run_quant(tmp_path, "-q", "3")
    assert r.returncode == 3 and "quantizer not implemented" in r.stderr
    h = subprocess.run([QUANT, "--help"], capture_output=True, text=True).stdout
    assert "1 median cut" in h and "2 median cut refined" in h
