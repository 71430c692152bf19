"""The exact sums' 16-bit register fields against the launch shapes that fill them (no GPU).

mean_sums_kernel adds a thread's rows in 16-bit fields and counts nothing; the grid of
quant_amd.host_mean_grid (mean_plan.hpp, the function launch_mean_sums calls) is what keeps every
thread within the 257 adds of 255 a field holds.  tests/helpers/sums_capacity_ref.py restates who
adds what.  Here: the restatement is honest (every code word once, on a small grid that runs all
three loops), the bound holds at every listed N, it did not hold under the grid the launcher used to
take, the launches up to 2^24 rows are the ones it used to make, and the device cases of
tests/helpers/sums_capacity_cases.py meet the conditions they are there for."""
import os
import re

import numpy as np
import pytest

import quant_amd
from helpers import sums_capacity_cases as sc
from helpers import sums_capacity_ref as ref
from oracle import oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "quant_amd", "csrc")
DIMS = [4, 12, 16, 20, 48, 64]   # Dp: both chunk-loop instantiations' neighbours, each U of the group loop


def _listed_n():
    ns = set(range(1, 5001))
    ks = list(range(250, 263)) + list(range(381, 385)) + list(range(511, 514))
    for c in [k << 18 for k in ks] + [1 << 26, 1 << 27, 1 << 31]:
        ns.update(range(c - 300, c + 301))
    ns.update(range((1 << 32) - 300, 1 << 32))
    return sorted(ns)


LISTED = _listed_n()


def test_the_list_has_every_residue_at_every_edge():
    """Windows of +-300 rows: N mod 4 = 0 .. 3 and N mod 256 on both sides of 4 (a leftover group or none)."""
    for c in [250 << 18, 1 << 26, 384 << 18, 1 << 27, 1 << 31, (1 << 32) - 150]:
        near = [n for n in LISTED if abs(n - c) <= 150]
        assert {n % 4 for n in near} == {0, 1, 2, 3}
        assert {(n % 256 >= 4, n % 4 != 0) for n in near} == {(a, b) for a in (False, True) for b in (False, True)}


def test_constants_match_the_sources():
    src = {f: open(os.path.join(CSRC, f)).read() for f in ("mean_plan.hpp", "k_misc.hip", "k_assign.hip")}
    p = quant_amd.host_mean_grid(1 << 22, 12)
    for name, val in (("MEAN_THREADS", p["block"]), ("MEAN_U", p["chunks_in_flight"]), ("MEAN_GROUP_ROWS", p["group_rows"]),
                      ("MEAN_CHUNK_GROUPS", p["chunk_groups"]), ("MEAN_FIELD_ADDS", sc.FIELD_ADDS)):
        m = re.search(r"constexpr \w+ %s = (\d+);" % name, src["mean_plan.hpp"])
        assert m and int(m.group(1)) == val, name
    assert sc.FIELD_ADDS == ref.FIELD_MAX // ref.U_MAX
    assert 'mean_plan(N, Dp).grid' in src["k_misc.hip"]                       # the launcher takes the plan's grid
    assert "acc[DP] == %d" % sc.RUN_CAP in src["k_misc.hip"]                  # update_runs_kernel's flush
    assert "acc[MF_D] == %d" % sc.RUN_CAP in src["k_assign.hip"]              # assign_small_kernel's flush
    assert "return DP > 32 ? 512 : %d;" % sc.URUN_THREADS in src["k_misc.hip"]
    assert "constexpr int R = DP <= 16 ? %d :" % sc.URUN_ROWS in src["k_misc.hip"]
    assert "const uint64_t lanes = (uint64_t)grid * %d * 64;" % sc.SMALL_WAVES in src["k_assign.hip"]
    # the byte terms: u <= 255 at 0x7F, the low term at most 128
    hi, lo = quant_amd.host_row_terms(np.arange(256, dtype=np.uint8))
    assert int(hi.max()) == ref.U_MAX == int(hi[0x7F]) and int(hi[0x80]) == 0 and int(lo.max()) <= 128


def test_plan_fields():
    for dim in (1, 3, 12, 16, 17, 33, 64):
        dp = (dim + 3) & ~3
        p = quant_amd.host_mean_grid(12345, dim)
        assert p["chunk_loop"] == (dp <= 16) and p["groups_in_flight"] == (4 if dp <= 16 else 2 if dp <= 32 else 1)
        assert (p["block"], p["group_rows"], p["chunk_groups"], p["chunks_in_flight"]) == (1024, 4, 64, 4)
    for bad in ((0, 12), (1 << 32, 12), (100, 0), (100, 65)):
        with pytest.raises(quant_amd.QVQError):
            quant_amd.host_mean_grid(*bad)


# ---- the restatement is honest ------------------------------------------------------------------------
MODEL = {"blocks": 2, "block": 128, "group_rows": 4, "chunk_groups": 64, "chunks_in_flight": 4}
# 2 * 128 threads = 4 waves.  A chunk is 256 rows: 4 * 4 * 256 rows fill one trip of the chunk loop
# (4 in flight), more take a second trip; N mod 256 >= 4 leaves groups, N mod 4 a tail.
MODEL_N = [1, 3, 4, 7, 255, 256, 259, 1023, 1024 + 4 * 37 + 3, 4096 + 255, 4 * 4 * 256 * 2 + 256 * 3 + 4 * 9 + 2, 9999,
           8 * 4 * 256 + 4 * 63 + 3]


@pytest.mark.parametrize("dp", DIMS)
def test_model_counts_every_word_once(dp):
    plan = dict(MODEL, chunk_loop=int(dp <= 16), groups_in_flight=4 if dp <= 16 else 2 if dp <= 32 else 1)
    ran = set()
    for n in MODEL_N:
        words, adds = ref.simulate(n, dp, plan)
        assert words.min() == 1 and words.max() == 1, (n, dp)
        # a thread's slots fill evenly, and the arithmetic forms give the literal loops' counts
        assert (adds == adds[:, :1]).all()
        per = ref.adds_per_thread(n, dp, plan)
        np.testing.assert_array_equal(adds[:, 0], per)
        assert per.sum() == n and per.max() == per[0] == ref.max_adds(n, dp, plan)
        groups = n // 4
        chunks = groups // 64 if dp <= 16 else 0
        ran |= {"chunks"} if chunks else set()
        ran |= {"second trip"} if chunks > 4 * 4 else set()
        ran |= {"groups"} if groups - 64 * chunks else set()
        ran |= {"groups second trip"} if groups - 64 * chunks > 256 * plan["groups_in_flight"] else set()
        ran |= {"tail"} if n % 4 else set()
    assert ran == ({"chunks", "second trip", "groups", "tail"} if dp <= 16 else {"groups", "groups second trip", "tail"})


@pytest.mark.parametrize("dp", [12, 48])
def test_thread_zero_is_the_busiest_at_full_size(dp):
    for n in (sc.N_EDGE, sc.N_BELOW, 1 << 26, 8191 ** 2, 100138758, 4999, (1 << 31) + 7):
        for plan in (quant_amd.host_mean_grid(n, dp), ref.with_blocks(quant_amd.host_mean_grid(n, dp), ref.parent_blocks(n))):
            per = ref.adds_per_thread(n, dp, plan)
            assert per.sum() == n and per.max() == per[0] == ref.max_adds(n, dp, plan)


# ---- the bound ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dp", DIMS)
def test_no_field_carries_at_any_listed_n(dp):
    bad = [(n, ref.max_adds(n, dp, p)) for n in LISTED for p in [quant_amd.host_mean_grid(n, dp)]
           if ref.U_MAX * ref.max_adds(n, dp, p) > ref.FIELD_MAX]
    assert not bad, bad[:10]


@pytest.mark.parametrize("dp", DIMS)
def test_the_former_grid_carried(dp):
    """The grid the launcher took before it counted adds (a block per 2^18 rows, 256 below): with the
    chunk loop, 261 adds from N = 66 060 548; without it (Dp > 16) 257 at the most, which fits."""
    worst = max((ref.max_adds(n, dp, ref.with_blocks(quant_amd.host_mean_grid(n, dp), ref.parent_blocks(n))), n)
                for n in LISTED)
    first = next((n for n in LISTED
                  if not ref.fits(n, dp, ref.with_blocks(quant_amd.host_mean_grid(n, dp), ref.parent_blocks(n)))), None)
    print(dp, "worst", worst, "first", first)
    if dp <= 16:
        assert worst[0] == 261 and first == 66060548
    else:
        assert worst[0] == 257 and first is None


@pytest.mark.parametrize("n, blocks, adds, fit", [(66060548, 256, 260, False), ((1 << 26) - 249, 256, 261, False),
                                                  (1 << 26, 256, 256, True), (8191 ** 2, 256, 257, True),
                                                  (100138758, 382, 261, False)])
def test_the_former_grid_worked_counts(n, blocks, adds, fit):
    now = quant_amd.host_mean_grid(n, 12)
    was = ref.with_blocks(now, ref.parent_blocks(n))
    assert (was["blocks"], ref.max_adds(n, 12, was), ref.fits(n, 12, was)) == (blocks, adds, fit)
    assert ref.fits(n, 12, now) and (now["blocks"] == blocks) == fit   # more blocks only where it carried


# ---- the launches that were right stay -----------------------------------------------------------------
# (rows, dim) -> summing blocks, from the former formula max(ceil(N / 2^18), 1, min(ceil(N / 4096), 256))
FORMER_GRIDS = [
    (1, 3, 1), (4095, 12, 1), (4096, 12, 1), (4097, 12, 2), (128 * 128 // 4, 12, 1), (1000003, 3, 245),
    (1 << 20, 48, 256),        # C4: 4096 x 4096, 4 x 4 blocks
    (1 << 20, 12, 256), (1048575, 12, 256), (1048577, 27, 256),
    (1 << 22, 12, 256),        # C3: 4096 x 4096, 2 x 2 blocks
    (1 << 22, 3, 256), (4194319, 12, 256), (1 << 24, 12, 256), (1 << 24, 3, 256), (1 << 24, 48, 256),
    ((1 << 24) - 1, 64, 256), ((1 << 24) - 253, 4, 256),
]


def test_launches_up_to_2_24_rows_are_unchanged():
    for n, dim, blocks in FORMER_GRIDS:
        assert ref.parent_blocks(n) == blocks, (n, dim)
        assert quant_amd.host_mean_grid(n, dim)["blocks"] == blocks, (n, dim)
    for dp in DIMS:   # and every listed N below 2^24, and the edges of 2^24
        for n in [n for n in LISTED if n <= 5000] + list(range((1 << 24) - 600, (1 << 24) + 1)):
            assert quant_amd.host_mean_grid(n, dp)["blocks"] == ref.parent_blocks(n), (n, dp)


# ---- the device cases meet their conditions -----------------------------------------------------------
def test_palette():
    b, lo = sc.lo_byte()
    assert lo == 128
    for dim in (3, 12):
        pal = sc.palette(dim, b)
        assert (pal[0] == 0x7F).all() and (pal[1] == 0x80).all() and (pal[2] == b).all()
        assert len({bytes(r) for r in pal}) == sc.P


def test_rows_are_what_the_cases_say():
    for case in (sc.S12, sc.S3):
        for i0 in (0, sc.BAND - 3000, 7 * sc.BAND - 3000, case.n - 3000):
            R = sc.rows_numpy(case, i0, i0 + 3000)
            i = np.arange(i0, i0 + 3000)
            assert (R[:, list(case.fixed)] == 0x7F).all()
            pal = sc.palette(case.dim, sc.lo_byte()[0])
            free = [d for d in range(case.dim) if d not in case.fixed]
            plain = ~sc.is_sprinkled(i)
            np.testing.assert_array_equal(R[plain][:, free], pal[(i[plain] >> 20) % sc.P][:, free])
            spr = R[~plain][:, free]
            assert len(spr) in (2, 3) and len({bytes(r) for r in spr}) == len(spr)   # ~1 in 1009, pseudo-random
    assert sc.SPRINKLE % 64 and sc.SPRINKLE % 4   # no lane or round keeps the sprinkled rows to itself


def test_lbg5_keeps_eight_cells_on_the_palette():
    """The oracle on S12 with bands of 32 rows in place of 2^20 (the same palette, proportions and sprinkled rows)."""
    X = oracle.lut(oracle.SCALED)[sc.rows_numpy(sc.S12, 0, 65 * 32 + 7, shift=5)]
    _, A, _ = oracle.lbg(X, 5, sum_mode=1)
    assert np.count_nonzero(np.bincount(A, minlength=32)) >= 8


@pytest.mark.parametrize("cus", [256, 128, 64])
def test_device_cases_reach_their_edges(cus):
    n = sc.N_EDGE
    assert n % 4 == 3 and 4 <= n % 256 < 8                       # tail rows, one leftover group
    assert sc.small_rows_per_lane(n, cus) > sc.RUN_CAP           # assign_small_kernel's cap flush
    assert sc.update_rows_per_lane(n, cus) > sc.RUN_CAP          # update_runs_kernel's, at A = 0
    assert 64 * sc.small_rows_per_lane(n, 256) < sc.BAND         # a wave's rows lie in one band (two at an edge)
    for case in (sc.S12, sc.S3, sc.S12_BELOW):
        dp = (case.dim + 3) & ~3
        now = quant_amd.host_mean_grid(case.n, case.dim)
        was = ref.with_blocks(now, ref.parent_blocks(case.n))
        assert ref.max_adds(case.n, dp, was) == 261 > sc.FIELD_ADDS and ref.max_adds(case.n, dp, now) <= sc.FIELD_ADDS
    assert ref.parent_blocks(sc.N_BELOW) == 256 and -(-sc.N_BELOW // (1 << 18)) == 256   # the cap, at its edge
    for K in (1, 2, 5):
        for case in (sc.S12, sc.S3):
            assert quant_amd.host_plan(case.dim, K, case.n)["update"] == quant_amd.PLAN_UPDATE_RUNS
    for bits in range(1, 6):
        p = quant_amd.host_plan(12, 1 << bits, n)
        assert p["search"] == quant_amd.PLAN_SEARCH_SMALL and p["fused"] == 1
    # a device of more CUs no longer reaches the caps at N_EDGE (the device test then skips)
    assert sc.small_rows_per_lane(n, 304) <= sc.RUN_CAP and sc.update_rows_per_lane(n, 304) <= sc.RUN_CAP
