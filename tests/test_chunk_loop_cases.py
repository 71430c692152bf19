"""tests/helpers/chunk_loop_cases.py held to what its cases are for, on the CPU: for several CU
counts the row counts give the wave / chunk patterns the GPU test's names promise, and the levels
and codebooks the GPU test runs dispatch to the D = 12 MFMA search.  A part with another CU count,
or an edit of the table, cannot quietly turn a case into something else."""
import pytest

import quant_amd
from helpers import chunk_loop_cases as cl
from helpers import shape_cases as sc

CU_COUNTS = (64, 256, 304)


@pytest.fixture(autouse=True)
def default_paths(monkeypatch):
    monkeypatch.delenv("QVQ_SEARCH", raising=False)
    monkeypatch.delenv("QVQ_KDTREE", raising=False)


@pytest.mark.parametrize("G", CU_COUNTS)
def test_row_counts_give_the_named_patterns(G):
    W = cl.waves(G)
    N = cl.row_counts(G)
    assert list(N) == list(cl.NAMES)

    p = cl.pattern(N["two_chunks"], G)
    assert p["nchunks"] == 2 and p["last_rows"] == 1
    assert p["waves_by_chunks"] == {0: W - 2, 1: 2}          # every other wave runs no chunk

    p = cl.pattern(N["one_each_ragged"], G)
    assert p["nchunks"] == W and p["last_rows"] == 63
    assert p["waves_by_chunks"] == {1: W}                    # no workgroup has a slot to claim
    assert p["last_wave"] == W - 1

    p = cl.pattern(N["one_extra_row"], G)
    assert p["nchunks"] == W + 1 and p["last_rows"] == 1
    assert p["waves_by_chunks"] == {1: W - 1, 2: 1}
    assert p["last_wave"] == 0 and p["last_wave_chunks"] == 2

    p = cl.pattern(N["two_each_plus"], G)
    assert p["nchunks"] == 2 * W + 1 and p["last_rows"] == 63
    assert p["waves_by_chunks"] == {2: W - 1, 3: 1}
    assert p["last_wave"] == 0 and p["last_wave_chunks"] == 3


def test_largest_case_stays_small():
    """On 256 CUs the largest case is 524,351 rows: milliseconds on the GPU, under a second of oracle."""
    assert max(cl.row_counts(256).values()) == 524351
    assert max(cl.row_counts(304).values()) < 2 ** 20


@pytest.mark.parametrize("G", CU_COUNTS)
def test_cases_run_the_mfma_search(G):
    """The lbg depth of every case reaches K >= 64 (the large cases K = 1024: 4-code-vector units at
    K = 64 / 128, pruned from K = 256, the fp32 table out of LDS at K = 1024), and those levels and the
    qvq_assign codebooks dispatch to assign_mf32_kernel."""
    mf32 = quant_amd.PLAN_SEARCH_MF32
    for name, N in cl.row_counts(G).items():
        bits = min(10, sc.row_bits(N))
        assert bits == (10 if name in cl.LARGE else 9)
        for level in range(6, bits):      # the search of level l + 1 runs on K = 2^l code vectors ... 2^(bits-1)
            plan = quant_amd.host_plan(12, 1 << level, N)
            assert plan["search"] == mf32, (name, level)
    N = cl.row_counts(G)[cl.UNFUSED_CASE]
    plans = {K: quant_amd.host_plan(12, K, N) for K in cl.UNFUSED_KS}
    assert all(p["search"] == mf32 for p in plans.values())
    assert [plans[K]["prune"] for K in cl.UNFUSED_KS] == [0, 1, 1]
    assert [plans[K]["c32_staged"] for K in cl.UNFUSED_KS][:2] == [1, 1]
    assert cl.NORMAL_CASE in cl.LARGE and cl.UNFUSED_CASE in cl.LARGE
