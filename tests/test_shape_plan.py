"""The tables of tests/test_gpu_shapes.py (tests/helpers/shape_cases.py) against the engine's
dispatch and against their own coverage claims, on the CPU, after the pattern of
tests/test_largek_plan.py: quant_amd.host_plan answers from the predicates the engine dispatches
with, so a case that claims a path really takes it; and the widths, row counts and raster
geometries the tables are there for are all still in them.  A pull request that moves a kernel's
capacity, or trims a table, fails here by the name of the case or of the condition it lost."""
import pytest

import quant_amd
from helpers import shape_cases as sc
from test_largek_plan import RECHECK, SEARCH, UPDATE, declared


@pytest.fixture(autouse=True)
def default_paths(monkeypatch):
    monkeypatch.delenv("QVQ_SEARCH", raising=False)
    monkeypatch.delenv("QVQ_KDTREE", raising=False)


# common.hpp, restated
def dp(D):
    return (D + 3) & ~3


def wide_dh(Dp):
    return (Dp + 7) & ~7


def wide_ks(Dp):
    return (2 * wide_dh(Dp) + 2 + 31) // 32


def plans(monkeypatch):
    """Every (label, declared fields, plan, D, K) of the tables: the assign shapes under the
    default dispatch and under QVQ_SEARCH=valu, the update shapes, the lbg levels."""
    out = []

    def add(label, fields, D, K, N):
        out.append((label, declared(fields), quant_amd.host_plan(D, K, N), D, K))

    def assign(label, c):
        for K, fields in c["assign"]:
            add("%s assign K=%d" % (label, K), fields, c["D"], K, c["N"])
            with monkeypatch.context() as m:
                m.setenv("QVQ_SEARCH", "valu")
                add("%s assign K=%d QVQ_SEARCH=valu" % (label, K), {"search": "valu"}, c["D"], K, c["N"])
        for K, fields in c["update"]:
            add("%s update K=%d" % (label, K), fields, c["D"], K, c["N"])

    for c in sc.WIDTH_CASES:
        label = "width D=%d" % c["D"]
        assign(label, c)
        for K, fields in c["levels"].items():
            assert K <= 1 << c["bits"], label
            add("%s lbg level K=%d" % (label, K), fields, c["D"], K, c["N"])
        if c["deep"]:
            for K, fields in c["deep"]["levels"].items():
                assert K == 1 << (c["deep"]["bits"]), label + ": the pruned level is the run's last"
                add("%s deep lbg level K=%d" % (label, K), fields, c["D"], K, c["N"])
    for c in sc.ROW_CASES:
        assign("rows D=%d N=%d" % (c["D"], c["N"]), c)
    return out


def test_cases_take_their_declared_paths(monkeypatch):
    bad = []
    for label, want, plan, _, _ in plans(monkeypatch):
        got = {f: plan[f] for f in want}
        if got != want:
            bad.append("%s: declared %s, host_plan %s" % (label, want, got))
    assert not bad, "\n".join(bad)


def test_first_streamed_k_is_the_boundary():
    """FIRST_STREAMED[Dp] is the first K assign_wide_kernel streams, for every Dp and any pad."""
    for Dp, K in sc.FIRST_STREAMED.items():
        for D in range(Dp - 3, Dp + 1):
            if D == 12:                      # the D = 12 kernels have no wide search
                continue
            assert quant_amd.host_plan(D, K - 1, 2000)["cb_resident"] == 1, "D=%d K=%d" % (D, K - 1)
            assert quant_amd.host_plan(D, K, 2000)["cb_resident"] == 0, "D=%d K=%d" % (D, K)


def test_width_table_covers_what_it_claims():
    Ds = [c["D"] for c in sc.WIDTH_CASES]
    assert len(set(Ds)) == len(Ds)
    for Dp in range(4, 65, 4):
        assert any(dp(D) == Dp for D in Ds), "no width with Dp = %d" % Dp
    for pad in range(4):
        assert any(dp(D) - D == pad for D in Ds), "no width with %d pad bytes" % pad
    assert 1 in Ds, "D = 1 is gone"
    assert 64 in Ds, "D = 64 (no pad at the widest Dp) is gone"
    assert any(dp(D) == 64 and D < 64 for D in Ds), "Dp = 64 with pad bytes is gone"
    assert any(D in (9, 10, 11) for D in Ds), "Dp = 12 off the D = 12 kernels is gone"
    assert 12 not in Ds      # D = 12 is ROW_CASES' and largek_cases'
    for ks in range(1, 6):
        assert any(wide_ks(dp(D)) == ks for D in Ds), "no width with wide_ks = %d" % ks
    assert any(wide_dh(dp(D)) != dp(D) for D in Ds) and any(wide_dh(dp(D)) == dp(D) for D in Ds)
    assert sum(D % 3 != 0 for D in Ds) >= 6, "fewer than six widths that no block shape gives"
    # mean_sums_kernel's three bodies, each at both ends of its range
    for Dp in (4, 16, 20, 32, 36, 64):
        assert any(dp(D) == Dp for D in Ds), "mean_sums_kernel boundary Dp = %d" % Dp
    Ns = [c["N"] for c in sc.WIDTH_CASES]
    for c in sc.WIDTH_CASES:
        N = c["N"]
        assert 1024 < N <= 3000 and N % 4 != 0 and N % 64 != 0, "width D=%d: N = %d is not ragged" % (c["D"], N)
    assert len(set(Ns)) > 1
    for D in sc.REFINE_WIDTHS:
        assert D in Ds, "refine width D=%d is no width case" % D
    assert {1, 10, 32, 64} <= set(sc.REFINE_WIDTHS) and len(sc.REFINE_WIDTHS) >= 6
    deep = [c for c in sc.WIDTH_CASES if c["deep"]]
    assert len({wide_ks(dp(c["D"])) for c in deep}) >= 3, "deeper lbg runs at fewer than three wide_ks"
    assert any(c["D"] >= 60 for c in deep), "no deeper lbg run at D >= 60"


def test_every_width_reaches_both_sides(monkeypatch):
    P = plans(monkeypatch)
    for c in sc.WIDTH_CASES + [c for c in sc.ROW_CASES if c["D"] != 12]:
        tag = ("width D=%d " % c["D"]) if "levels" in c else "rows D=%d N=%d " % (c["D"], c["N"])
        mine = [(p, K) for label, _, p, D, K in P if label.startswith(tag)]
        assert mine, tag
        assert any(p["search"] in (SEARCH["small"], SEARCH["valu"]) for p, _ in mine), tag + "small or valu search"
        assert any(p["search"] == SEARCH["wide"] and p["cb_resident"] == 1 for p, _ in mine), tag + "resident wide"
        assert any(p["search"] == SEARCH["wide"] and p["cb_resident"] == 0 for p, _ in mine), tag + "streamed wide"
        assert any(p["update"] == UPDATE["runs"] for p, _ in mine), tag + "update runs"
        assert any(p["update"] == UPDATE["sorted"] for p, _ in mine), tag + "update sorted"
        if "levels" in c:
            ks = [K for K, _ in c["assign"]]
            assert any(K < 128 for K in ks) and any(128 < K <= 400 and K % 32 for K in ks), tag
            assert c["host_tie_k"] in ks, tag
            (k0, _), (k1, _) = c["update"]
            assert k0 * c["D"] < 1536 <= k1 * c["D"] and k1 == k0 + 1, tag + "the runs / sorted boundary"


def test_d12_rows_reach_the_mfma_paths(monkeypatch):
    P = plans(monkeypatch)
    for N in sc.ROW_NS:
        tag = "rows D=12 N=%d " % N
        mine = [p for label, _, p, D, K in P if label.startswith(tag) and "QVQ_SEARCH" not in label]
        for field, names in (("search", ("small", "mf32")), ("recheck", ("mf32", "staged"))):
            table = SEARCH if field == "search" else RECHECK
            for name in names:
                assert any(p[field] == table[name] for p in mine), tag + "%s %s" % (field, name)
        for field in ("fused", "prune"):
            for v in (0, 1):
                assert any(p[field] == v for p in mine), tag + "%s %d" % (field, v)
        assert any(p["update"] == UPDATE["runs"] for p in mine) and any(p["update"] == UPDATE["sorted"] for p in mine)


def test_row_table_covers_what_it_claims():
    assert sorted({c["D"] for c in sc.ROW_CASES}) == [12, 27, 48]
    for D in (12, 27, 48):
        assert [c["N"] for c in sc.ROW_CASES if c["D"] == D] == sc.ROW_NS, "D=%d misses row counts" % D
    Ns = sc.ROW_NS
    for N in (1, 2, 3, 63, 64, 65, 255, 257, 1023, 1025):
        assert N in Ns, "N = %d is gone" % N
    assert any(4 <= N < 64 and N % 4 == 1 for N in Ns), "no N < 64 with N % 4 = 1"
    assert any(4097 <= N <= 4200 and N % 4 == 3 for N in Ns), "no N in 4097..4200 with N % 4 = 3"
    assert any(8193 <= N <= 8300 and N % 64 == 1 for N in Ns), "no N in 8193..8300 with N % 64 = 1"
    for c in sc.ROW_CASES:
        N, bits = c["N"], c["bits"]
        assert bits <= 10
        if N <= 3:
            assert bits <= 3
        elif N <= 257:
            assert 1 << bits > N, "N=%d: no level with more code vectors than rows" % N
        else:
            assert bits == 10
        assert sc.row_partner(N) in Ns and sc.row_partner(N) != N


def test_raster_table_covers_every_geometry():
    have = set()
    for c in sc.RASTER_CASES:
        assert 3 * c["bw"] * c["bh"] <= 64 and max(c["xs"], c["ys"]) <= 130, c["name"]
        assert 1 << c["bits"] <= 256, c["name"]
        have |= sc.raster_classes(c)
    for cls in sc.RASTER_CLASSES:
        assert cls in have, "no raster case of class %s" % cls
    one = next(c for c in sc.RASTER_CASES if c["xs"] == 1 and c["ys"] == 1)
    assert one["bits"] <= 1
    un = next(c for c in sc.RASTER_CASES if c["name"] == sc.UNALIGNED_RASTER)
    assert any(k.startswith("2x2_tile22") for k in sc.raster_classes(un)), "the unaligned case is off tile22's condition"
    names = [c["name"] for c in sc.RASTER_CASES]
    assert len(set(names)) == len(names)
