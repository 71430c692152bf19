"""The case table of the decode tests (tests/helpers/decode_cases.py, run by
tests/test_gpu_decode_paths.py) held to the engine's dispatch and to what it claims, on the CPU
(DESIGN.md 6.5): every declared qvq_decode_plan field is what quant_amd.host_decode_plan answers; the
table reaches all 16 + 2 + 1 kernel instantiations, both sides of the 48 KB boundary on both row
kernels, a second round of the grid-stride loop on the four capped paths and every alignment
fallback; its rasters hold the wraps of the reference's untile loop, measured on the oracle's own
output; and the identity-coded codebooks have no two equal pixels.

On the wraps.  A pixel (x, y) is written by the block pixels (x - m, y + m ys), m = 0, 1, ...; the
last write in loop order survives.  The surviving write has m = 0 or m = 1 and never more: with
bh <= ys the overhang is below bh <= ys, so no write comes from two raster rows up; with bh > ys
there is one block row, every write of a pixel comes from the same row of blocks, and the largest
x - m, that is m = 0, is last.  Writes with m >= 2 do exist (bh > ys) and must lose, so the tests
ask for them among all writes of the loop, and for m = 0 and m = 1 among the survivors."""
import numpy as np
import pytest

import quant_amd
from helpers import decode_cases as dc


def _plan_errors(cases):
    bad = []
    for c in cases:
        plan = quant_amd.host_decode_plan(c["K"], *dc.shape(c))
        got = {f: plan[f] for f in c["plan"]}
        if got != c["plan"]:
            bad.append("%s: declared %s, host_decode_plan %s" % (c["key"], c["plan"], got))
    return bad


def test_cases_take_their_declared_paths():
    bad = _plan_errors(dc.TABLE)
    assert not bad, "\n".join(bad)
    assert all({"kernel", "H", "lds", "coal"} <= set(c["plan"]) for c in dc.TABLE)


def test_sweep_takes_its_declared_paths():
    n, fam = 0, set()
    for bw in dc.SWEEP_BW:
        for xs, ys, _, bh in dc.sweep_shapes(bw):
            p = quant_amd.host_decode_plan(dc.SWEEP_K, xs, ys, bw, bh)
            assert p["kernel"] == dc.sweep_kernel(ys, bh), (xs, ys, bw, bh)
            assert p["rounds"] == 1 and p["grid"] == 1
            assert p["lds"] == (p["kernel"] != dc.PIXELS)
            fam.add(p["kernel"])
            n += 1
    assert n == 5508 and fam == {dc.PIXELS, dc.ROWS, dc.ROWS_H}


ALL_INSTANTIATIONS = ({(dc.ROWS_H, H, lds, coal) for H in (1, 2, 4, 8) for lds in (0, 1) for coal in (0, 1)} |
                      {(dc.ROWS, 0, 0, 0), (dc.ROWS, 0, 1, 0), (dc.PIXELS, 0, 0, 0)})


def test_table_reaches_every_instantiation():
    """All 16 + 2 + 1, from what host_decode_plan answers and not from what the table declares; the
    sixteen ROWS_H ones at both of their raster heights."""
    assert len(ALL_INSTANTIATIONS) == 19
    reached = {}
    for c in dc.TABLE:
        reached.setdefault(dc.instantiation(quant_amd.host_decode_plan(c["K"], *dc.shape(c))), []).append(c)
    missing = ALL_INSTANTIATIONS - set(reached)
    assert not missing, "no table case on %s" % sorted(missing)
    assert set(reached) == ALL_INSTANTIATIONS
    for inst, cases in reached.items():
        if inst[0] == dc.ROWS_H:
            assert ({512, 1024} if inst[3] else {8, 520}) <= {c["ys"] for c in cases}, inst
            assert all(c["xs"] % c["bw"] for c in cases if c["bw"] > 1 and c not in dc.CAP_CASES), \
                "a ragged last block column"
    assert [dc.instantiation(c["plan"]) for c in dc.first_per_instantiation()] == list(dict.fromkeys(
        dc.instantiation(c["plan"]) for c in dc.TABLE))
    assert len(dc.first_per_instantiation()) == 19


@pytest.mark.parametrize("kernel", [dc.ROWS_H, dc.ROWS], ids=["ROWS_H", "ROWS"])
def test_table_holds_both_sides_of_the_lds_boundary(kernel):
    """One case with K D = 49152 exactly (in LDS) and one with K one larger at the same block shape."""
    cases = [c for c in dc.TABLE if c["plan"]["kernel"] == kernel]
    full = {dc.shape(c): c for c in cases if c["K"] * c["bw"] * c["bh"] * 3 == dc.LDS_CB_BYTES}
    assert full
    pairs = [(full[dc.shape(c)], c) for c in cases if dc.shape(c) in full and c["K"] == full[dc.shape(c)]["K"] + 1]
    assert pairs
    for a, b in pairs:
        pa, pb = (quant_amd.host_decode_plan(c["K"], *dc.shape(c)) for c in (a, b))
        assert (pa["lds"], pb["lds"]) == (1, 0) and pa["kernel"] == pb["kernel"] == kernel
        stage = dc.STAGE_BYTES if pa["coal"] else 0
        assert (pa["lds_bytes"], pb["lds_bytes"]) == (dc.LDS_CB_BYTES + stage, stage)
    # every non-LDS case sits at the smallest K past the boundary, bar C4's own K
    for c in cases:
        if not c["plan"]["lds"] and c["key"] != "rowsh-c4":
            assert c["K"] == dc.k_past_lds(c["bw"], c["bh"]), c["key"]
    assert any(c["K"] * c["bw"] * c["bh"] * 3 % 2 for c in cases) or kernel == dc.ROWS   # an odd byte count in LDS


def test_table_holds_the_named_cases():
    hp = quant_amd.host_decode_plan
    rows_h = [c for c in dc.TABLE if hp(c["K"], *dc.shape(c))["kernel"] == dc.ROWS_H]
    rows = [c for c in dc.TABLE if hp(c["K"], *dc.shape(c))["kernel"] == dc.ROWS]
    # C4's block shape and K, from global memory with coalesced stores
    assert any((c["bw"], c["bh"], c["K"]) == (4, 4, 4096) and dc.instantiation(c["plan"]) == (dc.ROWS_H, 4, 0, 1)
               for c in rows_h)
    # an odd byte count staged in LDS, behind it the wave staging at the next multiple of 16
    odd = [c for c in rows_h if c["K"] * c["bw"] * c["bh"] * 3 % 2 and c["plan"]["lds"] and c["plan"]["coal"]]
    assert odd and all(hp(c["K"], *dc.shape(c))["lds_bytes"] % 16 == 0 for c in odd)
    # the full LDS codebook with and without the staging
    assert {c["plan"]["coal"] for c in rows_h if c["K"] * c["bw"] * c["bh"] * 3 == dc.LDS_CB_BYTES} == {0, 1}
    # ROWS: every (ys, h, bw) of the product, h = ys = 16, h > ys, and an overhang outside LDS
    have = {(c["ys"], c["bh"], c["bw"]) for c in rows}
    assert {(ys, h, bw) for ys in (8, 16, 24) for h in (3, 5, 6, 7, 9) for bw in (1, 2, 3, 4)} <= have
    assert any(ys == h == 16 for ys, h, _ in have) and any(h > ys and bw >= 3 for ys, h, bw in have)
    assert any(not c["plan"]["lds"] and c["ys"] % c["bh"] for c in rows)
    assert any(not c["plan"]["lds"] and c["ys"] % c["bh"] == 0 for c in rows)


def test_cap_cases_go_round_twice():
    want = {(dc.ROWS_H, 1, 1): dc.LDS_GRID_CAP, (dc.ROWS_H, 1, 0): dc.LDS_GRID_CAP, (dc.ROWS, 1, 0): dc.LDS_GRID_CAP,
            (dc.PIXELS, 0, 0): dc.GRID_CAP}
    got = {}
    for c in dc.TABLE:
        p = quant_amd.host_decode_plan(c["K"], *dc.shape(c))
        items = c["xs"] * c["ys"] // (1 if p["kernel"] == dc.PIXELS else 8)
        assert p["rounds"] == -(-items // (p["grid"] * dc.THREADS)), c["key"]
        if p["rounds"] >= 2:
            got[(p["kernel"], p["lds"], p["coal"])] = p["grid"]
            assert p["grid"] * dc.THREADS < items < 2 * p["grid"] * dc.THREADS   # a short second round
        else:
            assert p["grid"] == -(-items // dc.THREADS), c["key"]
    assert got == want


def test_alignment_cases_reach_every_fallback():
    by_key = {c["key"]: c for c in dc.TABLE}
    routes = set()
    for a in dc.ALIGN_CASES:
        c = by_key[a["base"]]
        flags = ((dc.RASTER_UNALIGNED if a["off_rgb"] % 8 else 0) | (dc.INDEX_UNALIGNED if a["off_idx"] % 16 else 0) |
                 (dc.CODEBOOK_ODD if a["off_cb"] % 2 else 0))
        assert flags == a["flags"] and flags in (1, 4, 8), a["key"]            # one misalignment at a time
        aligned = dc.instantiation(quant_amd.host_decode_plan(c["K"], *dc.shape(c)))
        got = dc.instantiation(quant_amd.host_decode_plan(c["K"], *dc.shape(c), flags))
        assert got == a["inst"], a["key"]
        assert aligned[0] != dc.PIXELS
        routes.add((dc.FAMILY[aligned[0]], flags, aligned[2], dc.FAMILY[got[0]]) + ((aligned[1],) if flags == 8 else ()))
    for fam in ("ROWS_H", "ROWS"):
        assert (fam, dc.RASTER_UNALIGNED, 1, "PIXELS") in routes
        assert (fam, dc.INDEX_UNALIGNED, 1, "PIXELS") in routes
    assert ("ROWS_H", dc.CODEBOOK_ODD, 1, "ROWS_H", 4) in routes              # byte-wise staging, the same kernel
    assert ("ROWS", dc.CODEBOOK_ODD, 1, "ROWS", 0) in routes
    assert ("ROWS_H", dc.CODEBOOK_ODD, 0, "ROWS", 4) in routes                # the 16-bit global reads avoided
    assert ("ROWS_H", dc.CODEBOOK_ODD, 0, "ROWS", 2) in routes
    assert ("ROWS_H", dc.CODEBOOK_ODD, 0, "ROWS_H", 1) in routes              # H = 1 reads bytes
    assert ("ROWS", dc.CODEBOOK_ODD, 0, "ROWS", 0) in routes
    assert {(a["off_rgb"], a["off_idx"]) for a in dc.ALIGN_CASES} >= {(1, 0), (4, 0), (0, 4), (0, 8)}


# ---------------------------------------------------------------------------------------------
# the wraps, from the oracle's untile
# ---------------------------------------------------------------------------------------------
def _wrap_stats(shapes):
    """Over the shapes: pixels whose surviving write has m = 0 / m = 1, pixels also written with m >= 2,
    pixels where the survivor is not the largest m of its own block column (decode_writer's m* < M),
    and where it is (m* = M > 0)."""
    s = {"m0": 0, "m1": 0, "m2_written": 0, "below_M": 0, "at_M": 0, "other_column": 0}
    for xs, ys, bw, bh in shapes:
        m, dx = dc.writers(xs, ys, bw, bh)
        count, m_all, m_own, m_last = dc.loop_writes(xs, ys, bw, bh)
        assert np.array_equal(m, m_last), "the restated loop's last write is not the oracle's"
        assert m.min() >= 0 and m.max() <= 1 and (m <= m_own).all() and (m_own <= m_all).all()
        if ys % bh == 0:
            assert not m.any(), "no overhang: a plain gather"
        s["m0"] += int(np.sum(m == 0))
        s["m1"] += int(np.sum(m == 1))
        s["m2_written"] += int(np.sum(m_all >= 2))
        s["below_M"] += int(np.sum(m < m_own))
        s["at_M"] += int(np.sum((m == m_own) & (m > 0)))
        s["other_column"] += int(np.sum(m_own < m_all))
    return s


def test_rows_cases_hold_every_wrap():
    s = _wrap_stats([dc.shape(c) for c in dc.ROWS_CASES])
    print(s)
    assert all(v > 0 for v in s.values()), s
    # the case with bh > ys alone: writes from two raster rows up, all of which lose
    one = _wrap_stats([dc.shape(c) for c in dc.ROWS_CASES if c["key"] == "rows-ys8-h20"])
    assert one["m2_written"] > 0 and one["below_M"] > 0 and one["m1"] == 0


@pytest.mark.parametrize("bw", list(dc.SWEEP_BW))
def test_sweep_holds_every_wrap(bw):
    pix = [s for s in dc.sweep_shapes(bw) if dc.sweep_kernel(s[1], s[3]) == dc.PIXELS]
    s = _wrap_stats(pix)
    print(s)
    assert s["m0"] > 0
    if bw == 1:      # one pixel column per block: every later write comes from another block column
        assert s["m1"] == s["below_M"] == s["at_M"] == 0 and s["other_column"] > 0
    else:
        assert s["m1"] > 0 and s["below_M"] > 0 and s["at_M"] > 0 and s["other_column"] > 0
        assert (s["m2_written"] > 0)
    # the row-kernel members of the sweep wrap as well
    rows = _wrap_stats([s for s in dc.sweep_shapes(bw) if dc.sweep_kernel(s[1], s[3]) == dc.ROWS])
    assert rows["m0"] > 0 and (bw == 1 or rows["m1"] > 0)


# ---------------------------------------------------------------------------------------------
# the identity coding
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", dc.TABLE, ids=dc.key)
def test_identity_coding(case):
    K, npx = case["K"], case["bw"] * case["bh"]
    assert K * npx < 1 << 24
    cb, A = dc.inputs(case, "identity")
    px = cb.reshape(K * npx, 3).astype(np.uint32)
    v = px[:, 0] | px[:, 1] << 8 | px[:, 2] << 16
    assert np.array_equal(v, np.arange(K * npx))                      # pixel p of code vector c is c bw bh + p
    assert len(A) == dc.nblocks(*dc.shape(case)) and A.dtype == np.uint32
    assert A.min() == 0 and A.max() == K - 1
    assert len(np.unique(A)) < len(A) or len(A) <= K                  # repeats wherever they fit
    rb, rA = dc.inputs(case, "random")
    assert np.array_equal(rA, A) and rb.shape == cb.shape and not np.array_equal(rb, cb)


def test_sweep_identity_coding():
    rng = np.random.default_rng(0)
    for nb in (1, 2, 3, 50):
        A = dc.indices(rng, dc.SWEEP_K, nb)
        assert A.max() == dc.SWEEP_K - 1 and (nb == 1 or A.min() == 0)
    assert dc.SWEEP_K * max(dc.SWEEP_BW) * max(dc.SWEEP_BH) < 1 << 24


# ---------------------------------------------------------------------------------------------
# the plan function's edges
# ---------------------------------------------------------------------------------------------
def test_plan_edges():
    hp = quant_amd.host_decode_plan
    # ys % 8 != 0 is PIXELS whatever the alignment
    for ys in (1, 7, 9, 15, 17, 511, 513, 1020):
        for flags in range(16):
            for bh in (1, 2, 3, 4, 8):
                assert hp(7, 9, ys, 2, bh, flags)["kernel"] == dc.PIXELS
    # a raster, original or index misalignment alone is PIXELS, from every row instantiation
    for c in dc.first_per_instantiation():
        if c["plan"]["kernel"] == dc.PIXELS or c["key"].startswith("cap-"):
            continue
        for flags in (dc.RASTER_UNALIGNED, dc.ORIG_UNALIGNED, dc.INDEX_UNALIGNED):
            p = hp(c["K"], *dc.shape(c), flags)
            assert dc.instantiation(p) == (dc.PIXELS, 0, 0, 0) and p["lds_bytes"] == 0, (c["key"], flags)
            assert p["grid"] == min(-(-c["xs"] * c["ys"] // dc.THREADS), dc.GRID_CAP)
            assert hp(c["K"], *dc.shape(c), flags | dc.CODEBOOK_ODD) == p
        # codebook parity only matters for ROWS_H, H >= 2, outside LDS
        even, odd = hp(c["K"], *dc.shape(c)), hp(c["K"], *dc.shape(c), dc.CODEBOOK_ODD)
        if c["plan"]["kernel"] == dc.ROWS_H and c["plan"]["H"] >= 2 and not c["plan"]["lds"]:
            assert dc.instantiation(odd) == (dc.ROWS, 0, 0, 0)
            assert (odd["grid"], odd["rounds"], odd["lds_bytes"]) == (even["grid"], even["rounds"], 0)
        else:
            assert odd == even, c["key"]
    # the boundary is K D <= 49152, at every block shape of the table
    for bw, bh in {(c["bw"], c["bh"]) for c in dc.TABLE}:
        k = dc.k_past_lds(bw, bh)
        assert (hp(k - 1, 2 * bw + 1, 8 * bh, bw, bh)["lds"], hp(k, 2 * bw + 1, 8 * bh, bw, bh)["lds"]) == (1, 0)
    # coal: ys % 512 == 0
    assert [hp(4, 3, ys, 1, 2)["coal"] for ys in (8, 504, 512, 520, 1024, 1536)] == [0, 0, 1, 0, 1, 1]
    # the row kernels stop below 2^40 pixels
    assert hp(4, 1 << 20, 1 << 20, 2, 2)["kernel"] == dc.PIXELS and hp(4, 1 << 19, 1 << 20, 2, 2)["kernel"] == dc.ROWS_H
    # what qvq_decode refuses, the plan refuses
    for args in ((0, 4, 4, 2, 2), (4, 0, 4, 2, 2), (4, 4, 0, 2, 2), (4, 4, 4, 0, 2), (4, 4, 4, 2, 0),
                 (4, 4, 0xFFFFFFFF, 2, 2), (4, 0xFFFFFFFF, 4, 2, 2), (4, 4, 4, 1 << 16, 1 << 16), (4, 4, 4, 2, 2, 16)):
        with pytest.raises(quant_amd.QVQError):
            hp(*args)
