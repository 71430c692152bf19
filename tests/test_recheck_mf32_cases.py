"""tests/helpers/recheck_mf32_cases.py held to what its cases are for, on the CPU: the codebooks
dispatch to the MFMA recheck, every site's code vectors sit at the tiles, halves and counts its name
promises, its rows have exactly that site's code vectors as their nearest, the near ties are inside
the search's flag threshold and outside the tie band, and the row counts give the group patterns
their names promise for several CU counts."""
import numpy as np
import pytest

import quant_amd
from helpers import neartie_cases as nt
from helpers import recheck_mf32_cases as rc

CODEBOOKS = [(K, cs) for K in rc.KS for cs in ("scaled", "normal")]
CU_COUNTS = (64, 256, 304)


@pytest.fixture(autouse=True)
def default_paths(monkeypatch):
    monkeypatch.delenv("QVQ_SEARCH", raising=False)
    monkeypatch.delenv("QVQ_KDTREE", raising=False)


def _half(i):
    return (i >> 2) & 1


@pytest.mark.parametrize("K", rc.KS)
def test_codebooks_run_the_mfma_search_and_recheck(K):
    for N in (rc.BACKGROUND_ROWS + 1, rc.BACKGROUND_ROWS + 70, 2048, 150000):
        plan = quant_amd.host_plan(rc.D, K, N)
        assert plan["search"] == quant_amd.PLAN_SEARCH_MF32 and plan["recheck"] == quant_amd.PLAN_RECHECK_MF32, (K, N)
    assert [rc.tiles(k) for k in rc.KS] == [16, 17, 32, 32]      # 544: an odd count; 1000: 24 padding positions


@pytest.mark.parametrize("K,cs", CODEBOOKS)
def test_sites_sit_where_their_names_say(K, cs):
    C, sites, background, U = rc.build_codebook(K, cs)
    last = rc.tiles(K) - 1
    used = np.concatenate([s["idx"] for s in sites.values()])
    assert len(set(used.tolist())) == len(used) and not set(used.tolist()) & set(background.tolist())
    assert len(used) + len(background) == K and used.max() < K
    tile = {n: [i // 32 for i in s["idx"]] for n, s in sites.items()}
    half = {n: [_half(i) for i in s["idx"]] for n, s in sites.items()}
    assert tile["pair:tile"][0] == tile["pair:tile"][1] and half["pair:tile"] == [0, 0]
    assert tile["pair:ends"] == [0, last]
    assert tile["pair:halves"][0] == tile["pair:halves"][1] and half["pair:halves"] == [0, 1]
    assert tile["pair:last"] == [last, last]
    for n in rc.CAPS:
        assert all(len(sites["cap:%d:%s" % (n, lay)]["idx"]) == n for lay in rc.CAP_LAYOUTS)
        assert set(half["cap:%d:half" % n]) == {0}
        counts = np.bincount(half["cap:%d:both" % n], minlength=2)
        assert abs(int(counts[0]) - int(counts[1])) <= 1
        assert len(set(tile["cap:%d:tiles" % n])) >= 12
    # 16 in one half of one tile: sixteen mask bits, and the list exactly full; 17: one past it
    assert len(set(tile["cap:16:half"])) == 1 and len(sites["cap:16:half"]["idx"]) == rc.RC_CAP
    assert len(set(tile["cap:17:half"])) == 2
    # split over the halves, 16 and 17 stay inside the lists; 40 overflows both
    assert max(np.bincount(half["cap:17:both"])) <= rc.RC_CAP < min(np.bincount(half["cap:40:both"]))
    assert len(set(tile["cap:16:both"])) == 1


@pytest.mark.parametrize("K,cs", CODEBOOKS)
def test_rows_see_their_own_site_only(K, cs):
    """The nearest code vectors of a site's row are that site's, every other one is CLEAR times farther;
    a cap site's are all within 1e-9 relative of one another; a pair's one-step rows are 4 NEAR u^2
    apart, the reference's tie band (1e-12 relative and less) far below and the search's per-row MFMA
    bound (at least 1.25 * 33 * 2^-24 * 12 max|c - mu|^2 > 0.6 u^2, engine.cpp mfma_setup) above."""
    C, sites, _, U = rc.build_codebook(K, cs)
    _, step = rc.affine(cs)
    for name, s in sites.items():
        for r in s["rows"]:
            d = ((U - r) ** 2).sum(axis=1)
            own = np.zeros(K, bool)
            own[s["idx"]] = True
            assert np.sqrt(d[~own].min()) > rc.CLEAR * rc.site_reach(U, s) >= rc.CLEAR * np.sqrt(d[own].max()), name
            if name.startswith("cap:"):
                assert d[own].max() - d[own].min() <= 1e-9 * d[own].min(), name
    for name in ("pair:tile", "pair:ends", "pair:halves", "pair:last"):
        s = sites[name]
        for r, nearer in zip(s["rows"][:2], s["idx"]):
            d = ((U[s["idx"]] - r) ** 2).sum(axis=1)
            gap = abs(d[0] - d[1])
            assert abs(gap - 4 * rc.NEAR) < 1e-9 and gap < 0.3 and gap > 1e-6 * d.min(), name
            assert s["idx"][int(np.argmin(d))] == nearer
        d = ((U[s["idx"]] - s["rows"][2]) ** 2).sum(axis=1)
        assert abs(d[0] - d[1]) <= 1e-12 * d[0]                       # the midpoint
    on = sites["on"]
    assert np.array_equal(U[on["idx"][0]], on["rows"][0])
    # the values: on the lut for rows, inside the data range for code vectors (a legal refine start)
    lut = rc.oracle.lut(rc.COLOUR[cs])
    assert C.min() >= lut.min() and C.max() <= lut.max()
    X, C2, at = rc.edges(K, cs)
    assert C2 is C and np.isin(X, lut).all() and len(at) == len(rc.site_row_names(K, cs)) == 22
    assert np.array_equal(X[at], rc.values(cs, np.concatenate([s["rows"] for s in sites.values()])))


@pytest.mark.parametrize("G", CU_COUNTS)
def test_counts_give_the_named_groups(G):
    n = rc.group_counts(G)
    assert tuple(n) == rc.COUNT_NAMES
    p = {k: rc.pattern(v, G) for k, v in n.items()}
    assert [p[k]["groups"] for k in ("one", "group_less_one", "group", "group_plus_one")] == [1, 1, 1, 2]
    assert [p[k]["last_rows"] for k in ("one", "group_less_one", "group", "group_plus_one")] == [1, 31, 32, 1]
    assert p["group_plus_one"]["last_block"] == 1 and p["group_plus_one"]["last_wave"] == 0
    w = p["wave_one"]
    assert (w["groups"], w["last_rows"], w["last_block"], w["last_wave"], w["trips_b0w0"]) == (G + 1, 1, 0, 1, 1)
    s = p["second_trip"]
    assert s["groups"] == rc.WAVES * G + 3 and s["last_rows"] == 5 and s["trips_b0w0"] == 2
    assert n["second_trip"] < 160000 or G > 256                   # ~140 k rows on 256 CUs: milliseconds


@pytest.mark.parametrize("K,cs", CODEBOOKS)
def test_scattered_near_ties_span_tiles_and_halves(K, cs):
    """After the permutation most pairs have their two code vectors in different tiles, half of those in
    different halves too, and at least MIN_ROWS * 4 rows are within 1e-9 relative (the search cannot
    order them in fp32: its provisional index is either one)."""
    X, C, perm = rc.scattered_neartie(K, cs)
    assert sorted(perm.tolist()) == list(range(K))
    _, _, i1, i2 = nt.top_two(X, C)
    gap = nt.rel_gap(X, C)
    close = gap < 1e-9
    far_apart = (i1 // 32 != i2 // 32) & (((i1 >> 2) & 1) != ((i2 >> 2) & 1))
    assert int(np.sum(close)) >= 4 * nt.MIN_ROWS
    assert int(np.sum(close & far_apart)) >= nt.MIN_ROWS
