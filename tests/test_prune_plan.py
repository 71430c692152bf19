"""The case table of tests/test_gpu_prune_bound.py (tests/helpers/prune_cases.py) held to its claims
on the CPU, against the engine's dispatch and the numpy model of the pruned
searches' window rule (tests/helpers/prune_ref.py): every declared plan field is what
quant_amd.host_plan answers; every codebook lies in the value range; the station cases' tiles are
pure (group sizes, bucket separation); under the rule as documented the model loses no row against
brute force and visits at most half of the tiles; under each mutation a case is declared for it
loses at least 64 rows; and the oracle's kd-tree gives on the tie rows what the compiled reference
kd-tree gave (tests/golden/ref_nn_prune.json, recorded by tests/helpers/record_ref_nn.py).  The
losses of tests/test_gpu_prune.py's own images under a bound a quarter of what it should be are
recorded beside them: the numbers that motivate the table."""
import functools
import json
import os

import numpy as np
import pytest

import quant_amd
from conftest import GOLDEN
from helpers import neartie_cases as nt
from helpers import prune_cases as pc
from helpers import prune_ref as pr
from oracle import oracle
from test_largek_plan import declared
from test_oracle_golden import _check_vs_reference

with open(os.path.join(GOLDEN, "ref_nn_prune.json")) as _f:
    REF_NN = json.load(_f)

MIN_LOST = 64


@pytest.fixture(autouse=True)
def default_paths(monkeypatch):
    monkeypatch.delenv("QVQ_SEARCH", raising=False)
    monkeypatch.delenv("QVQ_KDTREE", raising=False)


@functools.lru_cache(maxsize=None)
def _truth(k):
    """(d1, d2, i1, i2, tie) per row in long double over brute force's candidates."""
    c = next(c for c in pc.CASES if pc.key(c) == k)
    X, C, _ = pc.inputs(c)
    d1, d2, i1, i2 = nt.top_two(X, C)
    return d1, d2, i1, i2, (d2 - d1) <= pc.TIE_REL * d1


def _lost(case, mut=pr.Mutation()):
    X, C, _ = pc.inputs(case)
    _, _, i1, i2, tie = _truth(pc.key(case))
    res = pr.search(X, C, pc.COLOUR[case["cs"]], case["kind"], case["cpr"], mut=mut)
    return int(pr.lost(res, i1, i2, tie).sum()), res


def test_cases_take_their_declared_paths():
    bad = []
    for c in pc.CASES:
        want = declared(c["plan"])
        plan = quant_amd.host_plan(c["D"], c["K"], c["N"])
        got = {f: plan[f] for f in want}
        if got != want:
            bad.append("%s: declared %s, host_plan %s" % (pc.key(c), want, got))
        if c["first"] and quant_amd.host_plan(c["D"], c["K"] - 1, c["N"])["prune"]:
            bad.append("%s: K - 1 is pruned as well" % pc.key(c))
    assert not bad, "\n".join(bad)


def test_table_shape():
    """The families and edges DESIGN.md 6.6 lists, both colour spaces, a few thousand rows."""
    keys = {(c["D"], c["K"], c["name"]) for c in pc.CASES}
    for D, K in ((12, 256), (12, 2048), (48, 1024), (48, 2100), (48, 4000), (48, 4096), (3, pc.FIRST_K[3]),
                 (13, pc.FIRST_K[13]), (27, 1024), (46, 1024)):
        assert any(k[:2] == (D, K) for k in keys), (D, K)
    assert any(c["D"] == 12 and 2017 <= c["K"] <= 2047 for c in pc.CASES)
    assert {c["cpr"] for c in pc.CASES if c["geometry"]} == {1, 2, 3}
    assert any(c["recheck"] and c["plan"].get("recheck") == "chunked" and c["has_ties"] for c in pc.CASES)
    assert {c["degenerate"] for c in pc.CASES if c["family"] == "degenerate"} == {"one", "two", "outlier", "dups"}
    for c in pc.CASES:
        X, C, _ = pc.inputs(c)
        assert X.shape == (c["N"], c["D"]) and C.shape == (c["K"], c["D"]) and c["N"] <= 6000
        if c["both"]:
            assert {"scaled", "normal"} <= {o["cs"] for o in pc.CASES if (o["D"], o["K"], o["name"]) == (c["D"], c["K"], c["name"])}
    for D in (13, 27, 46):
        assert {c["cs"] for c in pc.CASES if c["D"] == D} == {"scaled", "normal"}
    # a ragged N leaves a partial last chunk and, in the wide search, a partial last task
    assert any(c["N"] % 64 and c["kind"] == "mf32" for c in pc.CASES)
    assert any(c["N"] % 64 and -(-c["N"] // 64) % 8 and c["kind"] == "wide" for c in pc.CASES)
    # image geometry: a task count that is no multiple of cpr
    assert any(c["geometry"] and -(-(c["N"] // 64) // 8) % c["cpr"] for c in pc.CASES if c["cpr"] > 1)


def _purity(case, C):
    """The station families' precondition: in the order of q the groups of one projection come in
    multiples of the window's unit (a tile; a slice of 4 tiles in the wide search), the last one
    excepted, and neighbouring groups lie at least two of prune_order's buckets apart."""
    q = np.sort(pr.projections(C, pc.COLOUR[case["cs"]]))
    cut = np.flatnonzero(np.diff(q) > 0.5) + 1
    sizes = np.diff(np.concatenate([[0], cut, [len(q)]]))
    unit = pr.TILE * (pr.WD_SLICE_TILES if case["kind"] == "wide" else 1)
    assert (sizes[:-1] % unit == 0).all(), sizes
    bucket = (q[-1] - q[0] + 1) / 256
    sep = np.diff(q)[cut - 1].min() / bucket
    assert sep >= 2.0, "groups %.2f buckets apart" % sep
    return len(sizes), sep


@pytest.mark.parametrize("case", pc.CASES, ids=pc.key)
def test_case(case):
    X, C, info = pc.inputs(case)
    cs = pc.COLOUR[case["cs"]]
    lut = oracle.lut(cs)
    # the value range: a legal C_start of qvq_refine; rows on the byte path
    assert C.min() >= lut.min() and C.max() <= lut.max()
    assert np.isin(X, lut).all()
    mu, sx = pr.TERMS[cs]
    assert np.allclose(lut[info["codes"][:64]], mu + (2.0 * (info["codes"][:64] ^ 0x80) - 255.0) * sx, rtol=0, atol=1e-12)
    if case["family"] == "stations":
        print("groups, least separation in buckets:", _purity(case, C))
    if case["geometry"]:
        xs, ys = case["geometry"]
        assert pr.cpr_of(ys // 4) == case["cpr"]
        Xt, codes = oracle.tile(pc.raster(case), xs, ys, 4, 4, cs=cs)
        assert np.array_equal(Xt, X) and np.array_equal(codes, info["codes"])
    # the rule as documented: no row lost against brute force (this checks the case and the model)
    n0, res = _lost(case)
    print("tiles visited: %.1f %% of %d" % (100 * res.visited, res.tiles))
    assert n0 == 0
    A = oracle.kdtree_nn(C, X)
    _, _, i1, i2, tie = _truth(pc.key(case))
    assert np.array_equal(res.answer[~tie], A[~tie])          # the model's answers over its windows alone
    if case["prunes"]:
        assert res.visited <= 0.5                             # a case that prunes nothing attacks nothing
    # each declared mutation narrows some window past a row's answer
    for m in case["mutations"]:
        n, _ = _lost(case, m)
        print("%s: %d rows lost" % (pc.MUT_NAMES[m], n))
        assert n >= MIN_LOST, pc.MUT_NAMES[m]
    if case["family"] == "stations" and 0.9 in case["ratios"] and case["pattern"] == "all":
        assert _lost(case, pr.Mutation(factor=0.9))[0] >= MIN_LOST
    # ties: both answers in far tiles on opposite sides; the reference's rule decides
    if case["has_ties"]:
        st = info["stations"]
        rows = np.flatnonzero(tie)
        assert len(rows) >= MIN_LOST
        s = info["station"][rows]
        assert all(st[j]["tie"] for j in set(s.tolist()))
        t = pr.tile_of(res.perm)
        lo = np.array([x["lo"] for x in st])[s]
        hi = np.array([x["hi"] for x in st])[s]
        assert np.array_equal(np.minimum(i1[rows], i2[rows]), np.minimum(lo, hi))
        assert (t[lo] < res.first[rows]).all() and (t[hi] > res.first[rows]).all()
        # the reference's rule takes the lo vector on some tie rows and the hi vector on others:
        # a search that answered these rows without the flag could not reproduce it
        n_lo, n_hi = int(np.sum(A[rows] == lo)), int(np.sum(A[rows] == hi))
        print("tie rows: %d, the reference answers lo on %d and hi on %d" % (len(rows), n_lo, n_hi))
        assert n_lo + n_hi == len(rows) and min(n_lo, n_hi) >= MIN_LOST
        _check_vs_reference(REF_NN["cases"][pc.key(case)], C, X[rows], A[rows], pc.key(case))
    if case["recheck"]:
        # the chunked recheck's sweep, per flagged row, from the distance to the search's index
        rows = np.flatnonzero(tie)
        t = pr.tile_of(res.perm)
        for m, least in ((pr.Mutation(), None), (pc.QUARTER, MIN_LOST)):
            w = pr.recheck_windows(X, C, cs, res.answer, rows, mut=m)
            miss = np.zeros(len(rows), bool)
            for i in (i1[rows], i2[rows]):
                miss |= (t[i] < w[:, 0]) | (t[i] > w[:, 1])
            print("recheck sweep, %s: %d of %d tie rows lose a candidate" % (pc.MUT_NAMES.get(m, "as documented"), miss.sum(), len(rows)))
            assert miss.sum() == 0 if least is None else miss.sum() >= least


def test_records_cover_the_tie_cases():
    assert set(REF_NN["cases"]) == {pc.key(c) for c in pc.CASES if c["has_ties"]}


# rows lost of 16,384 on the images of tests/test_gpu_prune.py, at the pruned levels K = 256, 512
# and 1024 of oracle.lbg's own split codebooks, under the rule as documented and under a quarter and
# a sixteenth of its bound: a bound wrong by a factor of 4 loses nothing there, which is what the
# suite could see before the station cases
OLD_IMAGES = {
    "smooth": {"rule": [0, 0, 0], "quarter": [0, 0, 0], "sixteenth": [0, 3, 1]},
    "flat": {"rule": [0, 0, 0], "quarter": [0, 0, 0], "sixteenth": [0, 0, 0]},
    "noise": {"rule": [0, 0, 0], "quarter": [0, 0, 0], "sixteenth": [0, 2, 9]},
}


@pytest.mark.parametrize("kind", sorted(OLD_IMAGES))
def test_old_images_under_a_quarter_bound(kind):
    from test_gpu_prune import _image
    S = 256
    X, _ = oracle.tile(_image(kind, S), S, S, 2, 2)
    _, _, _, splits, _ = oracle.lbg(X, 10, sum_mode=0, dump=True)
    got = {"rule": [], "quarter": [], "sixteenth": []}
    for Cs in splits[7:10]:
        d1, d2, i1, i2 = nt.top_two(X, Cs)
        tie = (d2 - d1) <= pc.TIE_REL * d1
        for name, m in (("rule", pr.Mutation()), ("quarter", pc.QUARTER), ("sixteenth", pr.Mutation(factor=1 / 16))):
            got[name].append(int(pr.lost(pr.search(X, Cs, oracle.SCALED, "mf32", mut=m), i1, i2, tie).sum()))
    print(kind, got)
    assert got == OLD_IMAGES[kind]


@pytest.mark.parametrize("image", pc.LBG_IMAGES, ids=lambda i: i["name"])
def test_lbg_images_are_sharp(image):
    """The two images of test_lbg_levels, on oracle.lbg's own split codebooks at the pruned levels:
    no row lost under the rule, at least one under a quarter of its bound at every level, and the
    measured losses pinned."""
    S, b = image["S"], image["block"]
    X, _ = oracle.tile(pc.lbg_raster(image), S, S, b, b)
    _, _, _, splits, _ = oracle.lbg(X, image["bits"], sum_mode=0, dump=True)
    X = X[:image["model_rows"]]
    got = []
    for lv in image["levels"]:
        Cs = splits[lv - 1]
        assert quant_amd.host_plan(X.shape[1], len(Cs), len(X))["prune"] == 1
        d1, d2, i1, i2 = nt.top_two(X, Cs)
        tie = (d2 - d1) <= pc.TIE_REL * d1
        n = [int(pr.lost(pr.search(X, Cs, oracle.SCALED, image["kind"], image["cpr"], mut=m), i1, i2, tie).sum())
             for m in (pr.Mutation(), pc.QUARTER)]
        assert n[0] == 0
        got.append(n[1])
    print(image["name"], "rows lost under a quarter of the bound:", got)
    assert min(got) >= 1 and got == image["lost_quarter"]
