"""The case table of tests/test_gpu_neartie.py (tests/helpers/neartie_cases.py) held to itself and to
the engine's dispatch, on the CPU: every declared plan field is what
quant_amd.host_plan answers; every codebook lies in the colour space's value range; every decade of
the relative gap from 1e-16 to 1e-3 holds rows; the reference's tie rule leaves the fp64 argmin on
the recorded number of rows; and the oracle's kd-tree gives, in this band, what the compiled
reference kd-tree gave (tests/golden/ref_nn_neartie.json, recorded by tests/helpers/record_ref_nn.py)."""
import json
import os

import numpy as np
import pytest

import quant_amd
from conftest import GOLDEN
from helpers import neartie_cases as nt
from oracle import oracle
from test_largek_plan import SEARCH, declared
from test_oracle_golden import _check_vs_reference

with open(os.path.join(GOLDEN, "ref_nn_neartie.json")) as _f:
    REF_NN = json.load(_f)


@pytest.fixture(autouse=True)
def default_paths(monkeypatch):
    monkeypatch.delenv("QVQ_SEARCH", raising=False)
    monkeypatch.delenv("QVQ_KDTREE", raising=False)


def test_cases_take_their_declared_paths(monkeypatch):
    bad = []
    for c in nt.CASES:
        want = declared(c["plan"])
        plan = quant_amd.host_plan(c["D"], c["K"], c["N"])
        got = {f: plan[f] for f in want}
        if got != want:
            bad.append("%s: declared %s, host_plan %s" % (nt.key(c), want, got))
        if c["valu"] is None:
            assert c["K"] <= 32, nt.key(c)          # every larger codebook also runs the VALU search
            continue
        with monkeypatch.context() as m:
            m.setenv("QVQ_SEARCH", "valu")
            want = dict(declared(c["valu"]), search=SEARCH["valu"])
            plan = quant_amd.host_plan(c["D"], c["K"], c["N"])
            got = {f: plan[f] for f in want}
            if got != want:
                bad.append("%s QVQ_SEARCH=valu: declared %s, host_plan %s" % (nt.key(c), want, got))
    assert not bad, "\n".join(bad)


def test_table_shape():
    """Both colour spaces everywhere, the near regime everywhere, the far regime at D = 12, 27, 48
    and 64, N <= 8192, K = 2 M, and the row count the table states."""
    keys = {nt.key(c) for c in nt.CASES}
    assert len(keys) == len(nt.CASES)
    for row in nt.TABLE:
        assert row["far"] == (row["D"] in (12, 27, 48, 64)), row
        for cs in ("scaled", "normal"):
            for regime in ("near", "far") if row["far"] else ("near",):
                assert "D%d-K%d-%s-%s" % (row["D"], row["K"], cs, regime) in keys
    for c in nt.CASES:
        X, C = nt.inputs(c)
        assert X.shape == (c["N"], c["D"]) and C.shape == (c["K"], c["D"]) and c["N"] <= 8192
    assert {c["D"] for c in nt.CASES if c["refine"]} == {12, 27, 48}


@pytest.mark.parametrize("case", nt.CASES, ids=nt.key)
def test_case(case):
    X, C = nt.inputs(case)
    lut = oracle.lut(nt.COLOUR[case["cs"]])
    # the value range: the codebook is also a legal C_start of qvq_refine
    assert C.min() >= lut.min() and C.max() <= lut.max()
    assert np.isin(X, lut).all()
    # band coverage, from the rows and the codebook alone
    gap = nt.rel_gap(X, C)
    counts = nt.band_counts(gap)
    print("rows per decade of the relative gap:", counts)
    short = {e: n for e, n in counts.items() if n < nt.MIN_ROWS}
    assert not short, "decades 1e%s of the relative gap hold fewer than %d rows" % (sorted(short), nt.MIN_ROWS)
    # the tie rule: the reference's answer is not always the fp64 argmin
    A = oracle.kdtree_nn(C, X)
    brute, _ = oracle.bruteforce(C, X)
    assert int(np.sum(A != brute)) == case["ties"]
    # the oracle against the compiled reference kd-tree's record (and the library, where built)
    _check_vs_reference(REF_NN["cases"][nt.key(case)], C, X, A, nt.key(case))


def test_tie_rule_is_exercised():
    assert sum(c["ties"] for c in nt.CASES) >= 10
    assert set(REF_NN["cases"]) == {nt.key(c) for c in nt.CASES}
