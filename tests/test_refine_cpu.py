"""The yardstick of the refinement tests, without a GPU: tests/helpers/refine_ref.py (the reference
loop over the oracle) reproduces the committed trace, and the CLI rejects bad --refine values."""
import json
import os
import subprocess

import pytest

from conftest import GOLDEN, ROOT
from helpers import refine_ref as ref

QUANT = os.path.join(ROOT, "quant_amd", "lib", "quant")


def test_helper_reproduces_committed_trace():
    with open(os.path.join(GOLDEN, "refine_trace.json")) as f:
        want = json.load(f)
    got = ref.record()
    assert set(got) == set(want) == set(ref.CASES)
    for name, w in want.items():
        g = got[name]
        assert g["iters"] == w["iters"] and g["stop"] == w["stop"] == ref.STOP_FIXED, name
        assert g["changed"] == w["changed"] and g["changed"][-1] == 0, name
        for key in ("d_lbg", "d_reassign", "d_first", "d_last"):
            assert g[key] == pytest.approx(w[key], rel=1e-12), (name, key)
        assert w["d_last"] < w["d_reassign"] < w["d_lbg"]
    # the figures the feature was specified with
    assert want["s128_b2_6"]["changed"][:13] == [1011, 506, 294, 184, 116, 113, 112, 113, 91, 62, 30, 17, 18]
    assert [want[n]["iters"] for n in ("s128_b2_6", "s64_b2_4", "s96_b4_5")] == [35, 12, 9]


def test_helper_stop_rules():
    _, X = ref.case_vectors(64, 2)
    start = ref.lbg_start(X, 4)
    _, _, _, info = ref.refine(X, *start, max_iters=3, eps=0.0)
    assert info["iters"] == 3 and info["stop"] == ref.STOP_MAXIT
    _, _, _, info = ref.refine(X, *start, max_iters=40, eps=0.5)
    assert info["iters"] == 1 and info["stop"] == ref.STOP_EPS
    _, _, _, info = ref.refine(X, start[0], max_iters=1, eps=0.5)   # warm start: no eps test at iteration 1
    assert info["changed"] == [X.shape[0]] and info["stop"] == ref.STOP_MAXIT
    with pytest.raises(ValueError):
        ref.refine(X, *start, max_iters=0)


@pytest.mark.parametrize("bad", [["--refine", "x"], ["--refine", "-3"], ["--refine=1.5"], ["--refine"],
                                 ["--refine", "2", "-q", "1"], ["--fresh=1"]])
def test_cli_rejects_bad_refine_values(bad):
    if not os.path.exists(QUANT):
        pytest.fail("quant CLI not built (run __graft_entry__.build())")
    r = subprocess.run([QUANT, "in.ppm", "-o", "out.quant", *bad], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "usage: quant" in r.stderr, (r.returncode, r.stderr)
