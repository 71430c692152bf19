"""qvq_lbg_lloyd without a GPU: the restatement of tests/helpers/lbg_lloyd_ref.py against the
committed trace and against the oracle's split-LBG, the paths the case table's levels reach
(quant_amd.host_plan), the eps cases' margins, the recorded quality claim, and the argument rules
of the CLI's --lloyd and of the Python class."""
import json
import os
import subprocess

import numpy as np
import pytest

import quant_amd
from conftest import ROOT
from helpers import lbg_lloyd_ref as ref
from helpers import refine_ref
from helpers.lbg_lloyd_cases import CASES, EPS_CASES, I1_CASES, ITER_CASES, LBG_SHAPES, RESEED_CASES, NORMAL, SCALED
from oracle import oracle

QUANT = os.path.join(ROOT, "quant_amd", "lib", "quant")
with open(ref.TRACE_PATH) as _f:
    TRACE = json.load(_f)


def test_the_table():
    assert sorted(TRACE) == sorted(CASES)
    assert sorted(set((CASES[n].S, CASES[n].block, CASES[n].bits) for n in I1_CASES)) == sorted(LBG_SHAPES)
    assert sorted(CASES[n].cs for n in I1_CASES) == [NORMAL] * 3 + [SCALED] * 3
    assert set(ITER_CASES) >= {"s64_b2_4_scaled_i3", "s128_b2_6_scaled_i3", "s96_b4_5_scaled_i3"}
    assert {CASES[n].cs for n in RESEED_CASES} == {NORMAL, SCALED}


@pytest.mark.parametrize("name", sorted(CASES))
def test_restatement_against_the_committed_trace(name):
    c, w = CASES[name], TRACE[name]
    X, (C, A, d, levels) = ref.run_case(name)
    assert dict(c._asdict()) == {f: w[f] for f in c._fields} and w["n"] == X.shape[0]
    assert len(levels) == c.bits == len(w["levels"])
    for v, t in zip(levels, w["levels"]):
        assert sorted(v) == sorted(ref.LEVEL_FIELDS) == sorted(t)
        assert all(v[f] == t[f] for f in ref.LEVEL_FIELDS), (v, t)   # (one machine's arithmetic: bit for bit)
    assert d == w["d_last"] == levels[-1]["distortion"]
    assert d == ref.distortion(X, C, A) and C.shape == (1 << c.bits, X.shape[1])
    assert levels[-1]["empty"] == int((np.bincount(A, minlength=1 << c.bits) == 0).sum())
    if not c.reseed:
        assert all(v["seeds"] == 0 for v in levels)


@pytest.mark.parametrize("name", I1_CASES)
def test_one_iteration_is_the_oracles_lbg_with_exact_sums(name):
    c = CASES[name]
    X, (C, A, d, levels) = ref.run_case(name)
    C_o, A_o, d_o = oracle.lbg(X, c.bits, sum_mode=1)
    assert np.array_equal(A, A_o) and np.array_equal(C, C_o)
    assert abs(d - d_o) <= 1e-12 * d_o
    assert all(v["iters"] == 1 and v["stop"] == ref.STOP_MAXIT for v in levels)
    # ... and on these cases the reference's Kahan sums give the same indices: qvq_lbg's
    _, A_k, _ = oracle.lbg(X, c.bits, sum_mode=0)
    assert np.array_equal(A_k, A_o)


def test_levels_reach_every_path():
    plans = []
    for name, c in CASES.items():
        n = TRACE[name]["n"]
        for l in range(1, c.bits + 1):
            plans.append((3 * c.block * c.block, 1 << l, quant_amd.host_plan(3 * c.block * c.block, 1 << l, n)))

    def some(pred):
        return any(pred(D, K, p) for D, K, p in plans)

    assert some(lambda D, K, p: p["search"] == quant_amd.PLAN_SEARCH_SMALL)
    assert some(lambda D, K, p: p["search"] == quant_amd.PLAN_SEARCH_VALU)
    assert some(lambda D, K, p: p["search"] == quant_amd.PLAN_SEARCH_MF32 and p["fused"] and not p["prune"] and K >= 64)
    assert some(lambda D, K, p: p["search"] == quant_amd.PLAN_SEARCH_MF32 and p["fused"] and p["prune"] and K >= 256)
    assert some(lambda D, K, p: D == 48 and p["search"] == quant_amd.PLAN_SEARCH_WIDE and p["cb_resident"])
    assert some(lambda D, K, p: D == 48 and p["search"] == quant_amd.PLAN_SEARCH_WIDE and p["prune"] and K >= 1024)
    for kind in (quant_amd.PLAN_UPDATE_RUNS, quant_amd.PLAN_UPDATE_SORTED, quant_amd.PLAN_UPDATE_LDS):
        assert some(lambda D, K, p: p["update"] == kind and not p["fused"]), kind
    for kind in (quant_amd.PLAN_RECHECK_MF32, quant_amd.PLAN_RECHECK_STAGED, quant_amd.PLAN_RECHECK_CHUNKED,
                 quant_amd.PLAN_RECHECK_GLOBAL):
        assert some(lambda D, K, p: p["recheck"] == kind), kind


@pytest.mark.parametrize("name", EPS_CASES)
def test_eps_cases_keep_their_distance_from_eps(name):
    """The device's closed-form distortion agrees with the direct sum to 1e-9 relative, so a
    relative change can move by a few 1e-9: every one the loop tests stays 1e-3 eps away from eps."""
    c = CASES[name]
    X = ref.case_vectors(name)
    margins = []

    def on_level(l, S, info):
        tr = info["distortion"]
        for t in range(1, len(tr)):   # (iteration 1 of a warm start takes no eps test)
            if info["changed"][t] == 0 and not (info.get("reseeded") or [0] * len(tr))[t]:
                continue              # stopped FIXED before the eps test
            margins.append(abs(abs(tr[t - 1] - tr[t]) / tr[t - 1] - c.eps) / c.eps)

    _, _, _, levels = ref.lbg_lloyd(X, c.bits, c.iters, c.eps, c.cs, c.reseed, on_level=on_level)
    print(name, "closest relative change: %.3g of eps away" % min(margins), [v["iters"] for v in levels])
    assert margins and min(margins) >= 1e-3
    assert any(v["stop"] == ref.STOP_EPS and v["iters"] < c.iters for v in levels)
    if name == "s128_b2_6_scaled_eps":
        assert [v["iters"] for v in levels] == [3, 3, 6, 6, 6, 6]


def test_the_reseed_case_has_empty_cells_without_the_flag():
    plain, seeded = TRACE["s128_b2_10_scaled_eps"]["levels"], TRACE["s128_b2_10_scaled_eps_reseed"]["levels"]
    assert plain[-1]["empty"] == 337 and all(v["seeds"] == 0 for v in plain)
    assert seeded[-1]["empty"] == 0 and seeded[-1]["seeds"] > 0
    assert seeded[-1]["distortion"] < plain[-1]["distortion"]


def test_recorded_quality_claim():
    """gen_image(256), 2x2 blocks, 10 bits, SCALED: three iterations per level reach a lower distortion
    than split-LBG followed by twenty iterations at the final K, at 6138 against 22526 K-weighted
    searches."""
    X = ref.vectors(oracle.gen_image(256), 256, 256, 2, 2, SCALED)
    d_levels = ref.lbg_lloyd(X, 10, 3, 0.0)[2]
    C0, A0, d0 = refine_ref.lbg_start(X, 10)
    d_end = refine_ref.refine(X, C0, A0, d0, max_iters=20, eps=0.0)[2]
    print("lbg", d0, "lbg + refine(20)", d_end, "3 iterations per level", d_levels)
    assert d_levels < d_end < d0


def test_cpp_factory(tmp_path):
    lib = os.path.join(ROOT, "quant_amd", "lib")
    if not os.path.exists(os.path.join(lib, "libquant_amd.so")):
        pytest.fail("libquant_amd.so not built (run __graft_entry__.build())")
    exe = str(tmp_path / "test_lbg_lloyd_api")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "test_lbg_lloyd_api.cpp"), "-L" + lib, "-lquant_amd", "-lqvq",
                    "-Wl,-rpath," + lib, "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr


def run_quant(*args):
    if not os.path.exists(QUANT):
        pytest.fail("quant CLI not built (run __graft_entry__.build())")
    return subprocess.run([QUANT, "in.ppm", "-o", "out.quant", *args], capture_output=True, text=True, timeout=60)


@pytest.mark.parametrize("bad", [["--lloyd"],                               # takes a value
                                 ["--lloyd", "-1"],
                                 ["--lloyd", "x"],
                                 ["--lloyd", "3", "-q", "1"],               # needs LBG
                                 ["--lloyd", "3", "--reseed", "-q", "2"],
                                 ["--reseed", "--lloyd", "0"],              # --reseed needs one of the two > 0
                                 ["--reseed", "--lloyd", "0", "--refine", "0"]])
def test_cli_rejects(bad):
    r = run_quant(*bad)
    assert r.returncode == 2 and "usage: quant" in r.stderr, (r.returncode, r.stderr)


@pytest.mark.parametrize("good", [["--lloyd", "3"], ["--lloyd=3", "--reseed"], ["--lloyd", "3", "--refine", "2", "--fresh"],
                                  ["--reseed", "--refine", "2", "--lloyd", "0"]])
def test_cli_accepts(good):
    r = run_quant(*good)   # past the arguments: the input file does not exist
    assert r.returncode == 3 and "usage: quant" not in r.stderr, (r.returncode, r.stderr)


def test_cli_help_names_the_option():
    r = subprocess.run([QUANT, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "--lloyd arg (=0)" in r.stdout and "--refine or --lloyd" in r.stdout


def test_python_class_arguments():
    with pytest.raises(quant_amd.QVQError):
        quant_amd.LBGQuantizer(reseed=True)
    with pytest.raises(quant_amd.QVQError):
        quant_amd.LBGQuantizer(reseed=True, lloyd_iters=0, refine_iters=0)
    with pytest.raises(quant_amd.QVQError):
        quant_amd.LBGQuantizer(lloyd_iters=-1)
    quant_amd.LBGQuantizer(reseed=True, lloyd_iters=2)     # no engine before quantize()
    quant_amd.LBGQuantizer(reseed=True, refine_iters=2)
    quant_amd.LBGQuantizer(lloyd_iters=2, refine_iters=2, fresh=True)
    assert quant_amd.LLOYD_RESEED == 1 and "qvq_lbg_lloyd" in quant_amd.EXPORTED
