"""The case table of tests/test_gpu_largek.py (tests/helpers/largek_cases.py) against the engine's
dispatch, on the CPU: quant_amd.host_plan reports the plan (plan_level) that run_level, launch_recheck,
launch_assign_valu and launch_update dispatch on, so a case that claims a path really takes it,
and the table as a whole reaches every path.  A pull request that moves a kernel's capacity fails
here, by the name of the case that no longer covers its path: move the case with the threshold."""
import pytest

import quant_amd
from helpers import largek_cases as lk

SEARCH = {"small": quant_amd.PLAN_SEARCH_SMALL, "mf32": quant_amd.PLAN_SEARCH_MF32,
          "wide": quant_amd.PLAN_SEARCH_WIDE, "valu": quant_amd.PLAN_SEARCH_VALU}
RECHECK = {"mf32": quant_amd.PLAN_RECHECK_MF32, "staged": quant_amd.PLAN_RECHECK_STAGED,
           "chunked": quant_amd.PLAN_RECHECK_CHUNKED, "global": quant_amd.PLAN_RECHECK_GLOBAL}
UPDATE = {"runs": quant_amd.PLAN_UPDATE_RUNS, "sorted": quant_amd.PLAN_UPDATE_SORTED,
          "lds": quant_amd.PLAN_UPDATE_LDS}
NAMES = {"search": SEARCH, "recheck": RECHECK, "update": UPDATE}


@pytest.fixture(autouse=True)
def default_paths(monkeypatch):
    monkeypatch.delenv("QVQ_SEARCH", raising=False)
    monkeypatch.delenv("QVQ_KDTREE", raising=False)


def declared(fields):
    return {f: NAMES[f][v] if f in NAMES else v for f, v in fields.items()}


def plans(monkeypatch):
    """Every (label, declared fields, plan, K, dim) of the table: the assign cases under the default
    dispatch and under QVQ_SEARCH=valu, the update cases, the lbg cases' levels."""
    out = []
    for c in lk.ASSIGN_CASES:
        D, n = lk.dim(c["bw"], c["bh"]), lk.rows(c["bw"], c["bh"])
        out.append(("assign %dx%d K=%d" % (c["bw"], c["bh"], c["K"]), declared(c["plan"]),
                    quant_amd.host_plan(D, c["K"], n), c["K"], D))
        if c["valu"] is not None:
            with monkeypatch.context() as m:
                m.setenv("QVQ_SEARCH", "valu")
                want = dict(declared(c["valu"]), search=SEARCH["valu"])
                out.append(("assign %dx%d K=%d QVQ_SEARCH=valu" % (c["bw"], c["bh"], c["K"]), want,
                            quant_amd.host_plan(D, c["K"], n), c["K"], D))
    for c in lk.UPDATE_CASES + lk.PLAN_ONLY_CASES:
        D = lk.dim(c["bw"], c["bh"])
        out.append(("update %dx%d K=%d" % (c["bw"], c["bh"], c["K"]), declared(c["plan"]),
                    quant_amd.host_plan(D, c["K"], c["n"] or lk.rows(c["bw"], c["bh"])), c["K"], D))
    for c in lk.LBG_CASES:
        D, n = lk.dim(c["bw"], c["bh"]), lk.rows(c["bw"], c["bh"], c["S"])
        for K, fields in c["levels"].items():
            assert K <= 1 << c["bits"]
            out.append(("lbg %s level K=%d" % (c["name"], K), declared(fields), quant_amd.host_plan(D, K, n), K, D))
    return out


def test_cases_take_their_declared_paths(monkeypatch):
    bad = []
    for label, want, plan, _, _ in plans(monkeypatch):
        got = {f: plan[f] for f in want}
        if got != want:
            bad.append("%s: declared %s, host_plan %s" % (label, want, got))
    assert not bad, "\n".join(bad)


def test_valu_cases_exist_for_every_other_width():
    for c in lk.ASSIGN_CASES:
        assert (c["valu"] is None) == (lk.dim(c["bw"], c["bh"]) == 12), c
    assert all(c["n"] is None for c in lk.UPDATE_CASES)          # GPU cases run on the case's own rows


def test_table_reaches_every_path(monkeypatch):
    P = plans(monkeypatch)

    def some(pred):
        return [label for label, _, p, K, D in P if pred(p, K, D)]

    # every search kernel: assign_small_kernel, assign_mf32_kernel, assign_wide_kernel, assign_valu_kernel
    for name, v in SEARCH.items():
        assert some(lambda p, K, D: p["search"] == v), "no case runs the %s search" % name
    # every recheck kernel: recheck_mf32_kernel, recheck_kernel<true>, recheck_chunked_kernel,
    # recheck_kernel<false, 0> (the codebook read from global memory)
    for name, v in RECHECK.items():
        assert some(lambda p, K, D: p["recheck"] == v), "no case runs the %s recheck" % name
    # every sums kernel: update_runs_kernel, sorted_sums_kernel, update_kernel
    for name, v in UPDATE.items():
        assert some(lambda p, K, D: p["update"] == v), "no case runs the %s update" % name
    mf32 = SEARCH["mf32"]
    # assign_mf32_kernel STAGED true and false (the flagged rows' fp32 recompute from LDS or global)
    assert some(lambda p, K, D: p["search"] == mf32 and p["c32_staged"] == 1)
    assert some(lambda p, K, D: p["search"] == mf32 and p["c32_staged"] == 0)
    # sums fused into the search and the separate pass inside qvq_lbg; pruned and unpruned levels
    assert some(lambda p, K, D: p["search"] == mf32 and p["fused"] == 1)
    assert some(lambda p, K, D: p["search"] == mf32 and p["fused"] == 0)
    assert some(lambda p, K, D: p["prune"] == 1 and D == 12) and some(lambda p, K, D: p["prune"] == 1 and D != 12)
    assert some(lambda p, K, D: p["prune"] == 0 and K > 2048)
    # assign_wide_kernel with the codebook resident in LDS and streamed in slices
    wide = SEARCH["wide"]
    assert some(lambda p, K, D: p["search"] == wide and p["cb_resident"] == 1)
    assert some(lambda p, K, D: p["search"] == wide and p["cb_resident"] == 0)
    # assign_valu_kernel's tile loop: a first, a middle and a partial last tile (min(KT, K - k0));
    # K = tiles * KT would divide by the tile count
    assert some(lambda p, K, D: p["search"] == SEARCH["valu"] and p["valu_tiles"] >= 3 and K % p["valu_tiles"] != 0)
    # update_runs_kernel's LDS replicas: the most, one, and a count in between (lane % C)
    runs = UPDATE["runs"]
    assert some(lambda p, K, D: p["update"] == runs and p["update_copies"] == 16)
    assert some(lambda p, K, D: p["update"] == runs and p["update_copies"] == 1)
    assert some(lambda p, K, D: p["update"] == runs and 1 < p["update_copies"] < 16)
    # update_kernel's passes: more than one, the last one partial (kl < kr, pdst[d * K + k0 + k]);
    # K = passes * KR would divide by the pass count
    assert some(lambda p, K, D: p["update"] == UPDATE["lds"] and p["update_copies"] >= 2
                and K % p["update_copies"] != 0)
    # the kd-tree past the device build's capacity
    assert some(lambda p, K, D: p["device_tree"] == 1) and some(lambda p, K, D: p["device_tree"] == 0 and K > 4096)


def test_plan_follows_the_path_knobs(monkeypatch):
    """QVQ_SEARCH=valu and QVQ_KDTREE=host change the plan as they change the dispatch."""
    assert quant_amd.host_plan(12, 1024, 4096)["search"] == SEARCH["mf32"]
    assert quant_amd.host_plan(48, 4096, 4096)["device_tree"] == 1
    monkeypatch.setenv("QVQ_SEARCH", "valu")
    p = quant_amd.host_plan(12, 1024, 4096)
    assert p["search"] == SEARCH["valu"] and p["fused"] == 0 and p["prune"] == 0 and p["recheck"] == RECHECK["staged"]
    monkeypatch.setenv("QVQ_SEARCH", "VALU")     # env_is compares the exact string
    assert quant_amd.host_plan(12, 1024, 4096)["search"] == SEARCH["mf32"]
    monkeypatch.setenv("QVQ_KDTREE", "host")
    assert quant_amd.host_plan(48, 4096, 4096)["device_tree"] == 0


def test_plan_rejects_bad_shapes():
    for dim, K, n in [(0, 1, 1), (12, 0, 1), (12, 1, 0), (65, 1, 1)]:
        with pytest.raises(quant_amd.QVQError):
            quant_amd.host_plan(dim, K, n)
