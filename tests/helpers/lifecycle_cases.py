"""One context through every lifetime transition of its buffers (tests/test_gpu_context_lifecycle.py;
DESIGN.md 2.1): a first training set, the same shape again (every buffer kept), a larger Kcap (the
level buffers rebuilt), an exact-mode set, a CIE1931 raster, back to the byte set with qvq_refine.
Each step's result is compared bit for bit with a fresh context that ran only that step, and with
the oracle.

As a program it runs the sequence in a process of its own, whose environment selects the schedule
(QVQ_SPECULATE=0, QVQ_KAHAN=0: the engine reads these once), and prints one JSON line:

    python lifecycle_cases.py kahan|exact-sum
"""
import functools
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
from helpers import cie_cases as cc  # noqa: E402
from helpers import refine_ref, reseed_ref  # noqa: E402
from oracle import oracle  # noqa: E402

KAHAN_RTOL = 1e-12   # tests/test_gpu_parity.py
# name, what it sets (None: the resident set stays), bits, refine (None, or the reseed flag)
STEPS = [("first", "raster32", 3, None), ("same-shape", "raster32", 3, None), ("kcap-grows", None, 5, None),
         ("exact", "rows64x5", 2, None), ("cie", "cie16", 2, None),
         ("back-refine", "raster32", 3, False), ("back-refine-reseed", None, 3, True)]
CYCLE = STEPS[:5]   # the leak check's cycle


@functools.lru_cache(maxsize=None)
def data(name):
    """(how to set it, the rows the oracle sees)."""
    if name == "raster32":   # 32 x 32, 2 x 2 blocks: N = 256, D = 12
        rgb = oracle.gen_image(32)
        return rgb, oracle.tile(rgb, 32, 32, 2, 2)[0]
    if name == "cie16":      # 16 x 16, 2 x 2 blocks under CIE1931: N = 64, D = 12, exact mode
        rgb = oracle.gen_image(16, 0x5EED + 1)
        return rgb, cc.cie_rows(rgb, 1, 16, 16, 2, 2)
    X = np.random.default_rng(5).standard_normal((64, 5))   # no byte image: exact mode
    return X, X


def set_data(engine, name):
    import quant_amd
    src, _ = data(name)
    if name == "raster32":
        engine.set_images(src, 1, 32, 32, 2, 2, quant_amd.SCALED)
    elif name == "cie16":
        engine.set_images(src, 1, 16, 16, 2, 2, quant_amd.CIE1931)
    else:
        engine.set_vectors(src)
        assert engine.training_info()["mode"] == quant_amd.MODE_EXACT


def run_step(engine, step, resident):
    """The step on engine, whose resident set is `resident`; (the set now resident, lbg's result,
    refine's result or None)."""
    name, sets, bits, reseed = step
    if sets:
        set_data(engine, sets)
        resident = sets
    got = engine.lbg(bits)
    refined = None if reseed is None else engine.refine(max_iters=2, eps=0.0, reseed=reseed)
    return resident, got, refined


def fresh_step(step, resident):
    """The same step alone on a context of its own."""
    import quant_amd
    with quant_amd.Engine(0) as eng:
        return run_step(eng, (step[0], step[1] or resident, step[2], step[3]), None)[1:]


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint64) if a.dtype == np.float64 else a,
                                                 b.view(np.uint64) if b.dtype == np.float64 else b)


def check_oracle(step, resident, got, refined, rule):
    """tests/test_gpu_parity.py's comparison for the byte sets (rule "exact-sum": QVQ_KAHAN=0, the
    oracle's exact-sum mode decides the indices), tests/test_gpu_cie_raster.py's for the exact
    ones, tests/test_gpu_reseed.py's same_run for qvq_refine."""
    name, _, bits, reseed = step
    X = data(resident)[1]
    C, A, d = got
    if resident != "raster32":
        C_r, A_r, _ = oracle.lbg(X, bits, sum_mode=0)
        assert same_bits(C, C_r) and np.array_equal(A, A_r), name
        return
    C_k, A_k, d_k = oracle.lbg(X, bits, sum_mode=1 if rule == "exact-sum" else 0)
    assert np.array_equal(A, A_k), name
    assert np.array_equal(C, oracle.centroids(X, A_k, 1 << bits, sum_mode=1)), name
    assert np.max(np.abs(C - C_k) / np.maximum(np.abs(C_k), 1e-300)) <= KAHAN_RTOL, name
    assert abs(d - d_k) <= 1e-9 * abs(d_k), name
    if refined is None or rule == "exact-sum":   # (refine_ref starts from the reference rule's indices)
        return
    C0, A0, d0 = refine_ref.lbg_start(X, bits)
    if reseed:
        want = reseed_ref.refine(X, C0, reseed_ref.SCALED, A0, d0, max_iters=2, eps=0.0)
    else:
        want = refine_ref.refine(X, C0, A0, d0, max_iters=2, eps=0.0)
    C_w, A_w, d_w, info_w = want
    C_g, A_g, d_g, info = refined
    assert info["iters"] == info_w["iters"] and info["stop"] == info_w["stop"], name
    assert info["changed"] == info_w["changed"], name
    assert info["reseeded"] == info_w.get("reseeded", [0] * info_w["iters"]), name
    assert np.array_equal(A_g, A_w) and np.array_equal(C_g, C_w), name
    np.testing.assert_allclose(info["distortion"], info_w["distortion"], rtol=1e-9, atol=0)
    assert abs(d_g - d_w) <= 1e-9 * abs(d_w), name


def run_sequence(engine, rule="kahan", steps=STEPS):
    """Every step on engine, each against a fresh context and the oracle."""
    resident = None
    for step in steps:
        before = resident
        resident, got, refined = run_step(engine, step, resident)
        alone, alone_refined = fresh_step(step, before)
        for g, a in zip(got[:2], alone[:2]):
            assert same_bits(g, a), "%s: differs from a fresh context" % step[0]
        assert got[2] == alone[2], "%s: distortion differs from a fresh context" % step[0]
        if refined is not None:
            for g, a in zip(refined[:2], alone_refined[:2]):
                assert same_bits(g, a), "%s: refine differs from a fresh context" % step[0]
            assert refined[2] == alone_refined[2] and refined[3] == alone_refined[3], step[0]
        check_oracle(step, resident, got, refined, rule)


def main():
    import quant_amd
    with quant_amd.Engine(0) as eng:
        run_sequence(eng, sys.argv[1])
    print(json.dumps({"ok": True, "steps": len(STEPS)}), flush=True)


if __name__ == "__main__":
    main()
