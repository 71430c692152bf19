"""qvq_refine (include/qvq.h): Lloyd refinement at fixed K on the device against
the reference loop of tests/helpers/refine_ref.py (oracle.kdtree_nn -> oracle.centroids(sum_mode=1)
-> direct distortion) -- indices and codebook bit for bit, the distortion trace within 1e-9
relative (the closed form against the direct sum, as __graft_entry__.smoke)."""
import functools
import json
import os
import subprocess

import numpy as np
import pytest

import quant_amd
from conftest import GOLDEN, ROOT, load_png_rgb
from helpers import refine_ref as ref
from oracle import oracle

pytestmark = pytest.mark.gpu
QUANT = os.path.join(ROOT, "quant_amd", "lib", "quant")
QVQ_EINVAL, QVQ_EUNSUPPORTED, QVQ_ESTATE = 1, 5, 6
with open(os.path.join(GOLDEN, "refine_trace.json")) as _f:
    TRACE = json.load(_f)


@functools.lru_cache(maxsize=None)
def case(name, max_iters=100, eps=0.0):
    """(rgb, X, bits, lbg start, the helper's refinement from it), computed once per case."""
    S, b, bits = ref.CASES[name]
    rgb, X = ref.case_vectors(S, b)
    start = ref.lbg_start(X, bits)
    return rgb, X, bits, start, ref.refine(X, *start, max_iters=max_iters, eps=eps)


def lbg_on(engine, name):
    S, b, bits = ref.CASES[name]
    rgb = case(name)[0]
    engine.set_images(rgb, 1, S, S, b, b, quant_amd.SCALED)
    return engine.lbg(bits)


def same_run(got, want):
    C, A, d, info = got
    C_r, A_r, d_r, info_r = want
    assert info["iters"] == info_r["iters"] and info["stop"] == info_r["stop"]
    assert info["changed"] == info_r["changed"]
    assert np.array_equal(A, A_r), "indices differ from the reference loop"
    assert np.array_equal(C, C_r), "codebook differs from the reference loop"
    print("distortion trace", info["distortion"], "reference", info_r["distortion"])
    np.testing.assert_allclose(info["distortion"], info_r["distortion"], rtol=1e-9, atol=0)
    assert abs(d - d_r) <= 1e-9 * abs(d_r)


@pytest.mark.parametrize("name", ["s128_b2_6",    # D = 12, MFMA search with fused sums; a kd-tree tie at iteration 13
                                  "s64_b2_4",     # the small-K scan
                                  "s96_b4_5"])    # D = 48, K * D = 1536: the counting-sort sums
def test_fixed_point(engine, name):
    lbg_on(engine, name)
    got = engine.refine(max_iters=40, eps=0.0)
    want = case(name)[4]
    assert got[3]["iters"] == TRACE[name]["iters"] and got[3]["stop"] == quant_amd.STOP_FIXED
    assert got[3]["changed"] == TRACE[name]["changed"]
    same_run(got, want)
    assert abs(got[2] - TRACE[name]["d_last"]) <= 1e-9 * TRACE[name]["d_last"]


def test_pruned_search_k512(engine):
    """K = 512: the pruned MFMA search over the same-K finalize_kernel's tile order, the MFMA recheck."""
    S, bits = 256, 9
    rgb, X = ref.case_vectors(S, 2)
    engine.set_images(rgb, 1, S, S, 2, 2, quant_amd.SCALED)
    engine.lbg(bits)
    same_run(engine.refine(max_iters=3, eps=0.0), ref.refine(X, *ref.lbg_start(X, bits), max_iters=3, eps=0.0))


def test_eps_stop(engine):
    """The oracle's relative changes are 0.183, 0.092, 0.042, 0.021, 0.00965: eps = 0.01 stops at 5."""
    lbg_on(engine, "s128_b2_6")
    got = engine.refine(max_iters=40, eps=0.01)
    assert got[3]["iters"] == 5 and got[3]["stop"] == quant_amd.STOP_EPS
    same_run(got, case("s128_b2_6", 40, 0.01)[4])


def test_fresh_indices_of_lbg_codebook(engine):
    _, X, _, (C0, _, _), _ = case("s128_b2_6")
    C_l, _, _ = lbg_on(engine, "s128_b2_6")
    C, A, d, info = engine.refine(max_iters=0, fresh=True)
    assert info["iters"] == 0 and info["changed"] == []
    assert np.array_equal(C, C_l) and np.array_equal(C, C0)
    A_ref = oracle.kdtree_nn(C0, X)
    assert np.array_equal(A, A_ref)
    direct = ref.distortion(X, C0, A_ref)
    print("fresh distortion", d, "direct", direct)
    assert abs(d - direct) <= 1e-9 * direct and abs(direct - 0.0195710) < 1e-6
    lbg_on(engine, "s128_b2_6")
    with pytest.raises(quant_amd.QVQError) as e:
        engine.refine(max_iters=0, fresh=False)
    assert e.value.status == QVQ_EINVAL


def test_equals_assign_update_loop(engine):
    """Three iterations through the existing ABI (Engine.assign + Engine.update) bit for bit."""
    C, _, _ = lbg_on(engine, "s128_b2_6")
    K = C.shape[0]
    for _ in range(3):
        A = engine.assign(C)
        C, _ = engine.update(A, K)
    lbg_on(engine, "s128_b2_6")
    C_r, A_r, _, info = engine.refine(max_iters=3, eps=0.0)
    assert info["iters"] == 3 and info["stop"] == quant_amd.STOP_MAXIT
    assert np.array_equal(A_r, A) and np.array_equal(C_r, C)


def test_warm_start(engine):
    """Case 1's final codebook refined on another image: no A_0, changed[0] = N."""
    C_fix = case("s128_b2_6")[4][0]
    rgb, X = ref.case_vectors(128, 2, seed=0xBEEF)
    engine.set_images(rgb, 1, 128, 128, 2, 2, quant_amd.SCALED)
    got = engine.refine(C=C_fix, max_iters=4, eps=0.0)
    assert got[3]["changed"][0] == X.shape[0]
    same_run(got, ref.refine(X, C_fix, max_iters=4, eps=0.0))
    bad = C_fix.copy()
    bad[3, 5] = 2.0
    with pytest.raises(quant_amd.QVQError) as e:
        engine.refine(C=bad, max_iters=4)
    assert e.value.status == QVQ_EINVAL


def test_state_rules(engine):
    S, b, bits = ref.CASES["s64_b2_4"]
    rgb, X = case("s64_b2_4")[:2]
    engine.set_images(rgb, 1, S, S, b, b, quant_amd.SCALED)
    with pytest.raises(quant_amd.QVQError) as e:   # nothing to continue from
        engine.refine(K=1 << bits, max_iters=2)
    assert e.value.status == QVQ_ESTATE
    C1, A1, d1 = engine.lbg(bits)
    engine.assign(C1)
    with pytest.raises(quant_amd.QVQError) as e:   # an assign came in between
        engine.refine(max_iters=2)
    assert e.value.status == QVQ_ESTATE
    C1, A1, d1 = engine.lbg(bits)
    C_r, A_r, d_r, _ = engine.refine(max_iters=40, eps=0.0)
    assert d_r < d1
    C2, A2, d2 = engine.lbg(bits)                  # lbg again: what it gave before
    assert np.array_equal(C2, C1) and np.array_equal(A2, A1) and d2 == d1
    try:
        engine.set_vectors(X, exact=True)
        engine.lbg(bits)
        with pytest.raises(quant_amd.QVQError) as e:
            engine.refine(max_iters=2)
        assert e.value.status == QVQ_EUNSUPPORTED
    finally:
        engine.set_images(rgb, 1, S, S, b, b, quant_amd.SCALED)   # the shared engine leaves exact mode


def test_quantizer_class_refines():
    """LBGQuantizer(refine_iters, fresh) passes eps through; the defaults are plain lbg."""
    _, X, bits, (C0, A0, d0), want = case("s64_b2_4")
    C, A, d = quant_amd.LBGQuantizer().quantize(X, bits, 0.0)
    assert np.array_equal(C, C0) and np.array_equal(A, A0)
    C, A, d = quant_amd.LBGQuantizer(refine_iters=40).quantize(X, bits, 0.0)
    assert np.array_equal(C, want[0]) and np.array_equal(A, want[1])


def test_cli_refine(tmp_path):
    """quant --refine 40: the file's codebook bytes and indices are the helper's; the unchanged
    reader decodes it; the raport's distortion falls."""
    rgb, xs, ys = load_png_rgb("t.png")
    bits = 6
    ppm, out, dec = tmp_path / "in.ppm", tmp_path / "out.quant", tmp_path / "dec.ppm"
    with open(ppm, "wb") as f:
        f.write(b"P6\n%d %d\n255\n" % (xs, ys))
        f.write(rgb.tobytes())

    def run(*args):
        return subprocess.run([QUANT, *map(str, args)], capture_output=True, text=True, timeout=300)

    r = run(ppm, "-o", out, "-n", bits, "-e", "0", "--refine", 40)
    assert r.returncode == 0, r.stderr
    X, _ = oracle.tile(rgb, xs, ys, 2, 2)
    C, A, _, info = ref.refine(X, *ref.lbg_start(X, bits), max_iters=40, eps=0.0)
    assert info["iters"] >= 2
    cb = oracle.codebook_bytes(C)
    assert open(out, "rb").read() == oracle.quant_file_bytes(cb, A, bits, oracle.SCALED, xs, ys, 2, 2)
    r = run(out, "-o", dec)
    assert r.returncode == 0, r.stderr
    np.testing.assert_array_equal(oracle.read_ppm(dec)[0], oracle.decode(cb, A, xs, ys, 2, 2))

    def raport(*flags):
        r = run(ppm, "-o", tmp_path / "x.ppm", "-n", bits, "-e", "0", "-r", "1", *flags)
        assert r.returncode == 0, r.stderr
        lines = dict(ln.split(" = ") for ln in r.stdout.splitlines() if " = " in ln)
        return float(lines["Distortion       "])

    assert raport("--refine", 40) < raport()
