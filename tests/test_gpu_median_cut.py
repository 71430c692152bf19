"""qvq_median_cut (include/qvq.h) on the device against the numpy restatement of
tests/helpers/median_cut_ref.py: labels, cut counts and codebook bit for bit, the distortion within
1e-9 relative (the closed form against the direct sum, the tolerance of tests/test_gpu_refine.py).
The cases and the claims they exist for are tests/helpers/median_cut_cases.py's; test_median_cut_cpu.py
measures the claims on the restatement."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import quant_amd
from conftest import ROOT, load_png_rgb
from helpers import median_cut_cases as cases
from helpers import median_cut_ref as ref
from helpers import refine_ref, reseed_ref
from oracle import oracle

pytestmark = pytest.mark.gpu
QUANT = os.path.join(ROOT, "quant_amd", "lib", "quant")
QVQ_EINVAL, QVQ_EUNSUPPORTED, QVQ_ESTATE = 1, 5, 6


def same(got, want):
    C, A, d, cuts = got
    C_r, A_r, d_r, cuts_r = want
    print("cuts", cuts, "reference", cuts_r, "distortion", d, "reference", d_r)
    assert cuts == cuts_r, "cut counts differ from the restatement"
    assert np.array_equal(A, A_r), "labels differ from the restatement"
    assert np.array_equal(C, C_r), "codebook differs from the restatement"
    assert abs(d - d_r) <= 1e-9 * abs(d_r)


def load_case(engine, name):
    _, _, cs, bits = cases.CASES[name]
    engine.set_vectors(ref.values(cases.rows(name), cs))
    info = engine.training_info()
    assert info["mode"] == quant_amd.MODE_BYTE and info["colorspace"] == cs
    return bits


@pytest.mark.parametrize("name", list(cases.CASES))
def test_case_against_restatement(engine, name):
    print(name + ":", cases.CASES[name][0])
    bits = load_case(engine, name)
    same(engine.median_cut(bits), cases.expected(name))


def raster_rows(S, b, cs):
    rgb, X = reseed_ref.case_vectors(S, b, cs)
    return rgb, X, ref.ordinals_from_values(X, cs)


def test_colour_spaces_cut_alike(engine):
    """The same raster in NORMAL and SCALED: the same labels and cut counts."""
    out = {}
    for cs in (ref.NORMAL, ref.SCALED):
        rgb, X, u = raster_rows(128, 2, cs)
        engine.set_images(rgb, 1, 128, 128, 2, 2, cs)
        out[cs] = engine.median_cut(6)
        same(out[cs], ref.run(u, cs, 6))
    assert np.array_equal(out[ref.NORMAL][1], out[ref.SCALED][1]) and out[ref.NORMAL][3] == out[ref.SCALED][3]


def test_overhanging_blocks(engine):
    """A raster whose blocks hang over its edge: the components past the buffer are real components
    holding the space's zero code, and take part."""
    rgb, S, b = oracle.gen_image(50), 50, 4
    for cs in (ref.NORMAL, ref.SCALED):
        X, _ = oracle.tile(rgb, S, S, b, b, cs, 128 if cs == ref.SCALED else 0)
        engine.set_images(rgb, 1, S, S, b, b, cs)
        same(engine.median_cut(5), ref.run(ref.ordinals_from_values(X, cs), cs, 5))


def test_state_after_the_call(engine):
    rgb, X, u = raster_rows(128, 2, ref.SCALED)
    engine.set_images(rgb, 1, 128, 128, 2, 2, ref.SCALED)
    C_l, A_l, d_l = engine.lbg(6)
    C, A, d, cuts = engine.median_cut(6, want_assign=False)
    assert A is None
    # qvq_assign_device holds the labels: decoded on the device with a codebook whose row k is the byte k
    import torch
    cb = np.repeat(np.arange(64, dtype=np.uint8)[:, None], 12, axis=1)
    t_cb = torch.from_numpy(cb).to("cuda:0")
    t_rgb = torch.zeros(128 * 128 * 3, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    engine.decode_device(t_cb.data_ptr(), 64, engine.assign_device_ptr(), engine.n, 128, 128, 2, 2, t_rgb.data_ptr())
    assert np.array_equal(t_rgb.cpu().numpy(), oracle.decode(cb, ref.median_cut(u, 6)[0], 128, 128, 2, 2))
    # refine cannot continue from a median cut
    with pytest.raises(quant_amd.QVQError) as e:
        engine.refine(K=64, max_iters=2, eps=0.0)
    assert e.value.status == QVQ_ESTATE
    # lbg again: what it gave before
    C2, A2, d2 = engine.lbg(6)
    assert np.array_equal(C2, C_l) and np.array_equal(A2, A_l) and d2 == d_l
    same(engine.median_cut(6), ref.run(u, ref.SCALED, 6))   # and the median cut again


def test_errors():
    import torch   # noqa: F401  (opens the device before the engine does)
    L = quant_amd.lib()
    with quant_amd.Engine(0) as eng:
        assert L.qvq_median_cut(eng._h, 3, None, None, None, None) == QVQ_ESTATE   # no training set
        name = "dim3"
        u, cs = cases.rows(name), cases.CASES[name][2]
        eng.set_vectors(ref.values(u, cs))
        want = ref.run(u, cs, 4)
        same(eng.median_cut(4), want)
        A_dev = eng.assign_device_ptr()
        C = np.full(8, -7.0)   # (an error writes nothing)
        assert L.qvq_median_cut(eng._h, 21, C.ctypes.data_as(ctypes.c_void_p), None, None, None) == QVQ_EINVAL
        assert np.all(C == -7.0)
        assert eng.assign_device_ptr() == A_dev
        eng.comm_init_host(1, 0, lambda arr: None)   # one rank: still a communicator
        with pytest.raises(quant_amd.QVQError) as e:
            eng.median_cut(4)
        assert e.value.status == QVQ_EUNSUPPORTED
        assert L.qvq_median_cut(eng._h, 21, None, None, None, None) == QVQ_EINVAL   # bits before the communicator
    with quant_amd.Engine(0) as eng:
        eng.set_vectors(ref.values(u, cs))
        same(eng.median_cut(4), want)
        X = np.random.default_rng(5).random((300, 3))   # no byte image: exact mode
        eng.set_vectors(X)
        assert eng.training_info()["mode"] == quant_amd.MODE_EXACT
        with pytest.raises(quant_amd.QVQError) as e:
            eng.median_cut(4)
        assert e.value.status == QVQ_EUNSUPPORTED
        assert L.qvq_median_cut(eng._h, 21, None, None, None, None) == QVQ_EINVAL   # bits before the mode
        C_x, A_x, d_x = eng.lbg(3)   # the exact set is still usable
        assert len(A_x) == 300


@pytest.mark.parametrize("cs", [ref.SCALED, ref.NORMAL])
def test_lbg_median_cut_composition(engine, cs):
    """median_cut, then refine(C = its codebook): the restatement's refinement from the restatement's
    codebook, bit for bit."""
    rgb, X, u = raster_rows(128, 2, cs)
    C_mc = ref.run(u, cs, 6)[0]
    want = refine_ref.refine(X, C_mc, max_iters=100, eps=1e-3)
    engine.set_images(rgb, 1, 128, 128, 2, 2, cs)
    C0 = engine.median_cut(6)[0]
    assert np.array_equal(C0, C_mc)
    C, A, d, info = engine.refine(C=C0, max_iters=100, eps=1e-3)
    print("iters", info["iters"], "stop", info["stop"], "changed", info["changed"])
    assert info["iters"] == want[3]["iters"] and info["stop"] == want[3]["stop"]
    assert info["changed"] == want[3]["changed"]
    assert np.array_equal(A, want[1]) and np.array_equal(C, want[0])
    assert abs(d - want[2]) <= 1e-9 * want[2]


def test_lbg_median_cut_composition_reseed(engine):
    cs = ref.SCALED
    rgb, X, u = raster_rows(128, 2, cs)
    C_mc = ref.run(u, cs, 6)[0]
    want = reseed_ref.refine(X, C_mc, cs, max_iters=8, eps=0.0)
    engine.set_images(rgb, 1, 128, 128, 2, 2, cs)
    C, A, d, info = engine.refine(C=engine.median_cut(6)[0], max_iters=8, eps=0.0, reseed=True)
    assert info["iters"] == want[3]["iters"] and info["stop"] == want[3]["stop"]
    assert info["changed"] == want[3]["changed"] and info["reseeded"] == want[3]["reseeded"]
    assert np.array_equal(A, want[1]) and np.array_equal(C, want[0])
    assert abs(d - want[2]) <= 1e-9 * want[2]


def test_python_class(engine):
    cs = ref.SCALED
    rgb, X, u = raster_rows(128, 2, cs)
    want = ref.run(u, cs, 6)
    C, A, d = quant_amd.MedianCutQuantizer().quantize(X, 6, 1e-3)
    assert np.array_equal(C, want[0]) and np.array_equal(A, want[1]) and abs(d - want[2]) <= 1e-9 * want[2]
    engine.set_vectors(X)
    C_r, A_r, d_r, _ = engine.refine(C=engine.median_cut(6)[0], max_iters=5, eps=1e-3, fresh=True)
    C2, A2, d2 = quant_amd.MedianCutQuantizer(refine_iters=5, fresh=True).quantize(X, 6, 1e-3)
    assert np.array_equal(C2, C_r) and np.array_equal(A2, A_r) and d2 == d_r
    with pytest.raises(quant_amd.QVQError):
        quant_amd.MedianCutQuantizer(reseed=True)
    assert quant_amd.getQuantizer(quant_amd.Quantizers.MEDIAN_CUT) is None


def _ppm(tmp_path):
    rgb, w, h = load_png_rgb("t.png")
    ppm = tmp_path / "in.ppm"
    with open(ppm, "wb") as f:
        f.write(b"P6\n%d %d\n255\n" % (w, h))
        f.write(rgb.tobytes())
    # (RGBImage reads the header's first number as xSize: oracle.read_ppm gives the same pair)
    return ppm, oracle.read_ppm(str(ppm))


@pytest.mark.parametrize("q", [1, 2])
def test_cli_drop_in(engine, tmp_path, q):
    """quant -q 1 / -q 2 (2x2 blocks, 6 bits, SCALED): the file's indices are Engine.median_cut's (or
    the composition's) on the same raster, its codebook bytes the oracle's conversion of that codebook."""
    ppm, (rgb, xs, ys) = _ppm(tmp_path)
    out = tmp_path / "out.quant"
    bits, eps = 6, float(np.float32(1e-3))   # (the CLI reads -e as a float)
    r = subprocess.run([QUANT, str(ppm), "-o", str(out), "-n", str(bits), "-e", "1e-3", "-q", str(q)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    engine.set_images(rgb, 1, xs, ys, 2, 2, ref.SCALED)
    C, A, _, _ = engine.median_cut(bits)
    if q == 2:
        C, A, _, _ = engine.refine(C=C, max_iters=100, eps=eps)
    else:   # the restatement too
        X, _ = oracle.tile(rgb, xs, ys, 2, 2)
        assert np.array_equal(A, ref.median_cut(ref.ordinals_from_values(X, ref.SCALED), bits)[0])
    assert open(out, "rb").read() == oracle.quant_file_bytes(oracle.codebook_bytes(C), A, bits, ref.SCALED, xs, ys, 2, 2)
    dec = tmp_path / "dec.ppm"
    r = subprocess.run([QUANT, str(out), "-o", str(dec)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr   # the file decodes


def test_cli_exact_mode_message(tmp_path):
    ppm, _ = _ppm(tmp_path)
    r = subprocess.run([QUANT, str(ppm), "-o", str(tmp_path / "o.quant"), "-q", "1", "-c", "2"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 3
    assert "median cut has no exact mode" in r.stderr
