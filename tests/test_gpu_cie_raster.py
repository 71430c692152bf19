"""CIE1931 rasters as exact-mode training sets, on the device (qvq_set_images, qvq_set_images_device,
qvq_set_synthetic with QVQ_CS_CIE1931; quant_amd/csrc/k_tile64.hip) and the read-back
qvq_get_vectors in both modes.  Every comparison is bit for bit against the restatement of
tests/helpers/cie_cases.py (the reference's tiling, then its map per pixel in numpy), which
tests/test_cie_cpu.py holds to the oracle on the CPU."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

import quant_amd
from conftest import ROOT, load_png_rgb
from helpers import cie_cases as cc
from oracle import oracle

pytestmark = pytest.mark.gpu

NORMAL, SCALED, CIE1931 = quant_amd.NORMAL, quant_amd.SCALED, quant_amd.CIE1931
EINVAL, EUNSUPPORTED, ESTATE = 1, 5, 6
QUANT = os.path.join(ROOT, "quant_amd", "lib", "quant")


@pytest.fixture(autouse=True)
def default_paths(monkeypatch):
    monkeypatch.delenv("QVQ_SEARCH", raising=False)
    monkeypatch.delenv("QVQ_KDTREE", raising=False)


def _info(engine):
    t = engine.training_info()
    return t["mode"], t["colorspace"], t["n"], t["dim"]


def _same_bits(got, want, what):
    assert got.shape == want.shape, what
    bad = np.flatnonzero(cc.bits(got).ravel() != cc.bits(want).ravel())
    assert len(bad) == 0, "%s: %d values differ, first at flat index %d: %r != %r" % (
        what, len(bad), bad[0], got.ravel()[bad[0]], want.ravel()[bad[0]])


def _set(engine, c, colorspace=CIE1931):
    engine.set_images(cc.raster(c["key"]), c["n_images"], c["xs"], c["ys"], c["bw"], c["bh"], colorspace)


def _lbg_equal(got, want):
    assert np.array_equal(cc.bits(got[0]), cc.bits(want[0]))
    np.testing.assert_array_equal(got[1], want[1])
    assert got[2] == want[2]


# -- 1. every input ---------------------------------------------------------------------------------
def test_every_colour_from_the_host(engine):
    """All 2^24 (r, g, b) at 1 x 1 blocks: the rows read back are the restatement's, and the raster is
    32 trips of the kernel's grid-stride loop."""
    c = cc.EVERY_CASE
    g = quant_amd.host_tile64_grid()
    assert cc.slots(c) > g["block"] * g["blocks"]
    _set(engine, c)
    assert _info(engine) == (quant_amd.MODE_EXACT, CIE1931, 1 << 24, 3)
    _same_bits(engine.get_vectors(), cc.expected(c["key"]), c["key"])


def test_every_colour_prefix_from_a_device_tensor(engine):
    c = cc.EVERY_SMALL
    t = torch.from_numpy(np.array(cc.raster(c["key"]))).cuda()
    assert t.dtype == torch.uint8
    engine.set_images_device(t.data_ptr(), 1, c["xs"], c["ys"], 1, 1, CIE1931)
    assert _info(engine) == (quant_amd.MODE_EXACT, CIE1931, 1 << 16, 3)
    _same_bits(engine.get_vectors(), cc.expected(c["key"]), c["key"])


# -- 2. geometry ------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", cc.GEOMETRY_CASES + [cc.STRIDE_CASE], ids=cc.key)
def test_geometry(engine, c):
    """Wrap, padding, block order and the image boundary at the smallest shapes that have them, and
    one shape past a trip of the grid-stride loop with every digit of the stride in play."""
    _set(engine, c)
    assert _info(engine) == (quant_amd.MODE_EXACT, CIE1931, cc.rows(c), 3 * c["bw"] * c["bh"])
    _same_bits(engine.get_vectors(), cc.expected(c["key"]), c["key"])


# -- 3. synthetic -----------------------------------------------------------------------------------
def test_synthetic(engine):
    s = cc.SYNTH
    engine.set_synthetic(s["S"], s["seed0"], s["n_images"], s["bw"], s["bh"], CIE1931)
    rgb = np.concatenate([oracle.gen_image(s["S"], s["seed0"] + i) for i in range(s["n_images"])])
    want = cc.cie_rows(rgb, s["n_images"], s["S"], s["S"], s["bw"], s["bh"])
    assert _info(engine) == (quant_amd.MODE_EXACT, CIE1931, len(want), 12)
    _same_bits(engine.get_vectors(), want, "synthetic")


# -- 4. quantize ------------------------------------------------------------------------------------
def _quantize_case(name):
    if name == "gen64":
        return oracle.gen_image(64), 64, 64, 2, 2, 4
    rgb, xs, ys = load_png_rgb("t.png")
    return rgb, xs, ys, 4, 4, 3


@pytest.mark.parametrize("name", ["gen64", "t.png"])
def test_quantize_equals_the_oracle_and_the_vector_route(engine, name):
    rgb, xs, ys, bw, bh, nbits = _quantize_case(name)
    X = cc.cie_rows(rgb, 1, xs, ys, bw, bh)
    C_r, A_r, _ = oracle.lbg(X, nbits, sum_mode=0)
    engine.set_images(rgb, 1, xs, ys, bw, bh, CIE1931)
    got = engine.lbg(nbits)
    assert np.array_equal(cc.bits(got[0]), cc.bits(C_r))
    np.testing.assert_array_equal(got[1], A_r)
    engine.set_vectors(X)
    assert _info(engine) == (quant_amd.MODE_EXACT, -1, len(X), 3 * bw * bh)
    _lbg_equal(engine.lbg(nbits), got)


# -- 5. state and errors ----------------------------------------------------------------------------
def test_errors_leave_the_resident_set_usable(engine):
    c = cc.GEOMETRY_CASES[3]                                      # 5 x 7, 2 x 2, three images
    _set(engine, c)
    before = engine.lbg(2)
    rgb = cc.raster(c["key"])
    with pytest.raises(quant_amd.QVQError) as e:                  # D = 3 * 2 * 11 = 66
        engine.set_images(rgb, c["n_images"], c["xs"], c["ys"], 2, 11, CIE1931)
    assert e.value.status == EINVAL and "above 64" in str(e.value)
    assert _info(engine) == (quant_amd.MODE_EXACT, CIE1931, cc.rows(c), 12)
    _lbg_equal(engine.lbg(2), before)
    with pytest.raises(quant_amd.QVQError) as e:
        engine.refine(K=4, max_iters=2)
    assert e.value.status == EUNSUPPORTED


def test_a_communicator_refuses_cie_rasters():
    c = cc.GEOMETRY_CASES[3]
    rgb = cc.raster(c["key"])
    args = (c["n_images"], c["xs"], c["ys"], c["bw"], c["bh"])
    with quant_amd.Engine(0) as eng:
        eng.comm_init_host(1, 0, lambda arr: None)                # one rank: the sum is the value
        eng.set_images(rgb, *args, SCALED)
        before = eng.lbg(2)
        t = torch.from_numpy(np.array(rgb)).cuda()
        for call in (lambda: eng.set_images(rgb, *args, CIE1931),
                     lambda: eng.set_images_device(t.data_ptr(), *args, CIE1931),
                     lambda: eng.set_synthetic(64, 1, 1, 2, 2, CIE1931)):
            with pytest.raises(quant_amd.QVQError) as e:
                call()
            assert e.value.status == EUNSUPPORTED
        with pytest.raises(quant_amd.QVQError) as e:              # the block size is named first
            eng.set_images(rgb, c["n_images"], c["xs"], c["ys"], 2, 11, CIE1931)
        assert e.value.status == EINVAL
        assert _info(eng) == (quant_amd.MODE_BYTE, SCALED, cc.rows(c), 12)
        _lbg_equal(eng.lbg(2), before)


def test_scaled_cie_scaled_on_one_context(engine):
    c = cc.GEOMETRY_CASES[9]                                      # 9 x 10, 4 x 4, three images
    _set(engine, c, SCALED)
    assert _info(engine) == (quant_amd.MODE_BYTE, SCALED, cc.rows(c), 48)
    before = engine.lbg(3)
    _set(engine, c)
    assert _info(engine) == (quant_amd.MODE_EXACT, CIE1931, cc.rows(c), 48)
    _same_bits(engine.get_vectors(), cc.expected(c["key"]), c["key"])
    engine.lbg(3)
    _set(engine, c, SCALED)
    assert _info(engine) == (quant_amd.MODE_BYTE, SCALED, cc.rows(c), 48)
    _lbg_equal(engine.lbg(3), before)


# -- 6. get_vectors on the byte path ------------------------------------------------------------------
@pytest.mark.parametrize("cs", [SCALED, NORMAL])
@pytest.mark.parametrize("geo", cc.BYTE_GEOMETRIES, ids=lambda g: "%dx%d-%dx%d" % g)
def test_get_vectors_on_the_byte_path(engine, cs, geo):
    """v64[code] of the dim real components, no pad bytes: oracle.tile of that colour space, at D = 12
    (no padding in a row) and D = 18 (two pad bytes); a sub-range starts at the right row."""
    c = next(t for t in cc.GEOMETRY_CASES if (t["xs"], t["ys"], t["bw"], t["bh"]) == geo and t["n_images"] == 3)
    _set(engine, c, cs)
    want = cc.oracle_tile(cc.raster(c["key"]), c["n_images"], c["xs"], c["ys"], c["bw"], c["bh"], cs)
    assert _info(engine) == (quant_amd.MODE_BYTE, cs, len(want), want.shape[1])
    _same_bits(engine.get_vectors(), want, c["key"])
    _same_bits(engine.get_vectors(5, 7), want[5:12], c["key"] + " rows 5..11")
    _same_bits(engine.get_vectors(len(want) - 1), want[-1:], c["key"] + " last row")
    before = engine.lbg(2)
    engine.get_vectors()
    _lbg_equal(engine.lbg(2), before)


def test_get_vectors_sub_range_in_exact_mode(engine):
    c = cc.STRIDE_CASE
    _set(engine, c)
    want = cc.expected(c["key"])
    _same_bits(engine.get_vectors(12345, 1000), want[12345:13345], "rows 12345..13344")


def test_get_vectors_errors(engine):
    L = quant_amd.lib()
    out = np.zeros((4, 64), np.float64)
    p = out.ctypes.data_as(ctypes.c_void_p)
    with quant_amd.Engine(0) as fresh:                            # no training set
        with pytest.raises(quant_amd.QVQError) as e:
            fresh.get_vectors(0, 1)
        assert e.value.status == ESTATE
    c = cc.GEOMETRY_CASES[2]                                      # 5 x 7, 2 x 2, one image: 12 rows
    n = cc.rows(c)
    for cs in (CIE1931, SCALED):
        _set(engine, c, cs)
        for row0, nrows, ptr in ((0, 0, p), (n, 1, p), (0, n + 1, p), (n - 1, 2, p), (1 << 63, 1 << 63, p),
                                 (0, 1, None)):
            assert L.qvq_get_vectors(engine._h, row0, nrows, ptr) == EINVAL, (cs, row0, nrows)
        assert L.qvq_get_vectors(engine._h, n - 1, 1, p) == 0
    assert not out[1:].any()


# -- 7. the command line ------------------------------------------------------------------------------
def test_cli_cie1931_file_matches_the_oracle(tmp_path):
    """quant -c 2: the .quant bytes are the oracle's Kahan-rule codebook through the reference's
    inverse map, and its indices.  (Also true before the raster route existed: it guards the C++
    layer's re-routing.)"""
    if not os.path.exists(QUANT):
        pytest.fail("quant CLI not built (run __graft_entry__.build())")
    rgb, xs, ys = load_png_rgb("t.png")
    ppm, quant = tmp_path / "t.ppm", tmp_path / "out.quant"
    with open(ppm, "wb") as f:
        f.write(b"P6\n%d %d\n255\n" % (xs, ys))
        f.write(rgb.tobytes())
    r = subprocess.run([QUANT, str(ppm), "-c", "2", "-w", "2", "-h", "2", "-n", "3", "-o", str(quant)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    X = cc.cie_rows(rgb, 1, xs, ys, 2, 2)
    C, A, _ = oracle.lbg(X, 3, sum_mode=0)
    want = oracle.quant_file_bytes(cc.rgb_bytes_of_cie(C), A, 3, CIE1931, xs, ys, 2, 2)
    assert open(quant, "rb").read() == want
