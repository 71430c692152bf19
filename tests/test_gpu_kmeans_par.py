"""qvq_kmeans_par (include/qvq.h) on the device against the restatement of
tests/helpers/kmeans_par_ref.py: rows, cand_rows, cand_weights, every info field and the codebook bit
for bit (the rule is integer arithmetic, the codebook a table lookup).  The cases and the claims they
exist for are tests/helpers/kmeans_par_cases.py's; test_kmeans_par_cpu.py measures the claims on the
restatement."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import quant_amd
from conftest import ROOT, load_png_rgb
from helpers import kmeans_par_cases as cases
from helpers import kmeans_par_ref as ref
from helpers import refine_ref, reseed_ref
from oracle import oracle

pytestmark = pytest.mark.gpu
QUANT = os.path.join(ROOT, "quant_amd", "lib", "quant")
QVQ_EINVAL, QVQ_EUNSUPPORTED, QVQ_ESTATE = 1, 5, 6


def same(got, want, engine=None):
    C, rows, crows, cwt, info = got
    C_r, rows_r, crows_r, cwt_r, info_r = want
    n = min(len(rows_r), 12)
    print("info", info)
    print("reference", info_r)
    print("rows", rows[:n], "reference", rows_r[:n])
    print("cand_rows", crows[:n], "reference", crows_r[:n], "weights", cwt[:n], "reference", cwt_r[:n])
    for k in ("candidates", "rounds_run", "truncated", "round_candidates", "potential", "placed"):
        assert info[k] == info_r[k], k + " differs from the restatement"
    assert np.array_equal(crows, crows_r), "cand_rows differ from the restatement"
    assert np.array_equal(cwt, cwt_r), "cand_weights differ from the restatement"
    assert np.array_equal(rows, rows_r), "rows differ from the restatement"
    assert np.array_equal(C, C_r), "codebook differs from the restatement"
    if engine is not None:   # the codebook is qvq_get_vectors of the rows, zeros from placed on
        for j in range(min(info["placed"], 8)):
            assert np.array_equal(C[j], engine.get_vectors(int(rows[j]), 1)[0])
        assert not C[info["placed"]:].any()


def load_case(engine, name):
    c = cases.table()[name]
    engine.set_vectors(ref.values(cases.rows(name), c["cs"]))
    info = engine.training_info()
    assert info["mode"] == quant_amd.MODE_BYTE and info["colorspace"] == c["cs"]
    return c["K"], c["seed"], c["opts"]


@pytest.mark.parametrize("name", cases.names())
def test_case_against_restatement(engine, name):
    print(name + ":", cases.table()[name]["claim"])
    K, seed, opts = load_case(engine, name)
    same(engine.kmeans_par(K, seed, **opts), cases.expected(name), engine)


@pytest.mark.parametrize("name", ["dim5", "dim13", "dim61", "pad_valued_scaled", "pad_valued_normal"])
def test_colour_spaces_seed_alike(engine, name):
    """The same ordinals as NORMAL and as SCALED values: the same rows, candidates and potentials, and
    the codebooks are the two tables' values of those rows."""
    u, c = cases.rows(name), cases.table()[name]
    out = {}
    for cs in (ref.NORMAL, ref.SCALED):
        engine.set_vectors(ref.values(u, cs))
        assert engine.training_info()["colorspace"] == cs
        out[cs] = engine.kmeans_par(c["K"], c["seed"], **c["opts"])
        same(out[cs], ref.run(u, cs, c["K"], c["seed"], **c["opts"]))
    for k in (1, 2, 3):
        assert np.array_equal(out[0][k], out[1][k])
    assert out[0][4] == out[1][4] and not np.array_equal(out[0][0], out[1][0])


def test_repeatable_and_seed_dependent(engine):
    K, seed, opts = load_case(engine, "k37")
    a, b, c = engine.kmeans_par(K, seed), engine.kmeans_par(K, seed), engine.kmeans_par(K, seed + 1)
    same(b, a)
    assert not np.array_equal(a[1], c[1]) and not np.array_equal(a[2], c[2])
    same(c, ref.run(cases.rows("k37"), cases.table()["k37"]["cs"], K, seed + 1))
    # a smaller call after a larger one on the cached buffers, then the larger again
    same(engine.kmeans_par(5, seed, rounds=2, ell=3), ref.run(cases.rows("k37"), cases.table()["k37"]["cs"], 5, seed, 2, 3))
    same(engine.kmeans_par(K, seed), a)


def raster_rows(S, b, cs):
    rgb, X = reseed_ref.case_vectors(S, b, cs)
    return rgb, X, ref.ordinals_from_values(X, cs)


def test_state_after_the_call(engine):
    """lbg -> kmeans_par -> refine(C=None) is lbg -> refine(C=None); qvq_assign_device is unchanged;
    a later lbg gives what it gave."""
    rgb, X, u = raster_rows(128, 2, ref.SCALED)
    engine.set_images(rgb, 1, 128, 128, 2, 2, ref.SCALED)
    C_l, A_l, d_l = engine.lbg(6)
    want = engine.refine(K=64, max_iters=4, eps=0.0)
    engine.lbg(6)
    A_dev = engine.assign_device_ptr()
    same(engine.kmeans_par(64, 3), ref.run(u, ref.SCALED, 64, 3))
    # qvq_assign_device still holds lbg's indices: decoded on the device with a codebook whose row k is the byte k
    import torch
    assert engine.assign_device_ptr() == A_dev
    cb = np.repeat(np.arange(64, dtype=np.uint8)[:, None], 12, axis=1)
    t_cb = torch.from_numpy(cb).to("cuda:0")
    t_rgb = torch.zeros(128 * 128 * 3, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    engine.decode_device(t_cb.data_ptr(), 64, A_dev, engine.n, 128, 128, 2, 2, t_rgb.data_ptr())
    assert np.array_equal(t_rgb.cpu().numpy(), oracle.decode(cb, A_l, 128, 128, 2, 2))
    got = engine.refine(K=64, max_iters=4, eps=0.0)   # continues from the lbg as if nothing had happened
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[2] == want[2]
    assert got[3] == want[3]
    C2, A2, d2 = engine.lbg(6)
    assert np.array_equal(C2, C_l) and np.array_equal(A2, A_l) and d2 == d_l


def test_null_outputs_and_null_opts(engine):
    L = quant_amd.lib()
    K, seed, _ = load_case(engine, "dim12")
    want = cases.expected("dim12")
    assert L.qvq_kmeans_par(engine._h, K, seed, None, None, None, None, None, None) == 0
    rows = np.empty(K, np.uint32)
    assert L.qvq_kmeans_par(engine._h, K, seed, None, None, rows.ctypes.data_as(ctypes.c_void_p), None, None, None) == 0
    assert np.array_equal(rows, want[1])
    cwt = np.empty(len(want[3]), np.uint64)
    info = quant_amd._KMeansParInfo()
    assert L.qvq_kmeans_par(engine._h, K, seed, None, None, None, None, cwt.ctypes.data_as(ctypes.c_void_p),
                            ctypes.byref(info)) == 0
    assert np.array_equal(cwt, want[3]) and quant_amd._kmeans_par_info(info) == want[4]
    t = engine.timings()
    print("timings", t)
    assert t["levels"] == 0 and t["total_ms"] > 0


@pytest.mark.parametrize("cs", [ref.SCALED, ref.NORMAL])
def test_refine_from_the_seeds(engine, cs):
    """kmeans_par, then refine(C = its codebook): the restatement's refinement from the restatement's
    codebook, bit for bit; placed = K, so no cell is empty at iteration 1."""
    rgb, X, u = raster_rows(128, 2, cs)
    C_par, _, _, _, info_r = ref.run(u, cs, 48, 11)
    assert info_r["placed"] == 48
    want = refine_ref.refine(X, C_par, max_iters=6, eps=0.0)
    engine.set_images(rgb, 1, 128, 128, 2, 2, cs)
    C0, rows, _, _, info = engine.kmeans_par(48, 11)
    assert np.array_equal(C0, C_par) and info["placed"] == 48
    A0 = engine.assign(C0)
    assert np.array_equal(A0[rows.astype(np.int64)], np.arange(48))   # each seed in its own cell
    assert np.all(engine.update(A0, 48)[1] >= 1)
    C, A, d, rinfo = engine.refine(C=C0, max_iters=6, eps=0.0)
    print("iters", rinfo["iters"], "stop", rinfo["stop"], "changed", rinfo["changed"])
    assert rinfo["iters"] == want[3]["iters"] and rinfo["stop"] == want[3]["stop"]
    assert rinfo["changed"] == want[3]["changed"]
    assert np.array_equal(A, want[1]) and np.array_equal(C, want[0])
    assert abs(d - want[2]) <= 1e-9 * want[2]


def test_errors():
    import torch   # noqa: F401  (opens the device before the engine does)
    L = quant_amd.lib()
    name = "dim3"
    u, cs = cases.rows(name), cases.table()[name]["cs"]
    K, seed = cases.table()[name]["K"], cases.table()[name]["seed"]
    O = quant_amd._KMeansParOpts

    def call(eng, K, opts=None, rows=None):
        return L.qvq_kmeans_par(eng._h, K, 0, ctypes.byref(opts) if opts is not None else None, None, rows, None, None, None)

    with quant_amd.Engine(0) as eng:
        assert call(eng, 0) == QVQ_ESTATE   # no training set, before K
        eng.set_vectors(ref.values(u, cs))
        same(eng.kmeans_par(K, seed), cases.expected(name))
        rows = np.full(4, 77, np.uint32)   # (an error writes nothing)
        p = rows.ctypes.data_as(ctypes.c_void_p)
        assert call(eng, 0, None, p) == QVQ_EINVAL
        assert call(eng, (1 << 16) + 1, None, p) == QVQ_EINVAL
        assert call(eng, 4, O(17, 0, 0), p) == QVQ_EINVAL
        assert call(eng, 4, O(0, (1 << 17) + 1, 0), p) == QVQ_EINVAL
        assert call(eng, 4, O(16, 0, 1 << 16), p) == QVQ_EINVAL   # 1 + 16 * 2^16 > 2^20
        assert call(eng, 1 << 16, O(16, 0, 0), p) == QVQ_EINVAL   # the default round_cap of ell = K = 2^16
        assert np.all(rows == 77)
        assert call(eng, 4, O(16, 1 << 17, 65535), None) == 0     # the limits themselves are legal
        eng.comm_init_host(1, 0, lambda arr: None)   # one rank: still a communicator
        with pytest.raises(quant_amd.QVQError) as e:
            eng.kmeans_par(K, seed)
        assert e.value.status == QVQ_EUNSUPPORTED
        assert call(eng, 0) == QVQ_EINVAL   # K before the communicator
    with quant_amd.Engine(0) as eng:
        X = np.random.default_rng(5).random((300, 3))   # no byte image: exact mode
        eng.set_vectors(X)
        assert eng.training_info()["mode"] == quant_amd.MODE_EXACT
        with pytest.raises(quant_amd.QVQError) as e:
            eng.kmeans_par(4)
        assert e.value.status == QVQ_EUNSUPPORTED
        assert call(eng, 0) == QVQ_EINVAL   # K before the mode
        assert call(eng, 4, O(17, 0, 0)) == QVQ_EINVAL   # the options before the mode
        eng.comm_init_host(1, 0, lambda arr: None)
        with pytest.raises(quant_amd.QVQError) as e:   # the mode before the communicator
            eng.kmeans_par(4)
        assert e.value.status == QVQ_EUNSUPPORTED and "exact" in str(e.value)
    with quant_amd.Engine(0) as eng:   # a new set drops the cached buffers: a larger set after a smaller one
        eng.set_vectors(ref.values(u[:100], cs))
        eng.kmeans_par(4, 1)
        eng.set_vectors(ref.values(u, cs))
        same(eng.kmeans_par(K, seed), cases.expected(name))


def test_python_class(engine):
    cs = ref.SCALED
    rgb, X, u = raster_rows(128, 2, cs)
    C_par = ref.run(u, cs, 64, 4)[0]
    C, A, d = quant_amd.KMeansParQuantizer(seed=4).quantize(X, 6, 1e-3)
    assert np.array_equal(C, C_par)   # no iteration: the seeds and their nearest-seed assignment
    assert np.array_equal(A, oracle.kdtree_nn(C_par, X))
    assert abs(d - refine_ref.distortion(X, C_par, A)) <= 1e-9 * d
    engine.set_vectors(X)
    C_r, A_r, d_r, _ = engine.refine(C=engine.kmeans_par(64, 4, rounds=3, ell=32)[0], max_iters=5, eps=1e-3, reseed=True)
    C2, A2, d2 = quant_amd.KMeansParQuantizer(seed=4, refine_iters=5, reseed=True, rounds=3, ell=32).quantize(X, 6, 1e-3)
    assert np.array_equal(C2, C_r) and np.array_equal(A2, A_r) and d2 == d_r
    with pytest.raises(quant_amd.QVQError):
        quant_amd.KMeansParQuantizer(reseed=True)


def _ppm(tmp_path):
    rgb, w, h = load_png_rgb("t.png")
    ppm = tmp_path / "in.ppm"
    with open(ppm, "wb") as f:
        f.write(b"P6\n%d %d\n255\n" % (w, h))
        f.write(rgb.tobytes())
    # (RGBImage reads the header's first number as xSize: oracle.read_ppm gives the same pair)
    return ppm, oracle.read_ppm(str(ppm))


def test_cli_drop_in(engine, tmp_path):
    """quant --init kmeans-par --seed 5 --refine 3 (2x2 blocks, 6 bits, SCALED): the file's indices are
    the composition's on the same raster, its codebook bytes the oracle's conversion of that codebook."""
    ppm, (rgb, xs, ys) = _ppm(tmp_path)
    out = tmp_path / "out.quant"
    bits, eps = 6, float(np.float32(1e-3))   # (the CLI reads -e as a float)
    r = subprocess.run([QUANT, str(ppm), "-o", str(out), "-n", str(bits), "-e", "1e-3", "--init", "kmeans-par",
                        "--seed", "5", "--refine", "3"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    engine.set_images(rgb, 1, xs, ys, 2, 2, ref.SCALED)
    C0, rows, _, _, info = engine.kmeans_par(1 << bits, 5)
    X, _ = oracle.tile(rgb, xs, ys, 2, 2)
    assert np.array_equal(rows, ref.kmeans_par(ref.ordinals_from_values(X, ref.SCALED), 1 << bits, 5)["rows"])
    C, A, _, _ = engine.refine(C=C0, max_iters=3, eps=eps)
    assert open(out, "rb").read() == oracle.quant_file_bytes(oracle.codebook_bytes(C), A, bits, ref.SCALED, xs, ys, 2, 2)
    dec = tmp_path / "dec.ppm"
    r = subprocess.run([QUANT, str(out), "-o", str(dec)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr   # the file decodes


@pytest.mark.parametrize("extra, message", [(["--lloyd", "2"], "cannot be combined with '--lloyd'"),
                                            (["-q", "1"], "needs the LBG quantizer")])
def test_cli_rejects(tmp_path, extra, message):
    ppm, _ = _ppm(tmp_path)
    r = subprocess.run([QUANT, str(ppm), "-o", str(tmp_path / "o.quant"), "--init", "kmeans-par"] + extra,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 2
    assert message in r.stderr
