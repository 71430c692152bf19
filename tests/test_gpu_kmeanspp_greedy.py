"""qvq_kmeanspp_greedy (include/qvq.h) on the device against the restatement of
tests/helpers/kmeanspp_greedy_ref.py: rows, potential, placed, trial, trial_rows, trial_potential and
codebook bit for bit (the rule is integer arithmetic, the codebook a table lookup).  The cases and the
claims they exist for are tests/helpers/kmeanspp_greedy_cases.py's; test_kmeanspp_greedy_cpu.py
measures the claims on the restatement."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import quant_amd
from conftest import ROOT, load_png_rgb
from helpers import kmeanspp_greedy_cases as cases
from helpers import kmeanspp_greedy_ref as ref
from helpers import refine_ref, reseed_ref
from oracle import oracle

pytestmark = pytest.mark.gpu
QUANT = os.path.join(ROOT, "quant_amd", "lib", "quant")
QVQ_EINVAL, QVQ_EUNSUPPORTED, QVQ_ESTATE = 1, 5, 6


def same(got, want):
    C, rows, pot, info = got
    C_r, rows_r, pot_r, info_r = want
    n = min(len(rows_r), 8)
    print("placed", info["placed"], "reference", info_r["placed"], "trials", info["trials"], "reference", info_r["trials"])
    print("rows", rows[:n], "reference", rows_r[:n])
    print("potential", pot[:n], "reference", pot_r[:n])
    print("trial", info["trial"][:n], "reference", info_r["trial"][:n])
    assert info["placed"] == info_r["placed"], "placed differs from the restatement"
    assert info["trials"] == info_r["trials"], "the trial count differs from the restatement"
    assert np.array_equal(info["trial_rows"], info_r["trial_rows"]), "trial_rows differ from the restatement"
    assert np.array_equal(info["trial_potential"], info_r["trial_potential"]), "trial_potential differs from the restatement"
    assert np.array_equal(info["trial"], info_r["trial"]), "the winning trials differ from the restatement"
    assert np.array_equal(rows, rows_r), "rows differ from the restatement"
    assert np.array_equal(pot, pot_r), "potentials differ from the restatement"
    assert np.array_equal(C, C_r), "codebook differs from the restatement"


def load_case(engine, name):
    c = cases.table()[name]
    engine.set_vectors(ref.values(cases.rows(name), c["cs"]))
    info = engine.training_info()
    assert info["mode"] == quant_amd.MODE_BYTE and info["colorspace"] == c["cs"]
    return c["K"], c["seed"], c["trials"]


@pytest.mark.parametrize("name", cases.names())
def test_case_against_restatement(engine, name):
    print(name + ":", cases.table()[name]["claim"])
    K, seed, trials = load_case(engine, name)
    got = engine.kmeanspp_greedy(K, seed, trials)
    same(got, cases.expected(name))
    C, rows, _, info = got
    if info["placed"] == K:   # K distinct seeds: K non-empty cells, each seed in its own
        A = engine.assign(C)
        assert np.array_equal(A[rows.astype(np.int64)], np.arange(K))
        assert np.all(engine.update(A, K)[1] >= 1)


@pytest.mark.parametrize("name", ["trials_1", "trials_9", "k300", "width_57"])
def test_one_trial_is_kmeanspp(engine, name):
    """L = 1 against Engine.kmeanspp on the same context, and the case's own L after it."""
    K, seed, trials = load_case(engine, name)
    C_p, rows_p, pot_p, placed_p = engine.kmeanspp(K, seed)
    C, rows, pot, info = engine.kmeanspp_greedy(K, seed, 1)
    assert info["placed"] == placed_p and info["trials"] == 1
    assert np.array_equal(rows, rows_p) and np.array_equal(pot, pot_p) and np.array_equal(C, C_p)
    assert np.all(info["trial"] == 0) and np.array_equal(info["trial_rows"][:, 0], rows)
    assert np.array_equal(info["trial_potential"][:, 0], pot) and np.all(info["trial_rows"][:, 1:] == ref.NO_ROW)
    same(engine.kmeanspp_greedy(K, seed, trials), cases.expected(name))
    again = engine.kmeanspp(K, seed)   # and qvq_kmeanspp is what it was
    assert np.array_equal(again[1], rows_p) and np.array_equal(again[2], pot_p)


def test_repeatable_and_seed_dependent(engine):
    K, seed, trials = load_case(engine, "k300")
    a, b, c = engine.kmeanspp_greedy(K, seed, trials), engine.kmeanspp_greedy(K, seed, trials), engine.kmeanspp_greedy(K, seed + 1, 3)
    same(b, a)
    assert not np.array_equal(a[1], c[1])
    same(c, ref.run(cases.rows("k300"), cases.table()["k300"]["cs"], K, seed + 1, 3))
    # a smaller K after a larger one on the cached buffers, with the larger call's trial count: its prefix
    small = engine.kmeanspp_greedy(7, seed, a[3]["trials"])
    assert np.array_equal(small[1], a[1][:7]) and np.array_equal(small[2], a[2][:7]) and small[3]["placed"] == 7
    assert np.array_equal(small[3]["trial_rows"], a[3]["trial_rows"][:7])
    same(engine.kmeanspp_greedy(K, seed, trials), a)   # and the larger one again


def test_colour_spaces_seed_alike(engine):
    """The same ordinals as NORMAL and as SCALED values: the same rows, trials and potentials, and the
    codebooks are the two tables' values of those rows."""
    u = cases.rows("width_6")
    out = {}
    for cs in (ref.NORMAL, ref.SCALED):
        engine.set_vectors(ref.values(u, cs))
        assert engine.training_info()["colorspace"] == cs
        out[cs] = engine.kmeanspp_greedy(16, 9, 5)
        same(out[cs], ref.run(u, cs, 16, 9, 5))
    assert np.array_equal(out[0][1], out[1][1]) and np.array_equal(out[0][2], out[1][2])
    assert np.array_equal(out[0][3]["trial_potential"], out[1][3]["trial_potential"])
    assert not np.array_equal(out[0][0], out[1][0])


def raster_rows(S, b, cs):
    rgb, X = reseed_ref.case_vectors(S, b, cs)
    return rgb, X, ref.ordinals_from_values(X, cs)


def test_state_after_the_call(engine):
    """lbg -> kmeanspp_greedy -> refine(C=None) is lbg -> refine(C=None); qvq_assign_device is
    unchanged; a later lbg gives what it gave."""
    rgb, X, u = raster_rows(128, 2, ref.SCALED)
    engine.set_images(rgb, 1, 128, 128, 2, 2, ref.SCALED)
    C_l, A_l, d_l = engine.lbg(6)
    want = engine.refine(K=64, max_iters=4, eps=0.0)
    engine.lbg(6)
    A_dev = engine.assign_device_ptr()
    same(engine.kmeanspp_greedy(64, 3), ref.run(u, ref.SCALED, 64, 3))
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


def test_null_outputs(engine):
    L = quant_amd.lib()
    K, seed, trials = load_case(engine, "width_48")
    want = cases.expected("width_48")
    assert L.qvq_kmeanspp_greedy(engine._h, K, seed, trials, None, None, None, None, None, None, None) == 0
    trial = np.empty(K, np.uint32)
    assert L.qvq_kmeanspp_greedy(engine._h, K, seed, trials, None, None, None, trial.ctypes.data_as(ctypes.c_void_p), None,
                                 None, None) == 0
    assert np.array_equal(trial, want[3]["trial"])
    tpot = np.empty((K, 16), np.uint64)
    assert L.qvq_kmeanspp_greedy(engine._h, K, seed, trials, None, None, None, None, None,
                                 tpot.ctypes.data_as(ctypes.c_void_p), None) == 0
    assert np.array_equal(tpot, want[3]["trial_potential"])
    trows = np.empty((K, 16), np.uint32)
    assert L.qvq_kmeanspp_greedy(engine._h, K, seed, trials, None, None, None, None, trows.ctypes.data_as(ctypes.c_void_p),
                                 None, None) == 0
    assert np.array_equal(trows, want[3]["trial_rows"])
    t = engine.timings()
    print("timings", t)
    assert t["levels"] == 0 and t["total_ms"] > 0


@pytest.mark.parametrize("cs", [ref.SCALED, ref.NORMAL])
def test_refine_from_the_seeds(engine, cs):
    """kmeanspp_greedy, then refine(C = its codebook): the restatement's refinement from the
    restatement's codebook, bit for bit, and K non-empty cells after iteration 1."""
    rgb, X, u = raster_rows(128, 2, cs)
    C_pp = ref.run(u, cs, 48, 11, 4)[0]
    want = refine_ref.refine(X, C_pp, max_iters=6, eps=0.0)
    engine.set_images(rgb, 1, 128, 128, 2, 2, cs)
    C0, _, _, info0 = engine.kmeanspp_greedy(48, 11, 4)
    assert np.array_equal(C0, C_pp) and info0["placed"] == 48
    C1, A1, _, _ = engine.refine(C=C0, max_iters=1, eps=0.0)
    assert np.all(np.bincount(A1, minlength=48) >= 1)   # every seed keeps a cell
    C, A, d, info = engine.refine(C=C0, max_iters=6, eps=0.0)
    print("iters", info["iters"], "stop", info["stop"], "changed", info["changed"])
    assert info["iters"] == want[3]["iters"] and info["stop"] == want[3]["stop"]
    assert info["changed"] == want[3]["changed"]
    assert np.array_equal(A, want[1]) and np.array_equal(C, want[0])
    assert abs(d - want[2]) <= 1e-9 * want[2]


def test_errors():
    import torch   # noqa: F401  (opens the device before the engine does)
    L = quant_amd.lib()
    name = "width_3"
    u, c = cases.rows(name), cases.table()[name]
    K, seed, trials, cs = c["K"], c["seed"], c["trials"], c["cs"]

    def call(eng, K, trials, p=None):
        return L.qvq_kmeanspp_greedy(eng._h, K, 0, trials, None, p, None, None, None, None, None)

    with quant_amd.Engine(0) as eng:
        assert call(eng, 0, 17) == QVQ_ESTATE   # no training set, before K and trials
        eng.set_vectors(ref.values(u, cs))
        same(eng.kmeanspp_greedy(K, seed, trials), cases.expected(name))
        rows = np.full(4, 77, np.uint32)   # (an error writes nothing)
        p = rows.ctypes.data_as(ctypes.c_void_p)
        assert call(eng, 0, 0, p) == QVQ_EINVAL
        assert call(eng, (1 << 20) + 1, 0, p) == QVQ_EINVAL
        assert call(eng, 4, 17, p) == QVQ_EINVAL
        assert np.all(rows == 77)
        with pytest.raises(quant_amd.QVQError):
            eng.kmeanspp_greedy(4, 0, 17)
        eng.comm_init_host(1, 0, lambda arr: None)   # one rank: still a communicator
        with pytest.raises(quant_amd.QVQError) as e:
            eng.kmeanspp_greedy(K, seed, trials)
        assert e.value.status == QVQ_EUNSUPPORTED
        assert call(eng, 0, 0) == QVQ_EINVAL and call(eng, 4, 17) == QVQ_EINVAL   # K and trials before the communicator
    with quant_amd.Engine(0) as eng:
        X = np.random.default_rng(5).random((300, 3))   # no byte image: exact mode
        eng.set_vectors(X)
        assert eng.training_info()["mode"] == quant_amd.MODE_EXACT
        with pytest.raises(quant_amd.QVQError) as e:
            eng.kmeanspp_greedy(4)
        assert e.value.status == QVQ_EUNSUPPORTED
        assert call(eng, 0, 0) == QVQ_EINVAL and call(eng, 4, 17) == QVQ_EINVAL   # K and trials before the mode
        eng.comm_init_host(1, 0, lambda arr: None)
        with pytest.raises(quant_amd.QVQError) as e:   # the mode before the communicator
            eng.kmeanspp_greedy(4)
        assert e.value.status == QVQ_EUNSUPPORTED and "exact" in str(e.value)
    with quant_amd.Engine(0) as eng:   # a new set drops the cached buffers: a larger set after a smaller one
        eng.set_vectors(ref.values(u[:100], cs))
        eng.kmeanspp_greedy(4, 1, 2)
        eng.set_vectors(ref.values(u, cs))
        same(eng.kmeanspp_greedy(K, seed, trials), cases.expected(name))


def test_python_class(engine):
    cs = ref.SCALED
    rgb, X, u = raster_rows(128, 2, cs)
    C_pp = ref.run(u, cs, 64, 4, 0)[0]
    C, A, d = quant_amd.GreedyKMeansPPQuantizer(seed=4).quantize(X, 6, 1e-3)
    assert np.array_equal(C, C_pp)   # no iteration: the seeds and their nearest-seed assignment
    assert np.array_equal(A, oracle.kdtree_nn(C_pp, X))
    assert abs(d - refine_ref.distortion(X, C_pp, A)) <= 1e-9 * d
    engine.set_vectors(X)
    C_r, A_r, d_r, _ = engine.refine(C=engine.kmeanspp_greedy(64, 4, 3)[0], max_iters=5, eps=1e-3, reseed=True)
    C2, A2, d2 = quant_amd.GreedyKMeansPPQuantizer(seed=4, trials=3, refine_iters=5, reseed=True).quantize(X, 6, 1e-3)
    assert np.array_equal(C2, C_r) and np.array_equal(A2, A_r) and d2 == d_r
    with pytest.raises(quant_amd.QVQError):
        quant_amd.GreedyKMeansPPQuantizer(reseed=True)
    with pytest.raises(quant_amd.QVQError):
        quant_amd.GreedyKMeansPPQuantizer(trials=17)


def _ppm(tmp_path):
    rgb, w, h = load_png_rgb("t.png")
    ppm = tmp_path / "in.ppm"
    with open(ppm, "wb") as f:
        f.write(b"P6\n%d %d\n255\n" % (w, h))
        f.write(rgb.tobytes())
    # (RGBImage reads the header's first number as xSize: oracle.read_ppm gives the same pair)
    return ppm, oracle.read_ppm(str(ppm))


def test_cli_drop_in(engine, tmp_path):
    """quant --init kmeans++ --trials 3 --seed 5 --refine 3 (2x2 blocks, 6 bits, SCALED): the file's
    indices are the composition's on the same raster, its codebook bytes the oracle's conversion of
    that codebook; without --trials the file is qvq_kmeanspp's, as before."""
    ppm, (rgb, xs, ys) = _ppm(tmp_path)
    bits, eps = 6, float(np.float32(1e-3))   # (the CLI reads -e as a float)
    engine.set_images(rgb, 1, xs, ys, 2, 2, ref.SCALED)
    X, _ = oracle.tile(rgb, xs, ys, 2, 2)
    u = ref.ordinals_from_values(X, ref.SCALED)
    for extra, start in ((["--trials", "3"], lambda: engine.kmeanspp_greedy(1 << bits, 5, 3)),
                         (["--trials", "0"], lambda: engine.kmeanspp_greedy(1 << bits, 5, 0)),
                         ([], lambda: engine.kmeanspp(1 << bits, 5))):
        out = tmp_path / "out.quant"
        r = subprocess.run([QUANT, str(ppm), "-o", str(out), "-n", str(bits), "-e", "1e-3", "--init", "kmeans++",
                            "--seed", "5", "--refine", "3", *extra], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        C0, rows = start()[:2]
        if extra:
            assert np.array_equal(rows, ref.kmeanspp_greedy(u, 1 << bits, 5, int(extra[1]))["rows"])
        C, A, _, _ = engine.refine(C=C0, max_iters=3, eps=eps)
        assert open(out, "rb").read() == oracle.quant_file_bytes(oracle.codebook_bytes(C), A, bits, ref.SCALED, xs, ys, 2, 2)
    dec = tmp_path / "dec.ppm"
    r = subprocess.run([QUANT, str(out), "-o", str(dec)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr   # the file decodes
