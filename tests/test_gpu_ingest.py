"""The fp64 front door on the device (qvq_set_vectors_device and, through the same pass, the host
entry points; quant_amd/csrc/k_ingest.hip): the packed codes read back through the
public API at every pad width and on both sides of the kernel's wave, block and grid edges; the mode
a set takes when one element is foreign; and what the device entry point promises about streams,
the caller's buffer, errors and the set that was resident.  Cases: tests/helpers/ingest_cases.py.

Device rows are gathered on the device from the uploaded oracle table (lut_t[codes_t.long()]) or
uploaded bit for bit from numpy; never built by arithmetic (u / 255.0 is not the table's value)."""
import functools

import numpy as np
import pytest
import torch

import quant_amd
from conftest import reference_lbg
from helpers import ingest_cases as ic
from oracle import oracle
from test_gpu_shapes import _same_as_reference_lbg

pytestmark = pytest.mark.gpu

NORMAL, SCALED = quant_amd.NORMAL, quant_amd.SCALED
EINVAL, EUNSUPPORTED = 1, 5


@pytest.fixture(autouse=True)
def default_paths(monkeypatch):
    monkeypatch.delenv("QVQ_SEARCH", raising=False)
    monkeypatch.delenv("QVQ_KDTREE", raising=False)


def _gather(cs, codes):
    """The rows of codes under cs, built on the device from the uploaded table."""
    lut_t = torch.from_numpy(np.array(ic.lut(cs))).cuda()
    return lut_t[torch.from_numpy(np.array(codes)).cuda().long()].contiguous()


def _upload(X):
    return torch.from_numpy(np.array(X)).cuda()


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def _info(engine):
    t = engine.training_info()
    return t["mode"], t["colorspace"], t["n"], t["dim"]


def _read_back(engine, X):
    """The resident byte-path rows are X: a cell per row returns the row itself (one-row sums are
    exact and fl(1/1) = 1); past READBACK_ROWS rows, the exact-sum centroids of i mod 257."""
    n = len(X)
    if n <= ic.READBACK_ROWS:
        C, cnt = engine.update(np.arange(n, dtype=np.uint32), n)
        np.testing.assert_array_equal(cnt, np.ones(n, np.uint64))
        np.testing.assert_array_equal(_bits(C), _bits(X))
    else:
        K = ic.READBACK_ROWS
        A = (np.arange(n) % K).astype(np.uint32)
        C, cnt = engine.update(A, K)
        np.testing.assert_array_equal(cnt, np.bincount(A, minlength=K).astype(np.uint64))
        np.testing.assert_array_equal(C, oracle.centroids(X, A, K, sum_mode=1))


def _expected_space(cs, X):
    """0.0 and 1.0 are images under both spaces and SCALED is asked first."""
    return SCALED if np.isin(X, (0.0, 1.0)).all() else cs


@functools.lru_cache(maxsize=None)
def _lbg_ref(key):
    c = {k["key"]: k for k in ic.LBG_CASES}[key]
    return reference_lbg(ic.case_rows(c)[0], ic.LBG_BITS)


# -- pack correctness, read back through the public API -----------------------------------------
@pytest.mark.parametrize("c", ic.PACK_CASES + ic.STRIDE_CASES, ids=lambda c: c["key"])
def test_packed_rows_read_back(engine, c):
    X, codes = ic.case_rows(c)
    engine.set_vectors(_gather(c["cs"], codes))
    cs = _expected_space(c["cs"], X)
    assert _info(engine) == (quant_amd.MODE_BYTE, cs, c["n"], c["D"])
    _read_back(engine, X)


@pytest.mark.parametrize("c", ic.LBG_CASES, ids=lambda c: c["key"])
def test_lbg_on_packed_rows(engine, c):
    """The searches read the pad bytes too (Dp-wide rows): a wrong pad code moves distances."""
    X, codes = ic.case_rows(c)
    engine.set_vectors(_gather(c["cs"], codes))
    assert _info(engine)[:2] == (quant_amd.MODE_BYTE, c["cs"])
    _same_as_reference_lbg(X, _lbg_ref(c["key"]), engine.lbg(ic.LBG_BITS))


# -- mode selection at the edges ------------------------------------------------------------------
@pytest.mark.parametrize("val", ic.EDGE_VALUE_NAMES)
@pytest.mark.parametrize("pos", list(ic.EDGE_POSITIONS))
def test_one_foreign_element_gives_exact_mode(engine, pos, val):
    X = ic.edge_rows(pos, ic.edge_values()[val])
    engine.set_vectors(_upload(X))
    assert _info(engine) == (quant_amd.MODE_EXACT, -1, len(X), ic.EDGE_D)
    if len(X) == 257:
        C, A, _ = engine.lbg(3)
        C_ref, A_ref, _ = oracle.lbg(X, 3, sum_mode=0)     # exact mode's contract: the reference's bits
        np.testing.assert_array_equal(A, A_ref)
        np.testing.assert_array_equal(C, C_ref)


@pytest.mark.parametrize("bad", list(ic.NONFINITE))
@pytest.mark.parametrize("pos", list(ic.EDGE_POSITIONS))
def test_nonfinite_is_refused_and_the_resident_set_stays(engine, pos, bad):
    X = ic.edge_rows(pos, ic.NONFINITE[bad])
    # the resident set has the failing call's shape: the case in which its buffers would be reused
    R, _ = ic.rows(SCALED, len(X), ic.EDGE_D, 99)
    engine.set_vectors(R)
    before = engine.lbg(3)
    with pytest.raises(quant_amd.QVQError) as e:
        engine.set_vectors(_upload(X))
    assert e.value.status == EINVAL
    assert _info(engine) == (quant_amd.MODE_BYTE, SCALED, len(R), ic.EDGE_D)
    after = engine.lbg(3)
    np.testing.assert_array_equal(after[0], before[0])
    np.testing.assert_array_equal(after[1], before[1])
    assert after[2] == before[2]
    # ... and the host entry point keeps the same promise
    with pytest.raises(quant_amd.QVQError) as e:
        engine.set_vectors(X)
    assert e.value.status == EINVAL
    np.testing.assert_array_equal(engine.lbg(3)[1], before[1])


def test_the_shared_values_and_the_selection_order(engine):
    rng = np.random.default_rng(11)
    X = rng.integers(0, 2, size=(257, 5)).astype(np.float64)       # 0.0 and 1.0 only
    engine.set_vectors(_upload(X))
    assert _info(engine) == (quant_amd.MODE_BYTE, SCALED, 257, 5)
    _read_back(engine, X)
    X[-1, -1] = 5.0                                                # SCALED-valid up to its last element
    engine.set_vectors(_upload(X))
    assert _info(engine) == (quant_amd.MODE_BYTE, NORMAL, 257, 5)
    _read_back(engine, X)
    Xi = rng.integers(-128, 128, size=(257, 7)).astype(np.float64)
    engine.set_vectors(_upload(Xi))
    assert _info(engine) == (quant_amd.MODE_BYTE, NORMAL, 257, 7)
    _read_back(engine, Xi)
    Xi[100, 3] = 128.0
    engine.set_vectors(_upload(Xi))
    assert _info(engine) == (quant_amd.MODE_EXACT, -1, 257, 7)


# -- device semantics -----------------------------------------------------------------------------
def _lbg_equal(a, b):
    np.testing.assert_array_equal(a[0], b[0])
    np.testing.assert_array_equal(a[1], b[1])
    assert a[2] == b[2]


@pytest.mark.parametrize("mode", ("byte", "exact"))
def test_tensor_and_host_array_agree_and_the_tensor_is_free_on_return(engine, mode):
    X = np.array(ic.rows(SCALED, 1500, 12, 123)[0])
    if mode == "exact":
        X[700, 5] = 0.3
    engine.set_vectors(X)                                          # the host path
    want_info, want = _info(engine), engine.lbg(5)
    assert want_info[0] == (quant_amd.MODE_BYTE if mode == "byte" else quant_amd.MODE_EXACT)
    engine.set_vectors(np.zeros((3, 2)))
    Xt = _upload(X)
    engine.set_vectors(Xt)
    Xt.zero_()                                                     # the engine keeps nothing of the caller's
    torch.cuda.synchronize()
    assert _info(engine) == want_info
    _lbg_equal(engine.lbg(5), want)
    engine.set_vectors(Xt.cpu())                                   # a CPU tensor goes through numpy
    assert _info(engine)[:2] == (quant_amd.MODE_BYTE, SCALED)      # all zeros now


def test_same_shape_twice_uses_the_second_data(engine):
    X1, c1 = ic.rows(SCALED, 257, 13, 1)
    X2, c2 = ic.rows(SCALED, 257, 13, 2)
    engine.set_vectors(_gather(SCALED, c1))
    _read_back(engine, X1)
    engine.set_vectors(_gather(SCALED, c2))
    _read_back(engine, X2)
    engine.set_vectors(X1)                                         # and through the host entry point
    _read_back(engine, X1)


def test_byte_exact_byte_on_one_context(engine):
    Xb, cb = ic.rows(NORMAL, 300, 6, 8)
    Xe = np.random.default_rng(4).normal(size=(300, 6))
    engine.set_vectors(_gather(NORMAL, cb))
    first = engine.lbg(4)
    engine.set_vectors(_upload(Xe))
    assert _info(engine) == (quant_amd.MODE_EXACT, -1, 300, 6)
    C, A, _ = engine.lbg(4)
    C_ref, A_ref, _ = oracle.lbg(Xe, 4, sum_mode=0)
    np.testing.assert_array_equal(A, A_ref)
    np.testing.assert_array_equal(C, C_ref)
    engine.set_vectors(_gather(NORMAL, cb))
    assert _info(engine) == (quant_amd.MODE_BYTE, NORMAL, 300, 6)
    _lbg_equal(engine.lbg(4), first)
    _same_as_reference_lbg(Xb, reference_lbg(Xb, 4), first)


def test_rows_produced_on_a_side_stream(engine):
    """The rows come out of work queued on a side stream that nobody synchronises; the engine must
    wait for it.  (This can show a missing wait; it cannot prove the ordering.)"""
    X, codes = ic.rows(SCALED, 20000, 12, 321)
    engine.set_vectors(X)
    want = engine.lbg(4)
    engine.set_vectors(np.zeros((3, 2)))
    lut_t = torch.from_numpy(np.array(ic.lut(SCALED))).cuda()
    codes_t = torch.from_numpy(np.array(codes)).cuda().long()
    a = torch.randn(2048, 2048, device="cuda")
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        for _ in range(30):                                        # a few ms ahead of the gather
            a = (a @ a) * 1e-3
        Xt = lut_t[codes_t].contiguous()                           # queued behind the matmuls
        engine.set_vectors(Xt)                                     # torch's current stream is `side`
    assert _info(engine) == (quant_amd.MODE_BYTE, SCALED, 20000, 12)
    _lbg_equal(engine.lbg(4), want)
    torch.cuda.synchronize()


def test_bad_arguments_are_refused_before_any_read(engine):
    R, _ = ic.rows(SCALED, 64, 3, 5)
    engine.set_vectors(R)
    Xt = _gather(SCALED, ic.codes_of(1, 12, 0))                    # one row
    calls = {"misaligned": (Xt.data_ptr() + 4, 1, 5), "null": (0, 1, 12), "n=0": (Xt.data_ptr(), 0, 12),
             "dim=65": (Xt.data_ptr(), 1, 65), "n=2^32": (Xt.data_ptr(), 1 << 32, 12)}
    for name, (ptr, n, dim) in calls.items():
        for exact in (False, True):
            with pytest.raises(quant_amd.QVQError) as e:
                engine.set_vectors_device(ptr, n, dim, exact=exact)
            assert e.value.status == EINVAL, name
    assert _info(engine) == (quant_amd.MODE_BYTE, SCALED, 64, 3)
    _read_back(engine, R)


def test_wrapper_refuses_tensors_it_cannot_pass(engine, monkeypatch):
    R, _ = ic.rows(SCALED, 64, 3, 5)
    engine.set_vectors(R)
    Xt = _gather(SCALED, ic.codes_of(16, 8, 3))
    bad = {"float32": Xt.float(), "strided": Xt[:, ::2], "transposed": Xt.t(), "1-D": Xt.reshape(-1)}
    for name, t in bad.items():
        with pytest.raises(quant_amd.QVQError) as e:
            engine.set_vectors(t)
        assert e.value.status == EINVAL, name
    # a tensor of another GPU than the engine's (the engine's index is what the wrapper compares)
    with monkeypatch.context() as m:
        m.setattr(engine, "_device", Xt.device.index + 1)
        with pytest.raises(quant_amd.QVQError) as e:
            engine.set_vectors(Xt)
        assert e.value.status == EINVAL
    assert _info(engine) == (quant_amd.MODE_BYTE, SCALED, 64, 3)   # nothing reached the library
    engine.set_vectors(Xt)
    assert _info(engine) == (quant_amd.MODE_BYTE, SCALED, 16, 8)


def test_non_byte_rows_with_a_communicator_are_unsupported():
    X = np.array(ic.rows(SCALED, 257, 12, 17)[0])
    with quant_amd.Engine(0) as eng:
        eng.comm_init_host(1, 0, lambda arr: None)                 # one rank: the sum is the value
        eng.set_vectors(_upload(X))
        assert _info(eng) == (quant_amd.MODE_BYTE, SCALED, 257, 12)
        before = eng.lbg(3)
        X[5, 5] = 0.3
        for rows in (_upload(X), X):
            with pytest.raises(quant_amd.QVQError) as e:
                eng.set_vectors(rows)
            assert e.value.status == EUNSUPPORTED
        X[6, 6] = np.nan                                           # the communicator is named first
        with pytest.raises(quant_amd.QVQError) as e:
            eng.set_vectors(_upload(X))
        assert e.value.status == EUNSUPPORTED
        _lbg_equal(eng.lbg(3), before)


def test_forced_exact_mode_on_byte_rows(engine):
    X, codes = ic.rows(SCALED, 400, 12, 55)
    engine.set_vectors(X, exact=True)
    assert _info(engine) == (quant_amd.MODE_EXACT, -1, 400, 12)
    want = engine.lbg(4)
    engine.set_vectors(np.zeros((3, 2)))
    Xt = _gather(SCALED, codes)
    engine.set_vectors_device(Xt.data_ptr(), 400, 12, exact=True,
                              stream=torch.cuda.current_stream().cuda_stream)
    assert _info(engine) == (quant_amd.MODE_EXACT, -1, 400, 12)
    _lbg_equal(engine.lbg(4), want)
    C_ref, A_ref, _ = oracle.lbg(X, 4, sum_mode=0)
    np.testing.assert_array_equal(want[1], A_ref)
    np.testing.assert_array_equal(want[0], C_ref)
    Xn = _upload(np.where(np.arange(400 * 12).reshape(400, 12) == 77, np.inf, X))
    with pytest.raises(quant_amd.QVQError) as e:
        engine.set_vectors(Xn, exact=True)
    assert e.value.status == EINVAL
    _lbg_equal(engine.lbg(4), want)


def test_quantizer_passes_a_device_tensor_through():
    X, codes = ic.rows(SCALED, 500, 12, 71)
    q = quant_amd.LBGQuantizer()
    try:
        got = q.quantize(_gather(SCALED, codes), 3, 1e-6)
        assert q._engine.training_info()["mode"] == quant_amd.MODE_BYTE
        _same_as_reference_lbg(X, reference_lbg(X, 3), got)
        _lbg_equal(q.quantize(X, 3, 1e-6), got)
    finally:
        q._engine.close()
