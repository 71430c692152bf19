"""The exact sums where their 16-bit register fields fill: 2^26 + 51 207 rows on the device.

mean_sums_kernel, assign_small_kernel (fused, packed sums) and update_runs_kernel add a lane's rows
in 16-bit fields; past 256 * 1024 rows per CU a lane takes more than 256 rows, so the runs' cap
flush (acc == 256) runs and the mean's grid has to grow.  The sets of
tests/helpers/sums_capacity_cases.py hold byte 0x7F (u = 255, the field's worst case) in one
component of every row (tests/test_sums_capacity_cpu.py checks what the cases claim).  They are built
on the device with torch and handed over as device rows; the reference is an integer bincount (torch
int64 on the device) over the same codes, the byte terms of quant_amd.host_row_terms, and
quant_amd.host_finalize.  Every sum is an integer: uint64 views, no tolerance."""
import functools

import numpy as np
import pytest

from helpers import sums_capacity_cases as sc
from helpers import sums_capacity_ref as ref
from oracle import oracle

pytestmark = pytest.mark.gpu

_codes = {}               # dim -> uint8 [N_EDGE, dim] on the device
_resident = [None]        # what the engine holds


def _torch():
    import torch
    return torch


@functools.lru_cache(maxsize=None)
def _tables():
    """(hi, lo) byte terms as int64 device tensors, the SCALED byte -> value table as a float64 one."""
    import quant_amd
    torch = _torch()
    hi, lo = quant_amd.host_row_terms(np.arange(256, dtype=np.uint8))
    return (torch.from_numpy(hi.astype(np.int64)).cuda(), torch.from_numpy(lo.astype(np.int64)).cuda(),
            torch.from_numpy(oracle.lut(oracle.SCALED)).cuda())


def _rows(n):
    torch = _torch()
    return torch.arange(n, dtype=torch.int64, device="cuda")


@pytest.fixture(scope="module")
def sets(engine):
    """The two sequences' codes, built once; the cases are their prefixes.  Freed at teardown."""
    torch = _torch()
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    if min(sc.small_rows_per_lane(sc.N_EDGE, cus), sc.update_rows_per_lane(sc.N_EDGE, cus)) <= sc.RUN_CAP:
        pytest.skip("%d CUs: %d rows no longer give a lane more than %d rows" % (cus, sc.N_EDGE, sc.RUN_CAP))
    i = _rows(sc.N_EDGE)
    for case in (sc.S12, sc.S3):
        pal = torch.from_numpy(sc.palette(case.dim, sc.lo_byte()[0]).astype(np.int64)).cuda()
        codes = torch.empty((case.n, case.dim), dtype=torch.uint8, device="cuda")
        for d in range(case.dim):
            codes[:, d] = sc.column(torch, i, d, pal[:, d].contiguous(), case.fixed).to(torch.uint8)
        _codes[case.dim] = codes
    del i
    yield _codes
    _codes.clear()
    _resident[0] = None
    engine.set_vectors(oracle.lut(oracle.SCALED)[np.zeros((4, 3), np.uint8)])   # the engine lets go of its 2^26 rows
    torch.cuda.empty_cache()


def _hand_over(engine, name, X):
    import quant_amd
    engine.set_vectors(X)
    info = engine.training_info()
    assert (info["mode"], info["colorspace"], info["n"], info["dim"]) == \
        (quant_amd.MODE_BYTE, quant_amd.SCALED, X.shape[0], X.shape[1]), info
    _resident[0] = name


def _load(engine, sets, name):
    """Make the case resident (fp64 device rows from its codes through the value table)."""
    if _resident[0] == name:
        return
    torch = _torch()
    case = sc.CASES[name]
    codes = sets[case.dim][:case.n]
    lut = _tables()[2]
    X = torch.empty((case.n, case.dim), dtype=torch.float64, device="cuda")
    for a in range(0, case.n, 1 << 23):
        X[a:a + (1 << 23)] = lut[codes[a:a + (1 << 23)].long()]
    _hand_over(engine, name, X)
    del X
    # the engine's rows are the case's (a slice at each end, across a band's edge and the last rows)
    for i0 in (0, sc.BAND - 1500, case.n - 3000):
        got = engine.get_vectors(i0, 3000)
        np.testing.assert_array_equal(got, oracle.lut(oracle.SCALED)[sc.rows_numpy(case, i0, i0 + 3000)])


def _ref_sums(codes, A, K):
    """Integer sums of the byte terms per cell: (hi [K, D], lo [K, D], cnt [K]) as uint64 numpy.
    codes uint8 [n, D] and A int64 [n] (None: one cell) on the device.  The largest sum, 255 n, is
    below 2^35."""
    torch = _torch()
    hi_t, lo_t, _ = _tables()
    n, D = codes.shape
    hi = torch.zeros((K, D), dtype=torch.int64, device="cuda")
    lo = torch.zeros((K, D), dtype=torch.int64, device="cuda")
    base = None if A is None else A * 256
    for d in range(D):
        key = codes[:, d].long()
        if base is not None:
            key += base
        h = torch.bincount(key, minlength=K * 256).view(K, 256)
        assert int(h.sum()) == n
        hi[:, d] = (h * hi_t).sum(1)
        lo[:, d] = (h * lo_t).sum(1)
    cnt = torch.full((1,), n, dtype=torch.int64) if A is None else torch.bincount(A, minlength=K)
    return hi.cpu().numpy().astype(np.uint64), lo.cpu().numpy().astype(np.uint64), cnt.cpu().numpy().astype(np.uint64)


@functools.lru_cache(maxsize=None)
def _ref_mean(name):
    import quant_amd
    case = sc.CASES[name]
    C = quant_amd.host_finalize(*_ref_sums(_codes[case.dim][:case.n], None, 1))
    C.setflags(write=False)
    return C


def _bits(C):
    return np.ascontiguousarray(C).view(np.uint64)


# ---- 1. the mean ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["S12", "S3", "S12-below"])
def test_mean(engine, sets, name):
    """lbg(0): the codebook is the mean.  Under the grid the launcher took before it counted adds,
    thread 0 of block 0 made 261 adds of 255 to the 0x7F components' fields (66 555: a carry into the
    neighbouring component, and the mean's high sum short by 65 536)."""
    import quant_amd
    case = sc.CASES[name]
    _load(engine, sets, name)
    C, _, _ = engine.lbg(0, want_assign=False)
    want = _ref_mean(name)
    print(name, "mean - reference:", (C - want).ravel().tolist())
    np.testing.assert_array_equal(_bits(C), _bits(want))
    # and the case is at the edge it is there for: the former grid carried here, this one does not
    dp = (case.dim + 3) & ~3
    plan = quant_amd.host_mean_grid(case.n, case.dim)
    was = ref.with_blocks(plan, ref.parent_blocks(case.n))
    assert ref.max_adds(case.n, dp, was) > sc.FIELD_ADDS >= ref.max_adds(case.n, dp, plan)


# ---- 2. qvq_update: update_runs_kernel<12> and <4> ------------------------------------------------------
@pytest.mark.parametrize("name, K, kind", [(name, K, kind) for name in ("S12", "S3") for K, kind in sc.UPDATE_CASES])
def test_update(engine, sets, name, K, kind):
    """At A = 0 every lane's run passes 256 rows (the cap flush); by band the runs end at the sprinkled
    rows' cells or at the cap, whichever comes first."""
    import quant_amd
    torch = _torch()
    case = sc.CASES[name]
    assert quant_amd.host_plan(case.dim, K, case.n)["update"] == quant_amd.PLAN_UPDATE_RUNS
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert sc.update_rows_per_lane(case.n, cus) > sc.RUN_CAP
    _load(engine, sets, name)
    A = sc.assignment(torch, kind, _rows(case.n), K)
    hi, lo, cnt = _ref_sums(sets[case.dim][:case.n], A, K)
    C, got_cnt = engine.update(A.to(torch.int32).cpu().numpy().view(np.uint32), K)
    np.testing.assert_array_equal(got_cnt, cnt)
    np.testing.assert_array_equal(_bits(C), _bits(quant_amd.host_finalize(hi, lo, cnt)))


# ---- 3. qvq_lbg: assign_small_kernel with fused, packed sums -------------------------------------------
@pytest.mark.parametrize("bits", [1, 2, 3, 4, 5])
def test_lbg_small_k(engine, sets, bits):
    import quant_amd
    torch = _torch()
    case, K = sc.S12, 1 << bits
    for b in range(1, bits + 1):
        p = quant_amd.host_plan(case.dim, 1 << b, case.n)
        assert p["search"] == quant_amd.PLAN_SEARCH_SMALL and p["fused"] == 1, p
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert sc.small_rows_per_lane(case.n, cus) > sc.RUN_CAP
    _load(engine, sets, "S12")
    C, A, d = engine.lbg(bits)
    A_dev = torch.from_numpy(A.view(np.int32)).cuda().long()
    assert int(A_dev.max()) < K
    hi, lo, cnt = _ref_sums(sets[case.dim], A_dev, K)
    assert int(cnt.sum()) == case.n
    print("bits", bits, "occupied", int(np.count_nonzero(cnt)), "distortion", d)
    np.testing.assert_array_equal(_bits(C), _bits(quant_amd.host_finalize(hi, lo, cnt)))
    if bits == 5:
        assert np.count_nonzero(cnt) >= 8
    del A_dev
    C2, A2, d2 = engine.lbg(bits)
    assert np.array_equal(_bits(C2), _bits(C)) and np.array_equal(A2, A) and d2 == d


# ---- 4. every row the same byte -------------------------------------------------------------------------
@pytest.mark.parametrize("byte, bits", [(0x80, 0), (0x80, 1), (0x7F, 0), (0x7F, 1)])
def test_constant_set(engine, sets, byte, bits):
    """One value in every component of every row: the mean is that value's finalize, one cell is
    occupied and the distortion is 0.  (At bits = 1 both children of the split are equally far from
    every row: 2^26 exact ties, which the engine answers by its synchronous redo, 4 s and 12 s.)"""
    import quant_amd
    torch = _torch()
    n, D = sc.N_EDGE, 12
    name = "constant %02x" % byte
    if _resident[0] != name:
        value = float(oracle.lut(oracle.SCALED)[byte])
        _hand_over(engine, name, torch.full((n, D), value, dtype=torch.float64, device="cuda"))
    hi, lo = quant_amd.host_row_terms(np.full((1, D), byte, np.uint8))
    mean = quant_amd.host_finalize(hi * np.uint64(n), lo * np.uint64(n), np.array([n], np.uint64))
    if bits == 0:
        C, _, d = engine.lbg(0, want_assign=False)
        np.testing.assert_array_equal(_bits(C), _bits(mean))
    else:
        C, A, d = engine.lbg(1)
        cnt = np.bincount(A, minlength=2)
        assert np.count_nonzero(cnt) == 1 and int(cnt.max()) == n
        np.testing.assert_array_equal(_bits(C[int(np.argmax(cnt))]), _bits(mean[0]))
    assert d == 0.0
