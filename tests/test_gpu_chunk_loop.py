"""The D = 12 MFMA search (assign_mf32_kernel) where a wave's sequence of chunks begins and ends
(tests/helpers/chunk_loop_cases.py): a wave starts on a fixed chunk, claims its further chunks from
its workgroup's counter and prefetches a chunk ahead, so the row counts put the waves at no chunk,
exactly one chunk each, one single-row chunk more, and two chunks each plus a ragged one.  The row
counts follow the device's CU count (the search grid is one workgroup per CU);
tests/test_chunk_loop_cases.py holds them to their patterns on the CPU.

References as in tests/test_gpu_shapes.py: reference_lbg for qvq_lbg (indices equal, codebook
bit-equal, distortion within its bound), oracle.kdtree_nn for qvq_assign."""
import functools

import numpy as np
import pytest

from conftest import reference_lbg
from helpers import chunk_loop_cases as cl
from helpers import shape_cases as sc
from oracle import oracle
from test_gpu_shapes import _same_as_reference_lbg

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def default_paths(monkeypatch):
    monkeypatch.delenv("QVQ_SEARCH", raising=False)
    monkeypatch.delenv("QVQ_KDTREE", raising=False)


@functools.lru_cache(maxsize=None)
def _cu_count():
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def _n(name):
    return cl.row_counts(_cu_count())[name]


@functools.lru_cache(maxsize=None)
def _rows(N, cs):
    X = sc.rows(12, N) if cs == oracle.SCALED else sc.vectors(N, 12, seed=31 * N + 12, cs=cs)
    X.setflags(write=False)
    return X


@functools.lru_cache(maxsize=None)
def _lbg_ref(N, cs, bits):
    C_e, A_k, d_k, C_k = reference_lbg(_rows(N, cs), bits)
    for a in (C_e, A_k, C_k):
        a.setflags(write=False)
    return C_e, A_k, d_k, C_k


def _lbg(engine, name, cs):
    N = _n(name)
    bits = min(10, sc.row_bits(N))
    X = _rows(N, cs)
    engine.set_vectors(X)
    got = engine.lbg(bits)
    _same_as_reference_lbg(X, _lbg_ref(N, cs, bits), got)
    flagged = engine.timings()["flagged"]
    print("N", N, "bits", bits, "flagged per level", flagged)
    return got


@pytest.mark.parametrize("name", cl.NAMES)
def test_lbg_at_the_chunk_edges(engine, name):
    """Every level from K = 64 on runs the fused search; from one_each_ragged on the 4-code-vector,
    the pruned LDS-table and the pruned HBM-table instantiations in one call."""
    _lbg(engine, name, oracle.SCALED)


def test_lbg_normal_colour_space(engine):
    _lbg(engine, cl.NORMAL_CASE, oracle.NORMAL)


def test_lbg_small_then_large_then_small(engine):
    """The idle waves of the two-chunk case after a run that used them all: nothing of the larger
    run's rows, and no store past N, shows in the smaller one (A is compared whole)."""
    first = _lbg(engine, "two_chunks", oracle.SCALED)
    _lbg(engine, "one_extra_row", oracle.SCALED)
    again = _lbg(engine, "two_chunks", oracle.SCALED)
    assert np.array_equal(first[0], again[0]) and np.array_equal(first[1], again[1]) and first[2] == again[2]


@pytest.mark.parametrize("K", cl.UNFUSED_KS)
def test_assign_one_extra_row(engine, K):
    """qvq_assign: its instantiations share the loop, the claims and the store."""
    N = _n(cl.UNFUSED_CASE)
    X = _rows(N, oracle.SCALED)
    C = sc.codebook(X, K, seed=K + 7 * 12)
    engine.set_vectors(X)
    A = engine.assign(C)
    assert A.shape == (N,)
    np.testing.assert_array_equal(A, oracle.kdtree_nn(C, X))
