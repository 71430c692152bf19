"""The fused exact sums of the D = 12 MFMA search (k_mf32.hip) on index patterns that decide how
its LDS atomics meet: qvq_lbg against the CPU oracle, indices and engine-rule centroids bit for
bit (tests/test_gpu_shapes.py _same_as_reference_lbg).  Ten levels, so every K from 64 to 1024 runs
with its own number of sums copies (16, 16, 4, 2, 1) and, from K = 256, the staggered component
order; a wrong sum at any level moves the next level's split and with it the final codebook.

Rows are bytes through oracle.lut (qvq_set_vectors' byte path).  What the oracle alone makes of the
inputs (occupied cells per level; rows of the last search with two equidistant nearest code vectors;
rows where the reference's kd-tree answer is not the brute-force one), so that no comparison is vacuous:

  A     4097 equal rows          1 cell at every level (intended: every lane of a chunk on one
                                 index, the other 1023 cells empty), 0 tied rows, distortion 0
  B2/B3 4160 rows, two vectors   2 cells at every level, 0 tied rows
  C     8257 uniform rows        2 4 8 16 31 62 119 235 453 860 cells, 5 tied rows, 2 kd != brute
  D     63 64 65 1023 1025 rows  46 48 46 61 61 of 64 cells at the last level; 3 2 1 0 1 tied rows
"""
import functools

import numpy as np
import pytest

from conftest import reference_lbg
from helpers import neartie_cases as nt
from oracle import oracle
from test_gpu_shapes import _same_as_reference_lbg

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def default_paths(monkeypatch):
    monkeypatch.delenv("QVQ_SEARCH", raising=False)
    monkeypatch.delenv("QVQ_KDTREE", raising=False)


def _equal(N):
    row = np.random.default_rng(11).integers(0, 256, 12)
    return np.tile(row, (N, 1))


def _two(N, mod):
    rng = np.random.default_rng(12)
    u, v = rng.integers(16, 64, 12), rng.integers(192, 240, 12)
    return np.where((np.arange(N) % mod == 0)[:, None], u, v)


def _uniform(N, seed):
    return np.random.default_rng(seed).integers(0, 256, (N, 12))


CASES = {
    "A-equal-4097": (lambda: _equal(4097), 10),
    "B-parity-4160": (lambda: _two(4160, 2), 10),
    "B-mod3-4160": (lambda: _two(4160, 3), 10),
    "C-uniform-8257": (lambda: _uniform(8257, 13), 10),
}
CASES.update({"D-uniform-%d" % n: (functools.partial(_uniform, n, 14 + n), 6) for n in (63, 64, 65, 1023, 1025)})


@functools.lru_cache(maxsize=None)
def _case(name):
    codes, bits = CASES[name]
    X = np.ascontiguousarray(oracle.lut(oracle.SCALED)[codes().astype(np.uint8)])
    X.setflags(write=False)
    return X, bits, reference_lbg(X, bits)


@pytest.mark.parametrize("name", list(CASES))
def test_lbg_sums(engine, name):
    X, bits, want = _case(name)
    engine.set_vectors(X)
    got = engine.lbg(bits)
    _same_as_reference_lbg(X, want, got)
    again = engine.lbg(bits)               # no sum, count or copy of the run before is seen
    assert np.array_equal(again[0], got[0]) and np.array_equal(again[1], got[1]) and again[2] == got[2]


@pytest.mark.parametrize("cs", ["scaled", "normal"])
def test_neartie_k64(engine, cs):
    """Near-tie pairs (tests/helpers/neartie_cases.py build) at K = 64, the smallest codebook of the
    32 x 32 MFMA search: every row's index is the reference's, through the flag band."""
    X, C = nt.build(12, 64, nt.COLOUR[cs], "near", seed=12064 + (7 if cs == "normal" else 0), copies=4)
    gap = nt.rel_gap(X, C)
    assert sum(1 for n in nt.band_counts(gap).values() if n >= nt.MIN_ROWS) >= 10      # the band is there
    engine.set_vectors(X)
    A = engine.assign(C)
    np.testing.assert_array_equal(A, oracle.kdtree_nn(C, X))
    assert engine.timings()["flagged"][0] > 0
