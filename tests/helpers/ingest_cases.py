"""The cases of tests/test_gpu_ingest.py and tests/test_ingest_cpu.py: the fp64 front door
(qvq_set_vectors*, qvq_set_vectors_device; quant_amd/csrc/k_ingest.hip, byte_image.hpp; DESIGN.md
3.12).  Plain data and seeded, pure-numpy builders; nothing here loads the engine.

Rows are always gathered from the oracle's own byte -> value table (oracle.lut), never built by
arithmetic: u / 255.0 is not the reference's u * fl(1/255) for 24 of the 256 bytes, and such a row
is no byte image."""
import functools
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from oracle import oracle  # noqa: E402

NORMAL, SCALED = 0, 1
SPACES = (SCALED, NORMAL)
PAD_CODE = {SCALED: 0x80, NORMAL: 0x00}

# the kernel's launch shape (quant_amd.host_ingest_grid; tests/test_ingest_cpu.py holds these to it):
# one lane per 4-byte code word, BLOCK lanes per block, at most BLOCKS blocks per trip
BLOCK, BLOCKS = 256, 2048

PACK_DS = (1, 2, 3, 5, 12, 13, 47, 48, 63, 64)
PACK_NS = (1, 63, 64, 65, 257, 4097)
READBACK_ROWS = 257          # up to here a row per cell reads the rows back; above, i mod 257
# one row count past one trip of the grid-stride loop, at the width of one word per row
STRIDE_D = 3
STRIDE_N = BLOCK * BLOCKS + 257
LBG_N, LBG_BITS = 257, 3

# what the table claims
assert {((D + 3) & ~3) - D for D in PACK_DS} == {0, 1, 2, 3}          # every count of pad bytes
assert 12 in PACK_DS and 48 in PACK_DS                                # both hot widths
assert min(PACK_DS) == 1 and max(PACK_DS) == 64                       # both ends of the legal range
for edge in (64, BLOCK):                                              # a wave and a block of one-word rows
    assert any(n < edge for n in PACK_NS) and any(n > edge for n in PACK_NS) and 64 in PACK_NS
assert any(n * ((D + 3) // 4) > BLOCK for n in PACK_NS for D in PACK_DS)    # more than one block
assert STRIDE_N * ((STRIDE_D + 3) // 4) > BLOCK * BLOCKS              # the second trip runs
assert max(PACK_NS) > READBACK_ROWS

PACK_CASES = [{"key": "pack-cs%d-D%d-n%d" % (cs, D, n), "cs": cs, "D": D, "n": n, "seed": 1000 * D + n + 7 * cs}
              for cs in SPACES for D in PACK_DS for n in PACK_NS]
STRIDE_CASES = [{"key": "stride-cs%d" % cs, "cs": cs, "D": STRIDE_D, "n": STRIDE_N, "seed": 31 + cs}
                for cs in SPACES]
LBG_CASES = [{"key": "lbg-cs%d-D%d" % (cs, D), "cs": cs, "D": D, "n": LBG_N, "seed": 50 * D + cs}
             for cs in SPACES for D in PACK_DS]

# mode selection at the edges: one SCALED set, one element replaced
EDGE_D = 12
EDGE_POSITIONS = {                       # name -> (rows, flat index of the element)
    "first": (257, 0),
    "last": (257, 257 * EDGE_D - 1),
    "row64": (257, 64 * EDGE_D),
    "last4097": (4097, 4097 * EDGE_D - 1),
}
EDGE_TABLE_BYTE = 0x80 + 100             # the table value the nextafter neighbours come from (u = 100)


def edge_values():
    """name -> the value that takes the place of one element: none of them a SCALED image, and
    (2.0, -3.0 and the SCALED neighbours) none a NORMAL one beside the set's other values."""
    t = oracle.lut(SCALED)[EDGE_TABLE_BYTE]
    return {"up": np.nextafter(t, np.inf), "down": np.nextafter(t, -np.inf), "negzero": -0.0, "half": 0.5,
            "two": 2.0, "minus3": -3.0}


EDGE_VALUE_NAMES = ("up", "down", "negzero", "half", "two", "minus3")
NONFINITE = {"nan": np.nan, "inf": np.inf}


def frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


@functools.lru_cache(maxsize=None)
def lut(cs):
    return frozen(oracle.lut(cs))


def codes_of(n, D, seed):
    return np.random.default_rng(seed).integers(0, 256, size=(n, D), dtype=np.uint8)


@functools.lru_cache(maxsize=None)
def rows(cs, n, D, seed):
    """(X [n, D] float64 gathered from oracle.lut(cs), codes [n, D] uint8)."""
    c = codes_of(n, D, seed)
    return frozen(np.ascontiguousarray(lut(cs)[c]), c)


def case_rows(c):
    return rows(c["cs"], c["n"], c["D"], c["seed"])


def edge_rows(pos, value):
    """The SCALED edge set of EDGE_POSITIONS[pos] with one element replaced by value (a copy)."""
    n, at = EDGE_POSITIONS[pos]
    X = rows(SCALED, n, EDGE_D, 4242 + n)[0].copy()
    X.reshape(-1)[at] = value
    return X


def padded(codes, cs):
    """codes [n, D] as the engine lays them out: [n, Dp], pad bytes the space's zero code."""
    n, D = codes.shape
    out = np.full((n, (D + 3) & ~3), PAD_CODE[cs], np.uint8)
    out[:, :D] = codes
    return out


def np_classify(X):
    """The rule restated with numpy alone: a value is a byte's image iff np.searchsorted finds its
    bits in the sorted table.  Returns (colour space or -1, padded codes or None)."""
    X = np.ascontiguousarray(X, np.float64)
    for cs in SPACES:
        t = lut(cs)
        order = np.argsort(t, kind="stable")
        ts = t[order]
        at = np.clip(np.searchsorted(ts, X), 0, 255)
        if np.array_equal(ts[at].view(np.int64), X.view(np.int64)):   # bits: -0.0 and NaN never match
            return cs, padded(order[at].astype(np.uint8), cs)
    return -1, None
