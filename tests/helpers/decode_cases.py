"""The cases the decode tests of tests/test_gpu_decode_paths.py run: qvq_decode, qvq_decode_mse and
qvq_decode_device (quant_amd/csrc/k_misc.hip, launch_decode) on every kernel instantiation the
dispatch of quant_amd/csrc/decode_plan.hpp can reach.  Plain data and the seeded,
pure-numpy input builders; nothing here loads the engine.

Every case names the qvq_decode_plan fields (include/qvq.h, quant_amd.host_decode_plan) it is there
for; tests/test_decode_plan.py checks them on the CPU, together with what the table claims to reach
(all 16 + 2 + 1 instantiations, both sides of the 48 KB boundary, the grid caps, the wraps of the
reference's untile loop).

The three families: ROWS_H = decode_rows_h_kernel<H, lds, coal> (ys % 8 == 0, no overhang, block
height 1, 2, 4 or 8), ROWS = decode_rows_kernel<lds> (ys % 8 == 0 otherwise), PIXELS =
decode_pixels_kernel (everything else).  lds: K * bw * bh * 3 <= 49152; coal: ys % 512 == 0."""
import functools
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from oracle import oracle  # noqa: E402

PIXELS, ROWS, ROWS_H = 0, 1, 2             # qvq_decode_plan.kernel (qvq.h)
FAMILY = {PIXELS: "PIXELS", ROWS: "ROWS", ROWS_H: "ROWS_H"}
RASTER_UNALIGNED, ORIG_UNALIGNED, INDEX_UNALIGNED, CODEBOOK_ODD = 1, 2, 4, 8   # qvq_host_decode_plan's flags
LDS_CB_BYTES = 48 * 1024
STAGE_BYTES = 4 * 1536
THREADS, LDS_GRID_CAP, GRID_CAP = 256, 2048, 65536


def frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


def k_past_lds(bw, bh):
    """The smallest K whose codebook leaves LDS."""
    return LDS_CB_BYTES // (3 * bw * bh) + 1


def _case(key, xs, ys, bw, bh, K, plan, why):
    return {"key": key, "xs": xs, "ys": ys, "bw": bw, "bh": bh, "K": K, "plan": plan, "why": why}


def _rows_h(H, lds, coal, **more):
    return dict({"kernel": ROWS_H, "H": H, "lds": int(lds), "coal": int(coal)}, **more)


def _rows(lds, **more):
    return dict({"kernel": ROWS, "H": 0, "lds": int(lds), "coal": 0}, **more)


# ---------------------------------------------------------------------------------------------
# (a) ROWS_H: H x lds x coal, each at two raster heights.  xs = 2 bw + 1: the last block column is
# ragged (one pixel wide).  Coalesced: ys = 512 (one wave per raster row), 1024 (two); not: ys = 8
# (one item per row), 520 (65 items per row: waves straddle raster rows, one past the coal condition).
# ---------------------------------------------------------------------------------------------
ROWS_H_BW = {1: (1, 3), 2: (3, 8), 4: (4, 1), 8: (2, 3)}       # block widths of the first and second height
ROWS_H_K_LDS = (37, 6)                                          # small codebooks: staged in LDS


def _rows_h_cases():
    out = []
    for H in (1, 2, 4, 8):
        for lds in (True, False):
            for coal in (True, False):
                for n, ys in enumerate((512, 1024) if coal else (8, 520)):
                    bw = ROWS_H_BW[H][n]
                    K = ROWS_H_K_LDS[n] if lds else k_past_lds(bw, H)
                    out.append(_case("rowsh-H%d-%s-%s-ys%d" % (H, "lds" if lds else "glb", "coal" if coal else "direct", ys),
                                     2 * bw + 1, ys, bw, H, K, _rows_h(H, lds, coal),
                                     "decode_rows_h_kernel<%d, %s, %s>" % (H, str(lds).lower(), str(coal).lower())))
    return out


ROWS_H_CASES = _rows_h_cases() + [
    # both sides of the 48 KB boundary at D = 48: the full LDS codebook with the staging behind it
    _case("rowsh-edge-K1024", 9, 512, 4, 4, 1024, _rows_h(4, True, True, lds_bytes=LDS_CB_BYTES + STAGE_BYTES),
          "K D = 49152: the largest codebook in LDS, 49152 + 6144 B of dynamic LDS"),
    _case("rowsh-edge-K1025", 9, 512, 4, 4, 1025, _rows_h(4, False, True, lds_bytes=STAGE_BYTES),
          "K D = 49200: the smallest codebook read from global memory"),
    _case("rowsh-edge-K1024-direct", 9, 520, 4, 4, 1024, _rows_h(4, True, False, lds_bytes=LDS_CB_BYTES),
          "the full LDS codebook without staging"),
    _case("rowsh-odd-bytes", 3, 512, 1, 1, 5, _rows_h(1, True, True, lds_bytes=16 + STAGE_BYTES),
          "K D = 15: the byte tail of stage_codebook and the 16-byte rounding of the wave-stage offset"),
    _case("rowsh-c4", 9, 512, 4, 4, 4096, _rows_h(4, False, True),
          "C4's block shape and K (196 KB of codebook) on a small raster"),
]

# ---------------------------------------------------------------------------------------------
# (b) ROWS: ys % 8 == 0 with an overhang, or a block height outside {1, 2, 4, 8}.
# ---------------------------------------------------------------------------------------------
ROWS_CASES = [_case("rows-ys%d-h%d-w%d" % (ys, h, bw), 2 * bw + 1, ys, bw, h, 5 + bw + h, _rows(True),
                    "overhang %d" % (-ys % h) if ys % h else "no overhang, h outside the set")
              for ys in (8, 16, 24) for h in (3, 5, 6, 7, 9) for bw in (1, 2, 3, 4)] + [
    _case("rows-ys16-h16", 5, 16, 2, 16, 9, _rows(True), "no overhang, h outside the set"),
    _case("rows-ys8-h20", 7, 8, 3, 20, 9, _rows(True),
          "h > ys: one block row, every pixel also written from one and two raster rows up, and those lose"),
    _case("rows-edge-K512", 5, 16, 2, 16, 512, _rows(True, lds_bytes=LDS_CB_BYTES), "K D = 49152 at D = 96: LDS full"),
    _case("rows-glb-K513", 5, 16, 2, 16, 513, _rows(False, lds_bytes=0), "decode_rows_kernel<false>"),
    _case("rows-glb-overhang", 7, 24, 3, 9, k_past_lds(3, 9), _rows(False, lds_bytes=0),
          "decode_rows_kernel<false> with an overhang"),
]

# ---------------------------------------------------------------------------------------------
# (c) one shape past each grid cap: the grid-stride loops go round a second time
# ---------------------------------------------------------------------------------------------
CAP_CASES = [
    _case("cap-rowsh-coal", 8200, 512, 2, 2, 1000, _rows_h(2, True, True, grid=LDS_GRID_CAP, rounds=2),
          "524800 items past 2048 blocks"),
    _case("cap-rowsh-direct", 524300, 8, 1, 2, 300, _rows_h(2, True, False, grid=LDS_GRID_CAP, rounds=2),
          "524300 items past 2048 blocks"),
    _case("cap-rows", 524300, 8, 1, 3, 300, _rows(True, grid=LDS_GRID_CAP, rounds=2), "524300 items past 2048 blocks"),
    _case("cap-pixels", 4096, 4097, 1, 1, 70001, {"kernel": PIXELS, "H": 0, "lds": 0, "coal": 0, "grid": GRID_CAP, "rounds": 2},
          "16781312 pixels past 65536 blocks"),
]

# (c0) PIXELS at table size, for the tests that take one case per instantiation; the sweep (d) is its
# real coverage
_PIXELS_PLAN = {"kernel": PIXELS, "H": 0, "lds": 0, "coal": 0, "lds_bytes": 0}
PIXELS_CASES = [
    _case("pixels-overhang", 13, 27, 3, 5, 41, _PIXELS_PLAN, "ys % 8 != 0, overhang 3, two blocks of threads"),
    _case("pixels-tall-block", 5, 9, 2, 20, 7, _PIXELS_PLAN, "h > ys"),
    _case("pixels-big-K", 129, 97, 4, 4, 1025, _PIXELS_PLAN, "a codebook past 48 KB makes no difference here"),
]

TABLE = ROWS_H_CASES + ROWS_CASES + PIXELS_CASES + CAP_CASES

# ---------------------------------------------------------------------------------------------
# (c') qvq_decode_device with pointers that lack the row kernels' alignment: a table case, the byte
# offsets of the raster, the indices and the codebook from 16-byte aligned memory, the flags these
# make, and the instantiation the plan must then name.
# ---------------------------------------------------------------------------------------------
_PIX = (PIXELS, 0, 0, 0)


def _align_cases():
    out = []
    for base, same in (("rowsh-H4-lds-coal-ys512", (ROWS_H, 4, 1, 1)), ("rows-ys16-h5-w3", (ROWS, 0, 1, 0))):
        out += [("raster+1", base, 1, 0, 0, RASTER_UNALIGNED, _PIX), ("raster+4", base, 4, 0, 0, RASTER_UNALIGNED, _PIX),
                ("index+4", base, 0, 4, 0, INDEX_UNALIGNED, _PIX), ("index+8", base, 0, 8, 0, INDEX_UNALIGNED, _PIX),
                # an odd codebook bound for LDS: stage_codebook's byte-wise branch, the same kernel
                ("codebook+1-lds", base, 0, 0, 1, CODEBOOK_ODD, same)]
    out += [
        # an odd codebook in global memory: the 16-bit reads of H >= 2 give way to decode_rows_kernel<false>
        ("codebook+1-glb", "rowsh-edge-K1025", 0, 0, 1, CODEBOOK_ODD, (ROWS, 0, 0, 0)),
        ("codebook+1-glb", "rowsh-H2-glb-direct-ys8", 0, 0, 1, CODEBOOK_ODD, (ROWS, 0, 0, 0)),
        # H = 1 reads bytes, and so does decode_rows_kernel<false>: no change
        ("codebook+1-glb", "rowsh-H1-glb-coal-ys512", 0, 0, 1, CODEBOOK_ODD, (ROWS_H, 1, 0, 1)),
        ("codebook+1-glb", "rows-glb-K513", 0, 0, 1, CODEBOOK_ODD, (ROWS, 0, 0, 0)),
    ]
    return [{"key": "%s-%s" % (b, n), "base": b, "off_rgb": r, "off_idx": i, "off_cb": c, "flags": f, "inst": inst}
            for n, b, r, i, c, f, inst in out]


ALIGN_CASES = _align_cases()

# ---------------------------------------------------------------------------------------------
# (d) the exhaustive sweep of small rasters, one group per block width.  ys = 8 and 16 go to the row
# kernels; everything else to PIXELS.  K = 3 everywhere.
# ---------------------------------------------------------------------------------------------
SWEEP_XS, SWEEP_YS, SWEEP_BW, SWEEP_BH = range(1, 10), range(1, 18), range(1, 5), range(1, 10)
SWEEP_K = 3


def sweep_shapes(bw):
    return [(xs, ys, bw, bh) for xs in SWEEP_XS for ys in SWEEP_YS for bh in SWEEP_BH]


def sweep_kernel(ys, bh):
    """The family a sweep member takes (aligned pointers), restated from the three rules above."""
    if ys % 8:
        return PIXELS
    return ROWS_H if ys % bh == 0 and bh in (1, 2, 4, 8) else ROWS


# ---------------------------------------------------------------------------------------------
# Inputs
# ---------------------------------------------------------------------------------------------
def nblocks(xs, ys, bw, bh):
    return -(-xs // bw) * -(-ys // bh)


def identity_codebook(K, bw, bh):
    """[K, bw*bh*3]: the three bytes of pixel p of code vector c are the 24-bit number c bw bh + p,
    low byte first: no two pixels of the codebook are equal, so a wrong writer, offset, index or
    word packing changes bytes."""
    n = K * bw * bh
    assert n < 1 << 24
    v = np.arange(n, dtype=np.uint32)
    return np.stack([v & 0xFF, (v >> 8) & 0xFF, v >> 16], axis=1).astype(np.uint8).reshape(K, bw * bh * 3)


def indices(rng, K, nb):
    """nb indices in [0, K) with repeats; index K - 1 is used, and index 0 where there are two blocks."""
    A = rng.integers(0, K, size=nb, dtype=np.uint32)
    at = rng.choice(nb, size=min(2, nb), replace=False)
    A[at[0]] = K - 1
    if nb > 1:
        A[at[1]] = 0
    return A


def build(xs, ys, bw, bh, K, kind, seed):
    """(codebook [K, D] u8, indices [nblocks] u32); kind "identity" or "random" (bytes)."""
    rng = np.random.default_rng(seed)
    A = indices(rng, K, nblocks(xs, ys, bw, bh))
    if kind == "identity":
        cb = identity_codebook(K, bw, bh)
    else:
        cb = rng.integers(0, 256, size=(K, bw * bh * 3), dtype=np.uint8)
    return cb, A


KINDS = ("identity", "random")
_BY_KEY = {c["key"]: c for c in TABLE}
assert len(_BY_KEY) == len(TABLE)


def key(c):
    return c["key"]


def shape(c):
    return c["xs"], c["ys"], c["bw"], c["bh"]


@functools.lru_cache(maxsize=None)
def _inputs(k, kind):
    c = _BY_KEY[k]
    seed = sum(ord(ch) * (i + 1) for i, ch in enumerate(k))
    return frozen(*build(*shape(c), c["K"], kind, seed))


def inputs(c, kind):
    """A table case's (codebook, indices), built once per process and read-only."""
    return _inputs(c["key"], kind)


@functools.lru_cache(maxsize=None)
def _decoded(k, kind):
    c = _BY_KEY[k]
    cb, A = _inputs(k, kind)
    return frozen(oracle.decode(cb, A, *shape(c)).ravel())


def oracle_decode(c, kind):
    """oracle.decode of a table case, computed once."""
    return _decoded(c["key"], kind)


def original(c):
    """The raster a case's MSE is taken against: seeded random bytes."""
    seed = sum(ord(ch) for ch in c["key"]) + 1
    return np.random.default_rng(seed).integers(0, 256, size=c["xs"] * c["ys"] * 3, dtype=np.uint8)


def instantiation(plan):
    """(kernel, H, lds, coal): PIXELS has one, ROWS two, ROWS_H sixteen."""
    return plan["kernel"], plan["H"], plan["lds"], plan["coal"]


def first_per_instantiation(cases=None):
    """The first case of TABLE on each instantiation, in table order."""
    seen, out = set(), []
    for c in TABLE if cases is None else cases:
        i = instantiation(c["plan"])
        if i not in seen:
            seen.add(i)
            out.append(c)
    return out


# ---------------------------------------------------------------------------------------------
# The wraps of the reference's untile loop (src/Compressor.cpp:64-85; oracle.untile)
# ---------------------------------------------------------------------------------------------
def writers(xs, ys, bw, bh):
    """Per pixel, from oracle.untile of a block array whose bytes name (block, offset): (m, dx) of
    the write that survived: it came from m raster rows up (the block pixel (x - m, y + m ys)) and from
    column dx of its block."""
    nb, hB = nblocks(xs, ys, bw, bh), -(-ys // bh)
    ras = oracle.untile(identity_codebook(nb, bw, bh), xs, ys, bw, bh).reshape(xs * ys, 3).astype(np.int64)
    v = ras[:, 0] | ras[:, 1] << 8 | ras[:, 2] << 16
    blk, p = v // (bw * bh), v % (bw * bh)
    i, j, dx, dy = blk // hB, blk % hB, p // bh, p % bh
    xw, yw = i * bw + dx, j * bh + dy
    P = np.arange(xs * ys)
    assert np.array_equal(xw * ys + yw, P), "the surviving write names another pixel"
    m = P // ys - xw
    assert np.array_equal(yw, P % ys + m * ys)
    return m, dx


def loop_writes(xs, ys, bw, bh):
    """The reference loop restated, every write and not just the last: per pixel (writes, the largest
    m among all its writes, the largest m among the writes from its own block column, the m of the
    last write in loop order)."""
    wB, hB = -(-xs // bw), -(-ys // bh)
    i, j, dx, dy = np.meshgrid(np.arange(wB), np.arange(hB), np.arange(bw), np.arange(bh), indexing="ij")
    x, y = (i * bw + dx).ravel(), (j * bh + dy).ravel()          # loop order: i, j, x, y
    idx = x * ys + y
    keep = idx < xs * ys
    x, idx = x[keep], idx[keep]
    m = idx // ys - x
    count = np.bincount(idx, minlength=xs * ys)
    m_all = np.zeros(xs * ys, np.int64)
    np.maximum.at(m_all, idx, m)
    own = x // bw == (idx // ys) // bw
    m_own = np.zeros(xs * ys, np.int64)
    np.maximum.at(m_own, idx[own], m[own])
    seq = np.zeros(xs * ys, np.int64)  # every pixel is written at least once (by its own block)
    np.maximum.at(seq, idx, np.arange(len(idx)))
    return count, m_all, m_own, m[seq]
