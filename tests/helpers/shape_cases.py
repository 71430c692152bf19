"""The cases of tests/test_gpu_shapes.py: every row width the kernels are instantiated for, ragged
row counts, and rasters that do not divide into their blocks.  tests/helpers/largek_cases.py is the
K axis; this is the D axis and the N axis.  Plain data and the input builders; nothing here loads
the engine.

Every case names the qvq_plan fields (include/qvq.h, quant_amd.host_plan) it is there for.
tests/test_shape_plan.py checks on the CPU that the engine's own dispatch predicates still give
those values and that the tables cover what their comments claim, so a later edit cannot quietly
drop a width, a row count or a raster geometry.

Field values are written as in largek_cases.py: search small | mf32 | wide | valu, recheck mf32 |
staged | chunked | global, update runs | sorted | lds."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from oracle import oracle  # noqa: E402
from helpers import largek_cases as lk  # noqa: E402


# ---------------------------------------------------------------------------------------------
# Input builders
# ---------------------------------------------------------------------------------------------
def vectors(N, D, seed, cs=oracle.SCALED):
    """N rows of D byte images (oracle.lut(cs)[codes]: qvq_set_vectors takes the fast path).  The
    codes are 150 prototype rows of uneven popularity plus noise of +-2: cells of very different
    sizes, some of them empty at the deeper levels, and equal rows (exact ties)."""
    rng = np.random.default_rng(seed)
    protos = rng.integers(0, 256, (150, D))
    w = 1.0 / (1.0 + np.arange(150))
    pick = rng.choice(150, N, p=w / w.sum())
    codes = np.clip(protos[pick] + rng.integers(-2, 3, (N, D)), 0, 255).astype(np.uint8)
    return np.ascontiguousarray(oracle.lut(cs)[codes])


def rows(D, N):
    """The training set of a width case or a row case."""
    return vectors(N, D, seed=31 * N + D)


def codebook(X, K, seed):
    """largek_cases.codebook (split pairs, zero vectors, duplicated rows: flagged rows and exact
    ties); below its smallest K = 20 the same ingredients with one duplicated row."""
    if K >= 20:
        return lk.codebook(X, K, seed)
    rng = np.random.default_rng(seed)
    base = X[rng.choice(len(X), max(1, (K - 3) // 2), replace=True)]
    C = np.concatenate([base[:1], base[:1], base * 1.2, base * 0.8, np.zeros((K, X.shape[1]))])[:K]
    return np.ascontiguousarray(C)


def raster(xs, ys, n_images, seed):
    """n_images rasters of xs * ys RGB pixels: smooth ramps plus noise (uneven cells), image-major."""
    rng = np.random.default_rng(seed)
    x, y = np.meshgrid(np.arange(xs), np.arange(ys), indexing="ij")
    out = []
    for i in range(n_images):
        ramp = np.stack([(5 * x + 3 * y + 40 * i) % 256, (2 * x * (i + 1) + 7 * y) % 256, (x * y) % 256], axis=-1)
        out.append(np.clip(ramp + rng.integers(-6, 7, ramp.shape), 0, 255).astype(np.uint8).ravel())
    return np.concatenate(out)


# ---------------------------------------------------------------------------------------------
# (a) WIDTH_CASES: one entry per width D.  Dp = D rounded up to 4 takes every value 4, 8, ..., 64,
# once each but for Dp = 64 (D = 61 with pad bytes and D = 64 without); 0-3 pad bytes; D = 1;
# D = 10 (Dp = 12 off the D = 12 kernels); wide_ks 1-5; DH != Dp (Dp = 4 mod 8) and DH = Dp.
# ---------------------------------------------------------------------------------------------
WIDTHS = [1, 5, 10, 13, 17, 24, 25, 32, 36, 37, 42, 45, 51, 54, 60, 61, 64]

# first K whose f16 codebook no longer stays resident in assign_wide_kernel's LDS, by Dp
FIRST_STREAMED = {4: 2049, 8: 2049, 12: 1121, 16: 1121, 20: 1121, 24: 1121, 28: 769, 32: 769, 36: 769, 40: 769,
                  44: 577, 48: 577, 52: 577, 56: 577, 60: 481, 64: 481}
# deeper qvq_lbg runs: (bits, K of the first streamed and pruned level); wide_ks 2, 3, 4 and 5
DEEP = {17: (11, 2048), 37: (10, 1024), 51: (10, 1024), 61: (10, 1024)}
REFINE_WIDTHS = [1, 10, 25, 32, 51, 64]


def _width(i, D):
    Dp = (D + 3) & ~3
    ks = FIRST_STREAMED[Dp]
    kb = 1535 // D                    # the last K with K * D < 1536: update_runs_kernel
    wide = {"search": "wide", "cb_resident": 1}
    levels = {2: {"search": "valu"}, 64: {"search": "valu"}, 128: dict(wide), 256: dict(wide)}
    return {
        "D": D,
        "N": 1027 + 92 * i,           # ragged: N % 4 = 3, N % 64 != 0, the second 1024-row block partial
        # (K, plan under the default dispatch); each also runs under QVQ_SEARCH=valu
        "assign": [
            ((127, 100, 77)[i % 3], {"search": "valu", "valu_tiles": 1}),
            ((333, 203, 397)[i % 3], wide),                      # K % 32 != 0: padding code vectors
            (ks - 1, wide),                                      # the last resident codebook
            (ks, {"search": "wide", "cb_resident": 0}),          # streamed in slices, the last one partial
        ],
        "host_tie_k": (333, 203, 397)[i % 3],                    # this K also with QVQ_KDTREE=host
        "update": [(kb, {"update": "runs"}), (kb + 1, {"update": "sorted"})],
        "bits": 8,
        "levels": levels,
        "deep": None if D not in DEEP else {
            "bits": DEEP[D][0], "levels": {DEEP[D][1]: {"search": "wide", "cb_resident": 0, "prune": 1}}},
    }


WIDTH_CASES = [_width(i, D) for i, D in enumerate(WIDTHS)]


# ---------------------------------------------------------------------------------------------
# (b) ROW_CASES: ragged N at D = 12 (the MFMA kernels), D = 48 (no pad) and D = 27 (one pad byte).
#   1, 2, 3      one row, less than a 4-row group
#   37           N < 64, N % 4 = 1: a partial wave
#   63, 64, 65   one 64-row chunk less one, whole, plus one
#   255, 257     the 256-row wave chunk of mean_sums_kernel / a workgroup of 256
#   1023, 1025   the 1024-row block of assign_mf32_kernel and of the Kahan sort, 512-row wide tasks
#   4099         N % 4 = 3 past 4096: a second summing block of mean_sums_kernel
#   8257         N % 64 = 1 past 8192
# Every assign shape also runs under QVQ_SEARCH=valu (assign_valu_kernel's row[r] < N).
# ---------------------------------------------------------------------------------------------
ROW_NS = [1, 2, 3, 37, 63, 64, 65, 255, 257, 1023, 1025, 4099, 8257]

_MF = {"search": "mf32"}
ROW_WIDTHS = {
    12: {"assign": [(16, {"search": "small", "fused": 1, "prune": 0, "recheck": "staged"}),
                    (100, dict(_MF, fused=1, prune=0, recheck="staged")),
                    (512, dict(_MF, fused=1, prune=1, recheck="mf32")),
                    (1100, dict(_MF, fused=0, prune=1, recheck="mf32"))],
         "update": [(127, {"update": "runs"}), (128, {"update": "sorted"})]},
    48: {"assign": [(127, {"search": "valu", "fused": 0, "prune": 0, "recheck": "staged"}),
                    (333, {"search": "wide", "cb_resident": 1, "fused": 0, "prune": 0, "recheck": "staged"}),
                    (577, {"search": "wide", "cb_resident": 0, "fused": 0, "prune": 0, "recheck": "staged"})],
         "update": [(31, {"update": "runs"}), (32, {"update": "sorted"})]},
    27: {"assign": [(127, {"search": "valu", "fused": 0, "prune": 0, "recheck": "staged"}),
                    (333, {"search": "wide", "cb_resident": 1, "fused": 0, "prune": 0, "recheck": "staged"}),
                    (769, {"search": "wide", "cb_resident": 0, "fused": 0, "prune": 0, "recheck": "staged"})],
         "update": [(56, {"update": "runs"}), (57, {"update": "sorted"})]},
}


def row_bits(N):
    """qvq_lbg's depth for N rows: K > N levels on purpose up to N = 257."""
    return 2 if N == 1 else 3 if N <= 3 else 9 if N <= 257 else 10


ROW_CASES = [{"D": D, "N": N, "bits": row_bits(N), **ROW_WIDTHS[D]} for D in ROW_WIDTHS for N in ROW_NS]


def row_partner(N):
    """Another N of the list, far from N: what the context held before (alloc_training frees and
    reallocates on a new N, and keeps every buffer on the same one)."""
    return ROW_NS[len(ROW_NS) - 1 - ROW_NS.index(N)] if N != 65 else 4099


# ---------------------------------------------------------------------------------------------
# (c) RASTER_CASES: qvq_set_images on rasters that do not divide into their blocks.
# ---------------------------------------------------------------------------------------------
def _r(name, xs, ys, bw, bh, bits, n_images=1, cs="scaled"):
    return {"name": name, "xs": xs, "ys": ys, "bw": bw, "bh": bh, "bits": bits, "n_images": n_images, "cs": cs}


RASTER_CASES = [
    # smaller than one block in each direction: one row, mostly pad
    _r("3x2_in_4x4", 3, 2, 4, 4, 2),
    _r("1x1_in_2x2", 1, 1, 2, 2, 1),
    # overhang in x only, in y only, in both
    _r("3x3_x", 50, 45, 3, 3, 8), _r("3x3_y", 48, 46, 3, 3, 8), _r("3x3_xy", 50, 46, 3, 3, 8),
    _r("4x4_x", 50, 44, 4, 4, 7), _r("4x4_y", 48, 45, 4, 4, 7), _r("4x4_xy", 50, 45, 4, 4, 7),
    _r("2x3_x", 51, 45, 2, 3, 8), _r("2x3_y", 50, 46, 2, 3, 8), _r("2x3_xy", 51, 46, 2, 3, 8),
    # 2x2 off tile22_kernel's condition (xSize even and ySize % 4 == 0), one way each
    _r("2x2_x_odd", 51, 48, 2, 2, 8), _r("2x2_y_2mod4", 50, 46, 2, 2, 8), _r("2x2_y_odd", 50, 45, 2, 2, 8),
    # several images: on the condition, and ragged (every image pads and wraps on its own)
    _r("2x2_tile22_3images", 48, 44, 2, 2, 8, n_images=3),
    _r("3x3_xy_3images", 50, 46, 3, 3, 8, n_images=3),
    # NORMAL: the pad code is 0, not 128
    _r("3x3_xy_normal", 49, 47, 3, 3, 8, cs="normal"),
    # widths of WIDTH_CASES' range through the image path
    _r("1x2_d6", 50, 45, 1, 2, 8), _r("2x5_d30", 51, 46, 2, 5, 7), _r("3x4_d36", 50, 45, 3, 4, 7),
    _r("4x5_d60", 50, 45, 4, 5, 6), _r("3x7_d63", 50, 45, 3, 7, 6),
]
UNALIGNED_RASTER = "2x2_tile22_3images"   # also through qvq_set_images_device at an odd address


def raster_classes(c):
    """The geometry classes of a raster case, by arithmetic on its sizes."""
    xs, ys, bw, bh = c["xs"], c["ys"], c["bw"], c["bh"]
    ox, oy = xs % bw != 0, ys % bh != 0
    out = set()
    if xs < bw and ys < bh:
        out.add("inside_one_%dx%d_block" % (bw, bh))
    elif (bw, bh) in ((3, 3), (4, 4), (2, 3)) and c["n_images"] == 1 and c["cs"] == "scaled":
        out.add("%dx%d_%s" % (bw, bh, "xy" if ox and oy else "x" if ox else "y" if oy else "even"))
    if (bw, bh) == (2, 2) and xs >= 2 and ys >= 2:
        if xs % 2 == 0 and ys % 4 == 0:
            out.add("2x2_tile22" + ("_images" if c["n_images"] > 1 else ""))
        elif xs % 2:
            out.add("2x2_x_odd")
        elif ys % 2:
            out.add("2x2_y_odd")
        else:
            out.add("2x2_y_2mod4")
    if c["n_images"] > 1 and (ox or oy):
        out.add("ragged_images")
    if c["cs"] == "normal" and (ox or oy):
        out.add("normal_overhang")
    if ox or oy:
        out.add("d%d_overhang" % (3 * bw * bh))
    return out


RASTER_CLASSES = (["inside_one_4x4_block", "inside_one_2x2_block", "2x2_tile22_images", "2x2_x_odd", "2x2_y_odd",
                   "2x2_y_2mod4", "ragged_images", "normal_overhang"] +
                  ["d%d_overhang" % d for d in (6, 30, 36, 60, 63)] +
                  ["%s_%s" % (b, o) for b in ("3x3", "4x4", "2x3") for o in ("x", "y", "xy")])


def raster_rows(c):
    """(rgb, the reference's rows): oracle.tile per image, image i's blocks after image i - 1's."""
    cs = oracle.NORMAL if c["cs"] == "normal" else oracle.SCALED
    rgb = raster(c["xs"], c["ys"], c["n_images"], seed=c["xs"] * 131 + c["ys"])
    per = c["xs"] * c["ys"] * 3
    X = np.concatenate([oracle.tile(rgb[i * per:(i + 1) * per], c["xs"], c["ys"], c["bw"], c["bh"], cs=cs,
                                    pad_code=128 if cs == oracle.SCALED else 0)[0] for i in range(c["n_images"])])
    return rgb, X
