"""The cases of tests/test_cie_cpu.py and tests/test_gpu_cie_raster.py: CIE1931 rasters as exact-mode
training sets (qvq_set_images* / qvq_set_synthetic with QVQ_CS_CIE1931; quant_amd/csrc/k_tile64.hip,
cie1931.hpp) and the read-back qvq_get_vectors.  Plain data and seeded, pure-numpy
builders; nothing here loads the engine.

The restatement every comparison is made against, bit for bit: the reference's tiling
(getBlocksAsVectorsFromImage, src/Compressor.cpp:31-62) over the raster's signed-byte values with
entries past the buffer as zeros -- tile_signed below, held to oracle.tile(..., NORMAL) by
tests/test_cie_cpu.py -- then the reference's map (src/ColorSpace.cpp:30-33) per pixel triple in numpy,
each product and sum rounded on its own, in the reference's order, and a true division."""
import functools
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from oracle import oracle  # noqa: E402

NORMAL, SCALED, CIE1931 = 0, 1, 2
PAD_CODE = {SCALED: 0x80, NORMAL: 0x00}

# the kernel's launch shape (quant_amd.host_tile64_grid; tests/test_cie_cpu.py holds these to it): one
# lane per (row, pixel in block) slot, BLOCK lanes per block, at most BLOCKS blocks per trip
BLOCK, BLOCKS = 256, 2048

# (xSize, ySize, bw, bh): the smallest shapes where wrap, pad and block order can each go wrong
GEOMETRIES = ((5, 3, 2, 1), (5, 7, 2, 2), (7, 5, 3, 2), (4, 4, 4, 4), (9, 10, 4, 4), (3, 3, 1, 7), (1, 1, 2, 2))
N_IMAGES = (1, 3)
GEOMETRY_CASES = [{"key": "geo-%dx%d-%dx%d-n%d" % (xs, ys, bw, bh, n), "xs": xs, "ys": ys, "bw": bw, "bh": bh,
                   "n_images": n, "seed": 7000 + 100 * xs + 10 * ys + bw + bh + n}
                  for (xs, ys, bw, bh) in GEOMETRIES for n in N_IMAGES]
# every (r, g, b) once: a 4096 x 4096 raster, 1 x 1 blocks (N = 2^24, D = 3); and its first 256 x 256
EVERY_CASE = {"key": "every-colour", "xs": 4096, "ys": 4096, "bw": 1, "bh": 1, "n_images": 1, "seed": None}
EVERY_SMALL = {"key": "every-colour-256", "xs": 256, "ys": 256, "bw": 1, "bh": 1, "n_images": 1, "seed": None}
# past one trip of the grid-stride loop with every digit of the stride in play: 5 x 3 blocks (the
# stride 2^19 has a nonzero digit under each of the radices 3, 5, 175, 141), two images, a wrapped
# last column and padded last blocks
STRIDE_CASE = {"key": "stride-701x523-5x3-n2", "xs": 701, "ys": 523, "bw": 5, "bh": 3, "n_images": 2, "seed": 99}
TABLE = GEOMETRY_CASES + [EVERY_CASE, EVERY_SMALL, STRIDE_CASE]
# qvq_get_vectors on the byte path: D = 12 (a multiple of 4) and D = 18 (two pad bytes)
BYTE_GEOMETRIES = ((5, 7, 2, 2), (7, 5, 3, 2))
SYNTH = {"S": 64, "seed0": 0x5EED, "n_images": 2, "bw": 2, "bh": 2}


def key(c):
    return c["key"]


def blocks(c):
    wB, hB = -(-c["xs"] // c["bw"]), -(-c["ys"] // c["bh"])
    return wB, hB


def rows(c):
    wB, hB = blocks(c)
    return wB * hB * c["n_images"]


def slots(c):
    return rows(c) * c["bw"] * c["bh"]


def pixel_index(c):
    """[wB, hB, bw, bh] raster entry of every block pixel: (i * bw + dx) * ySize + (j * bh + dy)."""
    wB, hB = blocks(c)
    i, j, dx, dy = np.meshgrid(np.arange(wB), np.arange(hB), np.arange(c["bw"]), np.arange(c["bh"]), indexing="ij")
    return (i * c["bw"] + dx) * c["ys"] + (j * c["bh"] + dy)


def wraps(c):
    """Some block pixel lies in a column past ySize and still inside the buffer: it reads the next raster row."""
    wB, hB = blocks(c)
    y = np.arange(hB * c["bh"]).reshape(1, hB, 1, c["bh"])   # j * bh + dy
    px = pixel_index(c)
    return bool(np.any((np.broadcast_to(y, px.shape) >= c["ys"]) & (px < c["xs"] * c["ys"])))


def padded_per_block(c):
    """[wB * hB] pixels of each block past the end of the image's buffer."""
    wB, hB = blocks(c)
    return np.sum(pixel_index(c) >= c["xs"] * c["ys"], axis=(2, 3)).reshape(wB * hB)


@functools.lru_cache(maxsize=None)
def all_colours():
    """Every (r, g, b) once, colour c = r << 16 | g << 8 | b at pixel c: [2^24, 3] uint8."""
    c = np.arange(1 << 24, dtype=np.uint32)
    rgb = np.stack([(c >> 16) & 255, (c >> 8) & 255, c & 255], axis=1).astype(np.uint8)
    rgb.setflags(write=False)
    return rgb


@functools.lru_cache(maxsize=None)
def raster(k):
    """The case's rasters, image-major: uint8 [n_images * xs * ys * 3]."""
    c = {t["key"]: t for t in TABLE}[k]
    npix = c["n_images"] * c["xs"] * c["ys"]
    if c["seed"] is None:
        rgb = all_colours()[:npix].reshape(-1)
    else:
        rgb = np.random.default_rng(c["seed"]).integers(0, 256, size=npix * 3, dtype=np.uint8)
        rgb.setflags(write=False)
    return rgb


def tile_signed(rgb, n_images, xs, ys, bw, bh):
    """The reference's tiling restated in numpy over the bytes read as signed chars: float64
    [n_images * wB * hB, 3 * bw * bh], entries past an image's buffer 0.0."""
    c = {"xs": xs, "ys": ys, "bw": bw, "bh": bh}
    wB, hB = blocks(c)
    px = pixel_index(c)
    inside = px < xs * ys
    img = np.asarray(rgb, np.uint8).view(np.int8).reshape(n_images, xs * ys, 3).astype(np.float64)
    out = np.zeros((n_images, wB, hB, bw, bh, 3), np.float64)
    out[:, inside] = img[:, px[inside]]
    return out.reshape(n_images * wB * hB, 3 * bw * bh)


def cie_map(P):
    """src/ColorSpace.cpp:30-33 over P [..., 3] (signed-byte values as float64), in its order."""
    r, g, b = P[..., 0], P[..., 1], P[..., 2]
    return np.stack([((r * 0.490 + g * 0.310) + b * 0.200) / 0.17697,
                     ((r * 0.17697 + g * 0.81240) + b * 0.01063) / 0.17697,
                     ((r * 0 + g * 0.01) + b * 0.99) / 0.17697], axis=-1)


def cie_rows(rgb, n_images, xs, ys, bw, bh):
    """The rows a CIE1931 raster stands for: tile_signed, then cie_map per pixel triple."""
    T = tile_signed(rgb, n_images, xs, ys, bw, bh)
    return np.ascontiguousarray(cie_map(T.reshape(len(T), bw * bh, 3)).reshape(len(T), 3 * bw * bh))


@functools.lru_cache(maxsize=None)
def expected(k):
    """cie_rows of the case's rasters, computed once and frozen."""
    c = {t["key"]: t for t in TABLE}[k]
    X = cie_rows(raster(k), c["n_images"], c["xs"], c["ys"], c["bw"], c["bh"])
    X.setflags(write=False)
    return X


def oracle_tile(rgb, n_images, xs, ys, bw, bh, cs):
    """oracle.tile image by image, concatenated: the values of colour space cs."""
    rgb = np.asarray(rgb, np.uint8).reshape(n_images, xs * ys * 3)
    return np.concatenate([oracle.tile(rgb[i], xs, ys, bw, bh, cs=cs, pad_code=PAD_CODE[cs])[0]
                           for i in range(n_images)])


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def rgb_bytes_of_cie(C):
    """Cie1931::colorSpaceToRGB (src/ColorSpace.cpp:35-47) restated over a codebook C [K, D]: per
    pixel triple the inverse linear map in the reference's order, std::round (half away from zero),
    the low byte of the integer."""
    P = np.ascontiguousarray(C, np.float64).reshape(-1, 3)
    x, y, z = P[:, 0], P[:, 1], P[:, 2]
    lin = np.stack([(x * 0.418 + y * (-0.15866)) + z * (-0.082835),
                    (x * (-0.091169) + y * 0.25243) + z * 0.015708,
                    (x * 0.0009209 + y * (-0.0025498)) + z * 0.17860], axis=1)
    t = np.trunc(lin)                                         # lin - t is exact
    rounded = t + np.where(np.abs(lin - t) >= 0.5, np.sign(lin), 0.0)
    return (rounded.astype(np.int64) & 0xFF).astype(np.uint8).reshape(np.shape(C))
