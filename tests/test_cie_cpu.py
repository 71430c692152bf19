"""CIE1931 rasters, the CPU side: the one statement of the colour map
(quant_amd/csrc/cie1931.hpp, through qvq_host_cie1931) against the numpy restatement over every
colour; the helper's tiling restatement against the oracle's; and the case table of
tests/helpers/cie_cases.py held to the kernel's launch shape and to its own coverage claims.
Every comparison is bit for bit."""
import numpy as np
import pytest

import quant_amd
from helpers import cie_cases as cc


def test_case_table_matches_the_kernels_launch_shape():
    g = quant_amd.host_tile64_grid()
    assert (g["block"], g["blocks"]) == (cc.BLOCK, cc.BLOCKS)


def test_host_map_equals_the_restatement_on_every_colour():
    """All 2^24 (r, g, b), 2^16 at a time: the bits of the library's map are numpy's, and no output
    is -0.0 (r * 0 is -0.0 for a negative r; the sum with g * 0.01 takes the sign away)."""
    rgb = cc.all_colours()
    neg_zero = np.float64(-0.0).view(np.int64)
    step = 1 << 16
    for at in range(0, 1 << 24, step):
        part = rgb[at:at + step]
        got = quant_amd.host_cie1931(part)
        want = cc.cie_map(part.view(np.int8).astype(np.float64))
        assert np.array_equal(cc.bits(got), cc.bits(want)), "colours %d..%d" % (at, at + step)
        assert not np.any(cc.bits(got) == neg_zero)
    assert np.array_equal(cc.bits(quant_amd.host_cie1931(np.zeros((1, 3), np.uint8))), np.zeros((1, 3), np.int64))


@pytest.mark.parametrize("c", cc.GEOMETRY_CASES + [cc.STRIDE_CASE], ids=cc.key)
def test_tiling_restatement_equals_the_oracle(c):
    """tile_signed is oracle.tile under NORMAL (signed-byte values, entries past the buffer 0.0),
    image by image."""
    rgb = cc.raster(c["key"])
    got = cc.tile_signed(rgb, c["n_images"], c["xs"], c["ys"], c["bw"], c["bh"])
    want = cc.oracle_tile(rgb, c["n_images"], c["xs"], c["ys"], c["bw"], c["bh"], cc.NORMAL)
    assert got.shape == (cc.rows(c), 3 * c["bw"] * c["bh"])
    assert np.array_equal(cc.bits(got), cc.bits(want))


def test_case_table_covers_what_it_claims():
    geo = cc.GEOMETRY_CASES
    assert {(c["xs"], c["ys"], c["bw"], c["bh"]) for c in geo} == set(cc.GEOMETRIES)
    assert all({c["n_images"] for c in geo if (c["xs"], c["ys"], c["bw"], c["bh"]) == g} == {1, 3}
               for g in cc.GEOMETRIES)
    # a column past ySize that reads the next raster row
    assert any(cc.wraps(c) for c in geo)
    # several raster rows crossed by one block (bh = 7 over ySize = 3), at D = 21
    assert any(c["bh"] > 2 * c["ys"] and 3 * c["bw"] * c["bh"] == 21 for c in geo)
    assert any(3 * c["bw"] * c["bh"] == 48 for c in geo)
    # pixels past the buffer.  A *whole* block cannot lie past it while the buffer holds xSize *
    # ySize pixels: block (i, j)'s first pixel is entry i * bw * ySize + j * bh with i * bw <= xSize - 1
    # and j * bh <= ySize - 1, which is inside.  The most a block can lose is all but that pixel
    # (1 x 1 raster, 2 x 2 blocks); whole pixel rows of a block past the buffer come with it.
    for c in cc.TABLE:
        assert np.all(cc.padded_per_block(c) < c["bw"] * c["bh"])
    assert any(np.max(cc.padded_per_block(c)) == c["bw"] * c["bh"] - 1 and c["bw"] * c["bh"] > 1 for c in geo)
    # the last block of image i padded while image i + 1 follows
    assert any(c["n_images"] > 1 and cc.padded_per_block(c)[-1] > 0 for c in geo)
    assert cc.STRIDE_CASE["n_images"] > 1 and cc.padded_per_block(cc.STRIDE_CASE)[-1] > 0
    # more slots than one trip of the grid-stride loop: every colour at 1 x 1, and a 5 x 3 shape whose
    # stride has a nonzero digit in every radix (dy, dx, j, i) so that each carry is taken
    assert cc.slots(cc.EVERY_CASE) == 1 << 24 > cc.BLOCK * cc.BLOCKS
    assert cc.BLOCK * cc.BLOCKS < cc.slots(cc.STRIDE_CASE) < 2 * cc.BLOCK * cc.BLOCKS
    s, digits = cc.BLOCK * cc.BLOCKS, []
    wB, hB = cc.blocks(cc.STRIDE_CASE)
    for radix in (cc.STRIDE_CASE["bh"], cc.STRIDE_CASE["bw"], hB, wB):
        digits.append(s % radix)
        s //= radix
    assert all(d > 0 for d in digits), digits
    assert cc.slots(cc.EVERY_SMALL) < cc.BLOCK * cc.BLOCKS
    # every raster has bytes on both sides of the sign
    for c in geo + [cc.STRIDE_CASE]:
        r = cc.raster(c["key"])
        assert c["xs"] * c["ys"] * c["n_images"] < 4 or (r.min() < 128 <= r.max())


def test_inverse_map_restatement_rounds_half_away_from_zero():
    """rgb_bytes_of_cie's rounding is std::round's and its byte the integer's low byte."""
    # X = v / 0.418 alone gives r ~ v; checked on values whose products are exact halves
    C = np.array([[0.0, 0.0, 2.5 / 0.17860], [0.0, 0.0, -2.5 / 0.17860], [0.0, 0.0, 300.0 / 0.17860]])
    lin = C[:, 2] * 0.17860
    want = [int(np.copysign(np.floor(abs(v) + 0.5), v)) & 0xFF for v in lin]
    assert list(cc.rgb_bytes_of_cie(C)[:, 2]) == want
