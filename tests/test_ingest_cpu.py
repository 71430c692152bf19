"""The value -> code rule of the fp64 front door on the host (qvq_host_classify and
qvq_host_colorspace_values: quant_amd/csrc/byte_image.hpp, the function the device pass of
k_ingest.hip applies), against the oracle's table and a numpy restatement.  No GPU."""
import numpy as np
import pytest

import quant_amd
from helpers import ingest_cases as ic
from oracle import oracle

NORMAL, SCALED = quant_amd.NORMAL, quant_amd.SCALED


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def _cs(X):
    return quant_amd.host_classify(np.asarray(X, np.float64).reshape(len(X), -1))[0]


@pytest.mark.parametrize("cs", ic.SPACES)
def test_colorspace_values_are_the_oracles_table(cs):
    np.testing.assert_array_equal(_bits(quant_amd.colorspace_values(cs)), _bits(oracle.lut(cs)))


def test_case_tables_match_the_engine():
    g = quant_amd.host_ingest_grid()
    assert (g["block"], g["blocks"]) == (ic.BLOCK, ic.BLOCKS)
    for cs in ic.SPACES:
        assert oracle.lut(cs)[ic.PAD_CODE[cs]] == 0.0 and not np.signbit(oracle.lut(cs)[ic.PAD_CODE[cs]])


@pytest.mark.parametrize("cs", ic.SPACES)
def test_every_byte_classifies_to_its_own_code(cs):
    t = oracle.lut(cs)
    b = np.arange(256, dtype=np.uint8)
    # one byte per row; 0.0 and 1.0 are images under both spaces, and SCALED is asked first
    for code in b:
        got_cs, codes = quant_amd.host_classify(t[[code]].reshape(1, 1))
        both = cs == NORMAL and t[code] in (0.0, 1.0)
        assert got_cs == (SCALED if both else cs), code
        want = code if not both else np.flatnonzero(_bits(oracle.lut(SCALED)) == _bits(t[[code]]))[0]
        assert codes[0, 0] == want, code
    # all 256 at once: a column, and a 4 x 64 block
    for shape in ((256, 1), (4, 64)):
        got_cs, codes = quant_amd.host_classify(t[b].reshape(shape))
        assert got_cs == cs
        np.testing.assert_array_equal(codes[:, :shape[1]], b.reshape(shape))


@pytest.mark.parametrize("cs", ic.SPACES)
def test_neighbours_of_table_values_are_rejected(cs):
    t = oracle.lut(cs)
    for v in np.concatenate([np.nextafter(t, np.inf), np.nextafter(t, -np.inf)]):
        assert _cs([[v]]) == -1, repr(v)


@pytest.mark.parametrize("v", [-0.0, np.nan, np.inf, -np.inf, 5e-324, 128.0, -129.0, 0.5], ids=repr)
def test_values_that_are_no_byte_images(v):
    assert _cs([[v]]) == -1
    # ... and among images of either space
    assert _cs([[0.0, 1.0, v]]) == -1
    assert _cs([[v], [1.0], [0.0]]) == -1


def test_the_shared_values_and_the_selection_order():
    rng = np.random.default_rng(3)
    X = rng.integers(0, 2, size=(40, 5)).astype(np.float64)
    cs, codes = quant_amd.host_classify(X)
    assert cs == SCALED
    want = np.where(X == 0.0, 0x80, 0x7F).astype(np.uint8)      # u = 0 and u = 255, code u ^ 0x80
    np.testing.assert_array_equal(codes, ic.padded(want, SCALED))
    X[-1, -1] = 5.0                                             # SCALED-valid up to its last element
    cs, codes = quant_amd.host_classify(X)
    assert cs == NORMAL
    np.testing.assert_array_equal(codes, ic.padded(X.astype(np.int8).view(np.uint8), NORMAL))
    X[0, 0] = oracle.lut(SCALED)[0x81]                          # fl(1 * fl(1/255)): SCALED only
    assert X[0, 0] == 1.0 * (1.0 / 255)
    assert quant_amd.host_classify(X) == (-1, None)


def test_division_is_not_the_table():
    """The trap qvq.h warns of: u / 255.0 differs from the table for 24 bytes, so a row built by
    division is no byte image."""
    t = oracle.lut(SCALED)
    u = np.arange(256)
    div = u / 255.0
    off = np.flatnonzero(div != t[u ^ 0x80])
    assert len(off) == 24 and list(off[:3]) == [33, 37, 41]
    assert _cs(div.reshape(-1, 1)) == -1
    assert _cs(np.delete(div, off).reshape(-1, 1)) == SCALED


@pytest.mark.parametrize("n", (1, 7, 1000))
def test_codes_equal_the_numpy_restatement(n):
    for cs in ic.SPACES:
        for D in range(1, 65):
            X, codes = ic.rows(cs, n, D, 9000 + 64 * n + D + cs)
            want_cs, want = ic.np_classify(X)
            got_cs, got = quant_amd.host_classify(X)
            # (a set of 0.0 and 1.0 only would be SCALED under either table; these are not)
            assert got_cs == want_cs == (cs if n * D > 8 else got_cs), (cs, D)
            np.testing.assert_array_equal(got, want)
            if got_cs == cs:
                np.testing.assert_array_equal(got, ic.padded(codes, cs))


def test_host_classify_rejects_bad_arguments():
    L = quant_amd.lib()
    import ctypes
    X = np.zeros((1, 65))
    cs = ctypes.c_int32()
    assert L.qvq_host_classify(X.ctypes.data_as(ctypes.c_void_p), 1, 65, ctypes.byref(cs), None) == 1
    assert L.qvq_host_classify(X.ctypes.data_as(ctypes.c_void_p), 0, 3, ctypes.byref(cs), None) == 1
    assert L.qvq_host_classify(None, 1, 3, ctypes.byref(cs), None) == 1
    assert L.qvq_host_colorspace_values(quant_amd.CIE1931, X.ctypes.data_as(ctypes.c_void_p)) == 5

