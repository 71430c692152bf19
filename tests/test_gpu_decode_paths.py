"""Every decode kernel instantiation against the oracle: the cases of
tests/helpers/decode_cases.py -- held to the engine's dispatch by tests/test_decode_plan.py -- through
qvq_decode, qvq_decode_mse and qvq_decode_device, bit-exact against oracle.decode
(CompressedImage::decompress, reference src/Compressor.cpp:156-165 over :64-85).  Every case runs
with an identity-coded codebook (pixel p of code vector c holds the number c bw bh + p, so a wrong
writer, offset, index or word packing changes bytes) and with random bytes."""
import numpy as np
import pytest

import quant_amd
from helpers import decode_cases as dc
from oracle import oracle

pytestmark = pytest.mark.gpu

QVQ_EINVAL = 1
GUARD = 64
FILL = 0xA5


def _up(n):
    return (n + 63) & ~63


def device_decode(engine, cb, A, xs, ys, bw, bh, off_rgb=0, off_idx=0, off_cb=0):
    """qvq_decode_device inside one torch uint8 buffer of 0xA5: codebook | indices | 64 guard bytes,
    the raster, 64 guard bytes, each part from a 64-byte boundary plus its offset.  Returns the
    raster after checking that no other byte of the buffer changed."""
    import torch
    n = xs * ys * 3
    o_cb = off_cb
    o_idx = _up(o_cb + cb.size) + off_idx
    o_guard = _up(o_idx + 4 * A.size)
    o_out = o_guard + GUARD + off_rgb
    host = np.full(o_out + n + GUARD, FILL, np.uint8)
    host[o_cb:o_cb + cb.size] = cb.ravel()
    host[o_idx:o_idx + 4 * A.size] = A.view(np.uint8)
    d = torch.from_numpy(host).cuda()
    base = d.data_ptr()
    assert base % 64 == 0
    flags = (((base + o_out) % 8 != 0) * dc.RASTER_UNALIGNED | ((base + o_idx) % 16 != 0) * dc.INDEX_UNALIGNED |
             ((base + o_cb) % 2 != 0) * dc.CODEBOOK_ODD)
    engine.decode_device(base + o_cb, cb.shape[0], base + o_idx, A.size, xs, ys, bw, bh, base + o_out,
                         torch.cuda.current_stream().cuda_stream)
    back = d.cpu().numpy()
    assert np.array_equal(back[:o_out], host[:o_out]), "bytes before the raster changed"
    assert (back[o_out + n:] == FILL).all(), "bytes after the raster changed"
    return back[o_out:o_out + n], flags


def first_diff(got, want):
    bad = np.flatnonzero(got != want)
    return "" if not len(bad) else "%d bytes differ, the first at byte %d (pixel %d): got %d, want %d" % (
        len(bad), bad[0], bad[0] // 3, got[bad[0]], want[bad[0]])


CASE_KINDS = [pytest.param(c, k, id="%s-%s" % (c["key"], k)) for c in dc.TABLE for k in dc.KINDS]


@pytest.mark.parametrize("case,kind", CASE_KINDS)
def test_table_host(engine, case, kind):
    cb, A = dc.inputs(case, kind)
    got = engine.decode(cb, A, *dc.shape(case))
    assert np.array_equal(got, dc.oracle_decode(case, kind)), first_diff(got, dc.oracle_decode(case, kind))


@pytest.mark.parametrize("case,kind", CASE_KINDS)
def test_table_device(engine, case, kind):
    cb, A = dc.inputs(case, kind)
    got, flags = device_decode(engine, cb, A, *dc.shape(case))
    assert flags == 0
    assert np.array_equal(got, dc.oracle_decode(case, kind)), first_diff(got, dc.oracle_decode(case, kind))


@pytest.mark.parametrize("bw", list(dc.SWEEP_BW))
def test_sweep(engine, bw):
    """xs 1..9 x ys 1..17 x bh 1..9 at this block width: identity-coded through both entry points,
    random bytes through qvq_decode_mse."""
    bad = []
    for xs, ys, _, bh in dc.sweep_shapes(bw):
        seed = ((xs * 32 + ys) * 8 + bw) * 16 + bh
        cb, A = dc.build(xs, ys, bw, bh, dc.SWEEP_K, "identity", seed)
        want = oracle.decode(cb, A, xs, ys, bw, bh).ravel()
        for how, got in (("host", engine.decode(cb, A, xs, ys, bw, bh)),
                         ("device", device_decode(engine, cb, A, xs, ys, bw, bh)[0])):
            if not np.array_equal(got, want):
                bad.append("%dx%d %dx%d %s identity: %s" % (xs, ys, bw, bh, how, first_diff(got, want)))
        cb, A = dc.build(xs, ys, bw, bh, dc.SWEEP_K, "random", seed)
        orig = np.random.default_rng(seed).integers(0, 256, size=xs * ys * 3, dtype=np.uint8)
        want = oracle.decode(cb, A, xs, ys, bw, bh).ravel()
        got, mse = engine.decode_mse(cb, A, xs, ys, bw, bh, orig)
        if not np.array_equal(got, want) or mse != oracle.raport_distortion(orig, want):
            bad.append("%dx%d %dx%d random: %s, mse %r" % (xs, ys, bw, bh, first_diff(got, want), mse))
    assert not bad, "%d of the sweep's decodes differ:\n%s" % (len(bad), "\n".join(bad[:20]))


@pytest.mark.parametrize("ac", dc.ALIGN_CASES, ids=dc.key)
def test_unaligned_device_pointers(engine, ac):
    case = next(c for c in dc.TABLE if c["key"] == ac["base"])
    cb, A = dc.inputs(case, "identity")
    got, flags = device_decode(engine, cb, A, *dc.shape(case), off_rgb=ac["off_rgb"], off_idx=ac["off_idx"],
                               off_cb=ac["off_cb"])
    assert flags == ac["flags"]
    assert dc.instantiation(quant_amd.host_decode_plan(case["K"], *dc.shape(case), flags)) == ac["inst"]
    assert np.array_equal(got, dc.oracle_decode(case, "identity")), first_diff(got, dc.oracle_decode(case, "identity"))


def test_index_pointer_off_by_two_is_refused(engine):
    case = next(c for c in dc.TABLE if c["key"] == "rowsh-H4-lds-coal-ys512")
    cb, A = dc.inputs(case, "identity")
    with pytest.raises(quant_amd.QVQError) as e:
        device_decode(engine, cb, A, *dc.shape(case), off_idx=2)
    assert e.value.status == QVQ_EINVAL


@pytest.mark.parametrize("case", dc.first_per_instantiation(), ids=dc.key)
def test_mse(engine, case):
    """qvq_decode_mse on every instantiation: an integer sum over a count, so exact."""
    cb, A = dc.inputs(case, "random")
    orig, want = dc.original(case), dc.oracle_decode(case, "random")
    img, mse = engine.decode_mse(cb, A, *dc.shape(case), orig)
    assert np.array_equal(img, want), first_diff(img, want)
    assert mse == oracle.raport_distortion(orig, want)
    none, mse2 = engine.decode_mse(cb, A, *dc.shape(case), orig, want_image=False)
    assert none is None and mse2 == mse


def test_mse_sum_past_32_bits(engine):
    """Every byte differs by 255 (0x80 = -128 against 0x7F = 127) on the 8200 x 512 cap shape: the
    sum is 12.6 M x 65025, about 8.2e11."""
    case = next(c for c in dc.CAP_CASES if c["key"] == "cap-rowsh-coal")
    xs, ys, bw, bh = dc.shape(case)
    _, A = dc.inputs(case, "random")
    cb = np.full((case["K"], bw * bh * 3), 0x80, np.uint8)
    orig = np.full(xs * ys * 3, 0x7F, np.uint8)
    assert xs * ys * 3 * 65025 > 1 << 32
    img, mse = engine.decode_mse(cb, A, xs, ys, bw, bh, orig)
    assert (img == 0x80).all()
    assert mse == 65025.0


BAD_INDEX_CASES = ["rowsh-H4-lds-coal-ys512", "rowsh-H2-lds-direct-ys520", "rowsh-H1-lds-direct-ys8", "rowsh-edge-K1025",
                   "rowsh-H8-glb-direct-ys520", "rows-ys16-h5-w3", "rows-glb-K513", "pixels-overhang"]


@pytest.mark.parametrize("name", BAD_INDEX_CASES)
def test_bad_index(engine, name):
    """An index equal to K, and 0xFFFFFFFF, at the first, a middle and the last block: QVQ_EINVAL
    from both entry points, and the next valid decode on the same context is right again (the flag
    and the error sum start from zero)."""
    case = next(c for c in dc.TABLE if c["key"] == name)
    cb, A = dc.inputs(case, "random")
    orig, want = dc.original(case), dc.oracle_decode(case, "random")
    for value in (case["K"], 0xFFFFFFFF):
        for at in (0, len(A) // 2, len(A) - 1):
            A2 = A.copy()
            A2[at] = value
            with pytest.raises(quant_amd.QVQError) as e:
                engine.decode_mse(cb, A2, *dc.shape(case), orig)
            assert e.value.status == QVQ_EINVAL, (value, at)
            with pytest.raises(quant_amd.QVQError) as e:
                device_decode(engine, cb, A2, *dc.shape(case))
            assert e.value.status == QVQ_EINVAL, (value, at)
            img, mse = engine.decode_mse(cb, A, *dc.shape(case), orig)
            assert np.array_equal(img, want) and mse == oracle.raport_distortion(orig, want), (value, at)
