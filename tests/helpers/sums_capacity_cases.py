"""Training sets at which the exact sums' 16-bit register fields fill (tests/test_gpu_sums_capacity.py;
the claims below are checked on the CPU by tests/test_sums_capacity_cpu.py).

Three kernels add the exact terms (u = b ^ 0x80 <= 255, lo8[b] <= 128) of a lane's rows in packed
16-bit fields: mean_sums_kernel (capped by its launcher's grid), assign_small_kernel and
update_runs_kernel (a run is flushed after RUN_CAP = 256 rows).  A lane takes more than 256 rows only
past 256 * 1024 rows per CU: N_EDGE, just past 2^26 on 256 CUs.

Rows, in training-set order (row i, component d), as a function of i alone, so every set is a prefix
of one sequence and the same text builds it with numpy (slices, on the CPU) and torch (whole, on
the device):
  - the FIXED components are byte 0x7F (u = 255) in every row: whichever lane holds the most adds
    holds them all at the field's maximum;
  - the others are constant over bands of BAND = 2^20 rows, band t the palette's row t mod P: a
    wave's 64 * 260 consecutive rows lie in one band, so runs reach the cap;
  - one row in SPRINKLE = 1009 (i mod 1009 == 504) has pseudo-random bytes: runs break at
    unaligned places, the cap's flushes and the index change's interleave."""
import numpy as np

N_EDGE = (1 << 26) + 256 * 200 + 7    # 67 160 071: N mod 4 = 3, N mod 256 = 7 (one leftover group)
N_BELOW = (1 << 26) - 249             # the mean's grid cap binds, not its rows-per-block term
BAND = 1 << 20
SPRINKLE, SPRINKLE_AT = 1009, 504
P = 13                                # palette rows

# from the kernels' text (held to it by test_sums_capacity_cpu.py::test_constants_match_the_sources)
RUN_CAP = 256          # assign_small_kernel, update_runs_kernel: rows in a run before it is flushed
SMALL_WAVES = 16       # assign_small_kernel: waves per block, one block per CU
URUN_THREADS = 1024    # update_runs_kernel at Dp <= 32, one block per CU
URUN_ROWS = 4          # ... rows per lane and round at Dp <= 16
FIELD_ADDS = 257       # 255 * 257 = 65535


class Case:
    def __init__(self, name, dim, n, fixed):
        self.name, self.dim, self.n, self.fixed = name, dim, n, fixed


S12 = Case("S12", 12, N_EDGE, (0, 6))
S3 = Case("S3", 3, N_EDGE, (0,))
S12_BELOW = Case("S12-below", 12, N_BELOW, (0, 6))   # S12's first N_BELOW rows
CASES = {c.name: c for c in (S12, S3, S12_BELOW)}


def palette(dim, lo_byte):
    """uint8 [P, dim]: all-0x7F, all-0x80, all-lo_byte (the byte of the largest low term), then
    fixed pseudo-random rows."""
    pal = np.random.default_rng(1200 + dim).integers(0, 256, (P, dim)).astype(np.uint8)
    pal[0], pal[1], pal[2] = 0x7F, 0x80, lo_byte
    return pal


def lo_byte():
    """The byte whose low term is the largest (from the engine's own table)."""
    import quant_amd
    _, lo = quant_amd.host_row_terms(np.arange(256, dtype=np.uint8))
    return int(np.argmax(lo)), int(lo.max())


def is_sprinkled(i):
    return i % SPRINKLE == SPRINKLE_AT


def column(xp, i, d, pal_col, fixed, shift=20):
    """Component d of rows i (an int64 array of xp = numpy or torch; pal_col = the palette's column d
    as an int64 array of the same kind) -> int64 byte values.  shift: log2 of the band length (a
    scaled-down set for the CPU oracle takes shorter bands)."""
    if d in fixed:
        return xp.zeros_like(i) + 0x7F
    h = (i * 0x9E3779B1 + d * 0x85EBCA77) & 0xFFFFFFFF      # i < 2^27: no int64 overflow
    h = ((h ^ (h >> 15)) * 0x2C1B3C6D) & 0xFFFFFFFF
    h = ((h ^ (h >> 12)) >> 8) & 0xFF
    return xp.where(is_sprinkled(i), h, pal_col[(i >> shift) % P])


def rows_numpy(case, i0, i1, shift=20):
    """uint8 [i1 - i0, dim]: rows i0 .. i1 - 1 of the case."""
    pal = palette(case.dim, lo_byte()[0]).astype(np.int64)
    i = np.arange(i0, i1, dtype=np.int64)
    return np.stack([column(np, i, d, pal[:, d], case.fixed, shift) for d in range(case.dim)], axis=1).astype(np.uint8)


# ---- assignments for qvq_update: A(i) for K cells -------------------------------------------------
def assignment(xp, kind, i, K):
    """zero: every row in cell 0; band: band t in cell t mod K; band_own: band t in cell t mod (K - 1)
    and the sprinkled rows in cell K - 1 (K >= 2)."""
    if kind == "zero":
        return xp.zeros_like(i)
    if kind == "band":
        return (i >> 20) % K
    assert kind == "band_own" and K >= 2
    return xp.where(is_sprinkled(i), xp.zeros_like(i) + (K - 1), (i >> 20) % (K - 1))


UPDATE_CASES = [(1, "zero"), (2, "zero"), (2, "band"), (2, "band_own"), (5, "zero"), (5, "band"), (5, "band_own")]


# ---- what a device of `cus` compute units gives a lane ---------------------------------------------
def small_rows_per_lane(n, cus):
    """assign_small_kernel: a wave's lanes take every 64th row of its share, a multiple of 4 each."""
    lanes = cus * SMALL_WAVES * 64
    return (-(-n // lanes) + 3) // 4 * 4


def update_rows_per_lane(n, cus, rows=URUN_ROWS, threads=URUN_THREADS):
    """update_runs_kernel: lane 0 of wave 0 takes `rows` consecutive rows a round, rounds n_waves apart."""
    per_round = cus * threads * rows
    full, rest = divmod(n, per_round)
    return full * rows + min(rest, rows)
