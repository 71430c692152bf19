"""The cases of tests/test_gpu_chunk_loop.py: row counts around the points where a wave's sequence of
chunks begins and ends in the D = 12 MFMA search (assign_mf32_kernel, k_mf32.hip).  Plain data and
arithmetic; nothing here loads the engine.

The search grid is one workgroup of 16 waves per CU.  With G CUs there are W = 16 G waves, a chunk is
64 consecutive rows, and chunk c is slot c div W of workgroup (c mod W) div 16: its wave (c mod W) mod
16 starts on it when c < W, and past that whichever wave of the workgroup claims the slot next.  A
wave prefetches its next chunk's rows and claims the slot after it a chunk ahead, so what can go
wrong sits where a sequence of chunks begins and ends: a wave with no chunk must do nothing (its
claim and its prefetch land past the end), a workgroup with exactly one chunk per wave has nothing
to claim, a single further slot goes to one wave only, and a ragged last chunk stores and sums only
its rows below N.

tests/test_chunk_loop_cases.py holds row_counts() to the patterns named here for several G."""
import numpy as np

WAVES_PER_CU = 16   # k_mf32.hip M32_WAVES
CHUNK_ROWS = 64     # k_mf32.hip M32_ROWS

# name -> N as a function of W, in the order the tests run them
CASES = (
    ("two_chunks", lambda W: 65),                  # two chunks, the second a single row; every other wave idle
    ("one_each_ragged", lambda W: 64 * W - 1),     # every wave exactly one chunk (no slot to claim), the last one 63 rows
    ("one_extra_row", lambda W: 64 * W + 1),       # one workgroup has a 17th slot, and it is a single row
    ("two_each_plus", lambda W: 128 * W + 63),     # 32 slots everywhere, a 33rd of 63 rows in one workgroup
)
NAMES = tuple(name for name, _ in CASES)
LARGE = NAMES[1:]                 # the cases whose lbg(10) runs every fused instantiation
NORMAL_CASE = "two_each_plus"     # also run in the NORMAL colour space
UNFUSED_CASE = "one_extra_row"    # qvq_assign (the unfused instantiations) runs here
UNFUSED_KS = (64, 256, 1024)      # 4-code-vector units; pruned with the fp32 table in LDS; pruned, table in HBM


def waves(G):
    return WAVES_PER_CU * G


def row_counts(G):
    """{case name: N} on a part with G CUs."""
    return {name: f(waves(G)) for name, f in CASES}


def pattern(N, G):
    """How N rows fall on the waves of G CUs when chunk c runs on wave c mod W (the waves' first
    chunks; an even hand-out of the claimed slots): the number of chunks, how many waves run 0, 1,
    2, ... chunks, the rows of the last chunk and the wave that runs it, and that wave's chunk count."""
    W = waves(G)
    nchunks = (N + CHUNK_ROWS - 1) // CHUNK_ROWS
    per_wave = np.bincount(np.arange(nchunks) % W, minlength=W)
    last_wave = (nchunks - 1) % W
    hist = {int(k): int(v) for k, v in zip(*np.unique(per_wave, return_counts=True))}
    return {"nchunks": int(nchunks), "waves_by_chunks": hist, "last_rows": int(N - (nchunks - 1) * CHUNK_ROWS),
            "last_wave": int(last_wave), "last_wave_chunks": int(per_wave[last_wave])}
