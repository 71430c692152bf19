"""The cases of tests/test_gpu_search_epilogue.py: the D = 12 MFMA search's recompute of the winning
unit where the unit holds padding positions (codebooks that end inside a tile), and its list of
flagged rows (a workgroup's rows in LDS, past its end the global list).  Plain data and seeded,
pure-numpy input builders; nothing here loads the engine, except the recorder at the end.

A search workgroup takes 1024 consecutive rows (16 waves x 64-row chunks) on training sets of up to
256 workgroups' rows, and keeps at most FLAG_CAP flagged rows in LDS.

The recorder (python tests/helpers/search_epilogue_cases.py OUT_DIR, with QVQ_LIB naming the build)
writes tests/golden/search_epilogue_parent.json and search_epilogue_parent_codebook.npy: what one
build returns for the cases -- flagged rows per qvq_assign, and the short qvq_lbg's codebook,
distortion and flagged rows per level.  The committed fixture was recorded with the build before the
LDS list (commit 7838b39), which every later build must reproduce bit for bit."""
import functools
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
if os.path.join(ROOT, "tests") not in sys.path:
    sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle import oracle  # noqa: E402
from helpers import largek_cases as lk  # noqa: E402
from helpers import neartie_cases as nt  # noqa: E402

GOLDEN_JSON = os.path.join(ROOT, "tests", "golden", "search_epilogue_parent.json")
GOLDEN_CODEBOOK = os.path.join(ROOT, "tests", "golden", "search_epilogue_parent_codebook.npy")

COLOUR = nt.COLOUR
KS = (64, 70, 128, 256, 300, 512, 1000, 1024)   # 70, 300, 1000: padding positions in the last tile
N_ROWS = 4096 + 37                              # a ragged last chunk
WG_ROWS = 1024                                  # rows of one search workgroup
FLAG_CAP = 384                                  # k_mf32.hip M32_FLAG_CAP: the most a workgroup lists
# K with padding in the last tile, by what the last tile's units hold.  1601: past the LDS capacity
# of the fp32 table (c32_staged 0), the recompute from the code-ordered table in HBM.
LAST_KS = (70, 300, 1000, 1601)    # some unit is partly padded
ONE_KS = (65, 257, 993, 1601)      # K = 1 mod 32: the last tile's first unit holds one real code vector
FLAG_KS = (64, 1024)
LBG_SIDE, LBG_BITS = 128, 10


@functools.lru_cache(maxsize=None)
def image_rows(cs, n=N_ROWS):
    """The first n 2 x 2 blocks of the 256 x 256 synthetic image, as values of colour space cs."""
    c = COLOUR[cs]
    X, _ = oracle.tile(oracle.gen_image(256), 256, 256, 2, 2, cs=c, pad_code=128 if c == oracle.SCALED else 0)
    X = np.ascontiguousarray(X[:n])
    X.setflags(write=False)
    return X


def unit_size(K):
    return 4 if K <= 128 else 8    # launch_assign_mf32: 4-code-vector units up to K = 128


def last_tile_units(K):
    """The last tile's units as lists of tile positions (k_mf32.hip: 8-unit q, half hh holds tile rows
    16 q + 4 hh + {0..3, 8..11}, 4-unit q rows 8 q + 4 hh + {0..3}).  Unpruned: position = index."""
    base = (K + 31) // 32 * 32 - 32
    if unit_size(K) == 8:
        return [[base + 16 * q + 4 * hh + o for o in (0, 1, 2, 3, 8, 9, 10, 11)] for q in range(2) for hh in range(2)]
    return [[base + 8 * q + 4 * hh + o for o in range(4)] for q in range(4) for hh in range(2)]


def _plant(X, C, targets, seed, near):
    """Rows on code vectors: code vector p of targets becomes a data row's value, and a block of rows
    takes that value (near: every other one of them with one byte moved by one step of the table)."""
    rng = np.random.default_rng(seed)
    X, C = X.copy(), C.copy()
    picks = rng.choice(len(X) // 128, len(targets), replace=False)
    for p, b in zip(targets, picks):
        x = X[128 * b + 127].copy()
        C[p] = x
        X[128 * b:128 * b + 100] = x      # crosses a chunk boundary
        if near:
            X[128 * b + 1:128 * b + 100:2, 5] = X[128 * b + 126, 5]   # another table value in one component
    return np.ascontiguousarray(X), np.ascontiguousarray(C)


@functools.lru_cache(maxsize=None)
def assign_case(key):
    """(rows X, codebook C) of a qvq_assign case, read-only.  Keys:
    idx-K<K>-<cs>    the image rows against lk.codebook (split pairs, zero vectors, duplicates)
    last-K<K>-<cs>   blocks of rows lying exactly on the last real code vector of every partly padded unit
    one-K<K>-<cs>    blocks of rows on and next to the one real code vector of the last tile's first unit
    flat-K<K>-<cs>   every row a near tie: a flat half (one row of an exactly tied pair, repeated) and
                     the near-tie helper's anchor rows with gaps under 1e-9 relative
    noise-K<K>-<cs>  uniform noise rows against noise code vectors, K / 32 of them in pairs 1e-12 apart:
                     the rows nearest to a pair are flagged, a few hundred in all"""
    kind, k, cs = key.split("-")
    K = int(k[1:])
    if kind in ("idx", "last", "one"):
        X = image_rows(cs)
        C = lk.codebook(X, K, seed=K)
        if kind == "last":
            units = [[p for p in u if p < K] for u in last_tile_units(K)]
            targets = [u[-1] for u in units if 0 < len(u) < unit_size(K)]
            assert targets
            X, C = _plant(X, C, targets, seed=K + 1, near=False)
        elif kind == "one":
            assert K % 32 == 1
            X, C = _plant(X, C, [K - 1], seed=K + 2, near=True)
    elif kind == "flat":
        Xn, C = nt.build(12, K, COLOUR[cs], "near", seed=77 + K)
        gap = nt.rel_gap(Xn, C)
        tight = np.unique(Xn[gap < 1e-9], axis=0)   # anchor rows with tiny gaps
        assert len(tight) >= 4
        exact = Xn[np.argmin(gap)]
        n = 4 * WG_ROWS + 512
        X = np.concatenate([np.tile(exact, (n // 2, 1)), tight[np.arange(n - n // 2) % len(tight)]])
        X = np.ascontiguousarray(X[np.random.default_rng(K).permutation(n)])
    elif kind == "noise":
        rng = np.random.default_rng(1000 + K)
        X = np.ascontiguousarray(oracle.lut(COLOUR[cs])[rng.integers(0, 256, (N_ROWS, 12)).astype(np.uint8)])
        C = oracle.lut(COLOUR[cs])[rng.integers(0, 256, (K, 12)).astype(np.uint8)]
        C[1:K // 16:2] = C[0:K // 16:2] * (1 + 1e-12)   # K / 32 near pairs: the rows nearest to them are flagged
        C = np.ascontiguousarray(C)
    else:
        raise KeyError(key)
    X.setflags(write=False)
    C.setflags(write=False)
    return X, C


def assign_keys():
    keys = ["idx-K%d-%s" % (K, cs) for K in KS for cs in COLOUR]
    keys += ["last-K%d-%s" % (K, cs) for K in LAST_KS for cs in COLOUR]
    keys += ["one-K%d-%s" % (K, cs) for K in ONE_KS for cs in COLOUR]
    keys += ["%s-K%d-scaled" % (kind, K) for kind in ("flat", "noise") for K in FLAG_KS]
    return keys


def refine_start(X, K, cs, seed):
    """A legal qvq_refine start of K code vectors: lk.codebook cut to the colour space's range."""
    lut = oracle.lut(COLOUR[cs])
    return np.ascontiguousarray(np.clip(lk.codebook(X, K, seed), lut.min(), lut.max()))


def golden():
    with open(GOLDEN_JSON) as f:
        g = json.load(f)
    return g, np.load(GOLDEN_CODEBOOK)


def record(out_dir):
    """What the build named by QVQ_LIB returns for the cases (needs the GPU)."""
    import quant_amd
    rec = {"lib": os.path.basename(os.path.dirname(quant_amd.LIB_PATH)), "assign_flagged": {}}
    with quant_amd.Engine(0) as eng:
        for key in assign_keys():
            X, C = assign_case(key)
            eng.set_vectors(X)
            eng.assign(C)
            rec["assign_flagged"][key] = int(eng.timings()["flagged"][0])
        eng.set_images(oracle.gen_image(LBG_SIDE), 1, LBG_SIDE, LBG_SIDE, 2, 2, quant_amd.SCALED)
        C, _, d = eng.lbg(LBG_BITS)
        rec["lbg_distortion_hex"] = float(d).hex()
        rec["lbg_flagged"] = [int(v) for v in eng.timings()["flagged"]]
    os.makedirs(out_dir, exist_ok=True)
    np.save(os.path.join(out_dir, os.path.basename(GOLDEN_CODEBOOK)), C)
    with open(os.path.join(out_dir, os.path.basename(GOLDEN_JSON)), "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    record(sys.argv[1])
