"""The cases of tests/test_gpu_recheck_mf32.py: D = 12 codebooks of K >= 512 code vectors whose flagged
rows put recheck_mf32_kernel (quant_amd/csrc/k_mf32.hip) at the edges of its tile sweep, its hit
masks, its per-lane candidate lists and its row groups.  Plain data and seeded, pure-numpy builders;
nothing here loads the engine.  tests/test_recheck_mf32_cases.py holds the builders to what they
promise, on the CPU.

The kernel: a wave takes 32 flagged rows through every 32-code-vector tile, two tiles per step; a
lane holds its row's 16 scores of a tile at the positions (v & 3) + 8 (v >> 2) + 4 h, h the lane's
half (bit 2 of the code vector's index), and lists the ones inside the row's band, up to RC_CAP per
lane; a row whose lane overflowed scans all K.  Row groups go round the workgroups first
(group = workgroup + grid * wave), the grid being one workgroup per CU.

Values: a byte b stands for u = b ^ 0x80 in 0 ... 255 and the value lut[b] = v0 + u step, in both
colour spaces.  Code vectors and rows are written in u units below; u need not be an integer for a
code vector.

A codebook (build_codebook) holds these sites, each an anchor row x of integer u in 64 ... 191 with
the code vectors around it, and random integer code vectors ("background") everywhere else, none of
them nearer to a site's rows than 3 times the site's own code vectors (checked on the CPU):

  pair:*    a = x + s, b = x - s with s_0 = NEAR and |s_d| in 3 ... 9 elsewhere; the rows x + e_0 and
            x - e_0, one byte step off the midpoint: their distances to a and b differ by 4 NEAR
            u^2 (0.2: under the search's per-row MFMA bound, which is above 0.6 u^2 for any row, and
            ~5e-4 of the distances, so flagged and never a tie), and the midpoint x itself, an exact
            tie in NORMAL and one within rounding in SCALED.
            pair:tile     both in one tile and one half
            pair:ends     in the first and in the last tile
            pair:halves   in one tile, index bit 2 clear and set
            pair:last     both in the last tile (K = 544: the tile the last step repeats; K = 1000:
                          the tile with padding positions)
  cap:N:*   N = 16, 17, 40 code vectors x + (signs) v, every one at the same distance from the row x
            (equal squares in the same order: bit-equal in NORMAL, within rounding in SCALED)
            cap:N:half    all at indices with bit 2 clear: 16 fill one lane's list exactly from one
                          tile (sixteen mask bits), 17 and 40 overflow it (the all-K scan)
            cap:N:both    split over both halves of as few tiles as hold them
            cap:N:tiles   one per tile and half in turn over 16 tiles
  on        the row is the code vector a itself, b = a + ON_STEP e_0: scores near -|x - mu|^2
            scaled, where the band's |m| term is largest
"""
import functools
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from oracle import oracle  # noqa: E402

D = 12
KS = (512, 544, 1000, 1024)
COLOUR = {"scaled": oracle.SCALED, "normal": oracle.NORMAL}
RC_CAP = 16          # k_mf32.hip
WAVES = 16           # waves per workgroup (M32_WAVES)
NEAR = 0.05          # u: half the distance of a pair's code vectors along component 0
ON_STEP = 0.25       # u
CAPS = (16, 17, 40)
CAP_LAYOUTS = ("half", "both", "tiles")
BACKGROUND_ROWS = 300
CLEAR = 3.0          # background code vectors are at least this many times farther (distance, not squared)


def tiles(K):
    return (K + 31) // 32


def affine(cs):
    """(v0, step): lut[b] == v0 + (b ^ 0x80) * step for every byte b (asserted)."""
    lut = oracle.lut(COLOUR[cs])
    v0, step = lut[0x80], lut[0x81] - lut[0x80]
    u = np.arange(256)
    assert np.array_equal(lut[u ^ 0x80], v0 + u * step)
    return v0, step


def values(cs, U):
    """fp64 values of u-unit vectors: straight from the lut where u is an integer (rows must be)."""
    v0, step = affine(cs)
    return v0 + np.asarray(U, np.float64) * step


class _Free:
    """Code vector indices not yet taken, handed out by tile and half."""

    def __init__(self, K):
        self.K = K
        self.free = np.ones(K, bool)

    def take(self, idx):
        assert 0 <= idx < self.K and self.free[idx], idx
        self.free[idx] = False
        return idx

    def first(self, tile, half):
        for p in range(32):
            i = tile * 32 + p
            if i < self.K and self.free[i] and ((p >> 2) & 1) == half:
                return self.take(i)
        raise AssertionError("tile %d half %d is full" % (tile, half))

    def room(self, tile, half):
        return sum(1 for p in range(32) if tile * 32 + p < self.K and self.free[tile * 32 + p] and ((p >> 2) & 1) == half)


def _cap_indices(fr, n, layout, t0):
    """Indices of a cap site's n code vectors from tile t0 on (see the module docstring)."""
    out = []
    if layout == "tiles":
        T = tiles(fr.K)
        open_tiles = [t for t in range(T) if fr.room(t, 0) + fr.room(t, 1) >= 3]
        sel = open_tiles[::max(1, len(open_tiles) // 16)][:16]
        for j in range(n):
            t, h = sel[j % len(sel)], (j // len(sel) + j) & 1
            out.append(fr.first(t, h if fr.room(t, h) else 1 - h))
        return out
    t = t0
    halves = (0,) if layout == "half" else (0, 1)
    while len(out) < n:
        took = False
        for h in halves:
            if len(out) < n and fr.room(t, h):
                out.append(fr.first(t, h))
                took = True
        if not took:
            t += 1
    return out


def site_reach(U, site):
    """The largest distance (u) from a row of the site to one of its code vectors, at least 10."""
    d = np.sqrt(((site["rows"][:, None, :] - U[site["idx"]][None]) ** 2).sum(axis=2))
    return max(10.0, float(d.max()))


@functools.lru_cache(maxsize=None)
def build_codebook(K, cs):
    """(C, sites, background, U): C [K, 12] the fp64 values of U (u units); sites maps a site's name to
    {"x": anchor (u), "idx": its code vectors' indices, "rows": its rows (u, integers)}; background
    the indices of the random code vectors."""
    assert K in KS
    rng = np.random.default_rng(977 * K + (5 if cs == "normal" else 0))
    T, last = tiles(K), tiles(K) - 1
    fr = _Free(K)
    U = np.zeros((K, D))
    sites = {}

    def anchor():
        return rng.integers(64, 192, D).astype(np.float64)

    def step():
        s = rng.integers(3, 10, D) * rng.choice([-1.0, 1.0], D)
        return s

    # near-tie pairs
    lastn = K - last * 32                       # valid positions of the last tile
    where = {"tile": (32 * 3 + 1, 32 * 3 + 2), "ends": (3, K - 2), "halves": (32 * 5 + 1, 32 * 5 + 5),
             "last": (last * 32, last * 32 + min(lastn - 1, 7))}
    for name, (ia, ib) in where.items():
        x, s = anchor(), step()
        s[0] = NEAR
        U[fr.take(ia)], U[fr.take(ib)] = x + s, x - s
        e0 = np.eye(D)[0]
        sites["pair:" + name] = {"x": x, "idx": [ia, ib], "rows": np.array([x + e0, x - e0, x])}
    # a row on a code vector
    x = anchor()
    ia, ib = fr.take(32 * 11 + 3), fr.take(32 * 12 + 20)
    U[ia], U[ib] = x, x + ON_STEP * np.eye(D)[0]
    sites["on"] = {"x": x, "idx": [ia, ib], "rows": x[None]}
    # the cap sites, from tile 1 on (K = 512: 16 tiles), each starting where the last one may have ended
    t0 = 1
    for layout in CAP_LAYOUTS:   # (the packed layouts first: "tiles" takes what they leave)
        for n in CAPS:
            x, v = anchor(), step()
            idx = _cap_indices(fr, n, layout, t0)
            signs = set()
            while len(signs) < n:
                signs.add(tuple(rng.choice([-1.0, 1.0], D)))
            for i, sg in zip(idx, sorted(signs)):
                U[i] = x + np.array(sg) * v
            sites["cap:%d:%s" % (n, layout)] = {"x": x, "idx": idx, "rows": x[None]}
            if layout != "tiles":
                t0 = max(idx) // 32 + 1
    assert t0 <= T
    # background: random integer code vectors, redrawn while one crowds a site
    rows = np.concatenate([s["rows"] for s in sites.values()])
    reach = np.concatenate([np.full(len(s["rows"]), site_reach(U, s)) for s in sites.values()])
    background = np.flatnonzero(fr.free)
    for i in background:
        while True:
            c = rng.integers(0, 256, D).astype(np.float64)
            if (np.sqrt(((rows - c) ** 2).sum(axis=1)) > CLEAR * reach).all():
                break
        U[i] = c
    C = values(cs, U)
    C.setflags(write=False)
    for s in sites.values():
        s["rows"].setflags(write=False)
    return C, sites, background, U


def _to_rows(cs, R):
    """Values of integer u rows through the lut (the byte path of set_vectors)."""
    R = np.asarray(R)
    assert np.array_equal(R, np.rint(R)) and R.min() >= 0 and R.max() <= 255
    lut = oracle.lut(COLOUR[cs])
    return np.ascontiguousarray(lut[R.astype(np.uint8) ^ 0x80])


def background_rows(K, cs):
    """(u) the first BACKGROUND_ROWS background code vectors as rows: distance 0 to their own code
    vector and far from every other, so the search does not flag them."""
    _, _, background, U = build_codebook(K, cs)
    return U[background[:BACKGROUND_ROWS]]


@functools.lru_cache(maxsize=None)
def edges(K, cs):
    """(X, C, flagged): every site's rows among the background rows (a site row every third row);
    flagged = the site rows' positions in X, each of which the search must flag."""
    C, sites, _, _ = build_codebook(K, cs)
    site_rows = np.concatenate([s["rows"] for s in sites.values()])
    bg = background_rows(K, cs)
    assert len(bg) >= 3 * len(site_rows)
    R = bg.copy()
    at = np.arange(len(site_rows)) * 3 + 1
    R = np.insert(R, at - np.arange(len(at)), site_rows, axis=0)
    assert np.array_equal(R[at], site_rows)
    X = _to_rows(cs, R)
    X.setflags(write=False)
    return X, C, at


def site_row_names(K, cs):
    """The site of each flagged row of edges(), in order."""
    _, sites, _, _ = build_codebook(K, cs)
    return [n for n, s in sites.items() for _ in range(len(s["rows"]))]


def group_counts(G):
    """Flagged-row counts by name for a grid of G workgroups: one row, one short of a group, a group,
    one more, the first group on wave 1 of workgroup 0 (group G, one row in it), and a second trip of
    wave 0 of workgroup 0 (group 16 G) with two more groups behind it and a ragged one."""
    return {"one": 1, "group_less_one": 31, "group": 32, "group_plus_one": 33, "wave_one": 32 * G + 1,
            "second_trip": 32 * WAVES * G + 32 * 2 + 5}


COUNT_NAMES = tuple(group_counts(1))
COUNT_CODEBOOKS = ((544, "normal"), (1024, "scaled"))   # an odd tile count; the flagship's level


def pattern(n, G):
    """What n flagged rows do on a grid of G: groups, the rows of the last one, the wave and
    workgroup of the last group and the trips of wave 0 of workgroup 0."""
    groups = (n + 31) // 32
    lastg = groups - 1
    return {"groups": groups, "last_rows": n - 32 * lastg, "last_block": lastg % G, "last_wave": (lastg // G) % WAVES,
            "trips_b0w0": len(range(0, groups, G * WAVES))}


def counted(K, cs, n):
    """(X, C): n copies of pair:halves' midpoint row (flagged, and a tie for the reference) behind
    the background rows."""
    C, sites, _, _ = build_codebook(K, cs)
    x = sites["pair:halves"]["x"]
    R = np.concatenate([background_rows(K, cs), np.repeat(x[None], n, axis=0)])
    return _to_rows(cs, R), C


def scattered_neartie(K, cs):
    """(X, C, perm): tests/helpers/neartie_cases.py's near regime (pairs whose distances to their anchor row
    differ by 1e-17 ... 1e-3 relative: below ~1e-7 the search's fp32 pick between them is arbitrary),
    the codebook permuted so that a pair's two code vectors lie in any two tiles and halves: the
    search's provisional index is then often the wrong one of the two, in another tile and the other
    half than the best -- and that index is what the recheck's band is seeded from.  perm: C is the
    builder's codebook[perm]."""
    from helpers import neartie_cases as nt
    X, C = nt.build(D, K, COLOUR[cs], "near", seed=4100 + K + (7 if cs == "normal" else 0))
    perm = np.random.default_rng(K).permutation(K)
    return X, np.ascontiguousarray(C[perm]), perm
