"""The pruned searches' window rule in numpy, stated from the design and
not from the kernels: which code tiles a group of rows visits, and what each row answers over the
visited tiles alone.  Real arithmetic (fp64 for the decisions, long double where a loss is judged),
no engine.  tests/test_prune_plan.py holds tests/helpers/prune_cases.py to it; a failing GPU test
prints its windows (tests/test_gpu_prune_bound.py).

The rule.  Every value is v = mu + w sx with w = 2u - 255 an integer (u the byte's ordinal), so
||x - c||^2 >= sx^2 (sum_d w_d - q_c)^2 / D with q_c = sum_d (c_d - mu) / sx.  The code vectors are
ordered by q and cut into tiles of 32; tile t's envelope is [floor(min q) - 1, ceil(max q) + 1],
made monotone (suffix minimum of the lows, prefix maximum of the highs).  A group of rows (one
64-row chunk of the D = 12 search, the 8 chunks of a workgroup of the wide search) with sums in
[qmn, qmx] first searches the unit (a tile; a slice of 4 tiles in the wide search) holding the
first tile whose envelope reaches floor((qmn + qmx) / 2), takes B = max over its rows of the row's
best distance in that unit, and then visits every tile whose gap g = max(0, lo - qmx, qmn - hi)
has g^2 <= B D / sx^2, as one contiguous range of units.  The kernels add their fp32 margins and
score errors to B: the model's window is a lower bound on theirs.

Mutation: every field only narrows a window.  The rule as documented is Mutation()."""
import collections

import numpy as np

TILE = 32
CHUNK = 64
WD_WAVES = 8       # chunks per workgroup of the wide search
WD_SLICE_TILES = 4  # tiles per streamed slice of the wide search
TERMS = {0: (-0.5, 0.5), 1: (0.5, 1.0 / 510.0)}   # colour space (oracle.NORMAL, oracle.SCALED) -> (mu, sx)

Mutation = collections.namedtuple(
    "Mutation", "factor reduce rows32 q_half d_half pad", defaults=(1.0, "max", False, False, False, False))
# factor: the bound times a factor;  reduce: "max" (the rule), "min" (minimum over the group's rows)
# or "first" (the first chunk's maximum stands for the workgroup's);  rows32: only rows 0-31 of a
# chunk feed the bound;  q_half: the code vectors' q in units of 2w;  d_half: D / 2 for D in the
# bound;  pad: the rows' pad bytes (value 0.0, up to the next multiple of 4) counted in sum w.


def row_sums(X, cs, pad=False):
    """sum_d w_d per row (exact integers) over the D real components; pad=True adds the pad
    bytes' w (the byte of value 0.0) for the components D .. Dp - 1, Dp the next multiple of 4."""
    mu, sx = TERMS[cs]
    w = np.rint((np.asarray(X, np.float64) - mu) / sx).astype(np.int64)
    assert np.all((w & 1) == 1) and np.abs(w).max() <= 255, "rows are not byte values"
    s = w.sum(axis=1)
    if pad:
        D = X.shape[1]
        s = s + (-(-D // 4) * 4 - D) * int(np.rint((0.0 - mu) / sx))
    return s


def projections(C, cs):
    mu, sx = TERMS[cs]
    return ((np.asarray(C, np.float64) - mu) / sx).sum(axis=1)


def tile_order(q):
    """(perm, lo, hi): positions -> code vectors by q (a full, stable sort), and the tiles'
    monotone integer envelopes."""
    perm = np.argsort(q, kind="stable")
    K = len(q)
    nt = -(-K // TILE)
    lo = np.array([np.floor(q[perm[TILE * t:TILE * t + TILE]].min()) - 1 for t in range(nt)], np.int64)
    hi = np.array([np.ceil(q[perm[TILE * t:TILE * t + TILE]].max()) + 1 for t in range(nt)], np.int64)
    return perm, np.minimum.accumulate(lo[::-1])[::-1], np.maximum.accumulate(hi)


def wide_chunk(task, wave, ntask, cpr):
    """The chunk of a workgroup's wave: whole groups of cpr tasks are stacked (a task's waves take
    chunks cpr apart), leftover tasks take consecutive chunks."""
    full = ntask // cpr * cpr
    if task < full:
        return task // cpr * cpr * WD_WAVES + task % cpr + wave * cpr
    return task * WD_WAVES + wave


def cpr_of(col_blocks):
    return max(1, (col_blocks + 32) // 64)


def groups(N, kind, cpr=1):
    """The row groups that share one window: lists of chunks (row index arrays, first chunk first)."""
    nchunks = -(-N // CHUNK)
    rows = [np.arange(CHUNK * c, min(N, CHUNK * c + CHUNK)) for c in range(nchunks)]
    if kind == "mf32":
        return [[r] for r in rows]
    assert kind == "wide"
    ntask = -(-nchunks // WD_WAVES)
    out = []
    for task in range(ntask):
        ch = [wide_chunk(task, w, ntask, cpr) for w in range(WD_WAVES)]
        out.append([rows[c] for c in ch if c < nchunks])
    assert sorted(int(r) for g in out for c in g for r in c) == list(range(N))
    return out


def _dist(X, C):
    """Squared distances [n, k] in fp64, direct form."""
    d = X[:, None, :] - C[None, :, :]
    return np.einsum("nkd,nkd->nk", d, d)


Result = collections.namedtuple("Result", "answer window visited tiles perm lo hi qw first")
# answer [N]: each row's nearest code vector among the visited tiles (fp64 argmin, first position);
# window [N, 2]: the row's group's tile range (inclusive);  visited: the mean share of the tiles a
# row's group visits;  tiles: the tile count;  perm, lo, hi: tile_order;  qw: row_sums;
# first [N]: the tile the group searched first.


def search(X, C, cs, kind="mf32", cpr=1, mut=Mutation(), margin=False):
    """The rule on rows X and codebook C.  kind "mf32": a window per 64-row chunk in tiles;
    "wide": a window per workgroup (groups(N, "wide", cpr)) in slices of 4 tiles, the bound taken
    from the whole first slice.  margin=True widens the bound as the kernels' fp32 form does
    (x 1.00001 + 1)."""
    X = np.asarray(X, np.float64)
    C = np.asarray(C, np.float64)
    N, D = X.shape
    mu, sx = TERMS[cs]
    q = projections(C, cs)
    perm, lo, hi = tile_order(q)
    if mut.q_half:      # the envelopes in units of 2w, the order unchanged
        _, lo, hi = tile_order(q / 2)
    nt = len(lo)
    qw = row_sums(X, cs, pad=mut.pad)
    spu = WD_SLICE_TILES if kind == "wide" else 1   # tiles per unit
    answer = np.zeros(N, np.int64)
    window = np.zeros((N, 2), np.int64)
    first = np.zeros(N, np.int64)
    share = 0.0
    scale = (D / 2 if mut.d_half else D) / (sx * sx)
    Cp = C[perm]
    for chunks in groups(N, kind, cpr):
        rows = np.concatenate(chunks)
        qmn, qmx = int(qw[rows].min()), int(qw[rows].max())
        mid = (qmn + qmx) >> 1
        t0 = min(int(np.sum(hi < mid)), nt - 1)
        u0 = t0 // spu
        p0, p1 = u0 * spu * TILE, min(len(q), (u0 + 1) * spu * TILE)
        feed = chunks[0] if mut.reduce == "first" else rows
        if mut.rows32:
            feed = feed[feed % CHUNK < 32]
        best = _dist(X[feed], Cp[p0:p1]).min(axis=1)
        B = (best.min() if mut.reduce == "min" else best.max()) * mut.factor
        thr = B * scale
        if margin:
            thr = thr * 1.00001 + 1.0
        gap = np.maximum(0, np.maximum(lo - qmx, qmn - hi)).astype(np.float64)
        win = np.flatnonzero(gap * gap <= thr)
        w_lo = min(t0, int(win[0])) if len(win) else t0
        w_hi = max(t0, int(win[-1])) if len(win) else t0
        w_lo, w_hi = w_lo // spu * spu, min(nt - 1, w_hi // spu * spu + spu - 1)
        a, b = w_lo * TILE, min(len(q), (w_hi + 1) * TILE)
        answer[rows] = perm[a + np.argmin(_dist(X[rows], Cp[a:b]), axis=1)]
        window[rows] = (w_lo, w_hi)
        first[rows] = t0
        share += len(rows) * (w_hi - w_lo + 1) / nt
    return Result(answer, window, share / N, nt, perm, lo, hi, row_sums(X, cs), first)


def tile_of(perm):
    """Code vector -> its tile."""
    pos = np.empty(len(perm), np.int64)
    pos[perm] = np.arange(len(perm))
    return pos // TILE


def lost(res, i1, i2, tie):
    """Rows whose window misses what the search owes them: the tile of the nearest code vector i1,
    and, where the two nearest tie (tie: bool per row), the tile of the runner-up i2 as well --
    without both in the window the row is not flagged and the reference's tie rule never runs."""
    t = tile_of(res.perm)
    out = (t[i1] < res.window[:, 0]) | (t[i1] > res.window[:, 1])
    miss2 = (t[i2] < res.window[:, 0]) | (t[i2] > res.window[:, 1])
    return out | (np.asarray(tie) & miss2)


def recheck_windows(X, C, cs, A, rows, mut=Mutation(), margin=False):
    """The chunked recheck's pruned sweep, per flagged row: the tiles whose gap
    to the row's own sum w passes (d_A + band) 1.001 D / sx^2, d_A the distance to the search's
    index A[row]; the band's alpha, beta and gamma taken as 0, so a lower bound on the kernel's
    window (which is the union over a group of 16 rows).  Returns [len(rows), 2] tile ranges."""
    X = np.asarray(X, np.float64)
    C = np.asarray(C, np.float64)
    D = X.shape[1]
    mu, sx = TERMS[cs]
    q = projections(C, cs)
    _, lo, hi = tile_order(q / 2 if mut.q_half else q)
    qw = row_sums(X, cs, pad=mut.pad)
    scale = (D / 2 if mut.d_half else D) / (sx * sx)
    out = np.zeros((len(rows), 2), np.int64)
    for j, r in enumerate(rows):
        e = X[r] - C[A[r]]
        thr = float(e @ e) * 1.001 * mut.factor * scale
        if margin:
            thr = thr * 1.00001 + 1.0
        gap = np.maximum(0, np.maximum(lo - qw[r], qw[r] - hi)).astype(np.float64)
        win = np.flatnonzero(gap * gap <= thr)
        out[j] = (win[0], win[-1]) if len(win) else (len(lo), -1)
    return out
