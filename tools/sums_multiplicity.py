"""How many lanes of a 64-row chunk meet on one LDS address in the fused sums of the D = 12 MFMA
search (k_mf32.hip), from the CPU oracle's per-level indices.  CPU only.

    python tools/sums_multiplicity.py [S] [bits] [every]

The training set is bench.py's (S x S synthetic image, 2 x 2 blocks; default 4096, 10 bits); every
`every`-th chunk (default 16) of each level K >= 64 is counted.  Per K, means over the chunks:
distinct indices (p90), runs of consecutive equal indices, the most lanes on one (copy, index)
with C copies (copy = lane % C), and the same for the kernel's own number of copies with the
staggered component order (lane L starts at component (L / copies) % 12: lanes meet only where
copy, index and start agree).
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import oracle  # noqa: E402

KERNEL_COPIES = {64: 16, 128: 16, 256: 4, 512: 2, 1024: 1}   # launch_assign_mf32, C3's staged levels


def most(keys):
    """Per chunk (row of keys): the largest number of equal keys."""
    s = np.sort(keys, axis=1)
    best = np.ones(len(s), np.int64)
    run = np.ones(len(s), np.int64)
    for j in range(1, s.shape[1]):
        run = np.where(s[:, j] == s[:, j - 1], run + 1, 1)
        best = np.maximum(best, run)
    return best


def main():
    S = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
    bits = int(sys.argv[2]) if len(sys.argv) > 2 else 10
    every = int(sys.argv[3]) if len(sys.argv) > 3 else 16
    X, _ = oracle.tile(oracle.gen_image(S), S, S, 2, 2)
    assigns = oracle.lbg(X, bits, dump=True)[4]
    lane = np.arange(64, dtype=np.int64)
    print("| K | distinct per chunk (p90) | consecutive runs | C=1 | C=2 | C=4 | C=16 | copies | staggered |")
    print("|---|---|---|---|---|---|---|---|---|")
    for lvl in range(6, bits + 1):
        K = 1 << lvl
        A = assigns[lvl - 1].astype(np.int64)
        A = A[:len(A) // 64 * 64].reshape(-1, 64)[::every]
        distinct = np.array([len(np.unique(r)) for r in A])
        runs = 1 + (A[:, 1:] != A[:, :-1]).sum(axis=1)
        cols = [most(A * 16 + lane % C).mean() for C in (1, 2, 4, 16)]
        c = KERNEL_COPIES.get(K, 1)
        stag = most((A * 16 + lane % c) * 12 + (lane // c) % 12).mean()
        print("| %d | %.1f (%d) | %.1f | %s | %d | %.1f |" % (K, distinct.mean(), np.percentile(distinct, 90), runs.mean(),
                                                       " | ".join("%.1f" % v for v in cols), c, stag))


if __name__ == "__main__":
    main()
