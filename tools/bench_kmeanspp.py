"""bench_kmeanspp.py -- qvq_kmeanspp on a synthetic workload, beside qvq_lbg.

Workload: one SIZE x SIZE synthetic image, BLOCK x BLOCK blocks, K = 2^BITS seeds (C3: 4096, 2, 10,
bench.py's default; C4: 4096, 4, 12), one context, data resident.  Needs an MI355X; reads nothing
outside the repository.  Prints one JSON object (and merges it into --out under the workload's name):

  kmeanspp_ms           wall time of Engine.kmeanspp, median of the calls after --warmup; every call
                        ends in the engine's own bounded wait
  round_us              kmeanspp_ms over the K - 1 rounds (a select and an update each)
  round_bytes           what a round streams at least: the rows N * Dp and m, 4 N read (the stores of
                        m where it fell are not counted)
  round_TBps            round_bytes over round_us, to set beside the ingest pass's rate
                        (profiles/ingest_c3.json)
  lbg_ms                Engine.lbg of this build on the same set, the calls alternating
  quality               distortion, empty cells and wall ms of: the seeds alone (refine with no
                        iteration: the nearest-seed assignment), kmeanspp + refine(ITERS), the same
                        with reseed, lbg + refine(ITERS) and lbg + refine(ITERS, reseed); eps = 0; the
                        legs' ms include their start
  other_k               with --other-k K2: kmeanspp_ms, round_us and the refine(ITERS) quality at a K
                        that is no power of two
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def wall(fn):
    t0 = time.perf_counter()
    r = fn()
    return (time.perf_counter() - t0) * 1e3, r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--block", type=int, default=2)
    ap.add_argument("--bits", type=int, default=10)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--other-k", type=int, default=0)
    ap.add_argument("--name", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch  # noqa: F401  (opens the device before the engine does)
    import quant_amd

    name = a.name or "%dx%d_b%d_bits%d" % (a.size, a.size, a.block, a.bits)
    res = {"workload": name, "seed": a.seed, "refine_iters_asked": a.iters}
    K = 1 << a.bits
    with quant_amd.Engine(0) as eng:
        eng.set_synthetic(a.size, 0x5EED, 1, a.block, a.block, quant_amd.SCALED)
        n, dp = eng.n, (eng.dim + 3) & ~3
        res.update(blocks=n, dim=eng.dim, K=K, plan=quant_amd.host_kmeanspp_plan(n))

        def timed(k):
            t_pp, t_lbg = [], []
            for rep in range(a.warmup + a.reps):
                ms_l = wall(lambda: eng.lbg(a.bits, want_assign=False))[0]
                ms_p, out = wall(lambda: eng.kmeanspp(k, a.seed))
                if rep >= a.warmup:
                    t_lbg.append(ms_l)
                    t_pp.append(ms_p)
            ms = statistics.median(t_pp)
            r = {"kmeanspp_ms": ms, "kmeanspp_ms_all": [round(x, 3) for x in t_pp], "placed": out[3],
                 "round_us": ms * 1e3 / max(k - 1, 1), "round_bytes": n * (dp + 4)}
            r["round_TBps"] = r["round_bytes"] / r["round_us"] / 1e6
            r["potential_first_last"] = [int(out[2][0]), int(out[2][-1])]
            return r, statistics.median(t_lbg), out[0]

        r, res["lbg_ms"], C_pp = timed(K)
        res.update(r)

        def quality(k, start, **kw):
            """start(): the starting codebook or None (continue from lbg)."""
            def run():
                C0 = start()
                return eng.refine(K=k, C=C0, **kw)
            ms, (C, A, d, info) = wall(run)
            return {"distortion": d, "empty": int((np.bincount(A, minlength=k) == 0).sum()), "ms": ms, "iters": info["iters"]}

        def lbg_start():
            eng.lbg(a.bits, want_assign=False)

        pp = lambda k: (lambda: eng.kmeanspp(k, a.seed)[0])   # noqa: E731
        q = {"kmeanspp": quality(K, pp(K), max_iters=0, fresh=True),
             "kmeanspp_refine": quality(K, pp(K), max_iters=a.iters, eps=0.0),
             "kmeanspp_refine_reseed": quality(K, pp(K), max_iters=a.iters, eps=0.0, reseed=True),
             "lbg_refine": quality(K, lbg_start, max_iters=a.iters, eps=0.0),
             "lbg_refine_reseed": quality(K, lbg_start, max_iters=a.iters, eps=0.0, reseed=True)}
        res["quality"] = q
        if a.other_k:
            r, _, _ = timed(a.other_k)
            r["K"] = a.other_k
            r["kmeanspp_refine"] = quality(a.other_k, pp(a.other_k), max_iters=a.iters, eps=0.0)
            res["other_k"] = r
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        allres = {}
        if os.path.exists(a.out):
            with open(a.out) as f:
                allres = json.load(f)
        allres.setdefault(name, {}).update(res)
        with open(a.out, "w") as f:
            json.dump(allres, f, indent=1, sort_keys=True)
            f.write("\n")


if __name__ == "__main__":
    main()
