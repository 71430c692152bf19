"""bench_kmeans_par.py -- qvq_kmeans_par on a synthetic workload, beside qvq_kmeanspp.

Workload: one SIZE x SIZE synthetic image, BLOCK x BLOCK blocks, K = 2^BITS seeds (C3: 4096, 2, 10,
bench.py's default; C4: 4096, 4, 12), one context, data resident.  Needs an MI355X; reads nothing
outside the repository.  Prints one JSON object (and merges it into --out under the workload's name):

  kmeans_par_ms         wall time of Engine.kmeans_par (default options), median of the calls after
                        --warmup; every call ends in the engine's own bounded wait
  kmeanspp_ms           Engine.kmeanspp of this build on the same set, the calls alternating
  ratio                 kmeanspp_ms over kmeans_par_ms; *_ms_all are the single calls (the span)
  phases_ms             one more call under set_timing(-3), device ms from HIP events: first (candidate
                        0's pass), sample and update per round, weights, reduce
  info                  candidates, rounds_run, truncated, round_candidates, placed of the timed call
  quality               per seed in --seeds, for both seedings: distortion and empty cells of the seeds
                        alone (refine with no iteration: the nearest-seed assignment) and after
                        refine(ITERS), eps = 0
"""
import argparse
import ctypes
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
    ap.add_argument("--seeds", type=int, nargs="*", default=[0, 1, 2])
    ap.add_argument("--name", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch  # noqa: F401  (opens the device before the engine does)
    import quant_amd

    name = a.name or "%dx%d_b%d_bits%d" % (a.size, a.size, a.block, a.bits)
    res = {"workload": name, "refine_iters_asked": a.iters}
    K = 1 << a.bits
    seed0 = a.seeds[0] if a.seeds else 0
    with quant_amd.Engine(0) as eng:
        eng.set_synthetic(a.size, 0x5EED, 1, a.block, a.block, quant_amd.SCALED)
        n = eng.n
        res.update(blocks=n, dim=eng.dim, K=K, plan=quant_amd.host_kmeans_par_plan(n, eng.dim, K))
        t_par, t_pp = [], []
        for rep in range(a.warmup + a.reps):
            ms_pp = wall(lambda: eng.kmeanspp(K, seed0))[0]
            ms_par, out = wall(lambda: eng.kmeans_par(K, seed0))
            if rep >= a.warmup:
                t_pp.append(ms_pp)
                t_par.append(ms_par)
        res["kmeans_par_ms"], res["kmeanspp_ms"] = statistics.median(t_par), statistics.median(t_pp)
        res["kmeans_par_ms_all"] = [round(x, 3) for x in t_par]
        res["kmeanspp_ms_all"] = [round(x, 3) for x in t_pp]
        res["ratio"] = res["kmeanspp_ms"] / res["kmeans_par_ms"]
        info = out[4]
        res["info"] = {k: info[k] for k in ("placed", "candidates", "rounds_run", "truncated")}
        res["info"]["round_candidates"] = info["round_candidates"][:info["rounds_run"]]
        res["info"]["potential_first_last"] = [info["potential"][0], info["potential"][info["rounds_run"]]]

        eng.set_timing(-3)
        eng.kmeans_par(K, seed0)
        t = quant_amd._Timings()
        quant_amd.lib().qvq_get_timings(eng._h, ctypes.byref(t))
        eng.set_timing(-2)
        R = info["rounds_run"]
        res["phases_ms"] = {"first": t.update_ms[0], "sample": [round(t.other_ms[r], 4) for r in range(R)],
                            "update": [round(t.assign_ms[r], 4) for r in range(R)], "weights": t.update_ms[1],
                            "reduce": t.update_ms[2], "wall": t.total_ms}

        def quality(C0, iters):
            C, A, d, rinfo = eng.refine(K=K, C=C0, max_iters=iters, eps=0.0, fresh=iters == 0)
            return {"distortion": d, "empty": int((np.bincount(A, minlength=K) == 0).sum()), "iters": rinfo["iters"]}

        res["quality"] = {}
        for seed in a.seeds:
            C_par, C_pp = eng.kmeans_par(K, seed)[0], eng.kmeanspp(K, seed)[0]
            res["quality"][str(seed)] = {"kmeans_par": quality(C_par, 0), "kmeans_par_refine": quality(C_par, a.iters),
                                         "kmeanspp": quality(C_pp, 0), "kmeanspp_refine": quality(C_pp, a.iters)}
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
