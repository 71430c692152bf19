"""bench_kmeanspp_greedy.py -- qvq_kmeanspp_greedy on a synthetic workload, beside qvq_kmeanspp.

Workload: one SIZE x SIZE synthetic image, BLOCK x BLOCK blocks, K = 2^BITS seeds (C3: 4096, 2, 10,
bench.py's default; C4: 4096, 4, 12), one context, data resident.  Needs an MI355X; reads nothing
outside the repository.  Prints one JSON object (and merges it into --out under the workload's name).
Per seed in --seeds:

  kmeanspp              ms (wall time of Engine.kmeanspp, median of the calls after --warmup; every
                        call ends in the engine's own bounded wait), round_us (ms over the K - 1
                        rounds) and potential (the last one)
  greedy                the same for Engine.kmeanspp_greedy at L = 1, the default count and 16, the
                        calls of the four alternating; wins_by_trial counts the rounds each trial won
  quality               distortion and empty cells after refine(ITERS, eps = 0) from kmeanspp's seeds,
                        from the greedy seeds at each L and from kmeans_par's (default options)
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
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--seeds", default="0,1,2")
    ap.add_argument("--name", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch  # noqa: F401  (opens the device before the engine does)
    import quant_amd

    name = a.name or "%dx%d_b%d_bits%d" % (a.size, a.size, a.block, a.bits)
    K = 1 << a.bits
    L_default = quant_amd.host_kmpp_trials(K)
    trials = [1, L_default, 16]
    res = {"workload": name, "refine_iters_asked": a.iters, "K": K, "default_trials": L_default, "seeds": {}}
    with quant_amd.Engine(0) as eng:
        eng.set_synthetic(a.size, 0x5EED, 1, a.block, a.block, quant_amd.SCALED)
        res.update(blocks=eng.n, dim=eng.dim, plan=quant_amd.host_kmeanspp_plan(eng.n))

        def quality(C0):
            C, A, d, info = eng.refine(K=K, C=C0, max_iters=a.iters, eps=0.0)
            return {"distortion": d, "empty": int((np.bincount(A, minlength=K) == 0).sum()), "iters": info["iters"]}

        for seed in [int(s) for s in a.seeds.split(",")]:
            legs = {"kmeanspp": lambda: eng.kmeanspp(K, seed)}
            for L in trials:
                legs["L%d" % L] = (lambda L: lambda: eng.kmeanspp_greedy(K, seed, L))(L)
            ms, out = {k: [] for k in legs}, {}
            for rep in range(a.warmup + a.reps):
                for k, fn in legs.items():
                    t, out[k] = wall(fn)
                    if rep >= a.warmup:
                        ms[k].append(t)

            def leg(k):
                m = statistics.median(ms[k])
                return {"ms": m, "ms_all": [round(x, 3) for x in ms[k]], "round_us": m * 1e3 / max(K - 1, 1),
                        "potential": int(out[k][2][-1])}

            r = {"kmeanspp": leg("kmeanspp"), "greedy": {}, "quality": {"kmeanspp": quality(out["kmeanspp"][0])}}
            r["kmeanspp"]["placed"] = out["kmeanspp"][3]
            for L in trials:
                k = "L%d" % L
                g, info = leg(k), out[k][3]
                g["placed"] = info["placed"]
                g["wins_by_trial"] = np.bincount(info["trial"][1:info["placed"]], minlength=L).tolist()
                r["greedy"][k] = g
                r["quality"]["greedy_" + k] = quality(out[k][0])
            assert np.array_equal(out["L1"][1], out["kmeanspp"][1]) and np.array_equal(out["L1"][2], out["kmeanspp"][2])
            r["quality"]["kmeans_par"] = quality(eng.kmeans_par(K, seed)[0])
            res["seeds"][str(seed)] = r
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        allres = {}
        if os.path.exists(a.out):
            with open(a.out) as f:
                allres = json.load(f)
        allres[name] = res
        with open(a.out, "w") as f:
            json.dump(allres, f, indent=1, sort_keys=True)
            f.write("\n")


if __name__ == "__main__":
    main()
