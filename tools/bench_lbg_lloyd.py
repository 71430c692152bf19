"""bench_lbg_lloyd.py -- qvq_lbg_lloyd on a synthetic workload, beside qvq_lbg and qvq_lbg + qvq_refine.

Workload: one SIZE x SIZE synthetic image, BLOCK x BLOCK blocks, BITS bits (C3: 4096, 2, 10, bench.py's
default; C4: 4096, 4, 12).  Needs an MI355X; reads nothing outside the repository.  Prints one JSON
object (and merges it into --out under the workload's name); every ms is the wall time of the calls
with the indices left on the device, the median of --reps calls after --warmup, eps = 0:

  lbg_ms                Engine.lbg of this build
  parent_lbg_ms         with --parent-lib: Engine.lbg of that build (QVQ_LIB) in child processes that
                        alternate with this build's, --rounds times; median of the children's medians
  lbg                   distortion and empty cells of Engine.lbg
  lbg_refine            per n in --refine: Engine.lbg + Engine.refine(n): ms of the two calls together,
                        the iterations run, distortion, empty cells
  lloyd                 per iterations-per-level in --iters, without and with reseed: ms, distortion,
                        empty cells (of the last level), the levels' iterations and seeds
  lloyd_eps             the levels' iterations and stops at eps = --eps (at most --eps-iters per level), ms
  levels_ms             with --level-times: host wall per level of one lbg_lloyd(ITERS) call, measured by
                        growing the schedule a level at a time (differences of whole calls' medians)
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, warmup, reps):
    """(median ms, the last call's result)."""
    t, r = [], None
    for _ in range(warmup + reps):
        t0 = time.perf_counter()
        r = fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(t[warmup:]), r


def leg(a):
    import numpy as np
    import torch  # noqa: F401  (opens the device before the engine does)
    import quant_amd

    res = {}
    K = 1 << a.bits
    empty = lambda A: int((np.bincount(A, minlength=K) == 0).sum())   # noqa: E731
    with quant_amd.Engine(0) as eng:
        eng.set_synthetic(a.size, 0x5EED, 1, a.block, a.block, quant_amd.SCALED)
        res["blocks"], res["dim"] = eng.n, eng.dim
        res["lbg_ms"], _ = timed(lambda: eng.lbg(a.bits, want_assign=False), a.warmup, a.reps)
        if a.leg == "lbg":   # an A/B build: its lbg only
            return res
        _, A, d = eng.lbg(a.bits)
        res["lbg"] = {"distortion": d, "empty": empty(A)}
        res["lbg_refine"] = {}
        for n in a.refine:
            def lbg_refine(want=False):
                eng.lbg(a.bits, want_assign=False)
                return eng.refine(max_iters=n, eps=0.0, want_assign=want)
            ms, _ = timed(lbg_refine, a.warmup, a.reps)
            _, A, d, info = lbg_refine(True)
            res["lbg_refine"][str(n)] = {"ms": ms, "iters": info["iters"], "distortion": d, "empty": empty(A)}
        res["lloyd"] = {}
        for it in a.iters:
            for reseed in (False, True):
                ms, (_, _, d, lv) = timed(lambda: eng.lbg_lloyd(a.bits, it, 0.0, reseed=reseed, want_assign=False),
                                          a.warmup, a.reps)
                res["lloyd"]["%d%s" % (it, "_reseed" if reseed else "")] = {
                    "ms": ms, "distortion": d, "empty": lv[-1]["empty"] if lv else 0,
                    "iters": [v["iters"] for v in lv], "seeds": [v["seeds"] for v in lv]}
        ms, (_, _, d, lv) = timed(lambda: eng.lbg_lloyd(a.bits, a.eps_iters, a.eps, want_assign=False), a.warmup, a.reps)
        res["lloyd_eps"] = {"eps": a.eps, "max_iters": a.eps_iters, "ms": ms, "distortion": d,
                            "empty": lv[-1]["empty"] if lv else 0, "iters": [v["iters"] for v in lv],
                            "stop": [v["stop"] for v in lv]}
        if a.level_times:
            whole = [timed(lambda: eng.lbg_lloyd(b, a.level_times, 0.0, want_assign=False), a.warmup, a.reps)[0]
                     for b in range(a.bits + 1)]
            res["levels_ms"] = {"iters": a.level_times, "bits0_ms": round(whole[0], 4),
                                "levels": [round(whole[b] - whole[b - 1], 4) for b in range(1, a.bits + 1)]}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--block", type=int, default=2)
    ap.add_argument("--bits", type=int, default=10)
    ap.add_argument("--iters", type=int, nargs="+", default=[1, 2, 3, 5])
    ap.add_argument("--refine", type=int, nargs="+", default=[4, 8, 20])
    ap.add_argument("--eps", type=float, default=1e-3)
    ap.add_argument("--eps-iters", type=int, default=50)
    ap.add_argument("--level-times", type=int, default=0, metavar="ITERS")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--leg", choices=["all", "lbg"], default="all")
    ap.add_argument("--parent-lib", default=None, help="libqvq.so of the parent commit's build")
    ap.add_argument("--name", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    name = a.name or "%dx%d_b%d_bits%d" % (a.size, a.size, a.block, a.bits)
    if a.parent_lib and a.leg == "all":
        # alternate whole processes: the parent build's lbg, then this build's; the other legs once
        me = [sys.executable, os.path.abspath(__file__), "--size", str(a.size), "--block", str(a.block), "--bits",
              str(a.bits), "--reps", str(a.reps), "--warmup", str(a.warmup)]
        parent, mine = [], []
        for _ in range(a.rounds):
            for lib, sink in ((a.parent_lib, parent), (None, mine)):
                env = dict(os.environ)
                env.pop("QVQ_LIB", None)
                if lib:
                    env["QVQ_LIB"] = os.path.abspath(lib)
                r = subprocess.run(me + ["--leg", "lbg"], env=env, capture_output=True, text=True, timeout=600)
                if r.returncode != 0:
                    sys.stderr.write(r.stderr)
                    sys.exit(r.returncode)
                sink.append(json.loads(r.stdout.strip().splitlines()[-1])["lbg_ms"])
        res = leg(a)
        res["lbg_ms_rounds"], res["parent_lbg_ms_rounds"] = mine, parent
        res["lbg_ms"], res["parent_lbg_ms"] = statistics.median(mine), statistics.median(parent)
    else:
        res = leg(a)
    res["workload"] = name
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
