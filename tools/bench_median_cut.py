"""bench_median_cut.py -- qvq_median_cut on a synthetic workload, beside qvq_lbg.

Workload: one SIZE x SIZE synthetic image, BLOCK x BLOCK blocks, BITS bits (C3: 4096, 2, 10, bench.py's
default; C4: 4096, 4, 12).  Needs an MI355X; reads nothing outside the repository.  Prints one JSON
object (and merges it into --out under the workload's name):

  median_cut_ms         wall time of Engine.median_cut (labels left on the device), median of the
                        calls after --warmup; every call ends in the engine's own bounded wait
  lbg_ms                the same for Engine.lbg of this build, the two calls alternating
  parent_lbg_ms         with --parent-lib: Engine.lbg of that build (QVQ_LIB) in child processes that
                        alternate with this build's, --rounds times; median of the children's medians
  levels                per level, from the engine's events under set_timing(-1) (a run of its own: each
                        record idles the GPU): rows_ms the two row passes, other_ms the rest
  quality               distortion, empty boxes / cells and wall ms of median_cut, median_cut +
                        refine(ITERS), lbg and lbg + refine(ITERS) (eps = 0; the refine legs' ms include
                        their start)
  kernels               with --trace CSV (a rocprofv3 --kernel-trace of `--leg trace`): the median-cut
                        kernels of the last call in launch order, us each, and for the row passes the
                        bytes they stream (rows N * Dp, labels 4 N read, 4 N written by the ranges pass)
                        over that time in TB/s
"""
import argparse
import csv
import json
import os
import re
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def wall(fn):
    t0 = time.perf_counter()
    r = fn()
    return (time.perf_counter() - t0) * 1e3, r


def leg(a):
    import numpy as np
    import torch  # noqa: F401  (opens the device before the engine does)
    import quant_amd

    res = {}
    K = 1 << a.bits
    with quant_amd.Engine(0) as eng:
        eng.set_synthetic(a.size, 0x5EED, 1, a.block, a.block, quant_amd.SCALED)
        res["blocks"], res["dim"] = eng.n, eng.dim
        if a.leg == "lbg":   # an A/B build: its lbg only
            t = [wall(lambda: eng.lbg(a.bits, want_assign=False))[0] for _ in range(a.warmup + a.reps)]
            res["lbg_ms"] = statistics.median(t[a.warmup:])
            res["lbg_ms_all"] = [round(x, 4) for x in t[a.warmup:]]
            return res
        if a.leg == "trace":
            for _ in range(a.warmup + 1):
                eng.median_cut(a.bits, want_assign=False)
            return res
        t_mc, t_lbg = [], []
        for rep in range(a.warmup + a.reps):
            ms_l, (_, _, d_l) = wall(lambda: eng.lbg(a.bits, want_assign=False))
            ms_m, (_, _, d_m, cuts) = wall(lambda: eng.median_cut(a.bits, want_assign=False))
            if rep >= a.warmup:
                t_lbg.append(ms_l)
                t_mc.append(ms_m)
        res.update(median_cut_ms=statistics.median(t_mc), lbg_ms=statistics.median(t_lbg),
                   median_cut_ms_all=[round(x, 4) for x in t_mc], lbg_ms_all=[round(x, 4) for x in t_lbg], cuts=cuts)
        eng.set_timing(-1)
        rows, other = [], []
        for rep in range(a.warmup + 3):
            eng.median_cut(a.bits, want_assign=False)
            if rep >= a.warmup:
                t = eng.timings()
                rows.append(t["assign_ms"][:a.bits])
                other.append(t["other_ms"][:a.bits])
        eng.set_timing(-2)
        res["levels"] = {"rows_ms": [round(statistics.median(x), 4) for x in zip(*rows)],
                         "other_ms": [round(statistics.median(x), 4) for x in zip(*other)]}
        empty = lambda A: int((np.bincount(A, minlength=K) == 0).sum())   # noqa: E731
        q = {}
        ms, (C, A, d, _) = wall(lambda: eng.median_cut(a.bits))
        q["median_cut"] = {"distortion": d, "empty": empty(A), "ms": ms}
        ms, (C, A, d, info) = wall(lambda: eng.refine(C=eng.median_cut(a.bits, want_assign=False)[0],
                                                      max_iters=a.iters, eps=0.0))
        q["median_cut_refine"] = {"distortion": d, "empty": empty(A), "ms": ms, "iters": info["iters"]}
        ms, (C, A, d) = wall(lambda: eng.lbg(a.bits))
        q["lbg"] = {"distortion": d, "empty": empty(A), "ms": ms}

        def lbg_refine():
            eng.lbg(a.bits, want_assign=False)
            return eng.refine(max_iters=a.iters, eps=0.0)
        ms, (C, A, d, info) = wall(lbg_refine)
        q["lbg_refine"] = {"distortion": d, "empty": empty(A), "ms": ms, "iters": info["iters"]}
        res["quality"] = q
        res["refine_iters_asked"] = a.iters
    return res


def kernels_of(path, n, dp, bits):
    """The last call's median-cut kernels from a rocprofv3 kernel trace."""
    with open(path) as f:
        rows = [r for r in csv.DictReader(f) if "mc_" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    per_call = 1 + 4 * bits + 1
    out = []
    for r in rows[-per_call:]:
        m = re.search(r"mc_\w+(<[^>]*>)?", r["Kernel_Name"])
        name = m.group(0) if m else r["Kernel_Name"]
        us = (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
        k = {"kernel": name, "us": round(us, 2)}
        if "mc_rows" in name or "mc_hist" in name:
            nbytes = n * dp + 4 * n + (4 * n if "mc_rows" in name else 0)
            k["TBps"] = round(nbytes / us / 1e6, 3)
        out.append(k)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--block", type=int, default=2)
    ap.add_argument("--bits", type=int, default=10)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--leg", choices=["all", "lbg", "trace"], default="all")
    ap.add_argument("--parent-lib", default=None, help="libqvq.so of the parent commit's build")
    ap.add_argument("--trace", default=None, help="kernel trace CSV of a --leg trace run")
    ap.add_argument("--name", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    name = a.name or "%dx%d_b%d_bits%d" % (a.size, a.size, a.block, a.bits)
    if a.trace:
        n = ((a.size + a.block - 1) // a.block) ** 2
        dp = (3 * a.block * a.block + 3) & ~3
        res = {"kernels": kernels_of(a.trace, n, dp, a.bits)}
    elif a.parent_lib and a.leg == "all":
        # alternate whole processes: the parent build's lbg, then this build's legs
        me = [sys.executable, os.path.abspath(__file__), "--size", str(a.size), "--block", str(a.block), "--bits",
              str(a.bits), "--iters", str(a.iters), "--reps", str(a.reps), "--warmup", str(a.warmup)]
        parent, mine = [], []
        for _ in range(a.rounds):
            for lib, extra, sink in ((a.parent_lib, ["--leg", "lbg"], parent), (None, [], mine)):
                env = dict(os.environ)
                env.pop("QVQ_LIB", None)
                if lib:
                    env["QVQ_LIB"] = os.path.abspath(lib)
                r = subprocess.run(me + extra, env=env, capture_output=True, text=True, timeout=600)
                if r.returncode != 0:
                    sys.stderr.write(r.stderr)
                    sys.exit(r.returncode)
                sink.append(json.loads(r.stdout.strip().splitlines()[-1]))
        res = mine[-1]
        res["median_cut_ms_rounds"] = [m["median_cut_ms"] for m in mine]
        res["lbg_ms_rounds"] = [m["lbg_ms"] for m in mine]
        res["parent_lbg_ms_rounds"] = [p["lbg_ms"] for p in parent]
        res["median_cut_ms"] = statistics.median(res["median_cut_ms_rounds"])
        res["lbg_ms"] = statistics.median(res["lbg_ms_rounds"])
        res["parent_lbg_ms"] = statistics.median(res["parent_lbg_ms_rounds"])
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
