"""bench_refine.py -- the device-resident Lloyd refinement (qvq_refine) on the C3 workload.

Workload: one 4096x4096 synthetic image, 2x2 blocks, 10 bits (bench.py's default, BASELINE.json
C3): Engine.lbg, then Engine.refine(max_iters=ITERS, eps=0) continuing from it.  Needs an MI355X;
reads nothing outside the repository.  Prints one JSON object (and writes it with --out):

  iter_ms               per-iteration time of the device loop, as the marginal cost of an iteration (the
                        entry reports no per-iteration times): (wall(refine(ITERS)) - wall(refine(1)))
                        / (ITERS - 1), median over reps
  refine_ms             wall time of refine(ITERS), indices left on the device, median over reps
  lbg_ms                wall time of the lbg before it, median over reps
  lbg_level10_ms        device time of that lbg's last level (search + sums + the rest, from the
                        engine's per-level events, a run of its own: the events cost time)
  composed_iter_ms      the same ITERS iterations through Engine.assign + Engine.update (indices over
                        PCIe both ways each iteration), per iteration, median over reps
  distortion_lbg / distortion_refined, iters, stop, changed (first run)

--reseed runs the refinement with QVQ_REFINE_RESEED (Engine.refine(reseed=True)) and adds:

  reseeded              seeds placed per iteration (first run)
  empty_cells           cells without a row in the final assignment (an untimed run with indices; also
                        reported without --reseed)
  refine_half_ms        wall time of refine(ITERS // 2), median over reps
  tail_iter_ms          (wall(refine(ITERS)) - wall(refine(ITERS // 2))) / (ITERS - ITERS // 2): the late
                        iterations, which have no empty cell left once `reseeded` has fallen to 0
  (refine_1_ms is then the cost of an iteration that reseeds: the first places nearly all the seeds)

--comm rccl1 joins a one-rank RCCL communicator before the timed loops: every collective of the
sharded schedule (per iteration the all-reduce of the level's sums and the rows changed) then runs
through ncclAllReduce, and the results stay the one-rank results.  --composed-reps 0 leaves the
composed loop out.

Every timed call ends in the engine's own wait for its results; the first --warmup repetitions of
each leg are not timed.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--block", type=int, default=2)
    ap.add_argument("--bits", type=int, default=10)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--composed-reps", type=int, default=2)
    ap.add_argument("--comm", choices=["none", "rccl1"], default="none")
    ap.add_argument("--reseed", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import numpy as np
    import torch  # noqa: F401  (opens the device before the engine does)
    import quant_amd

    def wall(fn):
        t0 = time.perf_counter()
        r = fn()
        return (time.perf_counter() - t0) * 1e3, r

    res = {"workload": "%dx%d_b%d_bits%d" % (a.size, a.size, a.block, a.bits), "iters_asked": a.iters,
           "comm": a.comm, "reseed": a.reseed}
    kw = {"reseed": True} if a.reseed else {}   # (an older A/B build's binding has no such argument)
    half = a.iters // 2
    with quant_amd.Engine(0) as eng:
        if a.comm == "rccl1":
            eng.comm_init(1, 0, quant_amd.Engine.comm_unique_id())
        eng.set_synthetic(a.size, 0x5EED, 1, a.block, a.block, quant_amd.SCALED)
        res["blocks"] = eng.n
        t_lbg, t_ref, t_one, t_half = [], [], [], []
        for rep in range(a.warmup + a.reps):
            ms_l, (C0, _, d0) = wall(lambda: eng.lbg(a.bits, want_assign=False))
            ms_r, (_, _, d1, info) = wall(lambda: eng.refine(max_iters=a.iters, eps=0.0, want_assign=False, **kw))
            eng.lbg(a.bits, want_assign=False)
            ms_1, _ = wall(lambda: eng.refine(max_iters=1, eps=0.0, want_assign=False, **kw))
            ms_h = None
            if a.reseed and half >= 1:
                eng.lbg(a.bits, want_assign=False)
                ms_h, _ = wall(lambda: eng.refine(max_iters=half, eps=0.0, want_assign=False, **kw))
            if rep == 0:
                res.update(distortion_lbg=d0, distortion_refined=d1, iters=info["iters"], stop=info["stop"],
                           changed=info["changed"])
                if a.reseed:
                    res["reseeded"] = info["reseeded"]
                eng.lbg(a.bits, want_assign=False)
                A = eng.refine(max_iters=a.iters, eps=0.0, **kw)[1]
                res["empty_cells"] = int((np.bincount(A, minlength=1 << a.bits) == 0).sum())
            if rep >= a.warmup:
                t_lbg.append(ms_l)
                t_ref.append(ms_r)
                t_one.append(ms_1)
                if ms_h is not None:
                    t_half.append(ms_h)
        n = res["iters"]
        res["lbg_ms"] = statistics.median(t_lbg)
        res["refine_ms"] = statistics.median(t_ref)
        res["refine_1_ms"] = statistics.median(t_one)
        res["iter_ms"] = statistics.median((r - o) / max(n - 1, 1) for r, o in zip(t_ref, t_one))
        res["refine_ms_all"] = [round(x, 4) for x in t_ref]
        if t_half and n == a.iters:
            res["refine_half_ms"] = statistics.median(t_half)
            res["tail_iter_ms"] = statistics.median((r - h) / (n - half) for r, h in zip(t_ref, t_half))
        # the last level of the same lbg, from the engine's events
        eng.set_timing(-1)
        lv = []
        for rep in range(a.warmup + 3):
            eng.lbg(a.bits, want_assign=False)
            t = eng.timings()
            if rep >= a.warmup:
                lv.append(t["assign_ms"][a.bits - 1] + t["update_ms"][a.bits - 1] + t["other_ms"][a.bits - 1])
        eng.set_timing(-2)
        res["lbg_level10_ms"] = statistics.median(lv)
        # the composed loop: the same iterations over the existing single-step entries
        K = 1 << a.bits
        t_comp = []
        for rep in range(1 + a.composed_reps if a.composed_reps else 0):
            C, _, _ = eng.lbg(a.bits, want_assign=False)
            t0 = time.perf_counter()
            for _ in range(n):
                A = eng.assign(C)
                C, _ = eng.update(A, K)
            if rep >= 1:
                t_comp.append((time.perf_counter() - t0) * 1e3 / n)
        if t_comp:
            res["composed_iter_ms"] = statistics.median(t_comp)
            res["composed_over_device"] = res["composed_iter_ms"] / res["iter_ms"]
        res["iter_over_level10"] = res["iter_ms"] / res["lbg_level10_ms"]
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
