"""bench_ingest.py -- the fp64 front door (qvq_set_vectors, qvq_set_vectors_device) on a C3-sized set.

Workload: 4,194,304 x 12 fp64 rows (the blocks of one 4096x4096 image in 2x2 blocks, BASELINE.json
C3) gathered from the colour space's own table, once SCALED and once NORMAL.  Needs an MI355X; reads
nothing outside the repository.  Prints one JSON object (and writes it with --out); per space:

  host_ms               wall time of Engine.set_vectors from a host array, median over reps (and all)
  device_ms             wall time of Engine.set_vectors from a float64 CUDA tensor, median over reps
  classify_ms, pack_ms  device time of the two passes of the tensor call (HIP events inside the
                        engine under set_timing(-3), a run of its own)
  classify_GBps         8 n dim bytes read / classify_ms
  pack_GBps             (8 n dim read + n Dp written) / pack_ms
  mean_ms, mean_GBps    the mean kernel of the same run (Engine.lbg(0) under set_timing(-3)), n Dp bytes
                        read: the project's yardstick for a streaming pass
  mode, colorspace      what the engine chose (training_info; absent on builds without it)

With QVQ_LIB naming an older build of libqvq.so (an A/B against the parent commit) the tensor legs
are left out where the library lacks the entry point, and host_ms is that build's host scan.
Every timed call returns only when the engine is done with the rows.
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
    ap.add_argument("--rows", type=int, default=4096 * 4096 // 4)
    ap.add_argument("--dim", type=int, default=12)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import numpy as np
    import torch
    import quant_amd

    L = quant_amd.lib()
    has_device = hasattr(L, "qvq_set_vectors_device")
    n, dim = a.rows, a.dim
    Dp = (dim + 3) & ~3

    def wall(fn):
        t0 = time.perf_counter()
        fn()
        return (time.perf_counter() - t0) * 1e3

    def med(fn):
        t = [wall(fn) for _ in range(a.warmup + a.reps)][a.warmup:]
        return statistics.median(t), [round(x, 3) for x in t]

    res = {"workload": "%dx%d_fp64" % (n, dim), "lib": os.path.basename(os.path.dirname(quant_amd.LIB_PATH)),
           "device_entry": has_device}
    rng = np.random.default_rng(0x5EED)
    codes = rng.integers(0, 256, size=(n, dim), dtype=np.uint8)
    with quant_amd.Engine(0) as eng:
        for name, cs in (("SCALED", quant_amd.SCALED), ("NORMAL", quant_amd.NORMAL)):
            r = {}
            lut = quant_amd.colorspace_values(cs) if hasattr(L, "qvq_host_colorspace_values") else None
            if lut is None:   # an older build: the same table from the reference's formulas
                s = np.arange(256, dtype=np.uint8).view(np.int8).astype(np.float64)
                lut = (s + 128.0) * (1.0 / 255) if cs == quant_amd.SCALED else s
            X = np.ascontiguousarray(lut[codes])
            r["host_ms"], r["host_ms_all"] = med(lambda: eng.set_vectors(X))
            if has_device:
                info = eng.training_info()
                r["mode"], r["colorspace"] = info["mode"], info["colorspace"]
                Xt = torch.from_numpy(lut).cuda()[torch.from_numpy(codes).cuda().long()].contiguous()
                torch.cuda.synchronize()
                r["device_ms"], r["device_ms_all"] = med(lambda: eng.set_vectors(Xt))
                eng.set_timing(-3)
                cl, pk, mn = [], [], []
                for _ in range(a.warmup + a.reps):
                    eng.set_vectors(Xt)
                    c_ms, p_ms = eng.ingest_ms()
                    eng.lbg(0, want_assign=False)
                    cl.append(c_ms)
                    pk.append(p_ms)
                    mn.append(eng.timings()["mean_ms"])
                eng.set_timing(-2)
                r["classify_ms"] = statistics.median(cl[a.warmup:])
                r["pack_ms"] = statistics.median(pk[a.warmup:])
                r["mean_ms"] = statistics.median(mn[a.warmup:])
                r["classify_GBps"] = 8.0 * n * dim / r["classify_ms"] / 1e6
                r["pack_GBps"] = (8.0 * n * dim + n * Dp) / r["pack_ms"] / 1e6
                r["mean_GBps"] = float(n * Dp) / r["mean_ms"] / 1e6
                del Xt
            res[name] = r
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
