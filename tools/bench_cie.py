"""bench_cie.py -- the tile-to-fp64 pass of a CIE1931 raster (qvq_set_images with QVQ_CS_CIE1931,
quant_amd/csrc/k_tile64.hip) on a C3-sized image.

Workload: one S x S raster (default 4096) of seeded random bytes in bw x bh blocks (default 2 x 2:
50 MB read, 403 MB written).  Needs an MI355X; reads nothing outside the repository.  Prints one JSON
object (and writes it with --out):

  tile64_ms      device time of the kernel (HIP events inside the engine under set_timing(-3)), median
                 over reps (and all)
  tile64_GBps    (3 S^2 read + 8 n dim written) / tile64_ms
  host_ms        wall time of Engine.set_images from the host raster, median over reps (and all)
  device_ms      wall time of Engine.set_images_device from a uint8 CUDA tensor
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
    ap.add_argument("--side", type=int, default=4096)
    ap.add_argument("--bw", type=int, default=2)
    ap.add_argument("--bh", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import numpy as np
    import torch
    import quant_amd

    S, bw, bh = a.side, a.bw, a.bh
    rgb = np.random.default_rng(0x5EED).integers(0, 256, size=S * S * 3, dtype=np.uint8)
    n = -(-S // bw) * -(-S // bh)
    dim = 3 * bw * bh

    def wall(fn):
        t0 = time.perf_counter()
        fn()
        return (time.perf_counter() - t0) * 1e3

    def med(fn):
        t = [wall(fn) for _ in range(a.warmup + a.reps)][a.warmup:]
        return statistics.median(t), [round(x, 3) for x in t]

    res = {"workload": "%dx%d_%dx%d_cie1931" % (S, S, bw, bh), "rows": n, "dim": dim}
    with quant_amd.Engine(0) as eng:
        res["host_ms"], res["host_ms_all"] = med(lambda: eng.set_images(rgb, 1, S, S, bw, bh, quant_amd.CIE1931))
        t = torch.from_numpy(rgb).cuda()
        torch.cuda.synchronize()
        res["device_ms"], res["device_ms_all"] = med(
            lambda: eng.set_images_device(t.data_ptr(), 1, S, S, bw, bh, quant_amd.CIE1931))
        eng.set_timing(-3)
        ms = []
        for _ in range(a.warmup + a.reps):
            eng.set_images_device(t.data_ptr(), 1, S, S, bw, bh, quant_amd.CIE1931)
            ms.append(eng.ingest_ms()[1])
        eng.set_timing(-2)
        res["tile64_ms"] = statistics.median(ms[a.warmup:])
        res["tile64_ms_all"] = [round(x, 4) for x in ms[a.warmup:]]
        res["tile64_GBps"] = (3.0 * S * S + 8.0 * n * dim) / res["tile64_ms"] / 1e6
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
