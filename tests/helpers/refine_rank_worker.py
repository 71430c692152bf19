"""One rank of the sharded qvq_refine tests (tests/test_gpu_refine_sharded.py): WORLD of these
processes share GPU 0 and exchange through the engine's test-only host communicator
(qvq_comm_init_host) over torch.distributed's gloo backend, as tests/helpers/rank_worker.py does
for qvq_lbg.  One process runs every case of its PLAN in sequence on its own rows and writes one
.npz, so the torch import is paid once per rank.

    python refine_rank_worker.py RANK WORLD RENDEZVOUS_FILE PLAN OUT.npz CUTS...
PLAN: a comma-separated list of the steps below.  CUTS: WORLD + 1 row cuts, each a fraction "a/b"
of the step's row count N (the row N * a // b) or an absolute row "=i": rank r holds the rows
cuts[r] .. cuts[r + 1] of every step's training set.

Per step `s` the file holds s_C, s_A, s_d, s_iters, s_stop, s_changed, s_trace and s_calls: the
element count of every all-reduce the step issued (the collective budget).
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def row_cuts(args, n):
    cuts = []
    for a in args:
        if a.startswith("="):
            cuts.append(int(a[1:]))
        else:
            num, den = a.split("/")
            cuts.append(n * int(num) // int(den))
    assert cuts[0] == 0 and cuts[-1] == n and cuts == sorted(cuts), cuts
    return cuts


def main():
    rank, world, rdv, plan, out = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3], sys.argv[4], sys.argv[5]
    cut_args = sys.argv[6:]
    assert len(cut_args) == world + 1
    import datetime
    import time
    import torch
    import torch.distributed as dist
    import quant_amd
    from helpers import refine_ref as ref
    os.environ.setdefault("GLOO_SOCKET_IFNAME", "lo")
    dist.init_process_group("gloo", init_method="file://" + rdv, rank=rank, world_size=world,
                            timeout=datetime.timedelta(seconds=60))
    calls = []

    def allreduce(arr):
        calls.append(arr.size)
        t = torch.from_numpy(arr.view(np.int64) if arr.dtype == np.uint64 else arr)   # shares arr's memory
        dist.all_reduce(t)   # int64 sums wrap like the engine's u64 sums

    eng = quant_amd.Engine(0)
    eng.comm_init_host(world, rank, allreduce)
    res = {"info": np.array(eng.comm_info())}

    def load(name, seed=0x5EED):
        S, b, bits = ref.CASES[name] if name in ref.CASES else (256, 2, 9)
        _, X = ref.case_vectors(S, b, seed)
        cuts = row_cuts(cut_args, X.shape[0])
        eng.set_vectors(X[cuts[rank]:cuts[rank + 1]])
        return bits

    def keep(key, got):
        C, A, d, info = got
        res.update({key + "_C": C, key + "_A": A, key + "_d": np.array([d]), key + "_iters": np.array([info["iters"]]),
                    key + "_stop": np.array([info["stop"]]), key + "_changed": np.array(info["changed"], np.uint64),
                    key + "_trace": np.array(info["distortion"], np.float64), key + "_calls": np.array(calls, np.uint64)})

    def refine(key, **kw):
        del calls[:]
        keep(key, eng.refine(**kw))

    def keep_lbg(key, got):
        C, A, d = got
        res.update({key + "_C": C, key + "_A": A, key + "_d": np.array([d])})

    def rejected(key, fn):
        """The status fn() raises and the seconds it took (-1: it did not raise)."""
        t0 = time.time()
        try:
            fn()
            st = -1
        except quant_amd.QVQError as e:
            st = e.status
        res[key] = np.array([st, time.time() - t0], np.float64)

    for step in plan.split(","):
        if step in ("fix_s128_b2_6", "fix_s64_b2_4", "fix_s96_b4_5"):   # cases 1, 2: to the fixed point
            eng.lbg(load(step[4:]))
            refine(step, max_iters=40, eps=0.0)
        elif step == "eps":                                              # case 3
            eng.lbg(load("s128_b2_6"))
            refine(step, max_iters=40, eps=0.01)
        elif step == "fresh0":                                           # case 4
            keep_lbg("fresh0_lbg", eng.lbg(load("s128_b2_6")))
            refine(step, max_iters=0, fresh=True)
        elif step == "fresh3":
            eng.lbg(load("s128_b2_6"))
            refine(step, max_iters=3, eps=0.0, fresh=True)
        elif step == "warm":                                             # case 5: case 1's codebook, another image
            C_fix = res["fix_s128_b2_6_C"]
            load("s128_b2_6", seed=0xBEEF)
            refine(step, C=C_fix, max_iters=4, eps=0.0)
        elif step == "k512":                                             # case 6
            eng.lbg(load("k512"))
            refine(step, max_iters=3, eps=0.0)
        elif step == "state":                                            # case 7
            bits = load("s64_b2_4")
            keep_lbg("state_lbg1", eng.lbg(bits))
            refine("state_r40", max_iters=40, eps=0.0)
            keep_lbg("state_lbg2", eng.lbg(bits))
            refine("state_r2", max_iters=2, eps=0.0)
            refine("state_r2r3", max_iters=3, eps=0.0)   # continues the refine before it
            eng.lbg(bits)
            refine("state_r5", max_iters=5, eps=0.0)
        elif step == "disagree":                                         # case 9
            bits = load("s64_b2_4")
            eng.lbg(bits)
            rejected("dis_iters", lambda: eng.refine(max_iters=7 if rank == 1 else 40, eps=0.0))
            C_l, _, _ = eng.lbg(bits)
            if rank == 1:
                eng.assign(C_l)   # ends this rank's state to continue from
            rejected("dis_state", lambda: eng.refine(max_iters=40, eps=0.0))
            eng.lbg(bits)
            refine("dis_after", max_iters=40, eps=0.0)
        else:
            raise SystemExit("unknown step " + step)
    np.savez(out, **res)
    eng.close()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
