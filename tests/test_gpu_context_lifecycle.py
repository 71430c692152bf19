"""One context through every lifetime transition of the buffers it owns (the steps
are tests/helpers/lifecycle_cases.py's): after each step the codebook, indices and distortion are
bit for bit those of a fresh context that ran only that step, and pass the oracle comparison of
tests/test_gpu_parity.py (byte sets), tests/test_gpu_cie_raster.py (exact sets) and
tests/test_gpu_reseed.py (qvq_refine).  The other Kahan schedules (QVQ_SPECULATE=0: two assignment
buffers swapped per level; QVQ_KAHAN=0: one) run the same sequence in a process of their own, since
the engine reads those switches once.  A second case holds the context to returning what it
allocates."""
import ctypes
import json
import os
import subprocess
import sys

import pytest

import quant_amd
from helpers import lifecycle_cases as lc

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def default_paths(monkeypatch):
    for name in ("QVQ_SEARCH", "QVQ_KDTREE"):
        monkeypatch.delenv(name, raising=False)


def test_every_transition_matches_a_fresh_context():
    """The default schedule: speculative Kahan levels, four assignment buffers in rotation."""
    import torch   # noqa: F401  (torch's bundled HIP runtime opens the device first: quant_amd.Engine)
    with quant_amd.Engine(0) as eng:
        lc.run_sequence(eng)


@pytest.mark.parametrize("env,rule", [({"QVQ_SPECULATE": "0"}, "kahan"), ({"QVQ_KAHAN": "0"}, "exact-sum")],
                         ids=["speculate0", "kahan0"])
def test_every_transition_under_the_other_schedules(env, rule):
    r = subprocess.run([sys.executable, os.path.abspath(lc.__file__), rule], env=dict(os.environ, **env),
                       capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert json.loads(r.stdout.strip().splitlines()[-1]) == {"ok": True, "steps": len(lc.STEPS)}


def test_memory_is_steady_and_returned():
    """Three cycles of the first five steps on one context: free device memory (hipMemGetInfo)
    after the third cycle equals that after the second (nothing leaks, nothing that fits is
    allocated again), and after close() it is back at the reading taken before the context was
    created.  Allowance: 0 bytes -- the parent commit's own readings on this sequence were exactly
    steady and exactly returned."""
    import torch
    torch.cuda.init()   # (torch's bundled HIP runtime opens the device first: quant_amd.Engine)
    # the readings come from the HIP runtime the engine's calls go to: the one copy this process
    # has loaded, or, next to torch's bundled copy, the other one
    quant_amd.lib()
    with open("/proc/self/maps") as f:
        loaded = sorted({line.split()[-1] for line in f if "libamdhip64" in line})
    own = [path for path in loaded if os.sep + "torch" + os.sep not in path] or loaded
    assert len(own) == 1, loaded
    hip = ctypes.CDLL(own[0])

    def free_bytes():
        free, total = ctypes.c_size_t(), ctypes.c_size_t()
        assert hip.hipDeviceSynchronize() == 0
        assert hip.hipMemGetInfo(ctypes.byref(free), ctypes.byref(total)) == 0
        return free.value

    with quant_amd.Engine(0) as warm:   # code objects loaded, the runtime's own pools made
        resident = None
        for step in lc.CYCLE:
            resident = lc.run_step(warm, step, resident)[0]
    before = free_bytes()
    eng = quant_amd.Engine(0)
    after_cycle = []
    for _ in range(3):
        resident = None
        for step in lc.CYCLE:
            resident = lc.run_step(eng, step, resident)[0]
        after_cycle.append(free_bytes())
    eng.close()
    closed = free_bytes()
    print("free bytes: before", before, "after cycles", after_cycle, "closed", closed)
    assert after_cycle[2] == after_cycle[1]
    assert closed == before
