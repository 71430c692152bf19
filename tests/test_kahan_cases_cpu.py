"""The Kahan chain case table measured on the CPU (no GPU).

Every case of tests/helpers/kahan_cases.py goes through the restatement of the device's
evaluation (tests/cpp/test_kahan_chain.cpp in file mode: the zero-skipping transient, the block,
8-segment and segment functions, the replays), which prints per chain what its evaluation did.
Here: every chain returns the bits of the sequential chain (whole and in the case's pieces), and
every claim of the table holds on those numbers -- so a later change of L, SPB, NE or the direct
threshold cannot leave a case silently short of its branch.  The constants the table was sized
for are held to the sources, and the sort's key windows (qvq_host_kahan_sort_plan) are covered."""
import os
import re
import struct
import subprocess

import numpy as np
import pytest

from helpers import kahan_cases as kc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "quant_amd", "csrc")
OPS = {"==": lambda a, b: a == b, ">": lambda a, b: a > b, ">=": lambda a, b: a >= b, "<": lambda a, b: a < b}


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("kahan_cases") / "test_kahan_chain")
    r = subprocess.run(["g++", "-O2", "-std=c++17", "-I", CSRC, "-o", out,
                        os.path.join(ROOT, "tests", "cpp", "test_kahan_chain.cpp")],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    return out


def _run(exe, tmp_path, chains):
    """chains: [(ordinals, local cuts or None)] -> ([KCHAIN dict], [KSPLIT dict])."""
    cut = chains[0][1] is not None
    with open(tmp_path / "chains.bin", "wb") as f, open(tmp_path / "cuts.bin", "wb") as g:
        f.write(struct.pack("<I", len(chains)))
        g.write(struct.pack("<I", len(chains)))
        for u, cuts in chains:
            b = (np.asarray(u, np.uint8) ^ 0x80).tobytes()
            f.write(struct.pack("<I", len(b)) + b)
            if cut:
                g.write(struct.pack("<I", len(cuts)) + np.asarray(cuts, "<u4").tobytes())
    args = [exe, str(tmp_path / "chains.bin")] + ([str(tmp_path / "cuts.bin")] if cut else [])
    r = subprocess.run(args, capture_output=True, text=True, timeout=600, env=dict(os.environ, KCHAIN="1"))
    assert r.returncode == 0 and "mismatches 0" in r.stdout, r.stdout[-3000:] + r.stderr
    lines = {"KCHAIN": [], "KSPLIT": []}
    for ln in r.stdout.splitlines():
        w = ln.split()
        if w and w[0] in lines:
            d = {w[i]: int(w[i + 1]) for i in range(2, len(w), 2)}
            d["index"] = int(w[1])
            lines[w[0]].append(d)
    assert len(lines["KCHAIN"]) == len(chains) and len(lines["KSPLIT"]) == (len(chains) if cut else 0)
    return lines


def test_constants_match_the_sources():
    hdr = open(os.path.join(CSRC, "kahan_par.hpp")).read()
    hip = open(os.path.join(CSRC, "k_kahan.hip")).read()

    def const(src, pat):
        return int(re.search(pat, src).group(1))
    assert const(hdr, r"constexpr uint32_t L = (\d+);") == kc.L
    assert const(hdr, r"constexpr uint32_t SPB = (\d+);") == kc.SPB
    assert const(hdr, r"constexpr int NE = (\d+);") == kc.NE
    assert const(hip, r"constexpr int WPB = (\d+);") == kc.WPB
    assert const(hip, r"\(uint64_t\)w\.blk_cap \* D \+ WPB - 1\) / WPB, (\d+)\)") == kc.GRID_CAP
    assert const(hip, r'"QVQ_KAHAN_DIRECT_MAX"\), nullptr, 10\)\s*:\s*(\d+);') == kc.DIRECT_MAX
    assert "if (j % 8 == 0)" in hip   # the 8-segment tier the length cases' 511 / 512 / 513 sit at


@pytest.mark.parametrize("name", [n for n in kc.CASES if n != "lengths_short_cuts"])
def test_case_claims_hold_on_the_restatement(exe, tmp_path, name):
    c = kc.case(name)
    chains = c.chains()
    lines = _run(exe, tmp_path, [(u, cuts) for _, _, u, cuts in chains])
    at = {(k, d): i for i, (k, d, _, _) in enumerate(chains)}
    for kind in ("KCHAIN", "KSPLIT"):
        for ln in lines[kind]:
            assert ln["ok"] == 1, (name, kind, ln)
    for k, d, kind, field, op, val in c.checks:
        got = lines[kind][at[(k, d)]][field]
        print("%s cell %d component %d %s %s = %d (claim %s %d)" % (name, k, d, kind, field, got, op, val))
        assert OPS[op](got, val), (name, k, d, kind, field, got, op, val)
    # the route the device must take, from the cells' lengths
    longest = max(len(ch[0]) for ch in c.cells.values())
    assert c.route == (kc.ROUTE_FUNCTIONS if longest > kc.DIRECT_MAX else kc.ROUTE_DIRECT)
    for key, (op, val) in list(c.device.items()) + list(c.totals.items()):
        field = {"block_misses": "miss", "replays": "replays", "blocks_not_composable": "bad"}.get(key, key)
        tot = sum(ln[field] for ln in lines["KCHAIN"])
        print("%s total %s = %d (claim %s %d)" % (name, field, tot, op, val))
        assert OPS[op](tot, val), (name, key, tot)


def test_block_miss_then_block_hit_occurs(exe, tmp_path):
    """The three-tier walk's claims over the table: some chain has a block function that does not
    answer and a later one that does (miss < blocks, miss > 0 on a chain of several blocks), some
    chain is answered by 8-segment functions, some replays segments, some composes no block."""
    seen = dict(miss_then_hit=0, hit8=0, replays=0, bad=0, treplay=0)
    for name in ("kinds_4134", "kinds_12289", "lengths_blocks", "long_scatter"):
        c = kc.case(name)
        for ln in _run(exe, tmp_path, [(u, None) for _, _, u, _ in c.chains()])["KCHAIN"]:
            seen["miss_then_hit"] += ln["blocks"] >= 3 and 0 < ln["miss"] < ln["blocks"] - 1
            seen["hit8"] += ln["hit8"] > 0
            seen["replays"] += ln["replays"] > 0
            seen["bad"] += ln["bad"] > 0
            seen["treplay"] += ln["treplay"] > 0
    print(seen)
    assert all(v > 0 for v in seen.values()), seen


def test_two_ranks_at_every_cut_of_the_short_cells(exe, tmp_path):
    c = kc.case("lengths_short_cuts")
    chains = []
    for _, _, u, _ in c.chains():
        chains += [(u, [0, p, len(u)]) for p in range(len(u) + 1)]
    _run(exe, tmp_path, chains)


def test_split_cases_are_the_cases_with_cuts():
    assert set(kc.SPLIT_CASES) == {n for n in kc.CASES if kc.case(n).cut_lists}


def test_layout_keeps_each_cells_order():
    c = kc.case("kinds_4134")
    codes, A = c.layout
    assert A.size == c.n and np.count_nonzero(np.diff(A.astype(np.int64))) > c.n // 4   # interleaved
    for k, d, u, _ in c.chains():
        np.testing.assert_array_equal(codes[A == k, d] ^ 0x80, u)
    for cuts in kc.case("transient").cuts() + c.cuts():
        assert cuts[0] == 0 and np.all(np.diff(cuts.astype(np.int64)) >= 0)
    assert c.cuts()[0][-1] == c.n


@pytest.mark.parametrize("K,windows", [(1, 1), (16384, 1), (16385, 1), (40960, 1), (40961, 2), (65536, 2),
                                        (81920, 2), (81921, 3), (1 << 20, 26)])
def test_sort_windows(K, windows):
    """The sort's LDS counters: at most 160 KB a workgroup, so K keys take ceil(K / 40960) windows."""
    import quant_amd
    p = quant_amd.host_kahan_sort_plan(K)
    assert p["window_keys"] * 4 == 160 * 1024
    assert p["windows"] == windows == -(-K // p["window_keys"])
    assert p["lds_bytes"] == 4 * min(K, p["window_keys"]) <= 160 * 1024


def test_sort_plan_rejects_no_keys():
    import quant_amd
    with pytest.raises(quant_amd.QVQError):
        quant_amd.host_kahan_sort_plan(0)
