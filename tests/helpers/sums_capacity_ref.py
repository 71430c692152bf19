"""Who adds what in mean_sums_kernel (quant_amd/csrc/k_misc.hip), restated on the CPU.

The kernel adds every component's exact term in 16-bit register fields and counts nothing: a field
holds FIELD_MAX // U_MAX = 257 adds of u = 255, and the launcher's grid (mean_plan.hpp, reported by
quant_amd.host_mean_grid) is what keeps every thread within them.  A plan here is that dict.

Three statements of the same mapping, from the literal to the closed form:

  simulate(n, dp, plan)          the three loops as the kernel runs them, thread by thread and 4-byte
                                 code word by code word (small n and grids only): how often every word
                                 of the training set was added, and every thread's adds per register slot
  adds_per_thread(n, dp, plan)   every thread's adds to one field, by arithmetic (numpy, any n)
  max_adds(n, dp, plan)          the busiest thread's: thread 0 of block 0, O(1)

A row adds once to every field of its thread, so one number per thread serves every field."""
import numpy as np

U_MAX = 255          # b ^ 0x80 at most (byte 0x7F, the value 1.0 of SCALED)
FIELD_MAX = 65535    # a 16-bit field
WAVE = 64


def parent_blocks(n):
    """The grid before the launcher counted adds: a block per 1024 * 256 rows, one per CU (256) below."""
    return max(-(-n // (1024 * 256)), 1, min(-(-n // 4096), 256))


def with_blocks(plan, blocks):
    return dict(plan, blocks=int(blocks))


def _check_plan(dp, plan):
    # what the restatement takes from the kernel's text and not from the plan: a group is the 4 rows
    # of dp / 4 16-byte loads, a chunk one group per lane of a wave
    assert dp % 4 == 0 and 4 <= dp <= 64
    assert plan["group_rows"] == 4 and plan["chunk_groups"] == WAVE and plan["block"] % WAVE == 0
    assert plan["chunk_loop"] == (dp <= 16)


def simulate(n, dp, plan):
    """-> (words [n, dp / 4]: times each 4-byte code word was added, adds [blocks * block, dp / 4]:
    each thread's adds per register slot)."""
    _check_plan(dp, plan)
    Q = dp // 4
    blocks, T, G, CG = plan["blocks"], plan["block"], plan["group_rows"], plan["chunk_groups"]
    groups = n // G
    words = np.zeros(n * Q, np.int64)
    adds = np.zeros((blocks * T, Q), np.int64)
    for b in range(blocks):
        for t in range(T):
            x, lane = b * T + t, t % WAVE
            g_begin = 0
            if plan["chunk_loop"]:
                chunks = groups // CG
                nwaves = blocks * (T // WAVE)
                U = plan["chunks_in_flight"]
                c = b * (T // WAVE) + t // WAVE
                while c < chunks:
                    for u in range(U):
                        if u > 0 and c + u * nwaves >= chunks:
                            break
                        first = (c + u * nwaves) * CG * G * Q   # the chunk's first 4-byte word
                        for j in range(Q):                      # 16-byte load j of the lane
                            for k in range(4):
                                w = first + 4 * (WAVE * j + lane) + k
                                slot = (256 * j + k) % Q
                                assert (slot + 4 * lane) % Q == w % Q   # the rotation at the loop's end
                                words[w] += 1
                                adds[x, slot] += 1
                    c += U * nwaves
                g_begin = chunks * CG
            U = plan["groups_in_flight"]
            stride = blocks * T
            g = g_begin + x
            while g < groups:
                for u in range(U):
                    if u > 0 and g + u * stride >= groups:
                        break
                    first = (g + u * stride) * G * Q
                    for i in range(G * Q):
                        words[first + i] += 1
                        adds[x, i % Q] += 1
                g += U * stride
            if b == 0 and t < n % G:
                for q in range(Q):
                    words[(groups * G + t) * Q + q] += 1
                    adds[x, q] += 1
    return words.reshape(n, Q), adds


def adds_per_thread(n, dp, plan):
    """int64 [blocks * block]: every thread's adds to one field."""
    _check_plan(dp, plan)
    blocks, T, G, CG = plan["blocks"], plan["block"], plan["group_rows"], plan["chunk_groups"]
    x = np.arange(blocks * T, dtype=np.int64)
    groups = n // G
    out = np.zeros(blocks * T, np.int64)
    left = groups
    if plan["chunk_loop"]:
        chunks, nwaves = groups // CG, blocks * (T // WAVE)
        out += G * np.maximum(0, -(-(chunks - x // WAVE) // nwaves))   # chunks wave, wave + nwaves, ...
        left = groups - chunks * CG
    out += G * np.maximum(0, -(-(left - x) // (blocks * T)))           # groups x, x + stride, ...
    out += x < n % G
    return out


def max_adds(n, dp, plan):
    """The busiest thread's adds to one field: thread 0 of block 0 (first in every loop's order)."""
    _check_plan(dp, plan)
    blocks, T, G, CG = plan["blocks"], plan["block"], plan["group_rows"], plan["chunk_groups"]
    groups = n // G
    a, left = 0, groups
    if plan["chunk_loop"]:
        chunks = groups // CG
        a += G * -(-chunks // (blocks * (T // WAVE)))
        left = groups - chunks * CG
    return a + G * -(-left // (blocks * T)) + (1 if n % G else 0)


def fits(n, dp, plan):
    return U_MAX * max_adds(n, dp, plan) <= FIELD_MAX
