"""The case table of qvq_lbg_lloyd's tests (tests/test_lbg_lloyd_cpu.py, tests/test_gpu_lbg_lloyd.py):
synthetic rasters (oracle.gen_image of side S), tiled in b x b blocks under a colour space, with the
schedule's bits, iterations per level, eps and reseed flag.  Chosen as the smallest shapes whose
levels still reach every search, recheck and update path the engine has (test_levels_reach_every_path
asserts that through quant_amd.host_plan)."""
import collections

NORMAL, SCALED = 0, 1

Case = collections.namedtuple("Case", "S block bits cs iters eps reseed")

# the shapes qvq_lbg is compared on (iters = 1), in both colour spaces
LBG_SHAPES = [(64, 2, 4), (128, 2, 6), (96, 4, 5)]

CASES = {}
for _S, _b, _bits in LBG_SHAPES:
    for _cs, _n in ((SCALED, "scaled"), (NORMAL, "normal")):
        CASES["s%d_b%d_%d_%s_i1" % (_S, _b, _bits, _n)] = Case(_S, _b, _bits, _cs, 1, 0.0, False)
    CASES["s%d_b%d_%d_scaled_i3" % (_S, _b, _bits)] = Case(_S, _b, _bits, SCALED, 3, 0.0, False)
CASES.update({
    # small K -> MFMA fused -> MFMA pruned (K >= 256)
    "s256_b2_9_scaled_i3": Case(256, 2, 9, SCALED, 3, 0.0, False),
    # D = 48: the wide search resident, then pruned (K >= 1024); K = 2048 over 4096 rows
    "s256_b4_11_scaled_i3": Case(256, 4, 11, SCALED, 3, 0.0, False),
    # D = 3, pad width 4, N = 2500 (no multiple of 64)
    "s50_b1_5_scaled_i3": Case(50, 1, 5, SCALED, 3, 0.0, False),
    # K = 128 over 64 rows
    "s16_b2_7_scaled_i3": Case(16, 2, 7, SCALED, 3, 0.0, False),
    # K = 32768 over 2500 rows: past the counting sort's capacity (the LDS sums pass) and the
    # staged rechecks (the recheck from global memory)
    "s50_b1_15_scaled_i2": Case(50, 1, 15, SCALED, 2, 0.0, False),
    # eps stops levels before iters: [3, 3, 6, 6, 6, 6] iterations
    "s128_b2_6_scaled_eps": Case(128, 2, 6, SCALED, 6, 0.01, False),
    # empty cells: without the flag 337 at the last level
    "s128_b2_10_scaled_eps": Case(128, 2, 10, SCALED, 6, 0.01, False),
    "s128_b2_10_scaled_eps_reseed": Case(128, 2, 10, SCALED, 6, 0.01, True),
    "s128_b2_8_normal_i3_reseed": Case(128, 2, 8, NORMAL, 3, 0.0, True),
})

I1_CASES = [n for n, c in CASES.items() if c.iters == 1]
ITER_CASES = [n for n, c in CASES.items() if c.iters in (2, 3) and c.eps == 0 and not c.reseed]
EPS_CASES = [n for n, c in CASES.items() if c.eps > 0]
RESEED_CASES = [n for n, c in CASES.items() if c.reseed]
