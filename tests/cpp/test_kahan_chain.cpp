// CPU check of the segment-parallel Kahan evaluator (quant_amd/csrc/kahan_par.hpp): for chains of
// many kinds, the pipeline the device runs (segment metadata, prefix sums, segment functions,
// 64-segment block composites, the checked evaluation with replays) must return the bits of the
// reference's sequential sumInArea (src/Quantizer.cpp:59-70).  Prints one summary line; exit
// status 1 on any mismatch.
//   test_kahan_chain [reps]            random chains
//   test_kahan_chain /path/chains.bin [/path/cuts.bin]
//       chains from a file ([u32 count] then per chain [u32 n][n bytes]); with cuts ([u32 count]
//       then per chain [u32 m][m u32 offsets from 0 to n]) each chain is also evaluated in those
//       pieces.  With KCHAIN set: a line "KCHAIN index n ... ok 0|1" per chain of what its
//       evaluation did (struct Info), and "KSPLIT ..." for the pieces.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <algorithm>
#include <vector>

#include "kahan_par.hpp"

using namespace qvq::kahan;

static double scaled(int b) { return ((double)(signed char)(unsigned char)b + 128.0) * (1.0 / 255); }

static double kahan_ref(const std::vector<uint8_t> &b, const ByteTab &tb) {
    double sum = 0, c = 0;
    for (uint8_t v : b) {
        double y = ldexp((double)tb.X[v], -60) - c;
        double t = sum + y;
        c = (t - sum) - y;
        sum = t;
    }
    return sum;
}

struct Stats {
    uint64_t segs = 0, raw = 0, blocks = 0, blk_bad = 0, blk_miss = 0, hit8 = 0, replays = 0;
};

// What one chain's evaluation did (summed over its pieces when it is split).
struct Info {
    uint32_t segs = 0, blocks = 0, raw = 0, bad = 0;   // segments, blocks, raw functions, blocks not composable
    uint32_t miss = 0, hit8 = 0, replays = 0;           // block functions that did not answer (raw ones included),
                                                        // 8-segment functions that did, segments replayed
    uint32_t treplay = 0;    // the transient ended inside a segment: a replay to the next boundary
    uint32_t tau = 0;        // the step (of the whole chain) at which the transient ended; n: never
    uint32_t left = 0;       // sum reached 2
    uint32_t skipped = 0;    // zero segments the transient skipped (c = 0)
    uint32_t held = 0;       // zero segments it stepped through because c != 0
    uint32_t gate_c = 0;     // pieces of zeros entered only because c != 0 with sum < 2
    uint32_t edge8 = 0;      // 8-segment hits that end a block the walk entered inside (the transient ended
                             // there): the next block's function has not been fetched by a block's start
};

// ks_eval_kernel (k_kahan.hip) on one piece of a chain, serially: the piece's n bytes pb, the
// exact prefix P0 at its first step, the state (sum, c) entering it (updated); at: the piece's
// offset in the chain (for tau).  The functions are the build kernel's: each segment's with the
// piece's own metadata, a tree over each block's 64 with the 8-segment functions taken at depth 3.
static void eval_piece(const ByteTab &tb, const uint8_t *pb, uint32_t n, u128 P0, uint32_t at, double &sum, double &c,
                       u128 &Pout, Info &in) {
    Pout = P0;
    if (n == 0) return;
    const uint32_t nseg = (n + L - 1) / L, nblk = (nseg + SPB - 1) / SPB;
    std::vector<SegMeta> meta(nseg);
    std::vector<u128> P(nseg + 1);
    P[0] = P0;
    for (uint32_t j = 0; j < nseg; j++) {
        meta[j] = seg_meta(tb, pb + j * L, std::min(L, n - j * L));
        P[j + 1] = P[j] + meta_sum(meta[j]);
    }
    const u128 Pn = P[nseg];
    Pout = Pn;
    std::vector<SegFn> segfn(nseg);
    std::vector<Fn> bf(nblk), bf8((size_t)nblk * 8);
    for (uint32_t bi = 0; bi < nblk; bi++) {
        const uint32_t s0 = bi * SPB, cnt = std::min(SPB, nseg - s0);
        std::vector<Fn> f(SPB);
        std::vector<bool> ok(SPB, false);
        for (uint32_t i = 0; i < cnt; i++) {
            const uint32_t j = s0 + i;
            int c_in;
            uint32_t off_in;
            input_structure([&](int q) { return meta[j - q]; }, (int)std::min<uint32_t>(8, j), c_in, off_in);
            build_fn(tb, pb + j * L, std::min(L, n - j * L), P[j], meta[j], c_in, off_in, j + 1 == nseg, 0, f[i]);
            pack_seg(f[i], segfn[j]);
            ok[i] = fkind(f[i]) != FK_RAW;
            in.segs++;
            in.raw += !ok[i];
        }
        for (uint32_t st = 1; st < SPB; st <<= 1) {
            for (uint32_t i = 0; i + st < cnt; i += 2 * st) {
                Fn h;
                const bool cmp = ok[i] && ok[i + st] && compose(f[i], f[i + st], h);
                ok[i] = cmp;
                if (cmp) f[i] = h;
            }
            if (st == 4)
                for (uint32_t i = 0; i < cnt; i += 8) {
                    Fn r = f[i];
                    if (!ok[i]) set_raw(r);
                    bf8[(size_t)bi * 8 + i / 8] = r;
                }
        }
        bf[bi] = f[0];
        if (!ok[0]) set_raw(bf[bi]);
        in.blocks++;
        in.bad += !ok[0];
    }
    // nothing to add: every value 0 while c = 0, or with sum >= 2 (a zero step is then exact)
    if (!(Pn != P0 || (c != 0.0 && !(sum >= 2.0)))) return;
    in.gate_c += Pn == P0;
    uint32_t i = 0;
    u128 Pt = P0;
    const bool was_in = !(sum >= 2.0);
    while (i < n && !(sum >= 2.0)) {
        const uint32_t b = i / (L * SPB);
        if (i % L == 0) {
            if (c == 0) {   // zero segments skipped, to the block's end at most
                uint32_t s = i / L;
                const uint32_t se = std::min(nseg, (b + 1) * SPB);
                while (s < se && meta_sum(meta[s]) == 0) s++;
                in.skipped += s - i / L;
                if (s == se) {
                    i = std::min(n, (b + 1) * L * SPB);
                    continue;
                }
                i = s * L;
            } else if (meta_sum(meta[i / L]) == 0) in.held++;
        }
        const uint32_t e = std::min(n, (i / L + 1) * L);
        while (i < e && !(sum >= 2.0)) {
            fstep(sum, c, ldexp((double)tb.X[pb[i]], -60));
            Pt += tb.X[pb[i]];
            i++;
        }
    }
    if (was_in) in.tau = at + i;
    if (!(sum >= 2.0)) return;
    if (was_in) in.left = 1;
    const u128 E = (u128)(to_units(sum) - to_units(c));
    int64_t D = (int64_t)(E - Pt);
    uint32_t F = (uint32_t)E & 511;
    uint32_t j = (i + L - 1) / L;
    if (i % L) {   // to the next boundary, exactly
        D += replay(tb, pb + i, std::min(n, j * L) - i, Pt, F, D);
        in.treplay++;
    }
    const uint32_t j0 = j;
    while (j < nseg) {
        if ((uint32_t)((P[j] + (u128)(i128)D) & 511) != F) abort();   // state consistency
        if (j % SPB == 0) {
            if (apply(bf[j / SPB], F, D)) {
                j = std::min(nseg, j + SPB);
                continue;
            }
            in.miss++;
        }
        if (j % 8 == 0 && apply(bf8[j / 8], F, D)) {
            j = std::min(nseg, j + 8);
            in.hit8++;
            in.edge8 += j % SPB == 0 && j < nseg && j0 % SPB != 0 && (j - 1) / SPB == j0 / SPB;
            continue;
        }
        const uint32_t end = std::min(nseg, (j / 8 + 1) * 8);
        for (; j < end; j++) {
            Fn f;
            unpack_seg(segfn[j], f);
            if (apply(f, F, D)) continue;
            in.replays++;
            D += replay(tb, pb + j * L, std::min(L, n - j * L), P[j], F, D);
        }
    }
    // the state is E = Pn + D exactly: sum = RN(E), c = sum - E
    const u128 Ef = Pn + (u128)(i128)D;
    sum = to_double(Ef);
    c = ldexp((double)(int64_t)(to_units(sum) - (i128)Ef), -60);
}

static void add(Stats &st, const Info &in) {
    st.segs += in.segs, st.raw += in.raw, st.blocks += in.blocks, st.blk_bad += in.bad;
    st.blk_miss += in.miss, st.hit8 += in.hit8, st.replays += in.replays + in.treplay;
}

// The device pipeline on one chain, serially.
static double run_chain(const std::vector<uint8_t> &b, const ByteTab &tb, Stats &st, Info &in) {
    double sum = 0, c = 0;
    u128 Pout;
    in = Info();
    in.tau = (uint32_t)b.size();
    eval_piece(tb, b.data(), (uint32_t)b.size(), 0, 0, sum, c, Pout, in);
    add(st, in);
    return sum;
}

// The chained evaluation (k_kahan.hip, several ranks): the chain split at cuts into pieces, each
// piece's segment functions built with the global exact prefix, each piece evaluated from the
// state (sum, c) the previous piece left -- rank by rank, as engine.cpp's relay runs it.
static double run_chain_split(const std::vector<uint8_t> &b, const std::vector<uint32_t> &cuts, const ByteTab &tb,
                              Stats &st, Info &in) {
    double sum = 0, c = 0;
    u128 P0 = 0;
    in = Info();
    in.tau = (uint32_t)b.size();
    for (size_t r = 0; r + 1 < cuts.size(); r++) {
        u128 Pout;
        eval_piece(tb, b.data() + cuts[r], cuts[r + 1] - cuts[r], P0, cuts[r], sum, c, Pout, in);
        P0 = Pout;
    }
    add(st, in);
    return sum;
}

static void print_info(const char *tag, size_t idx, size_t n, const Info &in, bool ok) {
    printf("%s %zu n %zu segs %u blocks %u raw %u bad %u miss %u hit8 %u replays %u treplay %u tau %u left %u "
           "skipped %u held %u gate_c %u edge8 %u ok %d\n",
           tag, idx, n, in.segs, in.blocks, in.raw, in.bad, in.miss, in.hit8, in.replays, in.treplay, in.tau, in.left,
           in.skipped, in.held, in.gate_c, in.edge8, (int)ok);
}

// cuts (file mode): this chain's cut offsets 0 = cuts[0] <= ... <= cuts.back() = n; without them
// the chain is split at random cuts.  idx >= 0: a parseable KCHAIN (and KSPLIT) line per chain.
static int check(const std::vector<uint8_t> &b, const ByteTab &tb, Stats &st, const char *what, long idx = -1,
                 const std::vector<uint32_t> *cuts_in = nullptr) {
    const double ref = kahan_ref(b, tb);
    Info in;
    const double got = run_chain(b, tb, st, in);
    const bool ok = memcmp(&ref, &got, 8) == 0;
    if (idx >= 0) print_info("KCHAIN", (size_t)idx, b.size(), in, ok);
    if (!ok) {
        printf("MISMATCH %s n %zu: ref %.17g got %.17g\n", what, b.size(), ref, got);
        return 1;
    }
    const uint32_t n = (uint32_t)b.size();
    if (cuts_in) {
        if (cuts_in->size() < 2 || cuts_in->front() != 0 || cuts_in->back() != n ||
            !std::is_sorted(cuts_in->begin(), cuts_in->end()))
            return 1;
        const double got2 = run_chain_split(b, *cuts_in, tb, st, in);
        const bool ok2 = memcmp(&ref, &got2, 8) == 0;
        if (idx >= 0) print_info("KSPLIT", (size_t)idx, b.size(), in, ok2);
        if (!ok2) printf("MISMATCH (cuts) %s n %zu: ref %.17g got %.17g\n", what, b.size(), ref, got2);
        return ok2 ? 0 : 1;
    }
    // the same chain split over 2..9 "ranks" at random cuts (some early: inside the transient,
    // some empty pieces), each piece evaluated from the state the previous one left
    static std::mt19937_64 rng(777);
    for (int rep = 0; rep < 3; rep++) {
        const int pieces = 2 + (int)(rng() % 8);
        std::vector<uint32_t> cuts = {0, n};
        for (int p = 1; p < pieces; p++) {
            const uint64_t r = rng();
            cuts.push_back(r % 4 == 0 ? (uint32_t)(r % std::min<uint32_t>(n + 1, 300)) : (uint32_t)(r % (n + 1)));
        }
        std::sort(cuts.begin(), cuts.end());
        const double got2 = run_chain_split(b, cuts, tb, st, in);
        if (memcmp(&ref, &got2, 8) != 0) {
            printf("MISMATCH (split %d) %s n %zu: ref %.17g got %.17g\n", pieces, what, b.size(), ref, got2);
            return 1;
        }
    }
    return 0;
}

static void report(const char *what, int cases, int bad, const Stats &st) {
    printf("%s: cases %d mismatches %d | segments %llu raw %llu | blocks %llu not composable %llu missed %llu | "
           "8-segment hits %llu replays %llu\n",
           what, cases, bad, (unsigned long long)st.segs, (unsigned long long)st.raw, (unsigned long long)st.blocks,
           (unsigned long long)st.blk_bad, (unsigned long long)st.blk_miss, (unsigned long long)st.hit8,
           (unsigned long long)st.replays);
}

int main(int argc, char **argv) {
    uint64_t Xt[256];
    for (int b = 0; b < 256; b++) Xt[b] = (uint64_t)ldexp(scaled(b), 60);
    static ByteTab tb;
    make_tab(Xt, tb);
    Stats st;
    int bad = 0, cases = 0;
    if (argc > 1 && argv[1][0] == '/') {
        FILE *fp = fopen(argv[1], "rb");
        FILE *fc = argc > 2 ? fopen(argv[2], "rb") : nullptr;
        if (!fp || (argc > 2 && !fc)) return 2;
        uint32_t nc = 0, ncc = 0;
        if (fread(&nc, 4, 1, fp) != 1) return 2;
        if (fc && (fread(&ncc, 4, 1, fc) != 1 || ncc != nc)) return 2;
        for (uint32_t i = 0; i < nc; i++) {
            uint32_t n = 0, m = 0;
            if (fread(&n, 4, 1, fp) != 1) return 2;
            std::vector<uint8_t> b(n);
            if (n && fread(b.data(), 1, n, fp) != n) return 2;
            std::vector<uint32_t> cuts;
            if (fc) {
                if (fread(&m, 4, 1, fc) != 1 || m < 2 || m > n + 2 + 64) return 2;
                cuts.resize(m);
                if (fread(cuts.data(), 4, m, fc) != m) return 2;
            }
            bad += check(b, tb, st, "file", getenv("KCHAIN") ? (long)i : -1, fc ? &cuts : nullptr);
            cases++;
        }
        report(argv[1], cases, bad, st);
        return bad ? 1 : 0;
    }
    const int reps = argc > 1 ? atoi(argv[1]) : 200;
    std::mt19937_64 rng(12345);
    // byte codes: code b has value (int8(b) + 128)/255, so u = b ^ 0x80 is the value index
    auto code = [](int u) { return (uint8_t)(u ^ 0x80); };
    for (int rep = 0; rep < reps; rep++) {
        const int kind = rep % 10;
        uint64_t n;
        if (rep % 5 == 0) n = 1 + rng() % 50;
        else if (rep % 5 == 1) n = 1 + rng() % 5000;
        else if (rep % 5 == 2) n = 1 + rng() % 200000;
        else n = 1 + rng() % 600000;
        std::vector<uint8_t> b(n);
        const int lo = (int)(rng() % 256), span = 1 + (int)(rng() % 40);
        const uint64_t period = 50 + rng() % 20000;
        for (uint64_t i = 0; i < n; i++) {
            int u;
            switch (kind) {
            case 0: u = (int)(rng() % 256); break;                                  // noise
            case 1: u = (rng() % 4 == 0) ? 255 : (int)(rng() % 256); break;          // saturated
            case 2: u = (int)(rng() % 8); break;                                     // dark
            case 3: u = std::min(255, lo + (int)(rng() % span)); break;             // narrow band
            case 4: u = (rng() % 3 == 0) ? 0 : (int)(rng() % 256); break;            // zeros
            case 5: u = 255; break;                                                  // flat 1.0
            case 6: u = (rng() % 2) ? 255 : 128 + (int)(rng() % 8); break;           // 1.0 and mid
            case 7: u = (int)(64 + rng() % 64); break;                               // [0.25, 0.5)
            case 8: u = ((i / period) % 2) ? (int)(rng() % 4) : (int)(128 + rng() % 128); break;   // dark/bright regions
            default: u = ((i / period) % 3 == 0) ? 0 : ((i / period) % 3 == 1) ? (int)(rng() % 6) : 255; break;
            }
            b[i] = code(u);
        }
        char what[64];
        snprintf(what, sizeof(what), "rep %d kind %d", rep, kind);
        bad += check(b, tb, st, what);
        cases++;
    }
    report("random", cases, bad, st);
    return bad ? 1 : 0;
}
