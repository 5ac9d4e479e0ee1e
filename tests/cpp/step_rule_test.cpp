// The host arithmetic of the step path (emba_amd/csrc/step_rule.h) on a CPU: the layout of the pack, the boolean rules on both sides of every size threshold and
// under every option value the GPU tests set, a sweep of the Gram launch's plan over its properties, and the plan at the shapes of DESIGN.md §6 as the
// expressions of emba_form_accumulate gave it before they moved into gram_plan (evaluated once from that commit, written here as literals).
// Prints "OK ..." and returns 0, or names what failed.
#include "../../emba_amd/csrc/step_rule.h"

#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace emba;

namespace {

int g_fail = 0;
#define CHECK(cond, ...)                                          \
    do {                                                          \
        if (!(cond)) {                                            \
            if (++g_fail <= 20) {                                 \
                std::printf("FAIL %s:%d: %s -- ", __FILE__, __LINE__, #cond); \
                std::printf(__VA_ARGS__);                         \
                std::printf("\n");                                \
            }                                                     \
        }                                                         \
    } while (0)

// kernels.h (tests/test_cpp_host.py passes the current values; the sweeps run with them, the literal answers were taken with these defaults)
#ifndef GRAM_BLOCK
#define GRAM_BLOCK 1024
#endif
#ifndef GRAM_CHUNK
#define GRAM_CHUNK 1024
#endif
#ifndef GRAM_CHUNK_MIN
#define GRAM_CHUNK_MIN 64
#endif
#ifndef EP_TAIL_BLK
#define EP_TAIL_BLK 4096
#endif
#ifndef REC_STRIDE
#define REC_STRIDE 16
#endif
#ifndef GATHER_MAX_UNITS
#define GATHER_MAX_UNITS 4096
#endif

constexpr GramSizes kSizes{GRAM_BLOCK, GRAM_CHUNK, GRAM_CHUNK_MIN, EP_TAIL_BLK};
constexpr bool kDefaultSizes = GRAM_BLOCK == 1024 && GRAM_CHUNK == 1024 && GRAM_CHUNK_MIN == 64 && EP_TAIL_BLK == 4096;

void check_pack_layout()
{
    // K = 21: A11 is 63 x 63 = 3969 doubles, b1 63 more: the rows begin at 4032
    const PackLayout p21(21);
    CHECK(p21.b1 == 3969 && p21.A22b2 == 4032 && p21.head == 4032, "K = 21");
    CHECK(p21.len(0) == 4032 && p21.len(7) == 4032 + 35 && p21.need(1000) == 9032, "K = 21: 5 doubles per pixel");
    for (int K : {2, 3, 21, 97, 201, 256, 1400, 65535}) {
        const PackLayout p(K);
        const size_t n = 3 * (size_t)K;
        CHECK(p.b1 == n * n, "K = %d: b1 follows A11", K);                       // contiguous: A11 | b1 | rows
        CHECK(p.A22b2 == p.b1 + n && p.head == p.A22b2, "K = %d: the rows follow b1", K);
        CHECK(p.len(1) - p.len(0) == 5 && p.len(0) == p.head, "K = %d: rows of 5", K);
        CHECK(p.need(12345) == p.len(12345), "K = %d: need", K);
        for (size_t extra : {(size_t)0, (size_t)1, (size_t)4, (size_t)5, (size_t)6, (size_t)5 * 68600 + 3, (size_t)1 << 33}) {
            const size_t cap = p.head + extra, mp = p.max_P(cap);
            CHECK(p.len(mp) <= cap && cap < p.len(mp + 1), "K = %d cap = head + %zu: max_P = %zu", K, extra, mp);
        }
    }
}

void check_evaluation_rules()
{
    const size_t npix = 1024 * 512;
    // option texel (REQUIRED: 1, 2, 3) at any size; auto: the full pack from more than four entries per panorama pixel
    for (size_t n : {(size_t)0, npix, 4 * npix, 4 * npix + 1, 100 * npix}) {
        CHECK(hessian_source(1, n, npix) == 1 && hessian_source(2, n, npix) == 0 && hessian_source(3, n, npix) == 3, "texel forced, n = %zu", n);
    }
    CHECK(hessian_source(0, 4 * npix, npix) == 3, "4 npix entries: the rectangle");
    CHECK(hessian_source(0, 4 * npix + 1, npix) == 1, "4 npix + 1 entries: the full pack");
    CHECK(hessian_source(0, 0, npix) == 3, "an empty window");
    // option segpose (REQUIRED: 1, 2; 0 auto = yes) — pixel order only
    CHECK(segpose_in_pixel_order(false, 0) && !segpose_in_pixel_order(false, 1) && segpose_in_pixel_order(false, 2), "segpose, pixel order");
    for (int m = 0; m <= 2; ++m) CHECK(!segpose_in_pixel_order(true, m), "segpose %d, tile order", m);
    // prep blocks: none on clean lines in front of a warp kernel; else one per 1024 pixels
    CHECK(prep_blocks(true, 1, npix) == 0 && prep_blocks(true, 0, npix) == 512 && prep_blocks(false, 1, npix) == 512, "prep blocks");
    CHECK(prep_blocks(false, 1, 1) == 1 && prep_blocks(false, 1, 1024) == 1 && prep_blocks(false, 1, 1025) == 2, "prep blocks round up");
    // non-temporal records: 144 MB of records = 1 179 648 slots of 128 B stay cached, one more does not; the tile order always streams
    CHECK(kRecCachedBytes == 150994944u, "144 MB");
    if (REC_STRIDE == 16) {
        CHECK(!records_non_temporal(false, 1179648, REC_STRIDE), "144 MB exactly: cached");
        CHECK(records_non_temporal(false, 1179649, REC_STRIDE), "144 MB + one record: streamed");
        CHECK(!records_non_temporal(false, 956800, REC_STRIDE), "BASELINE: cached");
    }
    CHECK(records_non_temporal(true, 1, REC_STRIDE) && !records_non_temporal(false, 0, REC_STRIDE), "tile order streams");
    // tile re-bin: more than a fifth of the inliers outside, and not within three evaluations of the last one (the stamps wrap)
    CHECK(!tile_rebin_due(true, 1000, 200, 10, 7) && tile_rebin_due(true, 1000, 201, 10, 7), "a fifth of the inliers");
    CHECK(!tile_rebin_due(true, 1000, 999, 9, 7) && tile_rebin_due(true, 1000, 999, 10, 7), "three evaluations");
    CHECK(!tile_rebin_due(false, 1000, 999, 10, 7) && !tile_rebin_due(true, 0, 0, 10, 7), "pixel order; no inliers");
    CHECK(tile_rebin_due(true, 1000, 999, 0u, 0u - 3u), "a new window: last = stamp - 3");
    CHECK(tile_rebin_due(true, 1000, 999, 1u, 0xFFFFFFFEu) && !tile_rebin_due(true, 1000, 999, 1u, 0xFFFFFFFFu), "wrapped stamps");
}

void check_form_rules()
{
    const long U = GATHER_MAX_UNITS;
    // option step_gather (REQUIRED: 0, 1, 3; default 2)
    CHECK(!gather_lists_ok(true, 0, false, 256, U, 956800, false), "step_gather 0: the sweeping kernel");
    for (int g : {1, 2, 3}) CHECK(gather_lists_ok(true, g, false, 256, U, 956800, false), "step_gather %d, pixel order", g);
    CHECK(!gather_lists_ok(false, 2, false, 256, U, 956800, false), "not the lines' only reader");
    CHECK(!gather_lists_ok(true, 2, true, 256, U, 956800, false), "A22 | b2 from the records");
    CHECK(gather_lists_ok(true, 2, false, U, U, 956800, false) && !gather_lists_ok(true, 2, false, U + 1, U, 956800, false), "units");
    CHECK(!gather_lists_ok(true, 2, false, 256, U, 0, false), "no candidates");
    // tile order: up to 3.5 M candidates; step_gather = 3 everywhere; pixel order everywhere
    CHECK(gather_lists_ok(true, 2, false, 256, U, 3500000, true) && !gather_lists_ok(true, 2, false, 256, U, 3500001, true), "3.5 M candidates in tile order");
    CHECK(gather_lists_ok(true, 1, false, 256, U, 3500000, true) && !gather_lists_ok(true, 1, false, 256, U, 3500001, true), "3.5 M candidates, step_gather 1");
    CHECK(gather_lists_ok(true, 3, false, 256, U, 3500001, true) && gather_lists_ok(true, 2, false, 256, U, 99956800, false), "step_gather 3; pixel order");
    CHECK(gather_uses_lists(true, true, false) && gather_uses_lists(true, false, true) && !gather_uses_lists(true, false, false) && !gather_uses_lists(false, true, true), "lists");
    CHECK(!global_counts_need_expanding(true, true, 1, false), "launch A reads the bytes");
    CHECK(global_counts_need_expanding(false, true, 1, false) && global_counts_need_expanding(true, false, 1, false) && global_counts_need_expanding(true, true, 0, false) &&
          global_counts_need_expanding(true, true, 1, true), "... in no other case");
    CHECK(!gather_rides_in_gram(true, 1) && gather_rides_in_gram(true, 2) && gather_rides_in_gram(true, 3) && !gather_rides_in_gram(false, 2), "in the Gram launch");
    // option gram_tags (REQUIRED: 0)
    CHECK(gram_tags(1, false, false) && !gram_tags(0, false, false) && !gram_tags(1, true, false) && !gram_tags(1, false, true), "gram_tags");
    // option gather_waves (REQUIRED: 1, 2, 4; 0 and 3: four)
    CHECK(gather_waves(0) == 4 && gather_waves(1) == 1 && gather_waves(2) == 2 && gather_waves(3) == 4 && gather_waves(4) == 4, "gather_waves");
    // option gram_sparse (REQUIRED: 0, 1; default -1): forced, else 2^21 slots at the least and 16 thres P_prev below them
    CHECK(gram_sparse(true, 1, 0, 1, 5) && !gram_sparse(false, 1, 0, 1, 5), "forced on: with tags only");
    CHECK(!gram_sparse(true, 0, 1000, 10000000, 5), "forced off");
    const size_t M = (size_t)1 << 21;
    CHECK(gram_sparse(true, -1, 1000, M, 5) && !gram_sparse(true, -1, 1000, M - 1, 5), "2^21 slots");
    CHECK(!gram_sparse(true, -1, 0, 10000000, 5), "no equations formed yet");
    CHECK(gram_sparse(true, -1, 100000, 8000001, 5) && !gram_sparse(true, -1, 100000, 8000000, 5), "16 thres P_prev = 8 M");
    CHECK(!gram_sparse(true, -1, 68600, 956800, 5), "BASELINE: dense");
    CHECK(gram_sparse(true, -1, 118859, 9956800, 5), "10 M events on 2048 x 4096: sparse");
    CHECK(!gram_sparse(false, -1, 118859, 9956800, 5), "no tags");
}

// ceil(a / b) rounded up to a multiple of 8
long ceil8(long a, long b) { return ((a + b - 1) / b + 7) / 8 * 8; }

void check_gram_plan_at(size_t n_cand, bool sparse, int sc, int n_cu, bool tail, size_t n_pm)
{
    const GramPlan g = gram_plan(n_cand, sparse, sc, n_cu, tail, n_pm, 0, kSizes);
    const long n = (long)n_cand, wpb = GRAM_BLOCK / 64, cap = sparse ? (long)sc * GRAM_CHUNK : GRAM_CHUNK, per_round = (long)n_cu * wpb;
    CHECK(g.chunk % 8 == 0 && g.chunk >= GRAM_CHUNK_MIN && g.chunk <= cap, "n = %ld cu = %d cap = %ld: chunk %d", n, n_cu, cap, g.chunk);
    CHECK(g.waves * g.chunk >= n && n > (g.waves - 1) * g.chunk, "n = %ld cu = %d cap = %ld: %ld waves of %d", n, n_cu, cap, g.waves, g.chunk);
    CHECK((long)g.n_gram_blocks * wpb >= g.waves && ((long)g.n_gram_blocks - 1) * wpb < g.waves, "n = %ld cu = %d: %d blocks for %ld waves", n, n_cu, g.n_gram_blocks, g.waves);
    const unsigned want_tail = tail ? (unsigned)((n_pm + EP_TAIL_BLK - 1) / EP_TAIL_BLK) : 0u;
    CHECK(g.ep_tail_blocks == want_tail && g.grid == (unsigned)g.n_gram_blocks + want_tail, "n = %ld n_pm = %zu tail %d: grid %u", n, n_pm, (int)tail, g.grid);
    // whole rounds of one block per CU: with `rounds` of them needed at the cap, the shares are those of exactly `rounds` rounds, equal up to the rounding to 8
    const long rounds = (n + per_round * cap - 1) / (per_round * cap);
    if (rounds > 1) {
        const long share = ceil8(n, per_round * rounds);
        CHECK(g.chunk == std::min(share, cap), "n = %ld cu = %d cap = %ld: chunk %d, share of %ld rounds %ld", n, n_cu, cap, g.chunk, rounds, share);
        CHECK(g.waves <= per_round * rounds && g.waves > per_round * (rounds - 1), "n = %ld cu = %d cap = %ld: %ld waves in %ld rounds", n, n_cu, cap, g.waves, rounds);
        CHECK((long)g.chunk * per_round * rounds - n < 8 * per_round * rounds || g.chunk == cap, "n = %ld: one rounding step", n);
    }
}

void check_gram_plan_sweep()
{
    std::vector<size_t> ns;
    for (size_t n = 1; n <= 300; ++n) ns.push_back(n);
    for (size_t n = 301; n < 250000000; n += n / 7 + 1) ns.push_back(n);
    long count = 0;
    for (int n_cu : {1, 64, 256, 304}) {
        for (int sc = 1; sc <= 8; ++sc) {
            for (int sparse = 0; sparse < 2; ++sparse) {
                if (!sparse && sc != 4) continue;      // (the dense form does not read the option)
                const long cap = sparse ? (long)sc * GRAM_CHUNK : GRAM_CHUNK, per_round = (long)n_cu * (GRAM_BLOCK / 64);
                std::vector<size_t> all = ns;
                for (long r = 1; r <= 64 && per_round * cap * r < 2100000000L; ++r)      // dense near the round boundaries
                    for (long d = -9; d <= 9; ++d) all.push_back((size_t)(per_round * cap * r + d));
                for (long r : {1L, 2L, 3L})                                              // ... and where the share crosses a multiple of 8
                    for (long d = -2; d <= 2; ++d) all.push_back((size_t)(per_round * r * (cap - 8) + d));
                for (size_t n : all) {
                    if (n < 1 || n > 2100000000u) continue;
                    check_gram_plan_at(n, sparse != 0, sc, n_cu, false, 0);
                    check_gram_plan_at(n, sparse != 0, sc, n_cu, true, n + n / 20 + 1);
                    count += 2;
                }
            }
        }
    }
    CHECK(count > 20000, "the sweep ran (%ld plans)", count);
    std::printf("%ld plans swept\n", count);
    // the ep tail on its own: one block per EP_TAIL_BLK pm-order entries, rounded up
    for (size_t n_pm : {(size_t)1, (size_t)EP_TAIL_BLK, (size_t)EP_TAIL_BLK + 1, (size_t)100000000})
        CHECK(gram_plan(1000, false, 4, 256, true, n_pm, 0, kSizes).ep_tail_blocks == (n_pm + EP_TAIL_BLK - 1) / EP_TAIL_BLK, "tail blocks for %zu entries", n_pm);
    for (int gw = 0; gw <= 4; ++gw) CHECK(gram_plan(1000, false, 4, 256, false, 0, gw, kSizes).gather_waves == gather_waves(gw), "gather_waves %d", gw);
}

// What the expressions of emba_form_accumulate gave at the commit before they moved (256 CUs unless stated; options at their defaults: gram_sparse -1,
// gram_sparse_chunk 4; thres 5), at the BASELINE shape and the shapes of DESIGN.md §6 — candidates and active pixels from profiles/r06_*_bench_profiled.json.
void check_gram_plan_known()
{
    if (!kDefaultSizes) return;
    struct Known { size_t n_cand, n_pm, P_prev; int thres; bool tags; int n_cu; bool sparse; int chunk; long waves; int n_gram_blocks; unsigned tail, grid; };
    const Known known[] = {
        {/* 1M BASELINE */ 956800ul, 1000000ul, 68600ul, 5, true, 256, /* -> */ false, 240, 3987l, 250, 245u, 495u},
        {/* shard 1M of 8M */ 1000000ul, 1000000ul, 92540ul, 5, true, 256, /* -> */ false, 248, 4033l, 253, 245u, 498u},
        {/* 2M */ 1956800ul, 2000000ul, 129400ul, 5, false, 256, /* -> */ false, 480, 4077l, 255, 489u, 744u},
        {/* 3M */ 2956800ul, 3000000ul, 141058ul, 5, false, 256, /* -> */ false, 728, 4062l, 254, 733u, 987u},
        {/* 5M */ 4956800ul, 5000000ul, 265488ul, 5, false, 256, /* -> */ false, 608, 8153l, 510, 1221u, 1731u},
        {/* city 10M */ 9692800ul, 10000000ul, 150111ul, 5, false, 256, /* -> */ false, 792, 12239l, 765, 2442u, 3207u},
        {/* shard 5M of 40M */ 5000000ul, 5000000ul, 103285ul, 5, false, 256, /* -> */ false, 616, 8117l, 508, 1221u, 1729u},
        {/* 10M 2048x4096 */ 9956800ul, 10000000ul, 118859ul, 5, true, 256, /* -> */ true, 2432, 4095l, 256, 2442u, 2698u},
        {/* shard 12.5M of 100M */ 12500000ul, 12500000ul, 575656ul, 5, false, 256, /* -> */ false, 1024, 12208l, 763, 3052u, 3815u},
        {/* 40M */ 39956800ul, 40000000ul, 1214040ul, 5, false, 256, /* -> */ false, 976, 40940l, 2559, 9766u, 12325u},
        {/* 100M */ 99956800ul, 100000000ul, 2266861ul, 5, false, 256, /* -> */ false, 1024, 97615l, 6101, 24415u, 30516u},
        {/* 1M BASELINE, 304 CUs */ 956800ul, 1000000ul, 68600ul, 5, true, 304, /* -> */ false, 200, 4784l, 299, 245u, 544u},
    };
    for (const Known& k : known) {
        const bool sparse = gram_sparse(k.tags, -1, k.P_prev, k.n_cand, k.thres);
        CHECK(sparse == k.sparse, "%zu candidates: sparse", k.n_cand);
        const GramPlan g = gram_plan(k.n_cand, sparse, 4, k.n_cu, true, k.n_pm, 0, kSizes);
        CHECK(g.chunk == k.chunk && g.waves == k.waves && g.n_gram_blocks == k.n_gram_blocks && g.ep_tail_blocks == k.tail && g.grid == k.grid && g.gather_waves == 4,
              "%zu candidates on %d CUs: chunk %d waves %ld blocks %d tail %u grid %u", k.n_cand, k.n_cu, g.chunk, g.waves, g.n_gram_blocks, g.ep_tail_blocks, g.grid);
        const GramPlan h = gram_plan(k.n_cand, sparse, 4, k.n_cu, false, k.n_pm, 0, kSizes);
        CHECK(h.grid == (unsigned)k.n_gram_blocks && h.ep_tail_blocks == 0 && h.chunk == k.chunk, "%zu candidates: without the tail", k.n_cand);
    }
}

}  // namespace

int main()
{
    check_pack_layout();
    check_evaluation_rules();
    check_form_rules();
    check_gram_plan_sweep();
    check_gram_plan_known();
    if (g_fail) { std::printf("%d checks failed\n", g_fail); return 1; }
    std::printf("OK step_rule\n");
    return 0;
}
