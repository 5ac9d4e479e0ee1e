// The pair-aligned plan of the Gram launch (emba_amd/csrc/step_rule.h: gram_pair_cuts, gram_paired) on a CPU: over random vectors of pair sizes (zeros
// included: a pair without slots has no run), hand cases and the benchmark's shape, the wave ranges cover every slot exactly once, none crosses the
// start of a pair's run, the grid stays within gram_plan's unless the runs alone outnumber its wave slots, and the rule takes the form where it may.
// Prints "OK ..." and returns 0, or names what failed.
#include "../../emba_amd/csrc/step_rule.h"

#include <cstdio>
#include <cstdlib>
#include <random>
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

constexpr GramSizes kSizes{GRAM_BLOCK, GRAM_CHUNK, GRAM_CHUNK_MIN, EP_TAIL_BLK};
constexpr long kWpb = GRAM_BLOCK / 64;

long g_cases = 0;

// sizes: slots per pair in key order (0: the pair has no run)
void check_cuts(const std::vector<long>& sizes, int n_sw, int n_cu, const char* what)
{
    ++g_cases;
    std::vector<uint32_t> run_start;
    size_t n = 0;
    for (long s : sizes) { if (s) run_start.push_back((uint32_t)n); n += (size_t)s; }
    if (!n) return;      // (no candidates: no Gram launch)
    const GramPlan base = gram_plan(n, false, 4, n_cu, false, 0, 0, kSizes);
    std::vector<uint32_t> cuts;
    const GramPairPlan g = gram_pair_cuts(run_start.data(), run_start.size(), n, n_sw, base, kSizes, cuts);
    const long share_max = ((kWpb * GRAM_CHUNK + n_sw - 1) / n_sw + 7) & ~7L;
    CHECK(g.share % 8 == 0 && g.share >= GRAM_CHUNK_MIN && g.share <= share_max, "%s: share %d", what, g.share);
    CHECK(cuts.size() == (size_t)g.n_gram_blocks * kWpb * 2, "%s: %zu words for %d blocks", what, cuts.size(), g.n_gram_blocks);
    // the grid: gram_plan's blocks, unless even the longest share leaves more waves than its slots hold — then what those waves need, and every run costs one wave at the most
    const long waves_min = (long)((n + share_max - 1) / share_max) + (long)run_start.size();
    const long bound = std::max<long>(base.n_gram_blocks, (waves_min + n_sw - 1) / n_sw);
    CHECK(g.n_gram_blocks >= 1 && g.n_gram_blocks <= bound, "%s: %d blocks, gram_plan %d, bound %ld", what, g.n_gram_blocks, base.n_gram_blocks, bound);
    if (g.share < share_max) CHECK(g.n_gram_blocks <= base.n_gram_blocks, "%s: %d blocks at share %d, gram_plan %d", what, g.n_gram_blocks, g.share, base.n_gram_blocks);
    CHECK(g.waves <= (long)g.n_gram_blocks * n_sw, "%s: %ld waves in %d blocks", what, g.waves, g.n_gram_blocks);
    // in wave order the ranges tile [0, n): every slot exactly once; each inside one run; slots behind the streaming waves stay empty
    size_t at = 0, run = 0;
    long used = 0;
    for (long b = 0; b < g.n_gram_blocks; ++b)
        for (long w = 0; w < kWpb; ++w) {
            const uint32_t s = cuts[(size_t)(b * kWpb + w) * 2], e = cuts[(size_t)(b * kWpb + w) * 2 + 1];
            if (w >= n_sw) { CHECK(s == 0 && e == 0, "%s: block %ld wave %ld is no streaming wave", what, b, w); continue; }
            CHECK(e >= s && e <= n, "%s: range [%u, %u)", what, s, e);
            if (e <= s) continue;
            ++used;
            CHECK((size_t)s == at, "%s: range starts at %u, covered up to %zu", what, s, at);
            CHECK((long)(e - s) <= g.share, "%s: range of %u slots, share %d", what, e - s, g.share);
            while (run + 1 < run_start.size() && run_start[run + 1] <= s) ++run;
            const size_t run_end = run + 1 < run_start.size() ? run_start[run + 1] : n;
            CHECK(s >= run_start[run] && e <= run_end, "%s: [%u, %u) crosses the run [%u, %zu)", what, s, e, run_start[run], run_end);
            at = e;
        }
    CHECK(at == n, "%s: covered %zu of %zu slots", what, at, n);
    CHECK(used <= g.waves, "%s: %ld ranges, %ld waves", what, used, g.waves);
}

void check_hand_cases()
{
    for (int n_sw : {12, 14, 15, 16}) {
        check_cuts({5000}, n_sw, 256, "K = 2: one pair");
        check_cuts({1}, n_sw, 256, "one slot");
        check_cuts({3000, 0, 2000}, n_sw, 256, "K = 3, one pair empty");
        check_cuts({0, 0, 7}, n_sw, 256, "only the last pair");
        check_cuts(std::vector<long>(210, 9), n_sw, 256, "210 pairs of 9 slots: fewer than a share each, more pairs than blocks");
        check_cuts({100, 40000, 3, 3, 3, 60000, 1}, n_sw, 256, "the longest pair spans many shares");
        check_cuts(std::vector<long>(4096, 1), n_sw, 8, "4096 one-slot pairs on 8 CUs: the grid grows");
    }
    // the benchmark's shape: ~1 M slots, K = 21 — a measurement's pair is (segment of the event, segment of its predecessor on the pixel), runs shrink geometrically with the distance
    std::vector<long> bench;
    for (int c = 0; c < 20; ++c)
        for (int p = 0; p <= c; ++p) { long s = 20500; for (int d = c - p; d > 1; --d) s = s * 3 / 10; bench.push_back(c - p <= 1 ? 20500 : s); }
    for (int n_sw : {12, 16}) check_cuts(bench, n_sw, 256, "benchmark shape");
}

void check_random()
{
    std::mt19937_64 rng(20240607);
    static const long kScale[5] = {1, 10, 300, 5000, 60000};
    static const int kSw[4] = {12, 14, 15, 16}, kCu[4] = {8, 64, 256, 304};
    for (int it = 0; it < 3000; ++it) {
        const int pairs = 1 + (int)(rng() % (it % 3 == 0 ? 400 : 40));
        const long scale = kScale[rng() % 5];
        std::vector<long> sizes(pairs);
        for (long& s : sizes) { const unsigned r = (unsigned)(rng() % 10); s = r < 2 ? 0 : r < 4 ? 1 + (long)(rng() % 8) : 1 + (long)(rng() % (unsigned long)scale); }
        const int n_sw = kSw[rng() % 4];
        const int n_cu = kCu[rng() % 4];
        check_cuts(sizes, n_sw, n_cu, "random");
    }
}

void check_rule()
{
    CHECK(gram_paired(0, true, false, false, true, false), "dense tag stream in pixel order, runs known, records cached");
    CHECK(!gram_paired(1, true, false, false, true, false), "option gram_multikey");
    CHECK(!gram_paired(0, false, false, false, true, false), "no tag stream");
    CHECK(!gram_paired(0, true, true, false, true, false), "sparse form");
    CHECK(!gram_paired(0, true, false, true, true, false), "tile order");
    CHECK(!gram_paired(0, true, false, false, false, false), "more runs than the order preparation keeps");
    CHECK(!gram_paired(0, true, false, false, true, true), "records past the Infinity Cache");
}

}  // namespace

int main()
{
    check_hand_cases();
    check_random();
    check_rule();
    if (g_fail) { std::printf("%d checks failed\n", g_fail); return 1; }
    std::printf("%ld plans\nOK gram_pair_rule\n", g_cases);
    return 0;
}
