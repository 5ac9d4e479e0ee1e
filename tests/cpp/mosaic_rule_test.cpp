// tests/cpp/mosaic_rule_test.cpp — emba_amd/csrc/mosaic_rule.h on a CPU (plain C++17, no HIP; tests/test_mosaic_rule_cpu.py builds and runs it, also under
// the address and undefined-behaviour sanitizers): the argument checks in the order the C ABI reports them, the cut of F frames of bytes into chunks, the
// 2^36 bound on the accumulated votes, and mean, log and gradient on a hand-written 3 x 4 plane with holes, the wrapped column and row 0.  Every plane here
// is exactly as large as the rule says it reads: a read past it is the sanitizer's to find.
#include "../../emba_amd/csrc/mosaic_rule.h"

#include <cstdio>
#include <cstdlib>
#include <limits>

using namespace emba;

static int g_fail = 0;
#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #cond); ++g_fail; } \
    } while (0)

static void test_args()
{
    using A = MosaicArgStatus;
    static_assert((int)A::ok == 0 && (int)A::frames_null == 1 && (int)A::times_null == 2 && (int)A::knots_null == 3 && (int)A::too_few_knots == 4 &&
                  (int)A::bad_dt == 5 && (int)A::too_many_frames == 6 && (int)A::too_many_votes == 7, "the order the C ABI reports them in");
    const size_t S = 35;
    CHECK(mosaic_args_ok(true, true, true, 3, S, 0, 2, 1) == A::ok);
    // every check fails at once: the first one in the order is reported; then one check fewer fails each time
    const size_t big = (size_t)1 << 31;
    CHECK(mosaic_args_ok(false, false, false, big, S, kMosaicMaxVotes, 1, 0) == A::frames_null);
    CHECK(mosaic_args_ok(true, false, false, big, S, kMosaicMaxVotes, 1, 0) == A::times_null);
    CHECK(mosaic_args_ok(true, true, false, big, S, kMosaicMaxVotes, 1, 0) == A::knots_null);
    CHECK(mosaic_args_ok(true, true, true, big, S, kMosaicMaxVotes, 1, 0) == A::too_few_knots);
    CHECK(mosaic_args_ok(true, true, true, big, S, kMosaicMaxVotes, 2, 0) == A::bad_dt);
    CHECK(mosaic_args_ok(true, true, true, big, S, kMosaicMaxVotes, 2, -5) == A::bad_dt);
    CHECK(mosaic_args_ok(true, true, true, big, S, kMosaicMaxVotes, 2, 1) == A::too_many_frames);
    CHECK(mosaic_args_ok(true, true, true, big - 1, S, kMosaicMaxVotes, 2, 1) == A::too_many_votes);
    // F = 0: the pointers are not read, so NULL is no refusal; K and dt_ns still are
    CHECK(mosaic_args_ok(false, false, false, 0, S, 0, 2, 1) == A::ok);
    CHECK(mosaic_args_ok(false, false, false, 0, S, 0, 1, 1) == A::too_few_knots);
    CHECK(mosaic_args_ok(false, false, false, 0, S, kMosaicMaxVotes - 1, 2, 1) == A::ok);

    using T = MosaicToneStatus;
    static_assert((int)T::ok == 0 && (int)T::bad_min_weight == 1 && (int)T::not_finite == 2 && (int)T::hi_not_above_lo == 3, "the order the C ABI reports them in");
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    CHECK(mosaic_get_args_ok(1, 0.0) == T::ok && mosaic_get_args_ok(0, nan) == T::bad_min_weight && mosaic_get_args_ok(1, nan) == T::not_finite);
    CHECK(mosaic_get_args_ok(256, -inf) == T::not_finite && mosaic_get_args_ok(~(uint64_t)0, -1e300) == T::ok);
    CHECK(mosaic_map_args_ok(256, 0.0, 1.0, 1.0 / 255.0) == T::ok && mosaic_map_args_ok(0, nan, nan, nan) == T::bad_min_weight);
    CHECK(mosaic_map_args_ok(1, nan, 1.0, 0.0) == T::not_finite && mosaic_map_args_ok(1, 0.0, inf, 0.0) == T::not_finite && mosaic_map_args_ok(1, 0.0, 1.0, nan) == T::not_finite);
    CHECK(mosaic_map_args_ok(1, 2.0, 1.0, inf) == T::not_finite);      // not finite goes before hi <= lo
    CHECK(mosaic_map_args_ok(1, 1.0, 1.0, 0.0) == T::hi_not_above_lo && mosaic_map_args_ok(1, 2.0, 1.0, 0.0) == T::hi_not_above_lo);
    CHECK(mosaic_map_args_ok(1, -1.0, -0.5, -3.0) == T::ok);            // a negative eps is the caller's business
}

static void test_chunks()
{
    // frames of bytes: view_chunk_frames(S, 1).  7 x 5: the frame limit cuts (65 535); 240 x 180: 32 MiB cut (776 frames); a frame above 32 MiB goes alone
    const size_t per = view_chunk_frames(35, 1);
    CHECK(per == 65535);
    CHECK(view_chunk_count(65535 + 3, per) == 2 && view_chunk(65538, per, 0).nf == 65535 && view_chunk(65538, per, 1).f0 == 65535 && view_chunk(65538, per, 1).nf == 3);
    const size_t per2 = view_chunk_frames(240 * 180, 1);
    CHECK(per2 == 776 && per2 * 240 * 180 <= kViewChunkMaxBytes && (per2 + 1) * 240 * 180 > kViewChunkMaxBytes);
    CHECK(view_chunk_count(1000, per2) == 2 && view_chunk(1000, per2, 1).f0 == 776 && view_chunk(1000, per2, 1).nf == 224);
    CHECK(view_chunk_count(100, per2) == 1 && view_chunk(100, per2, 0).nf == 100);
    CHECK(view_chunk_frames(((size_t)32 << 20) + 1, 1) == 1 && view_chunk_frames((size_t)32 << 20, 1) == 1 && view_chunk_frames((size_t)16 << 20, 1) == 2);
    CHECK(view_chunk_count(0, per) == 0);
}

static void test_bound()
{
    const uint64_t M = kMosaicMaxVotes;
    CHECK(M == (uint64_t)1 << 36);
    CHECK(65280ull * (M - 1) < ((uint64_t)1 << 53) && 256ull * (M - 1) < ((uint64_t)1 << 53));      // both sums convert exactly below the bound
    CHECK((double)(65280ull * (M - 1)) == 65280.0 * (double)(M - 1));
    CHECK(mosaic_votes_after(0, 3, 35) == 105 && mosaic_votes_after(100, 3, 35) == 205 && mosaic_votes_after(7, 0, 35) == 7 && mosaic_votes_after(7, 9, 0) == 7);
    // the last count below the bound is accepted, the bound itself is not
    CHECK(mosaic_votes_after(0, M - 1, 1) == M - 1 && mosaic_votes_after(0, M, 1) == M);
    CHECK(mosaic_votes_after(M - 36, 1, 35) == M - 1 && mosaic_votes_after(M - 35, 1, 35) == M && mosaic_votes_after(M - 1, 1, 1) == M);
    CHECK(mosaic_votes_after(M, 0, 35) == M && mosaic_votes_after(M + 5, 0, 0) == M);
    // F * S beyond 64 bits does not wrap round to a small number
    CHECK(mosaic_votes_after(0, ~(uint64_t)0, 43200) == M && mosaic_votes_after(0, (uint64_t)1 << 40, (uint64_t)1 << 40) == M && mosaic_votes_after(0, 2, ~(uint64_t)0) == M);
    using A = MosaicArgStatus;
    CHECK(mosaic_args_ok(true, true, true, 1, 35, M - 36, 2, 1) == A::ok && mosaic_args_ok(true, true, true, 1, 35, M - 35, 2, 1) == A::too_many_votes);
    CHECK(mosaic_args_ok(true, true, true, 0x7FFFFFFF, 43200, 0, 2, 1) == A::too_many_votes);      // 2^31 - 1 frames of 240 x 180
    CHECK(mosaic_args_ok(true, true, true, 1590728, 43200, 0, 2, 1) == A::ok && mosaic_args_ok(true, true, true, 1590729, 43200, 0, 2, 1) == A::too_many_votes);
}

static void test_plane_with_holes()
{
    // 3 x 4; min_weight 256.  Holes: (0, 1) no weight, (1, 0) one unit short, (2, 2) no weight.
    const int W = 4, H = 3;
    const uint64_t sw[12] = {256, 0, 512, 256, 255, 256, 256, 1024, 256, 256, 0, 256};
    const uint64_t sv[12] = {256 * 10, 0, 512 * 30, 256 * 255, 255 * 99, 256 * 20, 256 * 40, 1024 * 60, 0, 256 * 51, 0, 256 * 102};
    const double want_mean[12] = {10, -1, 30, 255, -1, 20, 40, 60, 0, 51, -1, 102};
    const bool want_cov[12] = {true, false, true, true, false, true, true, true, true, true, false, true};
    double mean[12], L[12];
    uint8_t cov[12];
    for (int c = 0; c < 12; ++c) {
        CHECK(mosaic_covered(sw[c], 256) == want_cov[c]);
        mean[c] = mosaic_mean(sw[c], sv[c], 256, -1.0);
        CHECK(mean[c] == want_mean[c]);
    }
    CHECK(mosaic_covered(255, 255) && mosaic_mean(255, 255 * 99, 1, -1.0) == 99.0 && mosaic_mean(3, 1, 1, -1.0) == 1.0 / 3.0);
    CHECK(mosaic_mean(0, 0, 1, 7.5) == 7.5);      // no weight is never covered: no division by zero
    // the largest sums the bound admits divide exactly
    CHECK(mosaic_mean(256ull * (kMosaicMaxVotes - 1), 65280ull * (kMosaicMaxVotes - 1), 256, 0.0) == 255.0);
    // the plane: lo = 0, hi = 255 makes I the mean itself; no logarithm
    for (int c = 0; c < 12; ++c) {
        L[c] = 0.0;
        cov[c] = mosaic_log(mean[c], want_cov[c], 0.0, 255.0, 0.0, 0, &L[c]) ? 1 : 0;
        CHECK(cov[c] == (want_cov[c] ? 1 : 0) && L[c] == (want_cov[c] ? want_mean[c] : 0.0));
    }
    const double want_gx[12] = {10.0 - 255.0, 0, 0, 255.0 - 30.0, 0, 0, 20, 20, 0.0 - 102.0, 51, 0, 0};
    const double want_gy[12] = {0, 0, 0, 0, 0, 0, 10, 60.0 - 255.0, 0, 31, 0, 42};
    for (int i = 0; i < H; ++i)
        for (int j = 0; j < W; ++j) {
            double gx = 9, gy = 9;
            mosaic_gradient(L, cov, W, i, j, &gx, &gy);
            CHECK(gx == want_gx[i * W + j] && gy == want_gy[i * W + j]);
        }
    // a panorama one column wide: the left neighbour of a cell is the cell itself
    {
        const double l1[2] = {3.0, 5.0};
        const uint8_t c1[2] = {1, 1};
        double gx, gy;
        mosaic_gradient(l1, c1, 1, 1, 0, &gx, &gy);
        CHECK(gx == 0.0 && gy == 2.0);
    }
    // the tone's inverse, in its order; the logarithm and the cells it uncovers
    double l = 77.0;
    CHECK(mosaic_log(51.0, true, 0.25, 1.75, 0.0, 0, &l) && l == 0.25 + 51.0 * (1.75 - 0.25) / 255.0);
    CHECK(mosaic_log(255.0, true, -2.0, 3.0, 0.0, 0, &l) && l == 3.0 && mosaic_log(0.0, true, -2.0, 3.0, 0.0, 0, &l) && l == -2.0);
    CHECK(mosaic_log(10.0, true, 0.0, 255.0, 0.0, 1, &l) && l == std::log(10.0));
    CHECK(mosaic_log(0.0, true, 0.0, 255.0, 0.5, 1, &l) && l == std::log(0.5));
    l = 77.0;
    CHECK(!mosaic_log(0.0, true, 0.0, 255.0, 0.0, 1, &l) && l == 77.0);           // I + eps = 0
    CHECK(!mosaic_log(10.0, true, 0.0, 255.0, -11.0, 1, &l) && l == 77.0);        // I + eps < 0
    CHECK(!mosaic_log(10.0, false, 0.0, 255.0, 0.5, 1, &l) && !mosaic_log(10.0, false, 0.0, 255.0, 0.5, 0, &l) && l == 77.0);
    CHECK(!mosaic_log(std::numeric_limits<double>::quiet_NaN(), true, 0.0, 255.0, 0.5, 1, &l) && l == 77.0);
    CHECK(mosaic_log(10.0, true, 0.0, 255.0, -11.0, 0, &l) && l == 10.0);         // without the logarithm eps is not read
}

int main()
{
    test_args();
    test_chunks();
    test_bound();
    test_plane_with_holes();
    if (g_fail) { std::printf("%d check(s) failed\n", g_fail); return 1; }
    std::printf("OK mosaic_rule\n");
    return 0;
}
