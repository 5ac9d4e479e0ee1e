// tests/cpp/view_rule_test.cpp — emba_amd/csrc/view_rule.h on a CPU (plain C++17, no HIP; tests/test_view_rule_cpu.py builds and runs it, also under the
// address and undefined-behaviour sanitizers): the bilinear sample at the corners of a cell, across the seam and at the pole rows, a pm that is not finite,
// the 8-bit tone at and beyond its limits, the frame of a timestamp, and the cut of F frames into chunks.  Every plane here is exactly as large as the rule
// says it reads: a read past it is the sanitizer's to find.
#include "../../emba_amd/csrc/view_rule.h"

#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

using namespace emba;

static int g_fail = 0;
#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #cond); ++g_fail; } \
    } while (0)

static void test_sample()
{
    const int W = 8, H = 5;
    std::vector<double> P((size_t)W * H);
    for (int r = 0; r < H; ++r)
        for (int c = 0; c < W; ++c) P[(size_t)r * W + c] = 100.0 * r + c + 0.5;      // a different value in every cell
    auto at = [&](int r, int c) { return P[(size_t)r * W + c]; };
    double v = -1.0;
    // the four corners of the cell (ix, iy) = (3, 1): at a corner the sample is that cell's value, exactly
    CHECK(view_sample(P.data(), W, H, 3.0, 1.0, &v) && v == at(1, 3));
    CHECK(view_sample(P.data(), W, H, 4.0, 1.0, &v) && v == at(1, 4));
    CHECK(view_sample(P.data(), W, H, 3.0, 2.0, &v) && v == at(2, 3));
    CHECK(view_sample(P.data(), W, H, 4.0, 2.0, &v) && v == at(2, 4));
    // inside: the stated formula, in its order
    {
        const double ax = 0.25, ay = 0.75;
        const double want = (1.0 - ay) * ((1.0 - ax) * at(1, 3) + ax * at(1, 4)) + ay * ((1.0 - ax) * at(2, 3) + ax * at(2, 4));
        CHECK(view_sample(P.data(), W, H, 3.25, 1.75, &v) && v == want);
    }
    // the seam: ix = W - 1 takes column 0 as its right-hand neighbour; at ax = 0 it is column W - 1 alone
    CHECK(view_sample(P.data(), W, H, (double)(W - 1), 2.0, &v) && v == at(2, W - 1));
    CHECK(view_sample(P.data(), W, H, W - 0.5, 2.0, &v) && v == 0.5 * at(2, W - 1) + 0.5 * at(2, 0));
    CHECK(view_sample(P.data(), W, H, -0.5, 2.0, &v) && v == 0.5 * at(2, W - 1) + 0.5 * at(2, 0));      // ix = -1 is column W - 1
    CHECK(view_sample(P.data(), W, H, (double)W, 2.0, &v) && v == at(2, 0));
    CHECK(view_sample(P.data(), W, H, 3.0 * W + 2.0, 2.0, &v) && v == at(2, 2));
    // the pole rows: iy = -1 is outside, iy = H - 2 is the last row pair, iy = H - 1 has no row below it
    v = 77.0;
    CHECK(!view_sample(P.data(), W, H, 3.0, -0.25, &v) && v == 77.0);
    CHECK(!view_sample(P.data(), W, H, 3.0, -1.0, &v));
    CHECK(view_sample(P.data(), W, H, 3.0, 0.0, &v) && v == at(0, 3));
    CHECK(view_sample(P.data(), W, H, 3.0, H - 2.0, &v) && v == at(H - 2, 3));
    CHECK(view_sample(P.data(), W, H, 3.0, H - 1.5, &v) && v == 0.5 * at(H - 2, 3) + 0.5 * at(H - 1, 3));
    CHECK(!view_sample(P.data(), W, H, 3.0, H - 1.0, &v));
    CHECK(!view_sample(P.data(), W, H, 3.0, H - 0.5, &v));
    CHECK(!view_sample(P.data(), W, H, 3.0, (double)H, &v));
    // not finite, or beyond 2^31: outside
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    CHECK(!view_sample(P.data(), W, H, nan, 1.0, &v) && !view_sample(P.data(), W, H, 1.0, nan, &v));
    CHECK(!view_sample(P.data(), W, H, inf, 1.0, &v) && !view_sample(P.data(), W, H, 1.0, -inf, &v));
    CHECK(!view_sample(P.data(), W, H, 2147483648.0, 1.0, &v) && !view_sample(P.data(), W, H, -2147483648.0, 1.0, &v));
    CHECK(view_sample(P.data(), W, H, 2147483647.5, 1.0, &v));      // column (2^31 - 1) % 8 = 7 and column 0
    CHECK(v == 0.5 * at(1, 7) + 0.5 * at(1, 0));
    // the smallest plane with a sample: H = 2, W = 1 (both columns are column 0)
    const double Q[2] = {2.0, 6.0};
    CHECK(view_sample(Q, 1, 2, 5.5, 0.0, &v) && v == 2.0);
    CHECK(view_sample(Q, 1, 2, 5.5, 0.5, &v) && v == 4.0);
    CHECK(!view_sample(Q, 1, 2, 5.5, 1.0, &v));
    CHECK(!view_sample(Q, 1, 1, 0.0, 0.0, &v));      // H = 1 has no row pair at all
}

static void test_sample_row_pair_of_two()
{
    // H = 2: iy = 0 is the only row pair, for every ay in [0, 1)
    const double Q[4] = {1.0, 3.0, 5.0, 7.0};      // [2, 2]
    double v;
    CHECK(view_sample(Q, 2, 2, 0.0, 0.5, &v) && v == 3.0);
    CHECK(view_sample(Q, 2, 2, 1.5, 0.5, &v) && v == 0.5 * (0.5 * 3.0 + 0.5 * 1.0) + 0.5 * (0.5 * 7.0 + 0.5 * 5.0));
    CHECK(!view_sample(Q, 2, 2, 0.0, 1.0, &v));
}

static void test_u8()
{
    // lo == hi: scale 1, so v - lo itself is rounded and saturated
    CHECK(view_scale(3.0, 3.0) == 1.0);
    CHECK(view_u8(3.0, 3.0, 1.0) == 0 && view_u8(5.4, 3.0, 1.0) == 2 && view_u8(400.0, 3.0, 1.0) == 255 && view_u8(-5.0, 3.0, 1.0) == 0);
    const double lo = -1.0, hi = 1.0, sc = view_scale(lo, hi);
    CHECK(sc == 127.5);
    CHECK(view_u8(lo, lo, sc) == 0 && view_u8(hi, lo, sc) == 255);
    CHECK(view_u8(-7.0, lo, sc) == 0 && view_u8(lo - 1e-9, lo, sc) == 0);            // below lo
    CHECK(view_u8(9.0, lo, sc) == 255 && view_u8(hi + 1e-9, lo, sc) == 255);         // above hi
    CHECK(view_u8(0.0, lo, sc) == 128);                                               // 127.5 rounds to the even 128
    CHECK(view_scale(0.0, 255.0) == 1.0 && view_u8(2.5, 0.0, 1.0) == 2 && view_u8(3.5, 0.0, 1.0) == 4);      // halves round to the even number
    CHECK(view_u8(std::numeric_limits<double>::quiet_NaN(), lo, sc) == 0);
    CHECK(view_u8(std::numeric_limits<double>::infinity(), lo, sc) == 255 && view_u8(-std::numeric_limits<double>::infinity(), lo, sc) == 0);
}

static void test_frame_of()
{
    const int64_t e[4] = {10, 20, 21, 50};      // F = 3
    CHECK(view_frame_of(e, 3, 9) == -1 && view_frame_of(e, 3, 10) == 0 && view_frame_of(e, 3, 19) == 0);
    CHECK(view_frame_of(e, 3, 20) == 1 && view_frame_of(e, 3, 21) == 2 && view_frame_of(e, 3, 49) == 2);
    CHECK(view_frame_of(e, 3, 50) == 3 && view_frame_of(e, 3, 1000) == 3);
    CHECK(view_frame_of(e, 0, 9) == -1 && view_frame_of(e, 0, 10) == 0);      // F = 0: one edge, before it or not
    CHECK(view_edges_ok(e, 3) && view_edges_ok(e, 0));
    const int64_t bad[3] = {1, 1, 2}, back[3] = {1, 3, 2};
    CHECK(!view_edges_ok(bad, 2) && !view_edges_ok(back, 2) && view_edges_ok(bad + 1, 1));
}

static void test_chunks()
{
    // small frames: the frame limit cuts — F = 0, 1, 65 535 and 65 536
    const size_t per = view_chunk_frames(35, 8);
    CHECK(per == 65535);
    CHECK(view_chunk_count(0, per) == 0);
    CHECK(view_chunk_count(1, per) == 1 && view_chunk(1, per, 0).f0 == 0 && view_chunk(1, per, 0).nf == 1);
    CHECK(view_chunk_count(65535, per) == 1 && view_chunk(65535, per, 0).nf == 65535);
    CHECK(view_chunk_count(65536, per) == 2);
    CHECK(view_chunk(65536, per, 0).f0 == 0 && view_chunk(65536, per, 0).nf == 65535);
    CHECK(view_chunk(65536, per, 1).f0 == 65535 && view_chunk(65536, per, 1).nf == 1);
    // 240 x 180 doubles: 345 600 B a frame, 97 frames in 32 MiB
    const size_t per2 = view_chunk_frames(240 * 180, 8);
    CHECK(per2 == 97 && per2 * 240 * 180 * 8 <= kViewChunkMaxBytes && (per2 + 1) * 240 * 180 * 8 > kViewChunkMaxBytes);
    CHECK(view_chunk_count(1000, per2) == 11 && view_chunk(1000, per2, 10).f0 == 970 && view_chunk(1000, per2, 10).nf == 30);
    CHECK(view_chunk_frames(240 * 180, 4) == 194);
    // the chunks tile [0, F) in order
    for (size_t F : {(size_t)1, (size_t)96, (size_t)97, (size_t)98, (size_t)1000}) {
        size_t next = 0;
        for (size_t i = 0; i < view_chunk_count(F, per2); ++i) {
            const ViewChunk c = view_chunk(F, per2, i);
            CHECK(c.f0 == next && c.nf >= 1 && c.nf <= per2);
            next += c.nf;
        }
        CHECK(next == F);
    }
    // a frame larger than 32 MiB still goes, alone; an empty sensor does not divide by zero
    CHECK(view_chunk_frames((size_t)8 << 20, 8) == 1 && view_chunk_frames(0, 8) == kViewChunkMaxFrames);
}

int main()
{
    test_sample();
    test_sample_row_pair_of_two();
    test_u8();
    test_frame_of();
    test_chunks();
    if (g_fail) { std::printf("%d check(s) failed\n", g_fail); return 1; }
    std::printf("OK view_rule\n");
    return 0;
}
