// tests/cpp/panorama_rule_test.cpp — emba_amd/csrc/panorama_rule.h on a CPU (plain C++17, no HIP; tests/test_panorama_cpu.py builds and runs it): the votes
// of one projected event (weights, the wrap of the columns, dropped rows, integers, non-finite pm), the batches of a range and the argument checks, the
// limit of 2^23 events included — through the rule function, nothing of that size is allocated.  Prints the votes of a few pm ("VOTE pm_x pm_y W H | four
// cells | four weights"): the Python side compares them with io.pano_votes.
#include "../../emba_amd/csrc/panorama_rule.h"

#include <cstdio>
#include <cstdlib>
#include <limits>

using namespace emba;

static int g_fail = 0;
#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #cond); ++g_fail; } \
    } while (0)

static int wsum(const PanoVotes& v) { return v.w[0] + v.w[1] + v.w[2] + v.w[3]; }
static bool none(const PanoVotes& v)
{
    for (int i = 0; i < 4; ++i)
        if (v.cell[i] != -1 || v.w[i] != 0) return false;
    return true;
}

static void test_votes()
{
    const int W = 512, H = 256;
    // the weights are 256 in all wherever pm is finite; inside the panorama the four cells are the 2x2 patch at (ix, iy)
    for (int i = 0; i < 4000; ++i) {
        const double x = -3.0 + (W + 6.0) * ((i * 7919) % 4000) / 4000.0, y = -3.0 + (H + 6.0) * ((i * 104729) % 4000) / 4000.0;
        const PanoVotes v = pano_vote(x, y, W, H);
        CHECK(wsum(v) == 256);
        for (int k = 0; k < 4; ++k) CHECK(v.w[k] >= 0 && v.w[k] <= 256 && v.cell[k] >= -1 && v.cell[k] < W * H);
    }
    PanoVotes v = pano_vote(10.25, 20.5, W, H);      // wx = 4, wy = 8
    CHECK(v.cell[0] == 20 * W + 10 && v.cell[1] == 20 * W + 11 && v.cell[2] == 21 * W + 10 && v.cell[3] == 21 * W + 11);
    CHECK(v.w[0] == 12 * 8 && v.w[1] == 4 * 8 && v.w[2] == 12 * 8 && v.w[3] == 4 * 8);
    // pm_x in [W - 1, W): the right-hand votes land in column 0
    v = pano_vote(W - 1 + 0.5, 7.0, W, H);
    CHECK(v.cell[0] == 7 * W + W - 1 && v.cell[1] == 7 * W + 0 && v.w[0] == 128 && v.w[1] == 128 && v.w[2] == 0 && v.w[3] == 0);
    // pm_x in [-1, 0): the left-hand votes land in column W - 1
    v = pano_vote(-0.25, 7.5, W, H);                 // ix = -1, wx = 12, wy = 8
    CHECK(v.cell[0] == 7 * W + W - 1 && v.cell[1] == 7 * W + 0 && v.cell[2] == 8 * W + W - 1 && v.cell[3] == 8 * W + 0);
    CHECK(v.w[0] == 4 * 8 && v.w[1] == 12 * 8 && v.w[2] == 4 * 8 && v.w[3] == 12 * 8);
    // pm_x = W exactly (azimuth +pi) is column 0; whole turns away too
    v = pano_vote((double)W, 3.0, W, H);
    CHECK(v.cell[0] == 3 * W && v.w[0] == 256);
    v = pano_vote(-2.0 * W + 5.0, 3.0, W, H);
    CHECK(v.cell[0] == 3 * W + 5 && v.w[0] == 256);
    // rows -1 and H are dropped: no cell, the weight stays for the caller to count
    v = pano_vote(100.0, -0.5, W, H);
    CHECK(v.cell[0] == -1 && v.cell[1] == -1 && v.cell[2] == 100 && v.cell[3] == 101 && v.w[0] == 128 && v.w[2] == 128 && v.w[1] == 0 && v.w[3] == 0);
    v = pano_vote(100.5, H - 1 + 0.25, W, H);
    CHECK(v.cell[0] == (H - 1) * W + 100 && v.cell[1] == (H - 1) * W + 101 && v.cell[2] == -1 && v.cell[3] == -1 && v.w[2] == 8 * 4 && v.w[3] == 8 * 4);
    v = pano_vote(100.0, (double)H, W, H);           // the pole itself: both rows outside
    CHECK(v.cell[0] == -1 && v.cell[2] == -1 && v.w[0] == 256);
    v = pano_vote(100.0, -1.5, W, H);
    CHECK(v.cell[0] == -1 && v.cell[1] == -1 && v.cell[2] == -1 && v.cell[3] == -1 && wsum(v) == 256);
    // a pm exactly on an integer puts 256 into one cell
    v = pano_vote(33.0, 44.0, W, H);
    CHECK(v.cell[0] == 44 * W + 33 && v.w[0] == 256 && v.w[1] == 0 && v.w[2] == 0 && v.w[3] == 0);
    v = pano_vote(0.0, 0.0, W, H);
    CHECK(v.cell[0] == 0 && v.w[0] == 256);
    // the largest fraction: wx = wy = 15
    v = pano_vote(std::nextafter(6.0, 0.0), std::nextafter(9.0, 0.0), W, H);
    CHECK(v.cell[0] == 8 * W + 5 && v.w[0] == 1 && v.w[1] == 15 && v.w[2] == 15 && v.w[3] == 225);
    // NaN / inf / beyond 2^31: no votes
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    CHECK(none(pano_vote(nan, 1.0, W, H)) && none(pano_vote(1.0, nan, W, H)) && none(pano_vote(inf, 1.0, W, H)) && none(pano_vote(1.0, -inf, W, H)));
    CHECK(none(pano_vote(2147483648.0, 1.0, W, H)) && none(pano_vote(1.0, -2147483648.0, W, H)) && !none(pano_vote(2147483647.5, 1.0, W, H)));
    // an odd width, one row
    v = pano_vote(6.5, 0.0, 7, 1);
    CHECK(v.cell[0] == 6 && v.cell[1] == 0 && v.cell[2] == -1 && v.w[0] == 128 && v.w[1] == 128);
}

static void test_batches_and_arguments()
{
    CHECK(pano_batch_count(0, 0) == 0 && pano_batch_count(5, 104) == 0 && pano_batch_count(5, 105) == 1 && pano_batch_count(300, 2850) == 25);
    CHECK(pano_events_used(300, 2850) == 2500 && pano_events_used(7, 3) == 0);
    const size_t n = (size_t)1 << 30;      // (a number, not an allocation)
    CHECK(pano_args_ok(0, 0, 0, 2, 1) == PanoArgStatus::ok && pano_args_ok(0, n, n, 6, 50000000) == PanoArgStatus::too_long);
    CHECK(pano_args_ok(5, 4, n, 6, 1) == PanoArgStatus::not_a_range && pano_args_ok(0, n + 1, n, 6, 1) == PanoArgStatus::not_a_range);
    CHECK(pano_args_ok(0, 10, n, 1, 1) == PanoArgStatus::too_few_knots && pano_args_ok(0, 10, n, 0, 1) == PanoArgStatus::too_few_knots);
    CHECK(pano_args_ok(0, 10, n, 2, 0) == PanoArgStatus::bad_dt && pano_args_ok(0, 10, n, 2, -5) == PanoArgStatus::bad_dt);
    // nn = 2^23 is refused, the last whole batch below it is taken; the tail does not count
    const size_t lim = (size_t)1 << 23;
    CHECK(kPanoMaxEvents == lim && lim % kPanoBatch != 0);
    const size_t nn_max = (lim - 1) / kPanoBatch * kPanoBatch;      // 8 388 600
    CHECK(pano_args_ok(7, 7 + nn_max + 99, n, 2, 1) == PanoArgStatus::ok);
    CHECK(pano_args_ok(7, 7 + nn_max + 100, n, 2, 1) == PanoArgStatus::too_long);
    CHECK(pano_args_ok(0, lim, n, 2, 1) == PanoArgStatus::ok);      // 2^23 events in the range, 8 388 600 of them used
    CHECK(pano_args_ok(0, lim + 92, n, 2, 1) == PanoArgStatus::too_long);
    CHECK(256ull * nn_max < (1ull << 31));                           // a cell holds every vote of the largest range
}

int main()
{
    test_votes();
    test_batches_and_arguments();
    const double probes[][2] = {{10.25, 20.5}, {511.5, 7.0}, {-0.25, 7.5}, {100.0, -0.5}, {100.5, 255.25}, {33.0, 44.0}, {512.0, 256.0}, {17.999999999999996, 3.0625}};
    for (const auto& p : probes) {
        const PanoVotes v = pano_vote(p[0], p[1], 512, 256);
        std::printf("VOTE %.17g %.17g 512 256 | %d %d %d %d | %d %d %d %d\n", p[0], p[1], v.cell[0], v.cell[1], v.cell[2], v.cell[3], v.w[0], v.w[1], v.w[2], v.w[3]);
    }
    if (g_fail) { std::printf("%d checks failed\n", g_fail); return 1; }
    std::printf("OK panorama_rule\n");
    return 0;
}
