// tests/cpp/track_exposure_rule_test.cpp — emba_amd/csrc/track_exposure_rule.h on a CPU (plain C++17, no HIP; tests/test_track_exposure_rule_cpu.py builds and
// runs it, also under the address and undefined-behaviour sanitizers): the argument checks behind track_rule.h's, track_exposure_pixel against track_pixel bit
// for bit at a = 1, b = 0 (every member of the term, the ten shared sums), against exposure_pixel on the materialised mean plane of level 0 under a
// non-trivial (a, b), the precedence of the classes, and the start gain and bias across lost frames.  Every plane here is exactly as large as the rule says
// it reads: a read past it is the sanitizer's to find.
#include "../../emba_amd/csrc/track_exposure_rule.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

using namespace emba;

static int g_fail = 0;
#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #cond); ++g_fail; } \
    } while (0)

static bool same_bits(double a, double b) { return std::memcmp(&a, &b, sizeof a) == 0; }

static uint64_t g_state = 0x9E3779B97F4A7C15ull;
static uint64_t next_u64()
{
    g_state ^= g_state << 13; g_state ^= g_state >> 7; g_state ^= g_state << 17;
    return g_state;
}
static double uniform() { return (double)(next_u64() >> 11) / 9007199254740992.0; }

// two sums of W x H cells: weights around min_weight (some cells below it), values as of bytes
static void make_sums(int W, int H, uint64_t min_weight, std::vector<uint64_t>* sw, std::vector<uint64_t>* sv)
{
    sw->resize((size_t)W * H); sv->resize((size_t)W * H);
    for (size_t i = 0; i < sw->size(); ++i) {
        const uint64_t w = next_u64() % 8 == 0 ? next_u64() % min_weight : min_weight + next_u64() % 4096;
        (*sw)[i] = w;
        (*sv)[i] = w * (next_u64() % 256) + (w ? next_u64() % w : 0);
    }
}

static void test_args()
{
    using A = TrackExposureArgStatus;
    static_assert((int)A::ok == 0 && (int)A::bad_bounds == 1 && (int)A::bad_estimate == 2, "the order the C ABI reports them in");
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    emba_track_exposure_settings s;
    std::memset(&s, 0, sizeof s);
    s.estimate = 3; s.gain_min = 0.25; s.gain_max = 4.0;
    CHECK(track_exposure_args_ok(s) == A::ok);
    for (int e = 0; e <= 3; ++e) { s.estimate = e; CHECK(track_exposure_args_ok(s) == A::ok); }
    s.estimate = 4; CHECK(track_exposure_args_ok(s) == A::bad_estimate);
    s.estimate = -1; CHECK(track_exposure_args_ok(s) == A::bad_estimate);
    s.gain_min = 0.0; CHECK(track_exposure_args_ok(s) == A::bad_bounds);      // (the bounds are reported in front of the estimate)
    s.estimate = 3;
    s.gain_min = 1.5; CHECK(track_exposure_args_ok(s) == A::bad_bounds);
    s.gain_min = nan; CHECK(track_exposure_args_ok(s) == A::bad_bounds);
    s.gain_min = 1.0; s.gain_max = 1.0; CHECK(track_exposure_args_ok(s) == A::ok);
    s.gain_max = 0.5; CHECK(track_exposure_args_ok(s) == A::bad_bounds);
    s.gain_max = inf; CHECK(track_exposure_args_ok(s) == A::bad_bounds);
}

// a = 1, b = 0: every member of the term is track_pixel's, and the ten shared sums are align_accumulate's
static void test_unit_exposure_is_track_pixel()
{
    const int W = 16, H = 8;
    const uint64_t min_weight = 256;
    std::vector<uint64_t> sw, sv;
    make_sums(W, H, min_weight, &sw, &sv);
    int classes[4] = {0, 0, 0, 0};
    double ten[kAlignSums] = {0}, all[kExposureSums] = {0};
    for (int n = 0; n < 4000; ++n) {
        const double pm_x = -20.0 + 56.0 * uniform(), pm_y = -2.0 + 12.0 * uniform();
        double J23[6];
        for (int j = 0; j < 6; ++j) J23[j] = -3.0 + 6.0 * uniform();
        const unsigned v = n % 7 == 0 ? 0u : (unsigned)(next_u64() % 256);
        for (int skip = 0; skip < 2; ++skip)
            for (double k : {0.0, 7.5}) {
                AlignTerm a{};
                ExposureTerm e{};
                const int ca = track_pixel(sw.data(), sv.data(), W, H, pm_x, pm_y, J23, v, min_weight, skip != 0, k, &a);
                const int ce = track_exposure_pixel(sw.data(), sv.data(), W, H, pm_x, pm_y, J23, v, min_weight, 1.0, 0.0, skip != 0, k, &e);
                CHECK(ca == ce);
                CHECK(same_bits(a.r, e.r));
                ++classes[ce];
                if (ce != kAlignUsed) continue;
                CHECK(same_bits(a.w, e.w) && same_bits(a.rho, e.rho) && same_bits(a.g[0], e.g[0]) && same_bits(a.g[1], e.g[1]) && same_bits(a.g[2], e.g[2]));
                CHECK(e.I0 == (double)v);
                align_accumulate(a, ten);
                exposure_accumulate(e, all);
            }
    }
    for (int k = 0; k < 4; ++k) CHECK(classes[k] > 50);      // every class was met
    for (int k = 0; k < kAlignSums; ++k) CHECK(same_bits(ten[k], all[exposure_shared_index(k)]));
}

// level 0 under a non-trivial (a, b): exposure_pixel on the materialised mean plane and its covered cells, lo = 0, hi = 255
static void test_against_exposure_pixel_on_the_mean_plane()
{
    const int W = 12, H = 6;
    const uint64_t min_weight = 32;
    std::vector<uint64_t> sw, sv;
    make_sums(W, H, min_weight, &sw, &sv);
    std::vector<double> P((size_t)W * H);
    std::vector<uint8_t> valid((size_t)W * H);
    for (size_t i = 0; i < P.size(); ++i) { P[i] = mosaic_mean(sw[i], sv[i], min_weight, 0.0); valid[i] = mosaic_covered(sw[i], min_weight) ? 1 : 0; }
    int used = 0;
    for (int n = 0; n < 3000; ++n) {
        const double pm_x = -15.0 + 42.0 * uniform(), pm_y = -1.0 + 8.0 * uniform();
        double J23[6];
        for (int j = 0; j < 6; ++j) J23[j] = -3.0 + 6.0 * uniform();
        const unsigned v = n % 5 == 0 ? 0u : (unsigned)(next_u64() % 256);
        const double gain = 0.5 + uniform(), bias = -30.0 + 60.0 * uniform();
        for (int skip = 0; skip < 2; ++skip)
            for (double k : {0.0, 4.0}) {
                ExposureTerm a{}, b{};
                const int ca = exposure_pixel(P.data(), valid.data(), W, H, pm_x, pm_y, J23, v, 0.0, 255.0, gain, bias, skip != 0, k, &a);
                const int cb = track_exposure_pixel(sw.data(), sv.data(), W, H, pm_x, pm_y, J23, v, min_weight, gain, bias, skip != 0, k, &b);
                CHECK(ca == cb);
                CHECK(same_bits(a.r, b.r));
                if (cb != kAlignUsed) continue;
                ++used;
                CHECK(same_bits(a.w, b.w) && same_bits(a.rho, b.rho) && same_bits(a.I0, b.I0));
                CHECK(same_bits(a.g[0], b.g[0]) && same_bits(a.g[1], b.g[1]) && same_bits(a.g[2], b.g[2]));
            }
    }
    CHECK(used > 1000);
}

// outside before masked before skipped; skipped tests the raw byte, whatever the gain and bias would make of it
static void test_precedence()
{
    const int W = 4, H = 3;
    const uint64_t min_weight = 10;
    std::vector<uint64_t> sw((size_t)W * H, 100), sv((size_t)W * H, 100 * 50);
    sw[1 * W + 2] = 9;      // one uncovered cell: row 1, column 2
    const double J23[6] = {1, 0, 0, 0, 1, 0};
    ExposureTerm t{};
    // outside (row -1), over an uncovered column, with a zero byte: outside wins
    CHECK(track_exposure_pixel(sw.data(), sv.data(), W, H, 1.5, -0.5, J23, 0, min_weight, 2.0, 5.0, true, 0.0, &t) == kAlignOutside && t.r == 0.0);
    CHECK(track_exposure_pixel(sw.data(), sv.data(), W, H, 1.5, 2.5, J23, 0, min_weight, 2.0, 5.0, true, 0.0, &t) == kAlignOutside);      // row 2 + 1 > H - 1
    // masked (the cell touches the uncovered one), with a zero byte: masked wins
    CHECK(track_exposure_pixel(sw.data(), sv.data(), W, H, 1.5, 0.5, J23, 0, min_weight, 2.0, 5.0, true, 0.0, &t) == kAlignMasked && t.r == 0.0);
    CHECK(track_exposure_pixel(sw.data(), sv.data(), W, H, 2.5, 1.5, J23, 7, min_weight, 2.0, 5.0, false, 0.0, &t) == kAlignMasked);
    // skipped: the raw byte is 0 although a * 0 + b is not
    CHECK(track_exposure_pixel(sw.data(), sv.data(), W, H, 0.25, 0.5, J23, 0, min_weight, 2.0, 5.0, true, 0.0, &t) == kAlignSkipped && t.r == 0.0);
    // ... and without skip_zero the same pixel is used, with r = 50 - (2 * 0 + 5)
    CHECK(track_exposure_pixel(sw.data(), sv.data(), W, H, 0.25, 0.5, J23, 0, min_weight, 2.0, 5.0, false, 0.0, &t) == kAlignUsed && t.r == 45.0 && t.I0 == 0.0);
    // used: r = val - (a v + b), multiply then add
    CHECK(track_exposure_pixel(sw.data(), sv.data(), W, H, 0.25, 0.5, J23, 20, min_weight, 1.5, -3.0, true, 0.0, &t) == kAlignUsed && t.r == 50.0 - (1.5 * 20.0 - 3.0));
    CHECK(t.I0 == 20.0 && t.w == 1.0 && t.g[0] == 0.0 && t.g[1] == 0.0);      // (a constant plane has no gradient)
    // the column wraps: the cell of column W - 1 reads column 0
    CHECK(track_exposure_pixel(sw.data(), sv.data(), W, H, 3.5, 0.5, J23, 20, min_weight, 1.0, 0.0, true, 0.0, &t) == kAlignUsed && t.r == 30.0);
}

// the start of a batch's gain and bias: the last tracked frame in front of it, lost frames skipped, the anchor counted
static void test_start_across_lost_frames()
{
    const int32_t A = EMBA_TRACK_ANCHOR, T = EMBA_TRACK_TRACKED, L = EMBA_TRACK_LOST;
    const int32_t status[6] = {A, T, L, L, T, 0};
    const double gain[6] = {1.0, 1.1, 7.0, 8.0, 1.3, 9.0}, bias[6] = {0.0, -2.0, 70.0, 80.0, -6.0, 90.0};
    double a = -1.0, b = -1.0;
    CHECK(!track_exposure_start(status, gain, bias, 0, &a, &b) && a == 1.0 && b == 0.0);      // nothing in front: the unit exposure
    CHECK(track_exposure_start(status, gain, bias, 1, &a, &b) && a == 1.0 && b == 0.0);       // the anchor
    CHECK(track_exposure_start(status, gain, bias, 2, &a, &b) && a == 1.1 && b == -2.0);
    CHECK(track_exposure_start(status, gain, bias, 3, &a, &b) && a == 1.1 && b == -2.0);      // across one lost frame
    CHECK(track_exposure_start(status, gain, bias, 4, &a, &b) && a == 1.1 && b == -2.0);      // across two: a lost frame's own start values are never read
    CHECK(track_exposure_start(status, gain, bias, 5, &a, &b) && a == 1.3 && b == -6.0);
    const int32_t none[3] = {L, 0, L};
    CHECK(!track_exposure_start(none, gain, bias, 3, &a, &b) && a == 1.0 && b == 0.0);
    // the compensated byte a tracked frame votes is exposure_rule.h's
    CHECK(exposure_byte(100, 1.3, -6.0) == 124u && exposure_byte(0, 1.3, -6.0) == 0u && exposure_byte(255, 1.3, -6.0) == 255u);
}

int main()
{
    test_args();
    test_unit_exposure_is_track_pixel();
    test_against_exposure_pixel_on_the_mean_plane();
    test_precedence();
    test_start_across_lost_frames();
    if (g_fail) { std::printf("%d checks failed\n", g_fail); return 1; }
    std::printf("OK track_exposure_rule\n");
    return 0;
}
