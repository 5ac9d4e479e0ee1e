// tests/cpp/cmax_rule_test.cpp — emba_amd/csrc/cmax_rule.h on a CPU (plain C++17, no HIP; tests/test_cmax_cpu.py builds and runs it): the vote grid of four
// sensors, the slice count, the compass search's schedule against its evaluation cap and on a known objective, the pinhole fit on known pinholes, the
// argument checks.  Prints the fit of one pinhole with all its digits ("FIT f cu cv"): the Python side compares it bit for bit with io.cmax_pinhole_fit.
#include "../../emba_amd/csrc/cmax_rule.h"

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

static std::vector<double> pinhole_lut(int w, int h, double fx, double fy, double cx, double cy)
{
    std::vector<double> lut((size_t)w * h * 3);
    for (int y = 0; y < h; ++y)
        for (int x = 0; x < w; ++x) {
            double* b = &lut[3 * ((size_t)y * w + x)];
            b[0] = (x - cx) / fx; b[1] = (y - cy) / fy; b[2] = 1.0;
        }
    return lut;
}

static void test_grid()
{
    struct { int w, h, shift, gw, gh; } cases[] = {{64, 48, 0, 64, 48}, {240, 180, 1, 120, 90}, {346, 260, 2, 87, 65}, {640, 480, 3, 80, 60}, {63, 47, 0, 63, 47},
                                                   {128, 128, 0, 128, 128}, {129, 128, 1, 65, 64}, {1, 1, 0, 1, 1}};
    for (const auto& c : cases) {
        const CmaxGrid g = cmax_grid(c.w, c.h);
        CHECK(g.shift == c.shift && g.w == c.gw && g.h == c.gh);
        CHECK(g.cells() * 4 <= kCmaxGridBytes);
        CHECK(((c.w - 1) >> g.shift) == g.w - 1 && ((c.h - 1) >> g.shift) == g.h - 1);      // the last pixel lies in the last cell
        if (g.shift) {                                                                       // ... and one shift less would not fit
            const size_t w1 = ((size_t)c.w + (1u << (g.shift - 1)) - 1) >> (g.shift - 1), h1 = ((size_t)c.h + (1u << (g.shift - 1)) - 1) >> (g.shift - 1);
            CHECK(w1 * h1 > kCmaxMaxCells);
        }
    }
    CHECK(kCmaxMaxCells == 16384);
    CHECK(2 * (kCmaxGridBytes + 1024) <= (size_t)160 << 10);      // LDS alone would admit two workgroups (grid + their few reduction slots) per compute unit
}

static void test_slices_and_args()
{
    CHECK(cmax_slice_count(0, 10) == 0 && cmax_slice_count(9, 10) == 0 && cmax_slice_count(10, 10) == 1 && cmax_slice_count(38965, 2000) == 19);
    CHECK(cmax_slice_count(100, 0) == 0 && cmax_slice_count(100, -3) == 0);
    CHECK(cmax_args_ok(1, 8.0) == CmaxArgStatus::ok && cmax_args_ok(10000, 1e-3) == CmaxArgStatus::ok);
    CHECK(cmax_args_ok(0, 8.0) == CmaxArgStatus::bad_slice && cmax_args_ok(-1, 8.0) == CmaxArgStatus::bad_slice);
    CHECK(cmax_args_ok(10, 0.0) == CmaxArgStatus::bad_omega_max && cmax_args_ok(10, -1.0) == CmaxArgStatus::bad_omega_max);
    CHECK(cmax_args_ok(10, std::numeric_limits<double>::infinity()) == CmaxArgStatus::bad_omega_max);
    CHECK(cmax_args_ok(10, std::numeric_limits<double>::quiet_NaN()) == CmaxArgStatus::bad_omega_max);
    CHECK(cmax_args_ok((int64_t)kCmaxMaxRange, 8.0) == CmaxArgStatus::ok && cmax_args_ok((int64_t)kCmaxMaxRange + 1, 8.0) == CmaxArgStatus::slice_too_long);
    CHECK(256ull * kCmaxMaxRange < (1ull << 32));      // a cell cannot overflow, so neither can the uint64 sum of squares
    CHECK(cmax_range_ok(0, 0, 0) == CmaxRangeStatus::ok && cmax_range_ok(3, 7, 7) == CmaxRangeStatus::ok);
    CHECK(cmax_range_ok(5, 4, 7) == CmaxRangeStatus::not_a_range && cmax_range_ok(0, 8, 7) == CmaxRangeStatus::not_a_range);
    CHECK(cmax_range_ok(0, kCmaxMaxRange + 1, (size_t)1 << 30) == CmaxRangeStatus::too_long);
}

// J(w) = 10^12 - |w - target|^2 scaled to integers: a concave objective the search must climb
static uint64_t toy_J(const double* w, const double* target)
{
    double d = 0;
    for (int i = 0; i < 3; ++i) d += (w[i] - target[i]) * (w[i] - target[i]);
    return (uint64_t)(1e12 - d * 1e8);
}

// the first of the six candidates with the largest J, as the kernel and emba_amd.io pick it
static void advance(CmaxSearch& st, const uint64_t* Jc)
{
    int best = 0;
    for (int c = 1; c < 6; ++c)
        if (Jc[c] > Jc[best]) best = c;
    st.advance(best, Jc[best]);
}

static void test_schedule()
{
    // nothing ever improves: twelve halvings from omega_max / 2 down to omega_max 2^-12, which is still used, then the search ends
    for (double wmax : {8.0, 1.0, 0.3, 1e-3, 1e6}) {
        CmaxSearch st(wmax, 100);
        const uint64_t Jc[6] = {100, 100, 100, 100, 100, 100};      // ties with the centre: no move
        int evals = 1;
        double last = 0;
        while (st.running()) { last = st.step; advance(st, Jc); evals += 6; }
        CHECK(st.iter == 12 && evals == 1 + 6 * 12 && evals <= kCmaxEvalCap);
        CHECK(last == wmax / 4096.0 && st.step == wmax / 8192.0);
        CHECK(st.w[0] == 0 && st.w[1] == 0 && st.w[2] == 0 && st.J == 100);
    }
    // something always improves: the cap of 64 iterations ends it
    {
        CmaxSearch st(8.0, 0);
        int evals = 1;
        while (st.running()) {
            const uint64_t Jc[6] = {st.J, st.J + 1, st.J + 1, st.J, st.J, st.J};      // -x and +y tie: the earlier one, -x
            advance(st, Jc);
            evals += 6;
        }
        CHECK(st.iter == kCmaxMaxIter && evals == kCmaxEvalCap && kCmaxEvalCap == 385);
        CHECK(st.w[0] == -4.0 * 64 && st.w[1] == 0 && st.w[2] == 0 && st.step == 4.0 && st.J == 64);
    }
    // a concave objective: the search ends within the cap, within the last step of the target in every axis, and every omega it visited is exact
    {
        const double target[3] = {1.37, -0.52, 2.9};
        const double zero[3] = {0, 0, 0};
        CmaxSearch st(8.0, toy_J(zero, target));
        int evals = 1;
        while (st.running()) {
            uint64_t Jc[6];
            for (int c = 0; c < 6; ++c) {
                double w[3];
                st.candidate(c, w);
                Jc[c] = toy_J(w, target);
                for (int i = 0; i < 3; ++i) CHECK(w[i] * 4096.0 / 8.0 == std::floor(w[i] * 4096.0 / 8.0));      // multiples of omega_max 2^-12
            }
            advance(st, Jc);
            evals += 6;
        }
        CHECK(evals <= kCmaxEvalCap && st.iter < kCmaxMaxIter);
        for (int i = 0; i < 3; ++i) CHECK(std::fabs(st.w[i] - target[i]) <= 8.0 / 4096.0);
    }
}

static void test_pinhole()
{
    struct { int w, h; double f, cx, cy; } cases[] = {{64, 48, 60.0, 32.0, 24.0}, {63, 47, 60.0, 31.5, 23.5}, {240, 180, 200.0, 120.0, 90.0}, {346, 260, 251.7, 170.3, 131.9},
                                                       {130, 100, 97.0, 61.25, 52.5}};
    for (const auto& c : cases) {
        const std::vector<double> lut = pinhole_lut(c.w, c.h, c.f, c.f, c.cx, c.cy);
        const CmaxPinhole p = cmax_pinhole_fit(lut.data(), c.w, c.h);
        CHECK(p.ok);
        CHECK(std::fabs(p.f - c.f) <= 1e-9 * c.f && std::fabs(p.cu - c.cx) <= 1e-9 * c.w && std::fabs(p.cv - c.cy) <= 1e-9 * c.h);
    }
    {   // fx != fy: the mean of the two slopes, each centre from its own line
        const std::vector<double> lut = pinhole_lut(64, 48, 60.0, 66.0, 30.0, 25.0);
        const CmaxPinhole p = cmax_pinhole_fit(lut.data(), 64, 48);
        CHECK(p.ok && std::fabs(p.f - 63.0) <= 1e-9 * 63.0);
        CHECK(std::fabs(p.cu - (31.5 - 63.0 * (31.5 - 30.0) / 60.0)) <= 1e-9 * 64 && std::fabs(p.cv - (23.5 - 63.0 * (23.5 - 25.0) / 66.0)) <= 1e-9 * 48);
    }
    {   // one row of pixels: the column has one entry, the row alone decides; no entry in front of the camera: no fit
        const std::vector<double> lut = pinhole_lut(64, 1, 60.0, 60.0, 32.0, 0.0);
        const CmaxPinhole p = cmax_pinhole_fit(lut.data(), 64, 1);
        CHECK(p.ok && std::fabs(p.f - 60.0) <= 1e-9 * 60.0 && std::fabs(p.cu - 32.0) <= 1e-7 && p.cv == 0.0);
        std::vector<double> back = pinhole_lut(8, 8, 10.0, 10.0, 4.0, 4.0);
        for (size_t i = 0; i < 64; ++i) back[3 * i + 2] = -1.0;
        CHECK(!cmax_pinhole_fit(back.data(), 8, 8).ok);
    }
    const std::vector<double> lut = pinhole_lut(63, 47, 60.0, 60.0, 31.5, 23.5);
    const CmaxPinhole p = cmax_pinhole_fit(lut.data(), 63, 47);
    std::printf("FIT %.17g %.17g %.17g\n", p.f, p.cu, p.cv);
}

int main()
{
    test_grid();
    test_slices_and_args();
    test_schedule();
    test_pinhole();
    if (g_fail) { std::printf("%d check(s) failed\n", g_fail); return 1; }
    std::printf("OK cmax_rule\n");
    return 0;
}
