// tests/cpp/contrast_rule_test.cpp — emba_amd/csrc/contrast_rule.h on a CPU (plain C++17, no HIP; tests/test_contrast_cpu.py builds and runs it, once plain
// and once with -fsanitize=address,undefined): the votes of one projected event and their derivatives (weights that sum to 1, derivatives that sum to 0 and
// agree with a difference quotient, the wrap of the columns, the pole rows, integers, non-finite pm), the gradient of one event, the argument checks and
// the span plan of the gradient kernel.  Prints the votes of a few pm ("VOTE pm_x pm_y W H | four cells | four weights | dwx | dwy"): the Python side
// compares them with io.contrast_votes.
#include "../../emba_amd/csrc/contrast_rule.h"

#include <cstdio>
#include <cstdlib>
#include <limits>

using namespace emba;

static int g_fail = 0;
#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #cond); ++g_fail; } \
    } while (0)

static double sum4(const double* a) { return (a[0] + a[1]) + (a[2] + a[3]); }
static bool none(const ContrastVotes& v)
{
    for (int i = 0; i < 4; ++i)
        if (v.cell[i] != -1 || v.w[i] != 0 || v.dwx[i] != 0 || v.dwy[i] != 0) return false;
    return true;
}

static void test_votes()
{
    const int W = 512, H = 256;
    for (int i = 0; i < 4000; ++i) {
        const double x = -3.0 + (W + 6.0) * ((i * 7919) % 4000) / 4000.0 + 1e-3, y = -3.0 + (H + 6.0) * ((i * 104729) % 4000) / 4000.0 + 2e-3;
        const ContrastVotes v = contrast_vote(x, y, W, H);
        CHECK(std::fabs(sum4(v.w) - 1.0) < 1e-15 && std::fabs(sum4(v.dwx)) < 1e-15 && std::fabs(sum4(v.dwy)) < 1e-15);
        for (int k = 0; k < 4; ++k) CHECK(v.w[k] >= 0 && v.w[k] <= 1 && v.cell[k] >= -1 && v.cell[k] < W * H);
        // the derivatives against a difference quotient inside the cell (the weights are bilinear: exact up to rounding)
        const double h = 1e-6;
        const ContrastVotes xp = contrast_vote(x + h, y, W, H), xm = contrast_vote(x - h, y, W, H), yp = contrast_vote(x, y + h, W, H), ym = contrast_vote(x, y - h, W, H);
        if (std::floor(x + h) == std::floor(x - h) && std::floor(y + h) == std::floor(y - h))
            for (int k = 0; k < 4; ++k) {
                CHECK(xp.cell[k] == v.cell[k] && ym.cell[k] == v.cell[k]);
                CHECK(std::fabs((xp.w[k] - xm.w[k]) / (2 * h) - v.dwx[k]) < 1e-8 && std::fabs((yp.w[k] - ym.w[k]) / (2 * h) - v.dwy[k]) < 1e-8);
            }
    }
    ContrastVotes v = contrast_vote(10.25, 20.5, W, H);
    CHECK(v.cell[0] == 20 * W + 10 && v.cell[1] == 20 * W + 11 && v.cell[2] == 21 * W + 10 && v.cell[3] == 21 * W + 11);
    CHECK(v.w[0] == 0.375 && v.w[1] == 0.125 && v.w[2] == 0.375 && v.w[3] == 0.125);
    CHECK(v.dwx[0] == -0.5 && v.dwx[1] == 0.5 && v.dwx[2] == -0.5 && v.dwx[3] == 0.5);
    CHECK(v.dwy[0] == -0.75 && v.dwy[1] == -0.25 && v.dwy[2] == 0.75 && v.dwy[3] == 0.25);
    // the wrap at column 0: pm_x in [W - 1, W) votes into column 0 on the right, pm_x in [-1, 0) into column W - 1 on the left
    v = contrast_vote(W - 1 + 0.5, 7.0, W, H);
    CHECK(v.cell[0] == 7 * W + W - 1 && v.cell[1] == 7 * W + 0 && v.w[0] == 0.5 && v.w[1] == 0.5 && v.w[2] == 0 && v.w[3] == 0);
    v = contrast_vote(-0.25, 7.5, W, H);
    CHECK(v.cell[0] == 7 * W + W - 1 && v.cell[1] == 7 * W + 0 && v.cell[2] == 8 * W + W - 1 && v.cell[3] == 8 * W + 0);
    CHECK(v.w[0] == 0.125 && v.w[1] == 0.375 && v.w[2] == 0.125 && v.w[3] == 0.375);
    v = contrast_vote((double)W, 3.0, W, H);
    CHECK(v.cell[0] == 3 * W && v.w[0] == 1.0);
    v = contrast_vote(-2.0 * W + 5.0, 3.0, W, H);
    CHECK(v.cell[0] == 3 * W + 5 && v.w[0] == 1.0);
    // the pole rows: rows -1 and H have no cell, the weight stays for the caller to count
    v = contrast_vote(100.0, -0.5, W, H);
    CHECK(v.cell[0] == -1 && v.cell[1] == -1 && v.cell[2] == 100 && v.cell[3] == 101 && v.w[0] == 0.5 && v.w[2] == 0.5 && v.w[1] == 0 && v.w[3] == 0);
    v = contrast_vote(100.5, H - 1 + 0.25, W, H);
    CHECK(v.cell[0] == (H - 1) * W + 100 && v.cell[1] == (H - 1) * W + 101 && v.cell[2] == -1 && v.cell[3] == -1 && v.w[2] == 0.125 && v.w[3] == 0.125);
    v = contrast_vote(100.0, (double)H, W, H);
    CHECK(v.cell[0] == -1 && v.cell[2] == -1 && v.w[0] == 1.0);
    // an exact integer: the whole weight in one cell, the derivatives are those towards the next cells
    v = contrast_vote(33.0, 44.0, W, H);
    CHECK(v.cell[0] == 44 * W + 33 && v.w[0] == 1.0 && v.w[1] == 0 && v.w[2] == 0 && v.w[3] == 0);
    CHECK(v.dwx[0] == -1.0 && v.dwx[1] == 1.0 && v.dwx[2] == 0.0 && v.dwx[3] == 0.0 && v.dwy[0] == -1.0 && v.dwy[1] == 0.0 && v.dwy[2] == 1.0 && v.dwy[3] == 0.0);
    // NaN / inf / beyond 2^31: no votes, no derivatives
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    CHECK(none(contrast_vote(nan, 1.0, W, H)) && none(contrast_vote(1.0, nan, W, H)) && none(contrast_vote(inf, 1.0, W, H)) && none(contrast_vote(1.0, -inf, W, H)));
    CHECK(none(contrast_vote(2147483648.0, 1.0, W, H)) && !none(contrast_vote(2147483647.5, 1.0, W, H)));
    // an odd width, one row
    v = contrast_vote(6.5, 0.0, 7, 1);
    CHECK(v.cell[0] == 6 && v.cell[1] == 0 && v.cell[2] == -1 && v.w[0] == 0.5 && v.w[1] == 0.5);
}

static void test_event_gradient()
{
    const int W = 512, H = 256;
    const ContrastVotes v = contrast_vote(10.25, 20.5, W, H);
    const double I4[4] = {1.0, 2.0, 3.0, 5.0};
    double D[12], ge[6];
    for (int j = 0; j < 12; ++j) D[j] = 0.5 * j - 2.0;
    // gp = (-0.5 + 1 - 1.5 + 2.5, -0.75 - 0.5 + 2.25 + 1.25) = (1.5, 2.25)
    contrast_event_grad(v, I4, D, 1.0, ge);
    for (int j = 0; j < 6; ++j) CHECK(ge[j] == 2.0 * (1.5 * D[j] + 2.25 * D[6 + j]));
    double gn[6];
    contrast_event_grad(v, I4, D, -1.0, gn);
    for (int j = 0; j < 6; ++j) CHECK(gn[j] == -ge[j]);
    // a dropped cell does not count, whatever stands in I4
    const ContrastVotes p = contrast_vote(100.5, H - 1 + 0.25, W, H);
    const double Ip[4] = {1.0, 2.0, 1e300, -1e300};
    contrast_event_grad(p, Ip, D, 1.0, ge);
    for (int j = 0; j < 6; ++j) CHECK(ge[j] == 2.0 * ((-0.75 + 1.5) * D[j] + (-0.5 - 1.0) * D[6 + j]));
    // a pm that is not finite, a D that is not: nothing
    const double nan = std::numeric_limits<double>::quiet_NaN();
    contrast_event_grad(contrast_vote(nan, 1.0, W, H), I4, D, 1.0, ge);
    for (int j = 0; j < 6; ++j) CHECK(ge[j] == 0.0);
    D[3] = nan; D[8] = std::numeric_limits<double>::infinity();
    contrast_event_grad(v, I4, D, 1.0, ge);
    CHECK(ge[3] == 0.0 && ge[2] == 0.0 && ge[0] == 2.0 * (1.5 * D[0] + 2.25 * D[6]));
}

static void test_arguments_and_span()
{
    const size_t n = (size_t)1 << 30;      // (a number, not an allocation)
    CHECK(contrast_args_ok(0, 0, 0, 2, 1) == PanoArgStatus::ok && contrast_args_ok(0, n, n, 6, 50000000) == PanoArgStatus::ok);      // no limit on the length
    CHECK(pano_args_ok(0, n, n, 6, 50000000) == PanoArgStatus::too_long);
    CHECK(contrast_args_ok(5, 4, n, 6, 1) == PanoArgStatus::not_a_range && contrast_args_ok(0, n + 1, n, 6, 1) == PanoArgStatus::not_a_range);
    CHECK(contrast_args_ok(0, 10, n, 1, 1) == PanoArgStatus::too_few_knots && contrast_args_ok(0, 10, n, 2, 0) == PanoArgStatus::bad_dt);
    CHECK(contrast_args_ok(0, n, n, 1, 1) == PanoArgStatus::too_few_knots);      // (the other checks still come first for a long range)
    // the span plan: control poses [first, last + 1], three components each
    ContrastSpan s = contrast_span(7, 7);
    CHECK(s.first == 7 && s.comps == 6 && s.fits);
    s = contrast_span(7, 9);
    CHECK(s.first == 7 && s.comps == 12 && s.fits);
    s = contrast_span(0, kContrastTableCps - 2);                    // exactly the table
    CHECK(s.comps == 3 * kContrastTableCps && s.fits);
    s = contrast_span(0, kContrastTableCps - 1);                    // one more
    CHECK(!s.fits && s.comps == 0);
    s = contrast_span(100, 100 + kContrastTableCps - 2);
    CHECK(s.first == 100 && s.fits && s.comps == 3 * kContrastTableCps);
    s = contrast_span(0x7FFFFFFF, -1);                              // a workgroup without a live event
    CHECK(s.comps == 0 && s.fits);
    s = contrast_span(0, 0x7FFFFFFE);                               // (no overflow)
    CHECK(!s.fits && s.comps == 0);
    // every index a workgroup forms lies inside the table it was planned for
    for (int first = 0; first < 5; ++first)
        for (int last = first; last < first + kContrastTableCps + 3; ++last) {
            const ContrastSpan p = contrast_span(first, last);
            if (p.fits)
                for (int cp = first; cp <= last; ++cp) CHECK(3 * (cp - p.first) + 5 < p.comps && p.comps <= 3 * kContrastTableCps);
        }
}

int main()
{
    test_votes();
    test_event_gradient();
    test_arguments_and_span();
    const double probes[][2] = {{10.25, 20.5}, {511.5, 7.0}, {-0.25, 7.5}, {100.0, -0.5}, {100.5, 255.25}, {33.0, 44.0}, {512.0, 256.0}, {17.999999999999996, 3.0625}};
    for (const auto& p : probes) {
        const ContrastVotes v = contrast_vote(p[0], p[1], 512, 256);
        std::printf("VOTE %.17g %.17g 512 256 | %d %d %d %d | %.17g %.17g %.17g %.17g | %.17g %.17g %.17g %.17g | %.17g %.17g %.17g %.17g\n", p[0], p[1], v.cell[0], v.cell[1],
                    v.cell[2], v.cell[3], v.w[0], v.w[1], v.w[2], v.w[3], v.dwx[0], v.dwx[1], v.dwx[2], v.dwx[3], v.dwy[0], v.dwy[1], v.dwy[2], v.dwy[3]);
    }
    if (g_fail) { std::printf("%d checks failed\n", g_fail); return 1; }
    std::printf("OK contrast_rule\n");
    return 0;
}
