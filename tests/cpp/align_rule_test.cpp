// tests/cpp/align_rule_test.cpp — emba_amd/csrc/align_rule.h on a CPU (plain C++17, no HIP; tests/test_align_rule_cpu.py builds and runs it, also under the
// address and undefined-behaviour sanitizers): the argument checks in the order the C ABI reports them, the sample with its gradient on a hand-written 3 x 4
// plane at the wrapped column and at both row limits, the gradient against a finite difference of view_sample, the classes of a pixel in their precedence,
// the Huber branches at |r| = k, the 3 x 3 solve, and align_step through accept, reject, the lambda transitions and every status.  Every plane here is
// exactly as large as the rule says it reads: a read past it is the sanitizer's to find.
#include "../../emba_amd/csrc/align_rule.h"

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

static emba_align_settings settings()
{
    emba_align_settings s;
    s.max_iters = 10; s.min_pixels = 3;
    s.lambda0 = 1e-3; s.lambda_up = 10.0; s.lambda_down = 10.0; s.lambda_min = 1e-9; s.lambda_max = 1e6; s.tol_rot = 1e-6; s.huber_k = 0.0;
    return s;
}

static void test_args()
{
    using A = AlignArgStatus;
    static_assert((int)A::ok == 0 && (int)A::frames_null == 1 && (int)A::q_null == 2 && (int)A::too_many_frames == 3 && (int)A::tone_not_finite == 4 &&
                  (int)A::hi_not_above_lo == 5 && (int)A::huber_not_finite == 6, "the order the C ABI reports them in");
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    const size_t big = (size_t)1 << 31;
    CHECK(align_args_ok(true, true, 3, 0.0, 1.0, 0.0) == A::ok);
    CHECK(align_args_ok(false, false, big, nan, nan, nan) == A::frames_null);
    CHECK(align_args_ok(true, false, big, nan, nan, nan) == A::q_null);
    CHECK(align_args_ok(true, true, big, nan, nan, nan) == A::too_many_frames);
    CHECK(align_args_ok(true, true, big - 1, nan, 1.0, nan) == A::tone_not_finite);
    CHECK(align_args_ok(true, true, big - 1, 0.0, inf, nan) == A::tone_not_finite);
    CHECK(align_args_ok(true, true, big - 1, 1.0, 1.0, nan) == A::hi_not_above_lo);
    CHECK(align_args_ok(true, true, big - 1, 0.0, 1.0, nan) == A::huber_not_finite);
    CHECK(align_args_ok(true, true, big - 1, 0.0, 1.0, -inf) == A::ok);      // (huber_k <= 0 is the quadratic cost)
    CHECK(align_args_ok(false, false, 0, 0.0, 1.0, 0.0) == A::ok);           // F = 0: the pointers are not read
    const double q[12] = {0, 0, 0, 1, 0, 0, 0, 0, 0, nan, 0, 1};
    CHECK(align_first_bad_q(q, 1) == 1 && align_first_bad_q(q, 2) == 1 && align_first_bad_q(q + 8, 1) == 0 && align_first_bad_q(q, 0) == 0);
    const double qi[4] = {inf, 0, 0, 1};
    CHECK(!align_q_ok(qi));

    using S = AlignSetStatus;
    emba_align_settings s = settings();
    CHECK(align_settings_ok(&s) == S::ok && align_settings_ok(nullptr) == S::null);
    s.max_iters = 0; CHECK(align_settings_ok(&s) == S::ok);
    s.max_iters = -1; CHECK(align_settings_ok(&s) == S::max_iters);
    s = settings(); s.lambda_up = 1.0; CHECK(align_settings_ok(&s) == S::factors);
    s = settings(); s.lambda_down = 1.0; CHECK(align_settings_ok(&s) == S::factors);
    s = settings(); s.lambda_up = nan; CHECK(align_settings_ok(&s) == S::factors);
    s = settings(); s.lambda0 = 0.0; CHECK(align_settings_ok(&s) == S::lambda0);
    s = settings(); s.lambda_min = -1.0; CHECK(align_settings_ok(&s) == S::lambda_range);
    s = settings(); s.lambda_max = nan; CHECK(align_settings_ok(&s) == S::lambda_range);
    s = settings(); s.tol_rot = -1e-9; CHECK(align_settings_ok(&s) == S::tol_rot);
    s = settings(); s.min_pixels = 2; CHECK(align_settings_ok(&s) == S::min_pixels);
    s = settings(); s.min_pixels = 3; s.tol_rot = 0.0; CHECK(align_settings_ok(&s) == S::ok);
}

// a 3 x 4 plane: P[i][j] = 10 i + j^2 (so the columns' differences are 1, 3, 5 and, wrapped, -9)
static void test_sample()
{
    const int W = 4, H = 3;
    std::vector<double> P(W * H);
    for (int i = 0; i < H; ++i) for (int j = 0; j < W; ++j) P[i * W + j] = 10.0 * i + j * j;
    double v = 0, gx = 0, gy = 0, ref = 0;
    // inside, at a quarter and three quarters
    CHECK(align_sample(P.data(), W, H, 1.25, 0.75, &v, &gx, &gy) && view_sample(P.data(), W, H, 1.25, 0.75, &ref) && same_bits(v, ref));
    CHECK(gx == 3.0 && gy == 10.0);
    // the wrapped column: c0 = 3, c1 = 0
    CHECK(align_sample(P.data(), W, H, 3.5, 1.0, &v, &gx, &gy) && view_sample(P.data(), W, H, 3.5, 1.0, &ref) && same_bits(v, ref));
    CHECK(gx == -9.0 && gy == 10.0 && v == 14.5);
    CHECK(align_sample(P.data(), W, H, -0.5, 1.0, &v, &gx, &gy) && gx == -9.0 && v == 14.5);          // ix = -1 wraps to column 3
    CHECK(align_sample(P.data(), W, H, 7.5 + 4.0 * 1000, 1.0, &v, &gx, &gy) && gx == -9.0);            // many turns on
    // the row limits: iy = 0 is the first row with a sample, iy + 1 = H - 1 the last; pm_y = H - 1 itself is outside
    CHECK(align_sample(P.data(), W, H, 0.0, 0.0, &v, &gx, &gy) && v == 0.0 && gx == 1.0 && gy == 10.0);
    CHECK(align_sample(P.data(), W, H, 2.0, 1.999, &v, &gx, &gy) && gx == 5.0);
    CHECK(!align_sample(P.data(), W, H, 2.0, 2.0, &v, &gx, &gy));
    CHECK(!align_sample(P.data(), W, H, 2.0, -1e-9, &v, &gx, &gy));
    CHECK(!align_sample(P.data(), W, H, std::numeric_limits<double>::quiet_NaN(), 1.0, &v, &gx, &gy));
    CHECK(!align_sample(P.data(), W, H, 2147483648.0, 1.0, &v, &gx, &gy) && !align_sample(P.data(), W, H, 1.0, -2147483648.0, &v, &gx, &gy));
    // the gradient is the derivative of view_sample inside a cell: a central difference (the sample is bilinear, so the difference is exact up to rounding)
    for (int i = 0; i < H; ++i) for (int j = 0; j < W; ++j) P[i * W + j] = std::sin(1.7 * i + 0.9 * j) + 0.1 * i * j;
    const double h = 1e-4;
    for (double y = 0.3; y < 1.9; y += 0.37)
        for (double x = -3.6; x < 8.0; x += 0.53) {
            if (std::floor(x - h) != std::floor(x + h) || std::floor(y - h) != std::floor(y + h)) continue;
            double a = 0, b = 0, c = 0, d = 0;
            CHECK(align_sample(P.data(), W, H, x, y, &v, &gx, &gy));
            CHECK(view_sample(P.data(), W, H, x + h, y, &a) && view_sample(P.data(), W, H, x - h, y, &b));
            CHECK(view_sample(P.data(), W, H, x, y + h, &c) && view_sample(P.data(), W, H, x, y - h, &d));
            CHECK(std::fabs((a - b) / (2 * h) - gx) < 1e-10 && std::fabs((c - d) / (2 * h) - gy) < 1e-10);
        }
}

static void test_pixel_classes_and_huber()
{
    const int W = 4, H = 3;
    std::vector<double> P(W * H);
    for (int i = 0; i < H; ++i) for (int j = 0; j < W; ++j) P[i * W + j] = 10.0 * i + j * j;
    std::vector<uint8_t> valid(W * H, 1);
    valid[1 * W + 0] = 0;      // a hole at row 1, column 0: the cells (3, 0) wrapped and (0, 1) touch it
    const double J[6] = {1, 0, 2, 0, 1, -1};
    AlignTerm t;
    // precedence: outside before masked before skipped
    CHECK(align_pixel(P.data(), valid.data(), W, H, 3.5, 2.5, J, 0, 0.0, 255.0, true, 0.0, &t) == kAlignOutside && t.r == 0.0);
    CHECK(align_pixel(P.data(), valid.data(), W, H, 3.5, 0.5, J, 0, 0.0, 255.0, true, 0.0, &t) == kAlignMasked && t.r == 0.0);
    CHECK(align_pixel(P.data(), valid.data(), W, H, 0.5, 1.5, J, 7, 0.0, 255.0, true, 0.0, &t) == kAlignMasked);
    CHECK(align_pixel(P.data(), valid.data(), W, H, 1.5, 0.5, J, 0, 0.0, 255.0, true, 0.0, &t) == kAlignSkipped && t.r == 0.0);
    CHECK(align_pixel(P.data(), nullptr, W, H, 3.5, 0.5, J, 0, 0.0, 255.0, false, 0.0, &t) == kAlignUsed);      // no mask, no skip_zero: used
    // used: val = 7.5 at (1.5, 0.5) (top 2.5, bottom 12.5), gx = 3, gy = 10; I = 0 + 5 * 255 / 255 = 5
    CHECK(align_pixel(P.data(), valid.data(), W, H, 1.5, 0.5, J, 5, 0.0, 255.0, true, 0.0, &t) == kAlignUsed);
    CHECK(t.r == 2.5 && t.w == 1.0 && t.rho == 6.25 && t.g[0] == 3.0 && t.g[1] == 10.0 && t.g[2] == -4.0);
    CHECK(same_bits(align_tone(37, -0.3, 1.9), -0.3 + 37.0 * (1.9 - -0.3) / 255.0) && align_tone(255, 0.0, 255.0) == 255.0 && align_tone(0, -2.0, 3.0) == -2.0);
    double sums[kAlignSums] = {0};
    align_accumulate(t, sums);
    align_accumulate(t, sums);
    CHECK(sums[0] == 18.0 && sums[1] == 60.0 && sums[2] == -24.0 && sums[3] == 200.0 && sums[4] == -80.0 && sums[5] == 32.0);
    CHECK(sums[6] == 15.0 && sums[7] == 50.0 && sums[8] == -20.0 && sums[9] == 12.5);
    // Huber: |r| = k is still quadratic, just beyond is linear, and the two meet there
    double w, rho;
    align_huber(2.5, 2.5, &w, &rho); CHECK(w == 1.0 && rho == 6.25);
    align_huber(-2.5, 2.5, &w, &rho); CHECK(w == 1.0 && rho == 6.25);
    align_huber(5.0, 2.5, &w, &rho); CHECK(w == 0.5 && rho == 2 * 2.5 * 5.0 - 6.25);
    align_huber(-5.0, 2.5, &w, &rho); CHECK(w == 0.5 && rho == 18.75);
    align_huber(std::nextafter(2.5, 3.0), 2.5, &w, &rho); CHECK(w < 1.0 && w > 0.999999 && std::fabs(rho - 6.25) < 1e-12);
    align_huber(5.0, 0.0, &w, &rho); CHECK(w == 1.0 && rho == 25.0);
    align_huber(5.0, -1.0, &w, &rho); CHECK(w == 1.0 && rho == 25.0);
    CHECK(align_pixel(P.data(), valid.data(), W, H, 1.5, 0.5, J, 5, 0.0, 255.0, true, 1.25, &t) == kAlignUsed && t.w == 0.5 && t.rho == 2 * 1.25 * 2.5 - 1.5625);
}

static void test_solve()
{
    // H = [[4, 2, 0], [2, 5, 1], [0, 1, 3]], delta = (1, -2, 3): -b = H delta = (0, -5, 7)
    double sums[kAlignSums] = {4, 2, 0, 5, 1, 3, 0, 5, -7, 0};
    double d[3] = {9, 9, 9};
    CHECK(align_solve(sums, 0.0, d) && std::fabs(d[0] - 1) < 1e-13 && std::fabs(d[1] + 2) < 1e-13 && std::fabs(d[2] - 3) < 1e-13);
    // with lambda = 1 the diagonal doubles: (8 2 0; 2 10 1; 0 1 6) delta = (0, -5, 7)
    CHECK(align_solve(sums, 1.0, d));
    CHECK(std::fabs(8 * d[0] + 2 * d[1]) < 1e-13 && std::fabs(2 * d[0] + 10 * d[1] + d[2] + 5) < 1e-13 && std::fabs(d[1] + 6 * d[2] - 7) < 1e-13);
    // a pivot that is not positive: the first, the second (a rank-1 H), the third, a NaN; delta is left alone
    d[0] = d[1] = d[2] = 9;
    double z[kAlignSums] = {0, 0, 0, 1, 0, 1, 1, 1, 1, 0};
    CHECK(!align_solve(z, 1e-3, d));
    double r1[kAlignSums] = {1, 2, 3, 4, 6, 9, 1, 1, 1, 0};
    CHECK(!align_solve(r1, 0.0, d));
    double r2[kAlignSums] = {1, 0, 1, 1, 1, 2, 1, 1, 1, 0};      // rows 0 + 1 = row 2
    CHECK(!align_solve(r2, 0.0, d));
    double nn[kAlignSums] = {std::numeric_limits<double>::quiet_NaN(), 0, 0, 1, 0, 1, 1, 1, 1, 0};
    CHECK(!align_solve(nn, 0.0, d) && d[0] == 9 && d[1] == 9 && d[2] == 9);
    CHECK(align_solve(r1, 1e-3, d));      // damping makes the rank-1 H solvable
    // the trial rotation: exp(delta) (x) q, normalised; a quarter turn about z on the identity, then on itself
    const double half_pi = 1.57079632679489661923, id[4] = {0, 0, 0, 1};
    const double dz[3] = {0, 0, half_pi};
    double q1[4], q2[4];
    align_apply(dz, id, q1);
    CHECK(std::fabs(q1[2] - std::sqrt(0.5)) < 1e-15 && std::fabs(q1[3] - std::sqrt(0.5)) < 1e-15 && q1[0] == 0 && q1[1] == 0);
    align_apply(dz, q1, q2);
    CHECK(std::fabs(q2[2] - 1) < 1e-15 && std::fabs(q2[3]) < 1e-15);
    const double tiny[3] = {1e-12, 0, 0};
    align_apply(tiny, id, q1);
    CHECK(std::fabs(q1[0] - 5e-13) < 1e-25 && q1[3] == 1.0);
    // left multiplication: exp(x) after a turn about z is not the turn about z after exp(x)
    const double dx[3] = {0.3, 0, 0};
    align_apply(dz, id, q1);
    align_apply(dx, q1, q2);      // R = Rx Rz: q = qx (x) qz
    const double sx = std::sin(0.15), cx = std::cos(0.15), s = std::sqrt(0.5);
    CHECK(std::fabs(q2[0] - sx * s) < 1e-15 && std::fabs(q2[1] + sx * s) < 1e-15 && std::fabs(q2[2] - cx * s) < 1e-15 && std::fabs(q2[3] - cx * s) < 1e-15);
}

static void test_step()
{
    const emba_align_settings set = settings();
    const double id[4] = {0, 0, 0, 1};
    const double good[kAlignSums] = {4, 2, 0, 5, 1, 3, 0, 5e-3, -7e-3, 100.0};
    const uint64_t n10[4] = {10, 1, 2, 3}, n2[4] = {2, 0, 0, 0};
    AlignFrame s;
    // the first evaluation becomes the frame's state and a trial is proposed; nothing is counted
    align_frame_init(&s, id, set.lambda0);
    CHECK(s.status == EMBA_ALIGN_RUNNING && s.lambda == 1e-3 && !s.have_trial);
    align_step(&s, good, n10, set);
    CHECK(s.status == EMBA_ALIGN_RUNNING && s.have_trial && s.iters == 0 && s.sums[9] == 100.0 && s.counts[0] == 10 && s.counts[3] == 3);
    CHECK(s.q[3] == 1.0 && s.q_trial[3] < 1.0 && s.dnorm > 1e-3 && s.dnorm < 1e-2);
    // a trial with a lower MEAN cost is accepted although its sum is higher: q moves, lambda goes down
    double better[kAlignSums];
    for (int k = 0; k < kAlignSums; ++k) better[k] = good[k];
    better[9] = 150.0;
    const uint64_t n20[4] = {20, 0, 0, 0};
    double qt[4];
    for (int k = 0; k < 4; ++k) qt[k] = s.q_trial[k];
    align_step(&s, better, n20, set);
    CHECK(s.status == EMBA_ALIGN_RUNNING && s.iters == 1 && s.lambda == 1e-4 && s.q[0] == qt[0] && s.q[1] == qt[1] && s.q[2] == qt[2] && s.q[3] == qt[3]);
    CHECK(s.sums[9] == 150.0 && s.counts[0] == 20);
    // the same mean is not lower: rejected, lambda goes up, q and the sums stay, and another trial from the same equations is proposed
    for (int k = 0; k < 4; ++k) qt[k] = s.q[k];
    align_step(&s, better, n20, set);
    CHECK(s.status == EMBA_ALIGN_RUNNING && s.iters == 2 && s.lambda == 1e-3 && s.q[0] == qt[0] && s.q[3] == qt[3] && s.counts[0] == 20);
    // a trial with too few pixels is rejected whatever its cost
    double cheap[kAlignSums] = {4, 2, 0, 5, 1, 3, 0, 0, 0, 0.0};
    align_step(&s, cheap, n2, set);
    CHECK(s.status == EMBA_ALIGN_RUNNING && s.iters == 3 && s.lambda == 1e-2 && s.counts[0] == 20);
    // lambda_min holds on accept
    s.lambda = 5e-9;
    better[9] = 100.0;
    align_step(&s, better, n20, set);
    CHECK(s.iters == 4 && s.lambda == 1e-9 && s.sums[9] == 100.0);
    // converged: an accepted step with |delta| < tol_rot
    s.dnorm = 1e-7;
    better[9] = 90.0;
    align_step(&s, better, n20, set);
    CHECK(s.status == EMBA_ALIGN_CONVERGED && s.iters == 5 && s.sums[9] == 90.0);
    const AlignFrame done = s;
    align_step(&s, good, n10, set);      // final: left alone
    CHECK(std::memcmp(&done, &s, sizeof s) == 0);
    // ... but a small rejected step does not converge
    align_frame_init(&s, id, set.lambda0);
    align_step(&s, good, n10, set);
    s.dnorm = 1e-7;
    align_step(&s, good, n10, set);
    CHECK(s.status == EMBA_ALIGN_RUNNING && s.lambda == 1e-2);
    // stalled: lambda over lambda_max on a rejection
    s.lambda = 5e5;
    align_step(&s, good, n10, set);
    CHECK(s.status == EMBA_ALIGN_STALLED && s.lambda == 5e6 && s.q[3] == 1.0);
    // iterations: max_iters trials evaluated; max_iters = 0 proposes none and leaves q and the first evaluation
    emba_align_settings two = set;
    two.max_iters = 2;
    align_frame_init(&s, id, set.lambda0);
    align_step(&s, good, n10, two);
    align_step(&s, good, n10, two);
    CHECK(s.status == EMBA_ALIGN_RUNNING && s.iters == 1);
    align_step(&s, good, n10, two);
    CHECK(s.status == EMBA_ALIGN_ITERATIONS && s.iters == 2 && s.q[3] == 1.0);
    two.max_iters = 0;
    align_frame_init(&s, id, set.lambda0);
    align_step(&s, good, n10, two);
    CHECK(s.status == EMBA_ALIGN_ITERATIONS && s.iters == 0 && !s.have_trial && s.sums[9] == 100.0 && s.q[3] == 1.0 && s.q_trial[3] == 1.0);
    // degenerate: n < min_pixels, and a pivot that is not positive; q is unchanged and the evaluation is kept
    align_frame_init(&s, id, set.lambda0);
    align_step(&s, good, n2, set);
    CHECK(s.status == EMBA_ALIGN_DEGENERATE && s.q[3] == 1.0 && s.counts[0] == 2 && !s.have_trial);
    const double flat[kAlignSums] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 3.0};
    align_frame_init(&s, id, set.lambda0);
    align_step(&s, flat, n10, set);
    CHECK(s.status == EMBA_ALIGN_DEGENERATE && s.q[3] == 1.0 && s.sums[9] == 3.0);
    const uint64_t n0[4] = {0, 35, 0, 0};
    align_frame_init(&s, id, set.lambda0);
    align_step(&s, flat, n0, two);      // (degenerate goes before the iterations' end)
    CHECK(s.status == EMBA_ALIGN_DEGENERATE && s.counts[1] == 35);
}

int main()
{
    test_args();
    test_sample();
    test_pixel_classes_and_huber();
    test_solve();
    test_step();
    if (g_fail) { std::printf("%d checks failed\n", g_fail); return 1; }
    std::printf("OK align_rule\n");
    return 0;
}
