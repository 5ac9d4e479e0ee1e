// tests/cpp/exposure_rule_test.cpp — emba_amd/csrc/exposure_rule.h on a CPU (plain C++17, no HIP; tests/test_exposure_rule_cpu.py builds and runs it, also
// under the address and undefined-behaviour sanitizers): the argument checks, the index of each of the 15 + 5 sums, the pixel against align_pixel, the
// compensated byte at its ties and both clamps, the step on a hand-written H, b under each of the four estimate masks, the leading block against align_solve
// and align_step bit for bit, the constant-byte frame, the gain bounds and the gauge.
#include "../../emba_amd/csrc/exposure_rule.h"

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

static emba_exposure_settings settings()
{
    emba_exposure_settings s;
    s.align.max_iters = 10; s.align.min_pixels = 3;
    s.align.lambda0 = 1e-3; s.align.lambda_up = 10.0; s.align.lambda_down = 10.0; s.align.lambda_min = 1e-9; s.align.lambda_max = 1e6; s.align.tol_rot = 1e-6;
    s.align.huber_k = 0.0;
    s.gain_min = 0.5; s.gain_max = 2.0;
    return s;
}

static void test_args()
{
    using A = ExposureArgStatus;
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    size_t bad = 99;
    const double g[3] = {1.0, 0.5, 2.0}, b[3] = {0.0, -3.0, 4.0};
    CHECK(exposure_args_ok(g, b, 3, &bad) == A::ok);
    CHECK(exposure_args_ok(nullptr, nullptr, 0, &bad) == A::ok);      // F = 0: the pointers are not read
    CHECK(exposure_args_ok(nullptr, b, 3, &bad) == A::gain_null && exposure_args_ok(g, nullptr, 3, &bad) == A::bias_null);
    const double g1[3] = {1.0, nan, 2.0}, g2[3] = {1.0, 1.0, inf}, g3[3] = {0.0, 1.0, 1.0}, g4[3] = {1.0, -1.0, 1.0}, b1[3] = {0.0, 0.0, nan}, b2[3] = {-inf, 0.0, 0.0};
    CHECK(exposure_args_ok(g1, b, 3, &bad) == A::gain_not_finite && bad == 1);
    CHECK(exposure_args_ok(g2, b, 3, &bad) == A::gain_not_finite && bad == 2);
    CHECK(exposure_args_ok(g3, b, 3, &bad) == A::gain_not_positive && bad == 0);
    CHECK(exposure_args_ok(g4, b, 3, &bad) == A::gain_not_positive && bad == 1);
    CHECK(exposure_args_ok(g, b1, 3, &bad) == A::bias_not_finite && bad == 2);
    CHECK(exposure_args_ok(g, b2, 3, &bad) == A::bias_not_finite && bad == 0);
    CHECK(exposure_estimate_ok(0) && exposure_estimate_ok(3) && !exposure_estimate_ok(4) && !exposure_estimate_ok(-1));
    CHECK(exposure_bounds_ok(0.5, 2.0) && exposure_bounds_ok(1.0, 1.0) && exposure_bounds_ok(1e-300, 1e300));
    CHECK(!exposure_bounds_ok(0.0, 2.0) && !exposure_bounds_ok(-1.0, 2.0) && !exposure_bounds_ok(1.5, 2.0) && !exposure_bounds_ok(0.5, 0.9));
    CHECK(!exposure_bounds_ok(nan, 2.0) && !exposure_bounds_ok(0.5, nan) && !exposure_bounds_ok(0.5, inf));
}

// J = (2, 3, 5, -7, -1), w = 0.5, r = 11: every product is a small integer or a half
static void test_sum_indices()
{
    static_assert(exposure_h_index(0, 0) == 0 && exposure_h_index(0, 4) == 4 && exposure_h_index(1, 1) == 5 && exposure_h_index(1, 4) == 8 &&
                  exposure_h_index(2, 2) == 9 && exposure_h_index(2, 4) == 11 && exposure_h_index(3, 3) == 12 && exposure_h_index(3, 4) == 13 &&
                  exposure_h_index(4, 4) == 14, "the upper triangle in row-major order");
    static_assert(kExposureSums == 21 && kExposureRhs == 15 && kExposureCost == 20, "15 + 5 + 1");
    ExposureTerm t;
    t.g[0] = 2; t.g[1] = 3; t.g[2] = 5; t.I0 = 7; t.w = 0.5; t.r = 11; t.rho = 121;
    const double J[5] = {2, 3, 5, -7, -1};
    double sums[kExposureSums] = {0};
    exposure_accumulate(t, sums);
    exposure_accumulate(t, sums);
    int seen = 0;
    for (int i = 0; i < 5; ++i)
        for (int j = i; j < 5; ++j, ++seen) {
            CHECK(exposure_h_index(i, j) == seen);
            CHECK(sums[seen] == 2 * 0.5 * J[i] * J[j]);
        }
    CHECK(seen == 15);
    for (int i = 0; i < 5; ++i) CHECK(sums[kExposureRhs + i] == 2 * 0.5 * J[i] * 11);
    CHECK(sums[kExposureCost] == 242.0);
    // the ten of align_accumulate, in its order
    AlignTerm at;
    at.r = t.r; at.w = t.w; at.rho = t.rho;
    for (int k = 0; k < 3; ++k) at.g[k] = t.g[k];
    double ten[kAlignSums] = {0}, shared[kAlignSums];
    align_accumulate(at, ten);
    align_accumulate(at, ten);
    exposure_shared_sums(sums, shared);
    for (int k = 0; k < kAlignSums; ++k) CHECK(same_bits(ten[k], shared[k]));
}

// a 3 x 4 plane: P[i][j] = 10 i + j^2, as in align_rule_test.cpp
static void test_pixel()
{
    const int W = 4, H = 3;
    std::vector<double> P(W * H);
    for (int i = 0; i < H; ++i) for (int j = 0; j < W; ++j) P[i * W + j] = 10.0 * i + j * j;
    std::vector<uint8_t> valid(W * H, 1);
    valid[1 * W + 0] = 0;
    const double J[6] = {1, 0, 2, 0, 1, -1};
    ExposureTerm t = {};
    AlignTerm a = {};
    // the precedence is align_pixel's, and skipped tests the raw byte whatever the gain and bias make of it
    CHECK(exposure_pixel(P.data(), valid.data(), W, H, 3.5, 2.5, J, 0, 0.0, 255.0, 2.0, 9.0, true, 0.0, &t) == kAlignOutside && t.r == 0.0);
    CHECK(exposure_pixel(P.data(), valid.data(), W, H, 3.5, 0.5, J, 0, 0.0, 255.0, 2.0, 9.0, true, 0.0, &t) == kAlignMasked && t.r == 0.0);
    CHECK(exposure_pixel(P.data(), valid.data(), W, H, 1.5, 0.5, J, 0, 0.0, 255.0, 2.0, 9.0, true, 0.0, &t) == kAlignSkipped && t.r == 0.0);
    CHECK(exposure_pixel(P.data(), valid.data(), W, H, 1.5, 0.5, J, 0, 0.0, 255.0, 2.0, 9.0, false, 0.0, &t) == kAlignUsed && t.r == 7.5 - 9.0 && t.I0 == 0.0);
    // used: val = 7.5, I0 = 5, I = 2 * 5 + 0.5 = 10.5
    CHECK(exposure_pixel(P.data(), valid.data(), W, H, 1.5, 0.5, J, 5, 0.0, 255.0, 2.0, 0.5, true, 0.0, &t) == kAlignUsed);
    CHECK(t.r == -3.0 && t.w == 1.0 && t.rho == 9.0 && t.g[0] == 3.0 && t.g[1] == 10.0 && t.g[2] == -4.0 && t.I0 == 5.0);
    CHECK(exposure_pixel(P.data(), valid.data(), W, H, 1.5, 0.5, J, 5, 0.0, 255.0, 2.0, 0.5, true, 1.5, &t) == kAlignUsed && t.w == 0.5 && t.rho == 2 * 1.5 * 3.0 - 2.25);
    // gain 1, bias 0: align_pixel's bits, under a tone that does not round to integers
    for (unsigned v = 0; v < 256; v += 5) {
        const int ce = exposure_pixel(P.data(), valid.data(), W, H, 2.25, 0.7, J, v, -0.3, 1.9, 1.0, 0.0, false, 0.4, &t);
        const int ca = align_pixel(P.data(), valid.data(), W, H, 2.25, 0.7, J, v, -0.3, 1.9, false, 0.4, &a);
        CHECK(ce == ca && same_bits(t.r, a.r) && same_bits(t.w, a.w) && same_bits(t.rho, a.rho) && same_bits(t.g[0], a.g[0]) && same_bits(t.g[2], a.g[2]));
        CHECK(same_bits(t.I0, align_tone(v, -0.3, 1.9)));
    }
}

static void test_byte()
{
    // ties to even
    CHECK(exposure_byte(0, 1.0, 0.5) == 0 && exposure_byte(1, 1.0, 0.5) == 2 && exposure_byte(2, 1.0, 0.5) == 2 && exposure_byte(3, 1.0, 0.5) == 4);
    CHECK(exposure_byte(5, 0.5, 0.0) == 2 && exposure_byte(7, 0.5, 0.0) == 4 && exposure_byte(253, 1.0, 1.5) == 254 && exposure_byte(254, 1.0, 0.5) == 254);
    // both clamps, and their edges
    CHECK(exposure_byte(200, 2.0, 0.0) == 255 && exposure_byte(255, 1.0, 0.4) == 255 && exposure_byte(255, 1.0, 0.6) == 255 && exposure_byte(254, 1.0, 0.6) == 255);
    CHECK(exposure_byte(3, 1.0, -10.0) == 0 && exposure_byte(0, 1.0, -0.4) == 0 && exposure_byte(0, 1.0, -0.6) == 0 && exposure_byte(1, 1.0, -0.4) == 1);
    CHECK(exposure_byte(1, 1.0, -0.5) == 0 && exposure_byte(255, 1e300, 1e300) == 255 && exposure_byte(255, 1e-300, -1e300) == 0);
    // the identity
    for (unsigned v = 0; v < 256; ++v) CHECK(exposure_byte(v, 1.0, 0.0) == v);
}

// H = M^T M + I for a fixed M: symmetric positive definite
static void spd5(double H[5][5])
{
    const double M[5][5] = {{2, 1, 0, 1, 0}, {0, 3, 1, 0, 1}, {1, 0, 2, 1, 1}, {0, 1, 0, 4, 1}, {1, 0, 1, 0, 3}};
    for (int i = 0; i < 5; ++i)
        for (int j = 0; j < 5; ++j) {
            H[i][j] = i == j ? 1.0 : 0.0;
            for (int k = 0; k < 5; ++k) H[i][j] += M[k][i] * M[k][j];
        }
}

static void test_solve_masks()
{
    double H[5][5];
    spd5(H);
    const double xt[5] = {1.0, -2.0, 3.0, 0.5, -4.0};
    for (int mask = 0; mask < 4; ++mask) {
        bool on[5] = {true, true, true, (mask & kExposureGain) != 0, (mask & kExposureBias) != 0};
        double sums[kExposureSums];
        for (int i = 0; i < 5; ++i) for (int j = i; j < 5; ++j) sums[exposure_h_index(i, j)] = H[i][j];
        // b = -H_active x_active on the active rows; the rows that are not estimated hold a value that would show
        for (int i = 0; i < 5; ++i) {
            double s = 0.0;
            for (int j = 0; j < 5; ++j) if (on[j]) s += H[i][j] * xt[j];
            sums[kExposureRhs + i] = on[i] ? -s : 1e300;
        }
        sums[kExposureCost] = 0.0;
        double x[5] = {9, 9, 9, 9, 9};
        CHECK(exposure_solve(sums, 0.0, mask, x));
        for (int i = 0; i < 5; ++i) {
            if (on[i]) CHECK(std::fabs(x[i] - xt[i]) < 1e-12);
            else CHECK(x[i] == 0.0);
        }
        // with lambda = 1 the active diagonal doubles: the residual of that system vanishes
        CHECK(exposure_solve(sums, 1.0, mask, x));
        for (int i = 0; i < 5; ++i) {
            if (!on[i]) continue;
            double s = H[i][i] * x[i];
            for (int j = 0; j < 5; ++j) if (on[j]) s += H[i][j] * x[j];
            CHECK(std::fabs(s + sums[kExposureRhs + i]) < 1e-11);
        }
        // a pivot that is not positive in an active row: degenerate, x left alone
        double z[kExposureSums];
        for (int k = 0; k < kExposureSums; ++k) z[k] = sums[k];
        z[exposure_h_index(1, 1)] = 0.0;
        x[0] = x[1] = x[2] = x[3] = x[4] = 9;
        CHECK(!exposure_solve(z, 1e-3, mask, x) && x[0] == 9 && x[4] == 9);
        // ... and in a photometric row only where that row is active
        for (int k = 0; k < kExposureSums; ++k) z[k] = sums[k];
        z[exposure_h_index(3, 3)] = -1.0;
        CHECK(exposure_solve(z, 1e-3, mask, x) == !(mask & kExposureGain));
        for (int k = 0; k < kExposureSums; ++k) z[k] = sums[k];
        z[exposure_h_index(4, 4)] = std::numeric_limits<double>::quiet_NaN();
        CHECK(exposure_solve(z, 1e-3, mask, x) == !(mask & kExposureBias));
    }
}

// the leading 3 x 3 block: exposure_cholesky<3> and exposure_solve(estimate = 0) against align_solve, bit for bit
static void test_leading_block()
{
    const double tens[3][kAlignSums] = {{4, 2, 0, 5, 1, 3, 0, 5, -7, 0}, {4.1, 2.3, -0.7, 5.9, 1.1, 3.3, 0.12, 5e-3, -7e-3, 100.0}, {1e3, 7.0, -3.0, 2e2, 0.5, 9.0, -1.0, 2.0, 3.0, 1.0}};
    const double lambdas[4] = {0.0, 1e-9, 1e-3, 10.0};
    for (const auto& ten : tens)
        for (double lam : lambdas) {
            double want[3] = {9, 9, 9}, got[3] = {9, 9, 9}, x[5] = {9, 9, 9, 9, 9};
            const bool ok = align_solve(ten, lam, want);
            const double A[9] = {ten[0], ten[1], ten[2], ten[1], ten[3], ten[4], ten[2], ten[4], ten[5]}, rhs[3] = {-ten[6], -ten[7], -ten[8]};
            CHECK(exposure_cholesky<3>(A, rhs, lam, got) == ok);
            for (int k = 0; k < 3; ++k) CHECK(same_bits(want[k], got[k]));
            double sums[kExposureSums];
            for (int k = 0; k < kExposureSums; ++k) sums[k] = 1e300;      // what estimate = 0 must not read
            for (int k = 0; k < kAlignSums; ++k) sums[exposure_shared_index(k)] = ten[k];
            CHECK(exposure_solve(sums, lam, 0, x) == ok);
            for (int k = 0; k < 3; ++k) CHECK(same_bits(want[k], x[k]));
            CHECK(x[3] == 0.0 && x[4] == 0.0);
        }
    // the same sequence of evaluations through align_step and exposure_step(estimate = 0, a = 1, b = 0): the same q, lambda, status and iterations
    const emba_exposure_settings xs = settings();
    const double id[4] = {0, 0, 0, 1};
    AlignFrame a;
    ExposureFrame e;
    align_frame_init(&a, id, xs.align.lambda0);
    exposure_frame_init(&e, id, 1.0, 0.0, xs.align.lambda0);
    const uint64_t n[4] = {10, 1, 2, 3};
    const double costs[8] = {100, 90, 95, 80, 80, 70, 60, 50};
    for (int it = 0; it < 8; ++it) {
        double ten[kAlignSums] = {4.1, 2.3, -0.7, 5.9, 1.1, 3.3, 0.12 / (it + 1), 5e-3, -7e-3 / (it + 1), costs[it]}, sums[kExposureSums];
        for (int k = 0; k < kExposureSums; ++k) sums[k] = 3.0 + k;
        for (int k = 0; k < kAlignSums; ++k) sums[exposure_shared_index(k)] = ten[k];
        align_step(&a, ten, n, xs.align);
        exposure_step(&e, sums, n, xs, 0);
        CHECK(a.status == e.status && a.iters == e.iters && a.have_trial == e.have_trial && same_bits(a.lambda, e.lambda) && same_bits(a.dnorm, e.dnorm));
        for (int k = 0; k < 4; ++k) CHECK(same_bits(a.q[k], e.q[k]) && same_bits(a.q_trial[k], e.q_trial[k]));
        CHECK(e.gain == 1.0 && e.bias == 0.0 && e.gain_trial == 1.0 && e.bias_trial == 0.0);
    }
    CHECK(a.iters == 7);
}

// a frame of one constant byte: I0 the same for every pixel, g and r varying
static void constant_frame_sums(double* sums, double I0)
{
    for (int k = 0; k < kExposureSums; ++k) sums[k] = 0.0;
    for (int s = 0; s < 200; ++s) {
        ExposureTerm t;
        t.g[0] = std::sin(0.3 * s); t.g[1] = std::cos(0.7 * s) + 0.2; t.g[2] = std::sin(1.1 * s + 0.4);
        t.I0 = I0; t.r = 0.01 * std::cos(0.9 * s); t.w = 1.0 / (1.0 + 0.01 * (s % 7)); t.rho = t.r * t.r;
        exposure_accumulate(t, sums);
    }
}

static void test_constant_byte()
{
    const emba_exposure_settings xs = settings();
    const double id[4] = {0, 0, 0, 1};
    const uint64_t n[4] = {200, 0, 0, 0};
    const double tones[3] = {align_tone(37, 0.0, 255.0), align_tone(200, -0.3, 1.9), align_tone(255, 0.0, 1.0)};
    for (double I0 : tones) {
        double sums[kExposureSums], x[5];
        constant_frame_sums(sums, I0);
        CHECK(exposure_collinear(sums));
        CHECK(!exposure_solve(sums, 1e-3, 3, x));                     // collinear under mask 3, whatever the damping
        CHECK(!exposure_solve(sums, 10.0, 3, x));
        CHECK(exposure_solve(sums, 1e-3, 0, x) && exposure_solve(sums, 1e-3, 1, x) && exposure_solve(sums, 1e-3, 2, x));
        ExposureFrame e;
        exposure_frame_init(&e, id, 1.25, -3.0, xs.align.lambda0);
        exposure_step(&e, sums, n, xs, 3);
        CHECK(e.status == EMBA_ALIGN_DEGENERATE && e.q[3] == 1.0 && e.gain == 1.25 && e.bias == -3.0 && !e.have_trial && e.iters == 0);
        exposure_frame_init(&e, id, 1.25, -3.0, xs.align.lambda0);
        exposure_step(&e, sums, n, xs, 0);
        CHECK(e.status == EMBA_ALIGN_RUNNING && e.have_trial && e.gain_trial == 1.25 && e.bias_trial == -3.0);
    }
    // two bytes are enough to tell a gain from a bias
    double sums[kExposureSums], more[kExposureSums], x[5];
    constant_frame_sums(sums, 37.0);
    constant_frame_sums(more, 38.0);
    for (int k = 0; k < kExposureSums; ++k) sums[k] += more[k];
    CHECK(!exposure_collinear(sums) && exposure_solve(sums, 1e-3, 3, x));
    // no weight at all
    for (int k = 0; k < kExposureSums; ++k) sums[k] = 0.0;
    CHECK(exposure_collinear(sums));
}

static void test_step_and_bounds()
{
    const emba_exposure_settings xs = settings();      // gain in [0.5, 2]
    const double id[4] = {0, 0, 0, 1};
    double H[5][5];
    spd5(H);
    double sums[kExposureSums];
    for (int i = 0; i < 5; ++i) for (int j = i; j < 5; ++j) sums[exposure_h_index(i, j)] = H[i][j];
    // b such that the undamped step is (1e-3, -2e-3, 3e-3, x_a, x_b)
    auto set_rhs = [&](double xa, double xb) {
        const double xt[5] = {1e-3, -2e-3, 3e-3, xa, xb};
        for (int i = 0; i < 5; ++i) {
            double s = 0.0;
            for (int j = 0; j < 5; ++j) s += H[i][j] * xt[j];
            sums[kExposureRhs + i] = -s;
        }
    };
    const uint64_t n[4] = {50, 0, 0, 0};
    double better[kExposureSums];
    // a trial inside the bounds with a lower mean cost is accepted: q, a, b move together
    set_rhs(0.5, -0.25);
    sums[kExposureCost] = 100.0;
    ExposureFrame e;
    exposure_frame_init(&e, id, 1.0, 0.0, 1e-12);
    exposure_step(&e, sums, n, xs, 3);
    CHECK(e.status == EMBA_ALIGN_RUNNING && e.have_trial && std::fabs(e.gain_trial - 1.5) < 1e-6 && std::fabs(e.bias_trial + 0.25) < 1e-6 && e.gain == 1.0 && e.bias == 0.0);
    CHECK(std::fabs(e.dnorm - std::sqrt(14.0) * 1e-3) < 1e-9);      // |delta|, the rotation alone
    for (int k = 0; k < kExposureSums; ++k) better[k] = sums[k];
    better[kExposureCost] = 90.0;
    const double at = e.gain_trial, bt = e.bias_trial, q0 = e.q_trial[0];
    exposure_step(&e, better, n, xs, 3);
    CHECK(e.status == EMBA_ALIGN_RUNNING && e.iters == 1 && e.gain == at && e.bias == bt && e.q[0] == q0 && e.sums[kExposureCost] == 90.0);
    // a trial past gain_max is rejected although its mean cost is lower: lambda goes up, nothing moves
    set_rhs(1.5, -0.25);
    exposure_frame_init(&e, id, 1.0, 0.0, 1e-12);
    exposure_step(&e, sums, n, xs, 3);
    CHECK(e.have_trial && e.gain_trial > 2.0);
    const double lam = e.lambda;
    exposure_step(&e, better, n, xs, 3);
    CHECK(e.status == EMBA_ALIGN_RUNNING && e.iters == 1 && e.gain == 1.0 && e.bias == 0.0 && e.q[3] == 1.0 && e.lambda == lam * 10.0 && e.sums[kExposureCost] == 100.0);
    // ... and one below gain_min
    set_rhs(-0.75, 0.0);
    exposure_frame_init(&e, id, 1.0, 0.0, 1e-12);
    exposure_step(&e, sums, n, xs, 1);
    CHECK(e.have_trial && e.gain_trial < 0.5 && e.bias_trial == 0.0);
    exposure_step(&e, better, n, xs, 1);
    CHECK(e.iters == 1 && e.gain == 1.0 && e.sums[kExposureCost] == 100.0);
    // a gain that is not estimated is not tested: it keeps its input value, outside the bounds or not
    set_rhs(0.0, -0.25);
    exposure_frame_init(&e, id, 3.0, 0.0, 1e-12);
    exposure_step(&e, sums, n, xs, 2);
    CHECK(e.have_trial && e.gain_trial == 3.0 && e.bias_trial != 0.0);
    exposure_step(&e, better, n, xs, 2);
    CHECK(e.iters == 1 && e.gain == 3.0 && e.sums[kExposureCost] == 90.0 && e.bias != 0.0);
    // converged tests the rotation alone: a large step in a and b with |delta| < tol_rot converges on acceptance
    exposure_frame_init(&e, id, 1.0, 0.0, 1e-12);
    set_rhs(0.5, -0.25);
    exposure_step(&e, sums, n, xs, 3);
    e.dnorm = 1e-7;
    exposure_step(&e, better, n, xs, 3);
    CHECK(e.status == EMBA_ALIGN_CONVERGED && e.gain == at);
    // n < min_pixels is degenerate under every mask
    const uint64_t few[4] = {2, 0, 0, 0};
    for (int mask = 0; mask < 4; ++mask) {
        exposure_frame_init(&e, id, 1.0, 0.0, 1e-3);
        exposure_step(&e, sums, few, xs, mask);
        CHECK(e.status == EMBA_ALIGN_DEGENERATE && e.gain == 1.0 && e.bias == 0.0);
    }
}

static void test_gauge()
{
    double a[4] = {1.0, 2.0, 3.0, 10.0}, b[4] = {4.0, -2.0, 1.0, 100.0};
    const uint8_t ok[4] = {1, 1, 1, 0};
    CHECK(exposure_gauge(a, b, ok, 4));      // alpha = 2, beta = 1; the frame that does not count is rescaled with the rest
    CHECK(a[0] == 0.5 && a[1] == 1.0 && a[2] == 1.5 && a[3] == 5.0 && b[0] == 1.5 && b[1] == -1.5 && b[2] == 0.0 && b[3] == 49.5);
    CHECK((a[0] + a[1] + a[2]) / 3 == 1.0 && b[0] + b[1] + b[2] == 0.0);
    CHECK(exposure_gauge(a, b, ok, 4) && a[0] == 0.5 && b[3] == 49.5);      // idempotent
    double c[2] = {2.0, 6.0}, d[2] = {1.0, 3.0};
    CHECK(exposure_gauge(c, d, nullptr, 2) && c[0] == 0.5 && c[1] == 1.5 && d[0] == -0.25 && d[1] == 0.25);      // no ok: every frame counts
    const uint8_t none[2] = {0, 0};
    CHECK(!exposure_gauge(c, d, none, 2) && c[0] == 0.5 && d[1] == 0.25);
    CHECK(!exposure_gauge(c, d, nullptr, 0));
    double neg[2] = {-1.0, -3.0}, z[2] = {0.0, 0.0};
    CHECK(!exposure_gauge(neg, z, nullptr, 2) && neg[0] == -1.0);
    // the compensated tone of a frame is unchanged relative to the others: (a_f I + b_f) -> ((a_f I + b_f) - beta) / alpha for one alpha, beta
}

int main()
{
    test_args();
    test_sum_indices();
    test_pixel();
    test_byte();
    test_solve_masks();
    test_leading_block();
    test_constant_byte();
    test_step_and_bounds();
    test_gauge();
    if (g_fail) { std::printf("%d checks failed\n", g_fail); return 1; }
    std::printf("OK exposure_rule\n");
    return 0;
}
