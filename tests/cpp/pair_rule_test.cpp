// tests/cpp/pair_rule_test.cpp — emba_amd/csrc/pair_rule.h on a CPU (plain C++17, no HIP; tests/test_pair_rule_cpu.py builds and runs it, also under the
// address and undefined-behaviour sanitizers): the argument checks in the order the C ABI reports them, D = 0 against the plain pinhole, the projection's
// Jacobian and Ju against central differences (with distortion), the sample at integer (u, v), every outside edge, the classes in their precedence, the
// term, pair_start and pair_information.  Every frame here is exactly as large as the rule says it reads: a read past it is the sanitizer's to find.
#include "../../emba_amd/csrc/pair_rule.h"

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
static const double kNaN = std::numeric_limits<double>::quiet_NaN(), kInf = std::numeric_limits<double>::infinity();
static const double kPlayroomLike[5] = {-0.37, 0.2, 3e-4, -2e-4, -0.07};      // a strong plumb_bob lens (not the fixture: any coefficients serve the derivatives)

static void test_args()
{
    using A = PairArgStatus;
    static_assert((int)A::ok == 0 && (int)A::frames_null == 1 && (int)A::pairs_null == 2 && (int)A::q_null == 3 && (int)A::too_many_pairs == 4 &&
                  (int)A::pair_out_of_range == 5 && (int)A::bad_q == 6 && (int)A::bad_exposure == 7 && (int)A::bad_focal == 8 && (int)A::bad_centre == 9 &&
                  (int)A::bad_distortion == 10 && (int)A::huber_not_finite == 11, "the order the C ABI reports them in");
    size_t at = 99;
    const int32_t pairs[6] = {0, 1, 1, 1, 2, 0};
    const double Q[12] = {0, 0, 0, 1, 0, 0, 0, 2, 0.1, 0, 0, 1};
    const double g[3] = {1, 0.5, 2}, b[3] = {0, -3, 4};
    CHECK(pair_args_ok(true, 3, pairs, 3, Q, g, b, 50, 50, 3, 2, nullptr, 0.0, &at) == A::ok);
    CHECK(pair_args_ok(true, 3, pairs, 3, Q, nullptr, nullptr, 50, 50, 3, 2, kPlayroomLike, -kInf, &at) == A::ok);
    CHECK(pair_args_ok(false, 0, nullptr, 0, nullptr, nullptr, nullptr, 50, 50, 3, 2, nullptr, 0.0, &at) == A::ok);      // P = 0: the pointers are not read
    // each refusal with every later one also wrong: the first is reported
    const int32_t bad_pairs[6] = {0, 1, 1, 3, -1, 0};
    const double bad_Q[12] = {0, 0, 0, 1, 0, 0, 0, 0, kNaN, 0, 0, 1};
    const double bad_g[3] = {1, 0.0, kInf}, bad_b[3] = {0, 0, kNaN}, bad_D[5] = {0, 0, kInf, 0, 0};
    CHECK(pair_args_ok(false, 3, nullptr, 3, nullptr, bad_g, bad_b, -1, kNaN, kNaN, 0, bad_D, kNaN, &at) == A::frames_null);
    CHECK(pair_args_ok(true, 3, nullptr, 3, nullptr, bad_g, bad_b, -1, kNaN, kNaN, 0, bad_D, kNaN, &at) == A::pairs_null);
    CHECK(pair_args_ok(true, 3, bad_pairs, 3, nullptr, bad_g, bad_b, -1, kNaN, kNaN, 0, bad_D, kNaN, &at) == A::q_null);
    CHECK(pair_args_ok(true, 3, bad_pairs, (size_t)1 << 31, bad_Q, bad_g, bad_b, -1, kNaN, kNaN, 0, bad_D, kNaN, &at) == A::too_many_pairs);
    CHECK(pair_args_ok(true, 3, bad_pairs, 3, bad_Q, bad_g, bad_b, -1, kNaN, kNaN, 0, bad_D, kNaN, &at) == A::pair_out_of_range && at == 1);
    CHECK(pair_args_ok(true, 4, bad_pairs, 3, bad_Q, bad_g, bad_b, -1, kNaN, kNaN, 0, bad_D, kNaN, &at) == A::pair_out_of_range && at == 2);
    CHECK(pair_args_ok(true, 3, pairs, 3, bad_Q, bad_g, bad_b, -1, kNaN, kNaN, 0, bad_D, kNaN, &at) == A::bad_q && at == 1);
    CHECK(pair_args_ok(true, 3, pairs, 1, bad_Q + 8, bad_g, bad_b, -1, kNaN, kNaN, 0, bad_D, kNaN, &at) == A::bad_q && at == 0);
    CHECK(pair_args_ok(true, 3, pairs, 3, Q, bad_g, bad_b, -1, kNaN, kNaN, 0, bad_D, kNaN, &at) == A::bad_exposure && at == 1);
    CHECK(pair_args_ok(true, 3, pairs, 3, Q, g, bad_b, -1, kNaN, kNaN, 0, bad_D, kNaN, &at) == A::bad_exposure && at == 2);
    CHECK(pair_args_ok(true, 3, pairs, 3, Q, g, b, -1, 50, kNaN, 0, bad_D, kNaN, &at) == A::bad_focal);
    CHECK(pair_args_ok(true, 3, pairs, 3, Q, g, b, 50, kInf, kNaN, 0, bad_D, kNaN, &at) == A::bad_focal);
    CHECK(pair_args_ok(true, 3, pairs, 3, Q, g, b, 50, 50, kNaN, 0, bad_D, kNaN, &at) == A::bad_centre);
    CHECK(pair_args_ok(true, 3, pairs, 3, Q, g, b, 50, 50, 3, 2, bad_D, kNaN, &at) == A::bad_distortion);
    CHECK(pair_args_ok(true, 3, pairs, 3, Q, g, b, 50, 50, 3, 2, nullptr, kNaN, &at) == A::huber_not_finite);
    CHECK(pair_bytes_ok(kPairMaxBytes / 64, 64) && !pair_bytes_ok(kPairMaxBytes / 64 + 1, 64) && pair_bytes_ok(0, 64) && pair_bytes_ok(5, 0));
    CHECK(pair_chunk_pairs(64) == 65535 && pair_chunk_pairs(240 * 180) == ((size_t)32 << 20) / (240 * 180));
}

static void test_projection()
{
    // D = 0 (and D = NULL) is the plain pinhole
    const PairCamera pin = pair_camera(55.0, 57.0, 31.5, 23.5, nullptr);
    const double zeros[5] = {0, 0, 0, 0, 0};
    const PairCamera pin0 = pair_camera(55.0, 57.0, 31.5, 23.5, zeros);
    const double rb[3] = {0.21, -0.13, 0.9};
    double uv[2], uv0[2], J[6], J0[6];
    CHECK(pair_project(pin, rb, uv, J) && pair_project(pin0, rb, uv0, J0));
    CHECK(same_bits(uv[0], 55.0 * (0.21 / 0.9) + 31.5) && same_bits(uv[1], 57.0 * (-0.13 / 0.9) + 23.5));
    for (int k = 0; k < 2; ++k) CHECK(same_bits(uv[k], uv0[k]));
    for (int k = 0; k < 6; ++k) CHECK(same_bits(J[k], J0[k]));
    CHECK(std::fabs(J[0] - 55.0 / 0.9) < 1e-12 && J[1] == 0.0 && std::fabs(J[2] + 55.0 * 0.21 / (0.9 * 0.9)) < 1e-12);
    // rb_z <= 0 and a NaN have no point
    const double behind[3] = {0.1, 0.1, 0.0}, neg[3] = {0.1, 0.1, -1.0}, nanz[3] = {0.1, 0.1, kNaN};
    CHECK(!pair_project(pin, behind, uv, J) && !pair_project(pin, neg, uv, J) && !pair_project(pin, nanz, uv, J));

    // the Jacobian with distortion against central differences, and Ju against a left perturbation of Q
    const PairCamera cam = pair_camera(55.0, 57.0, 31.5, 23.5, kPlayroomLike);
    const double pts[3][3] = {{0.21, -0.13, 0.9}, {-0.45, 0.33, 1.1}, {0.02, 0.5, 0.8}};
    for (const auto& p : pts) {
        CHECK(pair_project(cam, p, uv, J));
        for (int c = 0; c < 3; ++c) {
            const double h = 1e-6;
            double a[3] = {p[0], p[1], p[2]}, b[3] = {p[0], p[1], p[2]}, ua[2], ub[2], Jx[6];
            a[c] -= h; b[c] += h;
            CHECK(pair_project(cam, a, ua, Jx) && pair_project(cam, b, ub, Jx));
            for (int r = 0; r < 2; ++r) CHECK(std::fabs((ub[r] - ua[r]) / (2 * h) - J[3 * r + c]) < 1e-6 * (1.0 + std::fabs(J[3 * r + c])));
        }
    }
    const double Q[4] = {0.05, -0.08, 0.03, 0.995};
    double Qn[4];
    { const double n = std::sqrt(Q[0] * Q[0] + Q[1] * Q[1] + Q[2] * Q[2] + Q[3] * Q[3]); for (int k = 0; k < 4; ++k) Qn[k] = Q[k] / n; }
    const double bearing[3] = {0.3, -0.2, 1.0};
    double rbq[3], Ju[6];
    pair_turn(Qn, bearing, rbq);
    CHECK(pair_project(cam, rbq, uv, J));
    pair_left_jacobian(J, rbq, Ju);
    for (int c = 0; c < 3; ++c) {
        const double h = 1e-6;
        double uvs[2][2];
        for (int sgn = 0; sgn < 2; ++sgn) {
            double d[3] = {0, 0, 0}, Qp[4], r2[3], Jx[6];
            d[c] = sgn ? h : -h;
            align_apply(d, Qn, Qp);
            pair_turn(Qp, bearing, r2);
            CHECK(pair_project(cam, r2, uvs[sgn], Jx));
        }
        for (int r = 0; r < 2; ++r) CHECK(std::fabs((uvs[1][r] - uvs[0][r]) / (2 * h) - Ju[3 * r + c]) < 1e-5 * (1.0 + std::fabs(Ju[3 * r + c])));
    }
    // the identity turns a bearing into itself, bit for bit
    const double I4[4] = {0, 0, 0, 1};
    pair_turn(I4, bearing, rbq);
    for (int k = 0; k < 3; ++k) CHECK(same_bits(rbq[k], bearing[k]));
}

static void test_sample_and_classes()
{
    const int sw = 5, sh = 4;
    std::vector<uint8_t> f((size_t)sw * sh);
    for (int y = 0; y < sh; ++y) for (int x = 0; x < sw; ++x) f[(size_t)y * sw + x] = (uint8_t)(10 + 7 * x + 31 * y);
    const double Ju[6] = {1, 0, 0, 0, 1, 0};
    AlignTerm t;
    // at integer (u, v) the sample is the byte
    for (int y = 0; y < sh - 1; ++y)
        for (int x = 0; x < sw - 1; ++x) {
            const double uv[2] = {(double)x, (double)y};
            CHECK(pair_pixel(f.data(), sw, sh, true, uv, Ju, 0, 1.0, 0.0, false, 0.0, &t) == kAlignUsed);
            CHECK(same_bits(t.r, (double)f[(size_t)y * sw + x]));
            CHECK(t.g[0] == 7.0 && t.g[1] == 31.0 && t.g[2] == 0.0);
        }
    // the exposure: r = val - (a v + b)
    { const double uv[2] = {1.0, 1.0}; CHECK(pair_pixel(f.data(), sw, sh, true, uv, Ju, 20, 2.0, 3.0, false, 0.0, &t) == kAlignUsed && t.r == 48.0 - 43.0 && t.w == 1.0 && t.rho == 25.0); }
    { const double uv[2] = {1.0, 1.0}; CHECK(pair_pixel(f.data(), sw, sh, true, uv, Ju, 20, 2.0, 3.0, false, 2.0, &t) == kAlignUsed && t.w == 0.4 && t.rho == 16.0); }
    // every outside edge
    const double outs[][2] = {{-1e-9, 1.0}, {-1.0, 1.0}, {(double)sw - 1, 1.0}, {1.0, -1e-9}, {1.0, (double)sh - 1}, {kNaN, 1.0}, {1.0, kNaN}, {2147483648.0, 1.0},
                              {1.0, -2147483648.0}, {kInf, 1.0}};
    for (const auto& uv : outs) { CHECK(pair_pixel(f.data(), sw, sh, true, uv, Ju, 9, 1.0, 0.0, true, 0.0, &t) == kAlignOutside); CHECK(t.r == 0.0); }
    { const double uv[2] = {(double)sw - 2, (double)sh - 2}; CHECK(pair_pixel(f.data(), sw, sh, true, uv, Ju, 9, 1.0, 0.0, false, 0.0, &t) == kAlignUsed); }      // ix = sw - 2: the last cell
    { const double uv[2] = {(double)sw - 1 - 1e-9, (double)sh - 1 - 1e-9}; CHECK(pair_pixel(f.data(), sw, sh, true, uv, Ju, 9, 1.0, 0.0, false, 0.0, &t) == kAlignUsed); }
    { const double uv[2] = {1.0, 1.0}; CHECK(pair_pixel(f.data(), sw, sh, false, uv, Ju, 9, 1.0, 0.0, false, 0.0, &t) == kAlignOutside); }      // no projected point
    // the precedence: outside, masked, skipped, used
    std::vector<uint8_t> z = f;
    z[(size_t)2 * sw + 2] = 0;      // byte (2, 2): in the cells (1, 1), (1, 2), (2, 1), (2, 2)
    { const double uv[2] = {1.5, 1.5}; CHECK(pair_pixel(z.data(), sw, sh, true, uv, Ju, 0, 1.0, 0.0, true, 0.0, &t) == kAlignMasked); }      // masked before skipped
    { const double uv[2] = {1.5, 1.5}; CHECK(pair_pixel(z.data(), sw, sh, true, uv, Ju, 0, 1.0, 0.0, false, 0.0, &t) == kAlignUsed); }       // without skip_zero neither
    { const double uv[2] = {0.5, 0.5}; CHECK(pair_pixel(z.data(), sw, sh, true, uv, Ju, 0, 1.0, 0.0, true, 0.0, &t) == kAlignSkipped); }
    { const double uv[2] = {0.5, 0.5}; CHECK(pair_pixel(z.data(), sw, sh, true, uv, Ju, 1, 1.0, 0.0, true, 0.0, &t) == kAlignUsed); }
    { const double uv[2] = {-0.5, 1.5}; CHECK(pair_pixel(z.data(), sw, sh, true, uv, Ju, 0, 1.0, 0.0, true, 0.0, &t) == kAlignOutside); }    // outside before all
    // the bilinear value between four bytes
    { const double uv[2] = {0.25, 0.5}; CHECK(pair_pixel(f.data(), sw, sh, true, uv, Ju, 0, 1.0, 0.0, false, 0.0, &t) == kAlignUsed && std::fabs(t.r - (10 + 7 * 0.25 + 31 * 0.5)) < 1e-12); }

    // pair_term end to end on a 2 x 2 table of bearings: the identity pair of a frame with itself has r = 0 where it is used
    const int w2 = 4, h2 = 3;
    std::vector<double> lut((size_t)w2 * h2 * 3);
    std::vector<uint8_t> g2((size_t)w2 * h2);
    const PairCamera cam = pair_camera(8.0, 8.0, 1.5, 1.0, nullptr);
    for (int y = 0; y < h2; ++y)
        for (int x = 0; x < w2; ++x) {
            const size_t s = (size_t)y * w2 + x;
            lut[3 * s] = (x - 1.5) / 8.0; lut[3 * s + 1] = (y - 1.0) / 8.0; lut[3 * s + 2] = 1.0;
            g2[s] = (uint8_t)(3 + 5 * s);
        }
    const double I4[4] = {0, 0, 0, 1};
    int used = 0, outside = 0;
    for (int s = 0; s < w2 * h2; ++s) {
        double uv[2];
        const int cls = pair_term(lut.data(), s, I4, cam, g2.data(), w2, h2, g2[(size_t)s], 1.0, 0.0, false, 0.0, uv, &t);
        CHECK(uv[0] == (double)(s % w2) && uv[1] == (double)(s / w2));
        if (cls == kAlignUsed) { ++used; CHECK(t.r == 0.0); } else { ++outside; CHECK(cls == kAlignOutside); }
    }
    CHECK(used == (w2 - 1) * (h2 - 1) && outside == w2 * h2 - used);
    { double uv[2]; const double back[4] = {0, 1, 0, 0}; CHECK(pair_term(lut.data(), 0, back, cam, g2.data(), w2, h2, 1, 1.0, 0.0, false, 0.0, uv, &t) == kAlignOutside && uv[0] != uv[0]); }
}

static void test_start_and_information()
{
    const double qi[4] = {0.0, std::sin(0.1), 0.0, std::cos(0.1)}, qj[4] = {0.0, std::sin(0.25), 0.0, std::cos(0.25)};
    double Q[4], a, b;
    pair_start(qi, qj, 2.0, 10.0, 4.0, -6.0, Q, &a, &b);
    CHECK(std::fabs(Q[1] - std::sin(-0.15)) < 1e-15 && std::fabs(Q[3] - std::cos(0.15)) < 1e-15 && Q[0] == 0.0 && Q[2] == 0.0);
    CHECK(a == 0.5 && b == 4.0);
    pair_start(qi, qi, 1.0, 0.0, 1.0, 0.0, Q, &a, &b);
    CHECK(std::fabs(Q[3] - 1.0) < 1e-15 && std::fabs(Q[1]) < 1e-15 && a == 1.0 && b == 0.0);
    const double sums[10] = {8, 2, 4, 6, 10, 12, 0, 0, 0, 50};
    double info[6];
    pair_information(sums, 28, info);      // s^2 = 50 / 25 = 2
    for (int k = 0; k < 6; ++k) CHECK(info[k] == sums[k] / 2.0);
    pair_information(sums, 3, info);       // max(n - 3, 1) = 1
    for (int k = 0; k < 6; ++k) CHECK(info[k] == sums[k] / 50.0);
    pair_information(sums, 0, info);
    for (int k = 0; k < 6; ++k) CHECK(info[k] == sums[k] / 50.0);
}

int main()
{
    test_args();
    test_projection();
    test_sample_and_classes();
    test_start_and_information();
    if (g_fail) { std::printf("%d checks failed\n", g_fail); return 1; }
    std::printf("OK pair_rule\n");
    return 0;
}
