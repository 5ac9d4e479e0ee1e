// tests/cpp/pair_level_rule_test.cpp — emba_amd/csrc/pair_level_rule.h on a CPU (plain C++17, no HIP; tests/test_pair_level_rule_cpu.py builds and runs it, also
// under the address and undefined-behaviour sanitizers): the refusals in their order, the level sizes, the byte rule against a direct sum (the rounding tie, a
// zero in the box, with and without skip_zero; the cascade of boxes against the direct box), the level camera, the level table behind a pinhole against the
// analytic centre, Ju at a level against central differences, min_pixels per level, the schedule's hand-over and its degenerate end.  Every frame and table
// here is exactly as large as the rule says it reads: a read past it is the sanitizer's to find.
#include "../../emba_amd/csrc/pair_level_rule.h"

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
static const double kNaN = std::numeric_limits<double>::quiet_NaN();
static const double kLens[5] = {-0.3, 0.1, 1e-3, -2e-3, 0.0};

static emba_exposure_settings settings()
{
    emba_exposure_settings xs{};
    xs.align = emba_align_settings{30, 16, 1e-3, 10.0, 10.0, 1e-9, 1e6, 1e-6, 0.0};
    xs.gain_min = 0.25; xs.gain_max = 4.0;
    return xs;
}

// the pinhole table (x', y', 1) of a sensor [sh, sw]
static std::vector<double> pinhole_lut(int sw, int sh, double f, double cu, double cv)
{
    std::vector<double> lut(3 * (size_t)sw * sh);
    for (int y = 0; y < sh; ++y)
        for (int x = 0; x < sw; ++x) {
            double* b = &lut[3 * ((size_t)y * sw + x)];
            b[0] = (x - cu) / f; b[1] = (y - cv) / f; b[2] = 1.0;
        }
    return lut;
}

static void test_refusals()
{
    using L = PairLevelArgStatus;
    static_assert((int)L::ok == 0 && (int)L::levels_null == 1 && (int)L::too_many_levels == 2 && (int)L::level_out_of_range == 3 && (int)L::level_too_small == 4,
                  "the order the C ABI reports them in");
    using S = PairLevelsCallStatus;
    static_assert((int)S::ok == 0 && (int)S::pair_args == 1 && (int)S::levels == 2 && (int)S::estimate == 3 && (int)S::bounds == 4 && (int)S::settings == 5 &&
                  (int)S::bytes == 6, "the order the C ABI reports them in");
    size_t at = 99;
    const int32_t good[3] = {2, 1, 0}, nine[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, eight[8] = {0, 1, 2, 3, 3, 2, 1, 0}, out[3] = {1, 8, -1}, neg[2] = {0, -1};
    const int32_t small[3] = {0, 4, 5};
    CHECK(pair_levels_ok(good, 3, 64, 48, &at) == L::ok);
    CHECK(pair_levels_ok(eight, 8, 64, 48, &at) == L::ok);       // any order, a level twice
    CHECK(pair_levels_ok(nullptr, 3, 64, 48, &at) == L::levels_null && pair_levels_ok(good, 0, 64, 48, &at) == L::levels_null);
    CHECK(pair_levels_ok(nine, 9, 64, 48, &at) == L::too_many_levels);
    CHECK(pair_levels_ok(out, 3, 1, 1, &at) == L::level_out_of_range && at == 1);      // (also too small: the range is reported first)
    CHECK(pair_levels_ok(neg, 2, 64, 48, &at) == L::level_out_of_range && at == 1);
    CHECK(pair_levels_ok(small, 3, 20, 13, &at) == L::level_too_small && at == 1);     // 20 x 13: level 3 is 2 x 1, level 4 is 1 x 0
    const int32_t l3[1] = {3}, l2[1] = {2};
    CHECK(pair_levels_ok(l3, 1, 20, 13, &at) == L::level_too_small && at == 0 && pair_levels_ok(l2, 1, 20, 13, &at) == L::ok);
    // the call: each refusal with every later one also wrong
    emba_exposure_settings ok = settings(), bad_bounds = ok, bad_set = ok, bad_both = ok;
    bad_bounds.gain_min = 2.0; bad_set.align.min_pixels = 2; bad_both.gain_max = kNaN; bad_both.align.lambda0 = 0.0;
    const size_t bigF = kPairMaxBytes / 64 + 1;
    CHECK(pair_levels_call_ok(PairArgStatus::ok, L::ok, 3, &ok, 4, 64) == S::ok);
    CHECK(pair_levels_call_ok(PairArgStatus::bad_q, L::levels_null, 4, &bad_both, bigF, 64) == S::pair_args);
    CHECK(pair_levels_call_ok(PairArgStatus::ok, L::level_too_small, 4, &bad_both, bigF, 64) == S::levels);
    CHECK(pair_levels_call_ok(PairArgStatus::ok, L::ok, 4, &bad_both, bigF, 64) == S::estimate && pair_levels_call_ok(PairArgStatus::ok, L::ok, -1, &ok, 4, 64) == S::estimate);
    CHECK(pair_levels_call_ok(PairArgStatus::ok, L::ok, 3, &bad_both, bigF, 64) == S::bounds && pair_levels_call_ok(PairArgStatus::ok, L::ok, 0, &bad_bounds, 4, 64) == S::bounds);
    CHECK(pair_levels_call_ok(PairArgStatus::ok, L::ok, 3, &bad_set, bigF, 64) == S::settings && pair_levels_call_ok(PairArgStatus::ok, L::ok, 3, nullptr, bigF, 64) == S::settings);
    CHECK(pair_levels_call_ok(PairArgStatus::ok, L::ok, 3, &ok, bigF, 64) == S::bytes);
}

static void test_sizes()
{
    const int want64[8][2] = {{64, 48}, {32, 24}, {16, 12}, {8, 6}, {4, 3}, {2, 1}, {1, 0}, {0, 0}};
    for (int l = 0; l < 8; ++l) {
        CHECK(pair_level_dim(64, l) == want64[l][0] && pair_level_dim(48, l) == want64[l][1]);
        CHECK(pair_level_size_ok(64, 48, l) == (l <= 4));
    }
    CHECK(pair_level_dim(20, 1) == 10 && pair_level_dim(13, 1) == 6 && pair_level_dim(20, 2) == 5 && pair_level_dim(13, 2) == 3);      // 13: a row dropped
    CHECK(pair_level_size_ok(20, 13, 2) && !pair_level_size_ok(20, 13, 3));
    CHECK(pair_level_size_ok(8, 8, 2) && !pair_level_size_ok(8, 8, 3) && !pair_level_size_ok(8, 8, 8) && !pair_level_size_ok(8, 8, -1));
    CHECK(pair_level_size_ok(256, 256, 7) && !pair_level_size_ok(255, 256, 7));
}

static void test_bytes()
{
    // the rounding: (sum + 4^l / 2) >> 2l; the tie goes up
    CHECK(pair_box_byte(1 + 2 + 2 + 1, 1, false) == 2 && pair_box_byte(1 + 2 + 2 + 2, 1, false) == 2 && pair_box_byte(1 + 1 + 2 + 1, 1, false) == 1);
    CHECK(pair_box_byte(4 * 255, 1, true) == 255 && pair_box_byte(255u * 16384u, 7, true) == 255 && pair_box_byte(7, 0, false) == 7);
    // a zero in the box: 0 under skip_zero, the rounded mean without; a box without a zero gives 1 at the least
    const uint32_t z = pair_box_join(pair_box_of_byte(0), pair_box_of_byte(200), pair_box_of_byte(200), pair_box_of_byte(200));
    CHECK((z & kPairBoxZero) && pair_box_byte(z, 1, true) == 0 && pair_box_byte(z, 1, false) == 150);
    CHECK(pair_box_byte(pair_box_join(1, 1, 1, 1), 1, true) == 1 && pair_box_byte(16384u, 7, true) == 1);
    CHECK(pair_box_byte(pair_box_join(pair_box_of_byte(0), pair_box_of_byte(0), pair_box_of_byte(0), pair_box_of_byte(0)), 1, false) == 0);
    // a 20 x 13 frame: every level against a direct sum, and the cascade of boxes against the direct box
    const int sw = 20, sh = 13;
    std::vector<uint8_t> fr((size_t)sw * sh);
    uint32_t rnd = 12345;
    for (auto& v : fr) { rnd = rnd * 1664525u + 1013904223u; v = (uint8_t)((rnd >> 24) % 7 == 0 ? 0 : rnd >> 24); }
    for (int skip = 0; skip < 2; ++skip)
        for (int l = 0; l <= 2; ++l) {
            const int wl = sw >> l, hl = sh >> l, n = 1 << l;
            std::vector<uint8_t> out((size_t)wl * hl);      // (exactly the level's size)
            pair_level_bytes(fr.data(), sw, sh, l, skip != 0, out.data());
            for (int Y = 0; Y < hl; ++Y)
                for (int X = 0; X < wl; ++X) {
                    unsigned sum = 0;
                    bool zero = false;
                    for (int y = Y * n; y < (Y + 1) * n; ++y)
                        for (int x = X * n; x < (X + 1) * n; ++x) { sum += fr[(size_t)y * sw + x]; zero = zero || !fr[(size_t)y * sw + x]; }
                    const unsigned want = l == 0 ? fr[(size_t)Y * sw + X] : (skip && zero) ? 0u : (sum + (unsigned)(n * n) / 2) / (unsigned)(n * n);
                    CHECK(out[(size_t)Y * wl + X] == want);
                    if (l == 2) {
                        const uint32_t c = pair_box_join(pair_box_direct(fr.data(), sw, 2 * X, 2 * Y, 1), pair_box_direct(fr.data(), sw, 2 * X + 1, 2 * Y, 1),
                                                         pair_box_direct(fr.data(), sw, 2 * X, 2 * Y + 1, 1), pair_box_direct(fr.data(), sw, 2 * X + 1, 2 * Y + 1, 1));
                        CHECK(c == pair_box_direct(fr.data(), sw, X, Y, 2));
                    }
                }
        }
}

static void test_camera_and_table()
{
    const PairCamera c = pair_camera(33.3, 31.7, 30.9, 23.1, kLens);
    const PairCamera c0 = pair_level_camera(c, 0);
    CHECK(same_bits(c0.fu, c.fu) && same_bits(c0.fv, c.fv) && same_bits(c0.cu, c.cu) && same_bits(c0.cv, c.cv));
    for (int k = 0; k < 5; ++k) CHECK(same_bits(c0.D[k], c.D[k]));
    // a point's u_l against (u - (2^l - 1) / 2) / 2^l
    const double rb[3] = {0.21, -0.13, 1.1};
    double uv[2], J[6];
    CHECK(pair_project(c, rb, uv, J));
    for (int l = 1; l <= 4; ++l) {
        const PairCamera cl = pair_level_camera(c, l);
        double uvl[2], Jl[6];
        CHECK(pair_project(cl, rb, uvl, Jl));
        const double n = (double)(1 << l), half = (n - 1.0) / 2.0;
        CHECK(std::fabs(uvl[0] - (uv[0] - half) / n) < 1e-13 && std::fabs(uvl[1] - (uv[1] - half) / n) < 1e-13);
        for (int k = 0; k < 5; ++k) CHECK(same_bits(cl.D[k], c.D[k]));
    }
    // the level table behind a pinhole against the analytic centre: box (X, Y) is centred at X 2^l + (2^l - 1) / 2
    const int sw = 20, sh = 13;
    const double f = 10.0, cu = 9.5, cv = 6.0;
    const std::vector<double> lut = pinhole_lut(sw, sh, f, cu, cv);
    for (int l = 0; l <= 2; ++l) {
        const int wl = sw >> l, hl = sh >> l;
        std::vector<double> tl(3 * (size_t)wl * hl);
        pair_level_lut(lut.data(), sw, sh, l, tl.data());
        const double n = (double)(1 << l), half = (n - 1.0) / 2.0;
        for (int Y = 0; Y < hl; ++Y)
            for (int X = 0; X < wl; ++X) {
                const double* b = &tl[3 * ((size_t)Y * wl + X)];
                CHECK(std::fabs(b[0] - (X * n + half - cu) / f) < 1e-15 && std::fabs(b[1] - (Y * n + half - cv) / f) < 1e-15 && b[2] == 1.0);
                if (l == 0) CHECK(same_bits(b[0], lut[3 * ((size_t)Y * sw + X)]));
                // ... so the level's camera puts the level's bearing on the level pixel
                const PairCamera cl = pair_level_camera(pair_camera(f, f, cu, cv, nullptr), l);
                double p[2], Jp[6];
                CHECK(pair_project(cl, b, p, Jp) && std::fabs(p[0] - X) < 1e-12 && std::fabs(p[1] - Y) < 1e-12);
            }
    }
}

static void test_jacobian_at_a_level()
{
    // Ju of the level's camera against central differences of the level's uv in delta (Q <- exp(delta) Q), under the lens
    const PairCamera cl = pair_level_camera(pair_camera(32.0, 33.0, 31.5, 23.5, kLens), 2);
    const double b[3] = {0.3, -0.2, 1.0}, Q[4] = {0.02, -0.03, 0.01, 0.9993};
    double n = std::sqrt(Q[0] * Q[0] + Q[1] * Q[1] + Q[2] * Q[2] + Q[3] * Q[3]);
    const double q[4] = {Q[0] / n, Q[1] / n, Q[2] / n, Q[3] / n};
    double rb[3], uv[2], J23[6], Ju[6];
    pair_turn(q, b, rb);
    CHECK(pair_project(cl, rb, uv, J23));
    pair_left_jacobian(J23, rb, Ju);
    const double h = 1e-6;
    for (int k = 0; k < 3; ++k) {
        double up[2], um[2], Jx[6];
        for (int sgn = -1; sgn <= 1; sgn += 2) {
            double d[3] = {0, 0, 0}, qt[4], r2[3];
            d[k] = sgn * h;
            align_apply(d, q, qt);
            pair_turn(qt, b, r2);
            CHECK(pair_project(cl, r2, sgn > 0 ? up : um, Jx));
        }
        CHECK(std::fabs((up[0] - um[0]) / (2 * h) - Ju[k]) < 1e-6 * (1.0 + std::fabs(Ju[k])));
        CHECK(std::fabs((up[1] - um[1]) / (2 * h) - Ju[3 + k]) < 1e-6 * (1.0 + std::fabs(Ju[3 + k])));
    }
}

static void test_min_pixels()
{
    CHECK(pair_level_min_pixels(16, 0) == 16 && pair_level_min_pixels(16, 1) == 8 && pair_level_min_pixels(16, 2) == 8 && pair_level_min_pixels(16, 7) == 8);
    CHECK(pair_level_min_pixels(1000, 1) == 250 && pair_level_min_pixels(1000, 2) == 62 && pair_level_min_pixels(1000, 3) == 15 && pair_level_min_pixels(1000, 4) == 8);
    CHECK(pair_level_min_pixels(5, 0) == 5 && pair_level_min_pixels(5, 3) == 5 && pair_level_min_pixels(3, 7) == 3);
    const emba_exposure_settings xs = settings(), x2 = pair_level_settings(xs, 2);
    CHECK(x2.align.min_pixels == 8 && x2.align.max_iters == xs.align.max_iters && x2.align.lambda0 == xs.align.lambda0 && x2.gain_min == xs.gain_min &&
          x2.gain_max == xs.gain_max && x2.align.tol_rot == xs.align.tol_rot);
}

// a smooth textured 64 x 48 frame and the same scene turned by a small rotation, behind the pinhole of focal length 32
static double scene(double x, double y) { return 128.0 + 60.0 * std::sin(0.11 * x + 0.3) * std::cos(0.09 * y - 0.2) + 40.0 * std::sin(0.05 * x - 0.07 * y); }

static void test_schedule()
{
    const int sw = 64, sh = 48;
    const PairCamera cam = pair_camera(32.0, 32.0, 31.5, 23.5, nullptr);
    const std::vector<double> lut = pinhole_lut(sw, sh, 32.0, 31.5, 23.5);
    const double d[3] = {0.02, -0.015, 0.01}, id[4] = {0, 0, 0, 1};
    double Qt[4];
    align_apply(d, id, Qt);      // the true relative rotation: a bearing b of the source is R(Qt) b of the target
    std::vector<uint8_t> src((size_t)sw * sh), tgt((size_t)sw * sh);
    for (int y = 0; y < sh; ++y)
        for (int x = 0; x < sw; ++x) {
            // the target sees scene(u, v); the source pixel s sees what the target sees where s lands
            double rb[3], uv[2], J[6];
            pair_turn(Qt, &lut[3 * ((size_t)y * sw + x)], rb);
            pair_project(cam, rb, uv, J);
            const double a = 1.1, b = -7.0;      // the source's exposure against the target: v_tgt = a v_src + b
            tgt[(size_t)y * sw + x] = (uint8_t)std::lrint(scene(x, y));
            src[(size_t)y * sw + x] = (uint8_t)std::lrint((scene(uv[0], uv[1]) - b) / a);
        }
    const emba_exposure_settings xs = settings();
    const int32_t one[1] = {0}, three[3] = {2, 1, 0};
    // the hand-over: level k + 1 starts where level k ended — run (2), then (1) from its end, then (0) from that: the schedule (2, 1, 0) bit for bit
    const PairLevelsResult all = pair_levels_align(lut.data(), src.data(), tgt.data(), sw, sh, cam, id, 1.0, 0.0, false, three, 3, 3, xs);
    PairLevelsResult step{};
    double q[4] = {0, 0, 0, 1}, a = 1.0, b = 0.0;
    int32_t total = 0;
    for (int k = 0; k < 3; ++k) {
        step = pair_levels_align(lut.data(), src.data(), tgt.data(), sw, sh, cam, q, a, b, false, three + k, 1, 3, xs);
        CHECK(step.level_status[0] == all.level_status[k] && step.level_iters[0] == all.level_iters[k]);
        for (int i = 0; i < 4; ++i) q[i] = step.q[i];
        a = step.gain; b = step.bias; total += step.iters;
    }
    for (int i = 0; i < 4; ++i) CHECK(same_bits(step.q[i], all.q[i]));
    for (int i = 0; i < kExposureSums; ++i) CHECK(same_bits(step.sums[i], all.sums[i]));
    for (int i = 0; i < 6; ++i) CHECK(same_bits(step.info[i], all.info[i]));
    CHECK(same_bits(step.gain, all.gain) && same_bits(step.bias, all.bias) && total == all.iters && step.status == all.status && step.counts[0] == all.counts[0]);
    CHECK(all.status == EMBA_ALIGN_CONVERGED && all.iters == all.level_iters[0] + all.level_iters[1] + all.level_iters[2]);
    // it ends at the truth: the rotation within a milliradian, the exposure within a few per cent and a few bytes
    const double dq = 2.0 * std::sqrt((all.q[0] - Qt[0]) * (all.q[0] - Qt[0]) + (all.q[1] - Qt[1]) * (all.q[1] - Qt[1]) + (all.q[2] - Qt[2]) * (all.q[2] - Qt[2]));
    std::printf("schedule (2, 1, 0): status %d iters %d (%d %d %d) angle %.3e gain %.4f bias %.3f\n", all.status, all.iters, all.level_iters[0], all.level_iters[1],
                all.level_iters[2], dq, all.gain, all.bias);
    CHECK(dq < 1e-3 && std::fabs(all.gain - 1.1) < 0.02 && std::fabs(all.bias + 7.0) < 2.0);
    // cost0 and n0 are the first level's: level 2 is 16 x 12
    const PairLevelsResult first = pair_levels_align(lut.data(), src.data(), tgt.data(), sw, sh, cam, id, 1.0, 0.0, false, three, 1, 3, xs);
    CHECK(same_bits(all.cost0, first.cost0) && all.n0 == first.n0 && all.n0 <= 16 * 12 && all.n0 > 100);
    // level 0 alone with estimate = 0 is the loop of align_step on the ten shared sums: the ten sums of exposure_accumulate are align_accumulate's bits
    const PairLevelsResult l0 = pair_levels_align(lut.data(), src.data(), src.data(), sw, sh, cam, Qt, 1.0, 0.0, false, one, 1, 0, xs);
    {
        AlignFrame f;
        align_frame_init(&f, Qt, xs.align.lambda0);
        while (f.status == EMBA_ALIGN_RUNNING) {
            double es[kAlignSums] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
            uint64_t ec[4] = {0, 0, 0, 0};
            for (int s = 0; s < sw * sh; ++s) {
                double uv[2];
                AlignTerm t;
                const int cls = pair_term(lut.data(), s, f.q_trial, cam, src.data(), sw, sh, src[s], 1.0, 0.0, false, 0.0, uv, &t);
                if (cls == kAlignUsed) align_accumulate(t, es);
                ++ec[cls];
            }
            align_step(&f, es, ec, xs.align);
        }
        double ten[kAlignSums];
        exposure_shared_sums(l0.sums, ten);
        for (int i = 0; i < 4; ++i) CHECK(same_bits(f.q[i], l0.q[i]));
        for (int i = 0; i < kAlignSums; ++i) CHECK(same_bits(f.sums[i], ten[i]));
        CHECK(f.status == l0.status && f.iters == l0.iters && f.counts[0] == l0.counts[0] && l0.gain == 1.0 && l0.bias == 0.0);
    }
    // the degenerate end: a frame of one constant byte with estimate = 3 (gain and bias collinear) ends the pair at its first level, where it started
    std::vector<uint8_t> flat((size_t)sw * sh, 90);
    const PairLevelsResult deg = pair_levels_align(lut.data(), flat.data(), tgt.data(), sw, sh, cam, Qt, 1.2, 3.0, false, three, 3, 3, xs);
    CHECK(deg.status == EMBA_ALIGN_DEGENERATE && deg.level_status[0] == EMBA_ALIGN_DEGENERATE && deg.level_status[1] == 0 && deg.level_status[2] == 0);
    CHECK(deg.iters == 0 && deg.level_iters[1] == 0 && deg.gain == 1.2 && deg.bias == 3.0 && deg.n0 == deg.counts[0] && deg.n0 > 0);
    for (int i = 0; i < 4; ++i) CHECK(same_bits(deg.q[i], Qt[i]));
    // ... and with the bias alone it is a pair like any other
    const PairLevelsResult bias = pair_levels_align(lut.data(), flat.data(), tgt.data(), sw, sh, cam, Qt, 1.0, 0.0, false, three, 3, 2, xs);
    CHECK(bias.level_status[0] != 0 && bias.gain == 1.0);
    CHECK(pair_level_hands_on(EMBA_ALIGN_CONVERGED) && pair_level_hands_on(EMBA_ALIGN_STALLED) && pair_level_hands_on(EMBA_ALIGN_ITERATIONS) &&
          !pair_level_hands_on(EMBA_ALIGN_DEGENERATE));
}

int main()
{
    test_refusals();
    test_sizes();
    test_bytes();
    test_camera_and_table();
    test_jacobian_at_a_level();
    test_min_pixels();
    test_schedule();
    if (g_fail) { std::printf("%d checks failed\n", g_fail); return 1; }
    std::printf("OK pair_level_rule\n");
    return 0;
}
