// tests/cpp/track_rule_test.cpp — emba_amd/csrc/track_rule.h on a CPU (plain C++17, no HIP; tests/test_track_rule_cpu.py builds and runs it, also under the
// address and undefined-behaviour sanitizers): every argument refusal in the order the C ABI reports them, the geometry of a level at l = 0 and at the last
// level a panorama allows, the planes a frame votes into, the batches at F = 1, F = batch, F = batch + 1 and across a chunk edge, the prediction with zero,
// one and two tracked frames and unequal time gaps, one pixel against two hand-written sums, and the verdict at overlap == min_overlap and behind a
// degenerate last level.  Every plane here is exactly as large as the rule says it reads: a read past it is the sanitizer's to find.
#include "../../emba_amd/csrc/track_rule.h"

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

static emba_track_settings settings()
{
    emba_track_settings s;
    std::memset(&s, 0, sizeof s);
    s.n_levels = 3; s.levels[0] = 2; s.levels[1] = 1; s.levels[2] = 0;
    s.batch = 4; s.predict = 1; s.skip_zero = 1; s.min_weight = 256; s.min_overlap = 0.5;
    s.align.max_iters = 10; s.align.min_pixels = 3;
    s.align.lambda0 = 1e-3; s.align.lambda_up = 10.0; s.align.lambda_down = 10.0; s.align.lambda_min = 1e-9; s.align.lambda_max = 1e6; s.align.tol_rot = 1e-6;
    s.align.huber_k = 0.0;
    return s;
}

static void test_args()
{
    using A = TrackArgStatus;
    static_assert((int)A::ok == 0 && (int)A::frames_null == 1 && (int)A::times_null == 2 && (int)A::q0_null == 3 && (int)A::settings_null == 4 &&
                  (int)A::too_many_frames == 5 && (int)A::schedule_length == 6 && (int)A::level_range == 7 && (int)A::level_not_divisible == 8 &&
                  (int)A::level_too_few_rows == 9 && (int)A::bad_batch == 10 && (int)A::bad_min_overlap == 11 && (int)A::bad_min_weight == 12 &&
                  (int)A::times_not_increasing == 13 && (int)A::bad_q0 == 14 && (int)A::bad_align_settings == 15 && (int)A::too_many_votes == 16,
                  "the order the C ABI reports them in");
    const double nan = std::numeric_limits<double>::quiet_NaN();
    const double q0[4] = {0, 0, 0, 2}, qz[4] = {0, 0, 0, 0}, qn[4] = {0, nan, 0, 1};
    const int64_t t[4] = {10, 20, 30, 40}, tbad[4] = {10, 20, 20, 40};
    const size_t big = (size_t)1 << 31, S = 35;
    size_t where = 99;
    emba_track_settings s = settings();
    CHECK(track_args_ok(true, true, q0, &s, t, 4, S, 32, 16, &where) == A::ok && where == 0);
    CHECK(track_args_ok(false, false, nullptr, nullptr, nullptr, 0, S, 32, 16, &where) == A::q0_null);      // F = 0: frames and times are not read
    CHECK(track_args_ok(false, false, q0, &s, nullptr, 0, S, 32, 16, nullptr) == A::ok);
    // every refusal, each with everything behind it wrong as well
    emba_track_settings bad = s;
    bad.n_levels = 0; bad.batch = 0; bad.min_overlap = nan; bad.min_weight = 0; bad.align.lambda0 = 0.0;
    CHECK(track_args_ok(false, false, nullptr, nullptr, nullptr, big, S, 32, 16, &where) == A::frames_null);
    CHECK(track_args_ok(true, false, nullptr, nullptr, nullptr, big, S, 32, 16, &where) == A::times_null);
    CHECK(track_args_ok(true, true, nullptr, nullptr, tbad, big, S, 32, 16, &where) == A::q0_null);
    CHECK(track_args_ok(true, true, qz, nullptr, tbad, big, S, 32, 16, &where) == A::settings_null);
    CHECK(track_args_ok(true, true, qz, &bad, tbad, big, S, 32, 16, &where) == A::too_many_frames);
    CHECK(track_args_ok(true, true, qz, &bad, tbad, 4, S, 32, 16, &where) == A::schedule_length);
    bad.n_levels = 9;
    CHECK(track_args_ok(true, true, qz, &bad, tbad, 4, S, 32, 16, &where) == A::schedule_length);
    bad.n_levels = 3; bad.levels[1] = 8;
    CHECK(track_args_ok(true, true, qz, &bad, tbad, 4, S, 32, 16, &where) == A::level_range && where == 1);
    bad.levels[1] = -1;
    CHECK(track_args_ok(true, true, qz, &bad, tbad, 4, S, 32, 16, &where) == A::level_range && where == 1);
    bad.levels[1] = 1; bad.levels[2] = 2;
    CHECK(track_args_ok(true, true, qz, &bad, tbad, 4, S, 34, 16, &where) == A::level_not_divisible && where == 0);      // 34 is not divisible by 4
    CHECK(track_args_ok(true, true, qz, &bad, tbad, 4, S, 32, 18, &where) == A::level_not_divisible && where == 0);
    bad.levels[0] = 1; bad.levels[2] = 4;
    CHECK(track_args_ok(true, true, qz, &bad, tbad, 4, S, 32, 16, &where) == A::level_too_few_rows && where == 2);       // 16 >> 4 = 1 row
    bad.levels[2] = 0;
    CHECK(track_args_ok(true, true, qz, &bad, tbad, 4, S, 32, 16, &where) == A::bad_batch && where == 0);
    bad.batch = 1;
    CHECK(track_args_ok(true, true, qz, &bad, tbad, 4, S, 32, 16, &where) == A::bad_min_overlap);
    bad.min_overlap = 1.5;
    CHECK(track_args_ok(true, true, qz, &bad, tbad, 4, S, 32, 16, &where) == A::bad_min_overlap);
    bad.min_overlap = -0.1;
    CHECK(track_args_ok(true, true, qz, &bad, tbad, 4, S, 32, 16, &where) == A::bad_min_overlap);
    bad.min_overlap = 1.0;
    CHECK(track_args_ok(true, true, qz, &bad, tbad, 4, S, 32, 16, &where) == A::bad_min_weight);
    bad.min_weight = 1;
    CHECK(track_args_ok(true, true, qz, &bad, tbad, 4, S, 32, 16, &where) == A::times_not_increasing && where == 2);
    CHECK(track_args_ok(true, true, qz, &bad, tbad, 2, S, 32, 16, &where) == A::bad_q0);      // (the first two times do increase)
    CHECK(track_args_ok(true, true, qn, &bad, t, 4, S, 32, 16, &where) == A::bad_q0);
    CHECK(track_args_ok(true, true, q0, &bad, t, 4, S, 32, 16, &where) == A::bad_align_settings);
    bad.align.lambda0 = 1e-3; bad.align.huber_k = nan;
    CHECK(track_args_ok(true, true, q0, &bad, t, 4, S, 32, 16, &where) == A::bad_align_settings);
    bad.align.huber_k = 0.0;
    CHECK(track_args_ok(true, true, q0, &bad, t, 4, (size_t)1 << 34, 32, 16, &where) == A::too_many_votes);             // 4 * 2^34 = 2^36
    CHECK(track_args_ok(true, true, q0, &bad, t, 3, (size_t)1 << 34, 32, 16, &where) == A::ok);
}

static void test_levels()
{
    using L = TrackLevelStatus;
    TrackLevel g{};
    CHECK(track_level(32, 16, 0, &g) == L::ok && g.W == 32 && g.H == 16 && g.scale == 1.0);
    CHECK(track_level(32, 16, 3, &g) == L::ok && g.W == 4 && g.H == 2 && g.scale == 0.125);      // the last level 32 x 16 allows
    CHECK(track_level(32, 16, 4, &g) == L::too_few_rows && g.W == 4);                              // H_l = 1; g is left alone
    CHECK(track_level(32, 16, 5, nullptr) == L::not_divisible);                                    // 16 is not divisible by 32
    CHECK(track_level(2048, 1024, 7, &g) == L::ok && g.W == 16 && g.H == 8 && g.scale == 1.0 / 128.0);
    CHECK(track_level(2048, 1024, 8, nullptr) == L::out_of_range && track_level(32, 16, -1, nullptr) == L::out_of_range);
    CHECK(track_level(36, 16, 2, nullptr) == L::ok && track_level(36, 16, 3, nullptr) == L::not_divisible && track_level(32, 12, 3, nullptr) == L::not_divisible);
    CHECK(track_level(48, 3, 0, nullptr) == L::ok && track_level(48, 1, 0, nullptr) == L::too_few_rows);
    // the planes a frame votes into
    emba_track_settings s = settings();
    int lv[kTrackMaxPlanes];
    CHECK(track_vote_levels(s, lv) == 3 && lv[0] == 2 && lv[1] == 1 && lv[2] == 0);
    s.n_levels = 2;
    CHECK(track_vote_levels(s, lv) == 3 && lv[0] == 2 && lv[1] == 1 && lv[2] == 0);      // level 0 is voted whether the schedule names it or not
    s.n_levels = 8;
    for (int i = 0; i < 8; ++i) s.levels[i] = i < 4 ? 3 : 1;                              // a level named twice has one plane
    CHECK(track_vote_levels(s, lv) == 3 && lv[0] == 3 && lv[1] == 1 && lv[2] == 0);
    for (int i = 0; i < 8; ++i) s.levels[i] = 7 - i;
    CHECK(track_vote_levels(s, lv) == 8 && lv[7] == 0);
    for (int i = 0; i < 8; ++i) s.levels[i] = i == 7 ? 7 : i + 1;
    CHECK(track_vote_levels(s, lv) == 8 && lv[7] == 0);                                   // 1 ... 7 and level 0: eight planes, nine at the most by the bound
}

static std::vector<size_t> plan(size_t F, size_t per, size_t batch)
{
    std::vector<size_t> out;
    for (size_t f0 = 0; f0 < F;) { const size_t n = track_batch_frames(f0, F, per, batch); out.push_back(n); if (!n) break; f0 += n; }
    return out;
}
static void test_batches()
{
    CHECK((plan(1, 100, 4) == std::vector<size_t>{1}));                      // F = 1: the anchor alone
    CHECK((plan(4, 100, 4) == std::vector<size_t>{1, 3}));                   // F = batch
    CHECK((plan(5, 100, 4) == std::vector<size_t>{1, 4}));                   // F = batch + 1: the anchor and one whole batch
    CHECK((plan(6, 100, 4) == std::vector<size_t>{1, 4, 1}));
    CHECK((plan(5, 100, 1) == std::vector<size_t>{1, 1, 1, 1, 1}));
    CHECK((plan(12, 7, 4) == std::vector<size_t>{1, 4, 2, 4, 1}));           // a chunk edge at 7 inside the batch [5, 9): cut into [5, 7) and the next batch starts at 7
    CHECK((plan(8, 7, 100) == std::vector<size_t>{1, 6, 1}));
    CHECK((plan(3, 1, 4) == std::vector<size_t>{1, 1, 1}));                  // chunks of one frame
    size_t sum = 0;
    for (size_t n : plan(65538, 65535, 1000)) sum += n;
    CHECK(sum == 65538);
}

static double angle_between(const double* a, const double* b)
{
    double w[3];
    track_log_between(a, b, w);
    return std::sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
}
static void test_predict()
{
    const double axis[3] = {0.6, 0.0, 0.8}, id[4] = {0, 0, 0, 1};
    auto rot = [&](double angle, double* q) { const double d[3] = {axis[0] * angle, axis[1] * angle, axis[2] * angle}; align_apply(d, id, q); };
    double qa[4], qb[4], q[4] = {9, 9, 9, 9}, want[4];
    rot(0.10, qa); rot(0.30, qb);
    CHECK(!track_predict(0, qa, 0, qb, 0, 5, true, q) && q[0] == 9 && q[3] == 9);                    // no tracked frame: nothing to start from
    CHECK(track_predict(1, qa, 0, qb, 20, 30, true, q) && std::memcmp(q, qb, sizeof q) == 0);        // one: q_b
    CHECK(track_predict(2, qa, 10, qb, 20, 30, false, q) && std::memcmp(q, qb, sizeof q) == 0);      // predict off: q_b
    CHECK(track_predict(2, qa, 10, qb, 20, 30, true, q));                                            // equal gaps: 0.2 rad further
    rot(0.50, want);
    CHECK(angle_between(q, want) < 1e-12);
    CHECK(track_predict(2, qa, 10, qb, 20, 25, true, q));                                            // unequal gaps: half a gap is 0.1 rad
    rot(0.40, want);
    CHECK(angle_between(q, want) < 1e-12);
    CHECK(track_predict(2, qa, 10, qb, 20, 50, true, q));                                            // a lost frame (or two) in between: three gaps, 0.6 rad
    rot(0.90, want);
    CHECK(angle_between(q, want) < 1e-12);
    CHECK(std::fabs(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3] - 1.0) < 1e-15);
    // -q_b is the same rotation: the short way round
    double nb[4] = {-qb[0], -qb[1], -qb[2], -qb[3]};
    CHECK(track_predict(2, qa, 10, nb, 20, 30, true, q));
    rot(0.50, want);
    CHECK(angle_between(q, want) < 1e-12);
    // no motion: the start is q_b
    CHECK(track_predict(2, qb, 10, qb, 20, 30, true, q) && angle_between(q, qb) < 1e-15);
    double n[4];
    const double q2[4] = {0, 0, 0, 2};
    track_normalise(q2, n);
    CHECK(n[3] == 1.0 && n[0] == 0.0);
}

static void test_pixel()
{
    // a level of 4 x 3 cells; cell (row 1, column 3) is thin: weight 255 < 256
    const int W = 4, H = 3;
    std::vector<uint64_t> sw(W * H, 512), sv(W * H);
    for (int i = 0; i < W * H; ++i) sv[i] = 512 * (uint64_t)(10 * (i / W) + (i % W));      // mean = 10 row + column
    sw[1 * W + 3] = 255;
    const double J23[6] = {1, 0, 0, 0, 1, 0};
    AlignTerm t;
    CHECK(track_pixel(sw.data(), sv.data(), W, H, 0.25, 0.5, J23, 7, 256, true, 0.0, &t) == kAlignUsed);
    CHECK(same_bits(t.r, (0.5 * (0.75 * 0.0 + 0.25 * 1.0) + 0.5 * (0.75 * 10.0 + 0.25 * 11.0)) - 7.0) && t.g[0] == 1.0 && t.g[1] == 10.0 && t.g[2] == 0.0);
    CHECK(track_pixel(sw.data(), sv.data(), W, H, 2.5, 0.5, J23, 7, 256, true, 0.0, &t) == kAlignMasked && t.r == 0.0);      // the thin cell is one of the four
    CHECK(track_pixel(sw.data(), sv.data(), W, H, 3.5, 0.5, J23, 7, 256, true, 0.0, &t) == kAlignMasked);                    // ... also through the wrapped column
    CHECK(track_pixel(sw.data(), sv.data(), W, H, 2.5, 0.5, J23, 7, 255, true, 0.0, &t) == kAlignUsed);                      // min_weight = 255 covers it
    CHECK(track_pixel(sw.data(), sv.data(), W, H, 3.5, 0.0, J23, 0, 256, true, 0.0, &t) == kAlignMasked);                    // masked before skipped
    CHECK(track_pixel(sw.data(), sv.data(), W, H, 0.5, 1.0, J23, 0, 256, true, 0.0, &t) == kAlignSkipped);
    CHECK(track_pixel(sw.data(), sv.data(), W, H, 0.5, 1.0, J23, 0, 256, false, 0.0, &t) == kAlignUsed && same_bits(t.r, (0.5 * 10.0 + 0.5 * 11.0)));
    CHECK(track_pixel(sw.data(), sv.data(), W, H, 0.5, 2.0, J23, 7, 256, true, 0.0, &t) == kAlignOutside);                   // iy + 1 > H - 1
    CHECK(track_pixel(sw.data(), sv.data(), W, H, 0.5, -0.1, J23, 0, 256, true, 0.0, &t) == kAlignOutside);                  // outside before masked before skipped
    CHECK(track_pixel(sw.data(), sv.data(), W, H, -0.5, 1.0, J23, 7, 256, true, 0.0, &t) == kAlignMasked);                   // columns 3 and 0 of rows 1 and 2
}

static void test_verdict()
{
    CHECK(track_overlap(50, 0, 100) == 0.5 && track_overlap(30, 40, 100) == 0.5 && track_overlap(0, 100, 100) == 0.0 && track_overlap(0, 0, 0) == 0.0);
    CHECK(track_verdict(EMBA_ALIGN_CONVERGED, 0.5, 0.5) == EMBA_TRACK_TRACKED);                               // overlap == min_overlap is enough
    CHECK(track_verdict(EMBA_ALIGN_CONVERGED, std::nextafter(0.5, 0.0), 0.5) == EMBA_TRACK_LOST);
    CHECK(track_verdict(EMBA_ALIGN_STALLED, 1.0, 0.5) == EMBA_TRACK_TRACKED && track_verdict(EMBA_ALIGN_ITERATIONS, 1.0, 0.5) == EMBA_TRACK_TRACKED);
    CHECK(track_verdict(EMBA_ALIGN_DEGENERATE, 1.0, 0.0) == EMBA_TRACK_LOST);                                 // a degenerate last level, whatever the overlap
    CHECK(track_verdict(EMBA_ALIGN_CONVERGED, 0.0, 0.0) == EMBA_TRACK_TRACKED);
    CHECK(track_votes(EMBA_TRACK_ANCHOR) && track_votes(EMBA_TRACK_TRACKED) && !track_votes(EMBA_TRACK_LOST) && !track_votes(0));
}

int main()
{
    test_args();
    test_levels();
    test_batches();
    test_predict();
    test_pixel();
    test_verdict();
    if (g_fail) { std::printf("%d checks failed\n", g_fail); return 1; }
    std::printf("OK track_rule\n");
    return 0;
}
