// tests/cpp/refit_rule_test.cpp — emba_amd/csrc/refit_rule.h on a CPU (plain C++17, no HIP; tests/test_refit_rule_cpu.py builds and runs it, also under the
// address and undefined-behaviour sanitizers): the argument checks in the order the C ABI reports them, the un-vote of a vote as the identity on uint64 (a
// sum that wraps among it), the selectors, the sweep order with `alternate`, the start of a frame (its own values, the interpolation between two voting
// frames, one side only, across a run of lost frames), the refit code table and the rotation change.  Every array here is exactly as long as the rule says
// it reads: a read past it is the sanitizer's to find.
#include "../../emba_amd/csrc/refit_rule.h"

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

static void rot(double ax, double ay, double az, double* q)
{
    const double id[4] = {0.0, 0.0, 0.0, 1.0}, d[3] = {ax, ay, az};
    align_apply(d, id, q);
}

static emba_refit_settings settings()
{
    emba_refit_settings s;
    std::memset(&s, 0, sizeof s);
    s.track.gain_min = 0.25; s.track.gain_max = 4.0; s.track.estimate = 3;
    s.sweeps = 1; s.alternate = 1; s.recover = 1; s.sweep_tol = 0.0;
    return s;
}

static void test_args()
{
    using A = RefitArgStatus;
    static_assert((int)A::ok == 0 && (int)A::q_null == 1 && (int)A::gain_null == 2 && (int)A::bias_null == 3 && (int)A::status_null == 4 && (int)A::bad_sweeps == 5 &&
                      (int)A::bad_sweep_tol == 6 && (int)A::bad_status == 7 && (int)A::no_voting_frame == 8 && (int)A::bad_q == 9 && (int)A::bad_gain == 10 &&
                      (int)A::bad_bias == 11,
                  "the order the C ABI reports them in");
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    const size_t F = 3;
    std::vector<double> q(4 * F, 0.0), g(F, 1.0), b(F, 0.0);
    for (size_t f = 0; f < F; ++f) q[4 * f + 3] = 1.0;
    std::vector<int32_t> st = {EMBA_TRACK_ANCHOR, EMBA_TRACK_TRACKED, EMBA_TRACK_LOST};
    emba_refit_settings s = settings();
    size_t w = 99;
    CHECK(refit_args_ok(q.data(), g.data(), b.data(), st.data(), F, s, &w) == A::ok && w == 0);
    CHECK(refit_args_ok(q.data(), g.data(), b.data(), st.data(), F, s, nullptr) == A::ok);
    CHECK(refit_args_ok(nullptr, g.data(), b.data(), st.data(), F, s, &w) == A::q_null);
    CHECK(refit_args_ok(q.data(), nullptr, b.data(), st.data(), F, s, &w) == A::gain_null);
    CHECK(refit_args_ok(q.data(), g.data(), nullptr, st.data(), F, s, &w) == A::bias_null);
    CHECK(refit_args_ok(q.data(), g.data(), b.data(), nullptr, F, s, &w) == A::status_null);
    CHECK(refit_args_ok(nullptr, nullptr, nullptr, nullptr, 0, s, &w) == A::no_voting_frame);      // (no frame at all: none votes)
    s.sweeps = -1; CHECK(refit_args_ok(q.data(), g.data(), b.data(), st.data(), F, s, &w) == A::bad_sweeps);
    s.sweep_tol = -1.0; CHECK(refit_args_ok(q.data(), g.data(), b.data(), st.data(), F, s, &w) == A::bad_sweeps);      // (sweeps is reported first)
    s.sweeps = 0; CHECK(refit_args_ok(q.data(), g.data(), b.data(), st.data(), F, s, &w) == A::bad_sweep_tol);
    s.sweep_tol = nan; CHECK(refit_args_ok(q.data(), g.data(), b.data(), st.data(), F, s, &w) == A::bad_sweep_tol);
    s.sweep_tol = 0.0; CHECK(refit_args_ok(q.data(), g.data(), b.data(), st.data(), F, s, &w) == A::ok);
    st[2] = 0; CHECK(refit_args_ok(q.data(), g.data(), b.data(), st.data(), F, s, &w) == A::bad_status && w == 2);
    st[2] = 4; CHECK(refit_args_ok(q.data(), g.data(), b.data(), st.data(), F, s, &w) == A::bad_status && w == 2);
    st = {EMBA_TRACK_LOST, EMBA_TRACK_LOST, EMBA_TRACK_LOST};
    CHECK(refit_args_ok(q.data(), g.data(), b.data(), st.data(), F, s, &w) == A::no_voting_frame);
    st = {EMBA_TRACK_LOST, EMBA_TRACK_TRACKED, EMBA_TRACK_LOST};      // (no anchor at all is allowed)
    CHECK(refit_args_ok(q.data(), g.data(), b.data(), st.data(), F, s, &w) == A::ok);
    q[4 + 1] = nan; CHECK(refit_args_ok(q.data(), g.data(), b.data(), st.data(), F, s, &w) == A::bad_q && w == 1);
    q[4 + 1] = 0.0; q[4 + 3] = 0.0; CHECK(refit_args_ok(q.data(), g.data(), b.data(), st.data(), F, s, &w) == A::bad_q && w == 1);
    q[4 + 3] = 1.0;
    for (double bad : {nan, inf, 0.2, 4.5, -1.0}) {
        g[2] = bad; CHECK(refit_args_ok(q.data(), g.data(), b.data(), st.data(), F, s, &w) == A::bad_gain && w == 2);
    }
    g[2] = 0.25; CHECK(refit_args_ok(q.data(), g.data(), b.data(), st.data(), F, s, &w) == A::ok);      // (the bounds are inside)
    g[2] = 4.0; CHECK(refit_args_ok(q.data(), g.data(), b.data(), st.data(), F, s, &w) == A::ok);
    b[0] = inf; CHECK(refit_args_ok(q.data(), g.data(), b.data(), st.data(), F, s, &w) == A::bad_bias && w == 0);
    b[0] = nan; CHECK(refit_args_ok(q.data(), g.data(), b.data(), st.data(), F, s, &w) == A::bad_bias && w == 0);
}

static void test_unvote()
{
    CHECK(refit_signed(0, true) == 0 && refit_signed(0, false) == 0);
    CHECK(refit_signed(5, false) == 5 && refit_signed(5, true) == 0xFFFFFFFFFFFFFFFBull);
    // a sum of votes, taken out again in another order: the identity, whatever stood there before — also where the sum wrapped on the way
    for (uint64_t start : {(uint64_t)0, (uint64_t)12345, ~(uint64_t)0 - 100, ~(uint64_t)0}) {
        std::vector<uint64_t> votes(257);
        for (auto& v : votes) v = (next_u64() % 257) * (next_u64() % 256);      // w * v of one cell
        votes[7] = ~(uint64_t)0;                                                  // (nothing a frame casts, but the identity holds for every value)
        uint64_t sum = start;
        bool wrapped = false;
        for (uint64_t v : votes) { const uint64_t before = sum; sum += refit_signed(v, false); wrapped = wrapped || sum < before; }
        CHECK(wrapped);
        for (size_t i = votes.size(); i-- > 0;) sum += refit_signed(votes[i], true);
        CHECK(sum == start);
    }
    // a frame that leaves and comes back with other votes: what the others cast stays
    uint64_t others = 1000, mine = 300, mine_new = 17;
    uint64_t sum = others + mine;
    sum += refit_signed(mine, true);
    CHECK(sum == others);
    sum += refit_signed(mine_new, false);
    CHECK(sum == others + mine_new);
}

static void test_select_and_order()
{
    CHECK(refit_selected(kRefitSelectVoting, EMBA_TRACK_ANCHOR) && refit_selected(kRefitSelectVoting, EMBA_TRACK_TRACKED) && !refit_selected(kRefitSelectVoting, EMBA_TRACK_LOST));
    CHECK(!refit_selected(kRefitSelectMovable, EMBA_TRACK_ANCHOR) && refit_selected(kRefitSelectMovable, EMBA_TRACK_TRACKED) &&
          !refit_selected(kRefitSelectMovable, EMBA_TRACK_LOST));
    CHECK(!refit_active(EMBA_TRACK_ANCHOR, true) && refit_active(EMBA_TRACK_TRACKED, false) && refit_active(EMBA_TRACK_LOST, true) && !refit_active(EMBA_TRACK_LOST, false));
    const int32_t st[5] = {EMBA_TRACK_ANCHOR, EMBA_TRACK_ANCHOR, EMBA_TRACK_LOST, EMBA_TRACK_TRACKED, EMBA_TRACK_ANCHOR};
    CHECK(!refit_batch_active(st, 0, 2, true) && refit_batch_active(st, 1, 2, true) && !refit_batch_active(st, 1, 2, false) && refit_batch_active(st, 2, 2, false) &&
          !refit_batch_active(st, 4, 1, true));
    const size_t n = 5;
    for (size_t k = 0; k < n; ++k) {
        CHECK(refit_batch_index(0, k, n, true) == k && refit_batch_index(2, k, n, true) == k);
        CHECK(refit_batch_index(1, k, n, true) == n - 1 - k && refit_batch_index(3, k, n, true) == n - 1 - k);
        CHECK(refit_batch_index(1, k, n, false) == k && refit_batch_index(0, k, n, false) == k);
    }
    CHECK(refit_batch_index(1, 0, 1, true) == 0);
}

static void test_start()
{
    // six frames at uneven times; 0 and 4 vote, 1 ... 3 and 5 are lost
    const long F = 6;
    const long long t[F] = {100, 200, 350, 400, 500, 900};
    int32_t st[F] = {EMBA_TRACK_ANCHOR, EMBA_TRACK_LOST, EMBA_TRACK_LOST, EMBA_TRACK_LOST, EMBA_TRACK_TRACKED, EMBA_TRACK_LOST};
    double q[4 * F], g[F] = {1.0, 7.0, 7.0, 7.0, 2.0, 7.0}, b[F] = {0.0, 9.0, 9.0, 9.0, -40.0, 9.0};
    for (long f = 0; f < F; ++f) rot(0.0, 0.01 * (double)f * (double)f, 0.0, q + 4 * f);      // (the lost frames' own values are not what a start reads)
    rot(0.0, 0.0, 0.0, q);
    rot(0.0, 0.4, 0.0, q + 16);
    double qs[4], a, bb;
    // a voting frame: its own values, bit for bit
    CHECK(refit_start(st, t, q, g, b, F, 4, qs, &a, &bb));
    for (int k = 0; k < 4; ++k) CHECK(same_bits(qs[k], q[16 + k]));
    CHECK(a == 2.0 && bb == -40.0);
    // across the run of lost frames: the same two neighbours for all three, the angle and the exposure linear in time
    for (long f = 1; f <= 3; ++f) {
        CHECK(refit_start(st, t, q, g, b, F, f, qs, &a, &bb));
        const double frac = (double)(t[f] - t[0]) / (double)(t[4] - t[0]);
        double w[3];
        track_log_between(q, qs, w);
        CHECK(std::fabs(w[1] - 0.4 * frac) < 1e-14 && std::fabs(w[0]) < 1e-15 && std::fabs(w[2]) < 1e-15);
        CHECK(std::fabs(a - (1.0 + frac)) < 1e-14 && std::fabs(bb - (-40.0 * frac)) < 1e-12);
        // the formula is track_predict's with its negative factor
        double qp[4];
        track_predict(2, q, t[0], q + 16, t[4], t[f], true, qp);
        for (int k = 0; k < 4; ++k) CHECK(same_bits(qs[k], qp[k]));
        const double u = (double)(t[f] - t[4]) / (double)(t[4] - t[0]);
        CHECK(u < 0.0 && u > -1.0 && same_bits(a, g[4] + (g[4] - g[0]) * u));
    }
    // one side only: behind the last voting frame, and in front of the first
    CHECK(refit_start(st, t, q, g, b, F, 5, qs, &a, &bb));
    for (int k = 0; k < 4; ++k) CHECK(same_bits(qs[k], q[16 + k]));
    CHECK(a == 2.0 && bb == -40.0);
    st[0] = EMBA_TRACK_LOST;
    CHECK(refit_start(st, t, q, g, b, F, 0, qs, &a, &bb));
    for (int k = 0; k < 4; ++k) CHECK(same_bits(qs[k], q[16 + k]));
    CHECK(refit_start(st, t, q, g, b, F, 2, qs, &a, &bb) && a == 2.0 && bb == -40.0);
    // no frame votes: nothing is written
    st[4] = EMBA_TRACK_LOST;
    qs[0] = 42.0; a = 43.0;
    CHECK(!refit_start(st, t, q, g, b, F, 2, qs, &a, &bb) && qs[0] == 42.0 && a == 43.0);
    // a single frame
    const long long t1[1] = {5};
    const int32_t s1[1] = {EMBA_TRACK_TRACKED};
    CHECK(refit_start(s1, t1, q, g, b, 1, 0, qs, &a, &bb) && a == 1.0);
}

static void test_codes()
{
    CHECK(EMBA_REFIT_ANCHOR == 1 && EMBA_REFIT_MOVED == 2 && EMBA_REFIT_KEPT == 3 && EMBA_REFIT_RECOVERED == 4 && EMBA_REFIT_LOST == 5);
    CHECK(refit_code(EMBA_TRACK_ANCHOR, true) == EMBA_REFIT_ANCHOR && refit_code(EMBA_TRACK_ANCHOR, false) == EMBA_REFIT_ANCHOR);
    CHECK(refit_code(EMBA_TRACK_TRACKED, true) == EMBA_REFIT_MOVED && refit_code(EMBA_TRACK_TRACKED, false) == EMBA_REFIT_KEPT);
    CHECK(refit_code(EMBA_TRACK_LOST, true) == EMBA_REFIT_RECOVERED && refit_code(EMBA_TRACK_LOST, false) == EMBA_REFIT_LOST);
}

static void test_change()
{
    const size_t F = 3;
    double qa[4 * F], qb[4 * F];
    rot(0.1, 0.2, -0.3, qa); rot(-1.0, 0.0, 0.5, qa + 4); rot(0.0, 0.0, 0.0, qa + 8);
    std::memcpy(qb, qa, sizeof qa);
    CHECK(refit_rotation_change(qa, qb, F) == 0.0);
    CHECK(refit_rotation_change(qa, qb, 0) == 0.0);
    const double d[3] = {0.0, 0.003, 0.004};      // 5 mrad on frame 1, 1 mrad on frame 2
    align_apply(d, qa + 4, qb + 4);
    const double e[3] = {0.001, 0.0, 0.0};
    align_apply(e, qa + 8, qb + 8);
    CHECK(std::fabs(refit_rotation_change(qa, qb, F) - 0.005) < 1e-14);
    CHECK(std::fabs(refit_rotation_change(qb, qa, F) - 0.005) < 1e-14);
    for (int k = 0; k < 4; ++k) qb[4 + k] = -qb[4 + k];      // the same rotation under the other sign
    CHECK(std::fabs(refit_rotation_change(qa, qb, F) - 0.005) < 1e-14);
    CHECK(!refit_converged(0.0, 0.0) && !refit_converged(1e-9, 0.0) && refit_converged(1e-9, 1e-8) && !refit_converged(1e-8, 1e-8));
}

int main()
{
    test_args();
    test_unvote();
    test_select_and_order();
    test_start();
    test_codes();
    test_change();
    if (g_fail) { std::printf("%d checks failed\n", g_fail); return 1; }
    std::printf("OK refit_rule\n");
    return 0;
}
