// tests/cpp/match_rule_test.cpp — emba_amd/csrc/match_rule.h on a CPU (plain C++17, no HIP; tests/test_match_rule_cpu.py builds and runs it, also under the
// address and undefined-behaviour sanitizers): every refusal in its order, the shift count and the index <-> (i, j) map of the triangular table, the chunks
// at the 2^20 edge, the six sums of a hand-made 3 x 2 pair, the score of a frame against itself, what is not scored, the tie rule of shifts and of partners,
// and match_start (the identity bit for bit, and b_i turned onto b_j).  Every thumbnail here is exactly as large as the rule says it reads: a read past it is
// the sanitizer's to find.
#include "../../emba_amd/csrc/match_rule.h"

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
constexpr size_t kRecord = sizeof(MatchBest);

static void test_refusals()
{
    using M = MatchArgStatus;
    static_assert((int)M::ok == 0 && (int)M::frames_null == 1 && (int)M::bad_frames == 2 && (int)M::pairs_null == 3 && (int)M::too_many_pairs == 4 &&
                      (int)M::pair_out_of_range == 5 && (int)M::level_out_of_range == 6 && (int)M::level_too_small == 7 && (int)M::too_many_pixels == 8 &&
                      (int)M::bad_range == 9 && (int)M::n_min_zero == 10 && (int)M::bad_k == 11 && (int)M::bad_gap == 12 && (int)M::bad_score_min == 13 &&
                      (int)M::bytes == 14 && (int)M::table == 15,
                  "the order the C ABI reports them in");
    static_assert(kRecord == 24, "the record of the triangular table");
    const int sw = 64, sh = 48;
    const int32_t pairs[6] = {0, 1, 2, 2, 3, 0};
    size_t at = 99;
    const MatchCall good{true, 4, pairs, 3, 2, 6, 4, 8, false, 1, 0, 0.0};
    CHECK(match_args_ok(good, sw, sh, kRecord, &at) == M::ok);
    // each refusal with every later one also wrong: the first is reported
    MatchCall a = good;
    a.level = 9; a.rx = -1; a.n_min = 0;
    a.have_frames = false; a.F = 0; a.pairs = nullptr;
    CHECK(match_args_ok(a, sw, sh, kRecord, &at) == M::frames_null);
    a.have_frames = true;
    CHECK(match_args_ok(a, sw, sh, kRecord, &at) == M::bad_frames);
    a.F = (size_t)1 << 31;
    CHECK(match_args_ok(a, sw, sh, kRecord, &at) == M::bad_frames);
    a.F = 4;
    CHECK(match_args_ok(a, sw, sh, kRecord, &at) == M::pairs_null);
    a.P = 0;
    CHECK(match_args_ok(a, sw, sh, kRecord, &at) == M::level_out_of_range);      // (P = 0: no pairs are needed)
    a.P = (size_t)1 << 31; a.pairs = pairs;
    CHECK(match_args_ok(a, sw, sh, kRecord, &at) == M::too_many_pairs);
    a.P = 3; a.F = 3;
    CHECK(match_args_ok(a, sw, sh, kRecord, &at) == M::pair_out_of_range && at == 2);
    const int32_t neg[2] = {0, -1};
    a.pairs = neg; a.P = 1;
    CHECK(match_args_ok(a, sw, sh, kRecord, &at) == M::pair_out_of_range && at == 0);
    a.pairs = pairs; a.P = 3; a.F = 4;
    CHECK(match_args_ok(a, sw, sh, kRecord, &at) == M::level_out_of_range);
    a.level = -1;
    CHECK(match_args_ok(a, sw, sh, kRecord, &at) == M::level_out_of_range);
    a.level = 5;      // 2 x 1
    CHECK(match_args_ok(a, sw, sh, kRecord, &at) == M::level_too_small);
    a.level = 0;
    CHECK(match_args_ok(a, 240, 180, kRecord, &at) == M::too_many_pixels && match_smallest_level(240, 180) == 1 && match_smallest_level(64, 48) == 0);
    CHECK(match_args_ok(a, 128, 128, kRecord, &at) == M::bad_range);      // (16 384 pixels fit)
    CHECK(match_args_ok(a, 129, 128, kRecord, &at) == M::too_many_pixels);
    a.level = 2;      // 16 x 12
    CHECK(match_args_ok(a, sw, sh, kRecord, &at) == M::bad_range);
    a.rx = 16; a.ry = 0;
    CHECK(match_args_ok(a, sw, sh, kRecord, &at) == M::bad_range);
    a.rx = 15; a.ry = 12;
    CHECK(match_args_ok(a, sw, sh, kRecord, &at) == M::bad_range);
    a.ry = -1;
    CHECK(match_args_ok(a, sw, sh, kRecord, &at) == M::bad_range);
    a.ry = 11;
    CHECK(match_args_ok(a, sw, sh, kRecord, &at) == M::n_min_zero);
    a.n_min = 1;
    CHECK(match_args_ok(a, sw, sh, kRecord, &at) == M::ok);
    const size_t bigF = kPairMaxBytes / ((size_t)sw * sh) + 1;
    a.F = bigF;
    CHECK(match_args_ok(a, sw, sh, kRecord, &at) == M::bytes);
    // the search: k, min_gap, score_min behind n_min, in front of the bytes; the table last
    MatchCall s{true, bigF, nullptr, 0, 2, 6, 4, 0, true, 0, -1, kNaN};
    CHECK(match_args_ok(s, sw, sh, kRecord, &at) == M::n_min_zero);
    s.n_min = 8;
    CHECK(match_args_ok(s, sw, sh, kRecord, &at) == M::bad_k);
    s.k = 65;
    CHECK(match_args_ok(s, sw, sh, kRecord, &at) == M::bad_k);
    s.k = 64;
    CHECK(match_args_ok(s, sw, sh, kRecord, &at) == M::bad_gap);
    s.min_gap = 0;
    CHECK(match_args_ok(s, sw, sh, kRecord, &at) == M::bad_score_min);
    s.score_min = -std::numeric_limits<double>::infinity();
    CHECK(match_args_ok(s, sw, sh, kRecord, &at) == M::bytes);
    s.level = 0; s.rx = s.ry = 1;      // (8 x 8 frames)
    s.F = 9460;      // 44 741 070 pairs of 24 bytes: above 2^30 bytes; 9 459 frames fit
    CHECK(match_args_ok(s, 8, 8, kRecord, &at) == M::table);
    s.F = 9459;
    CHECK(match_args_ok(s, 8, 8, kRecord, &at) == M::ok && match_table_ok(9459, kRecord) && !match_table_ok(9460, kRecord));
    CHECK(match_table_bytes(9459, kRecord) == (size_t)9459 * 9458 / 2 * 24);
}

static void test_launch_arithmetic()
{
    CHECK(match_shift_count(0, 0) == 1 && match_shift_count(1, 1) == 9 && match_shift_count(8, 6) == 17 * 13 && match_shift_count(6, 0) == 13);
    for (int s = 0; s < match_shift_count(3, 2); ++s) {
        int dx, dy;
        match_shift_of(s, 3, 2, &dx, &dy);
        CHECK(dx >= -3 && dx <= 3 && dy >= -2 && dy <= 2 && match_shift_index(dx, dy, 3, 2) == s);
        if (s == 0) CHECK(dx == -3 && dy == -2);
        if (s == 1) CHECK(dx == -2 && dy == -2);
        if (s == 7) CHECK(dx == -3 && dy == -1);
    }
    // the triangular table: every index of F = 2, 3; the ends of every row of F = 4096
    for (uint64_t F : {(uint64_t)2, (uint64_t)3, (uint64_t)7}) {
        uint64_t p = 0;
        for (uint64_t i = 0; i + 1 < F; ++i)
            for (uint64_t j = i + 1; j < F; ++j, ++p) {
                uint64_t a, b;
                match_table_pair(F, p, &a, &b);
                CHECK(match_table_index(F, i, j) == p && a == i && b == j);
            }
        CHECK(p == match_table_pairs(F));
    }
    CHECK(match_table_pairs(2) == 1 && match_table_pairs(3) == 3 && match_table_pairs(4096) == 8386560ull && match_table_pairs(1450) == 1050525ull);
    const uint64_t F = 4096;
    for (uint64_t i = 0; i + 1 < F; ++i)
        for (uint64_t j : {i + 1, (i + F) / 2 + 1 < F ? (i + F) / 2 + 1 : F - 1, F - 1}) {
            uint64_t a, b;
            const uint64_t p = match_table_index(F, i, j);
            match_table_pair(F, p, &a, &b);
            CHECK(p < match_table_pairs(F) && a == i && b == j);
        }
    uint64_t a, b;
    match_table_pair(0x7FFFFFFFull, match_table_pairs(0x7FFFFFFFull) - 1, &a, &b);      // (the last pair of the largest F the arguments allow)
    CHECK(a == 0x7FFFFFFDull && b == 0x7FFFFFFEull);
    // chunks at the 2^20 edge
    const size_t M = (size_t)1 << 20;
    CHECK(match_chunk_pairs(9, false) == M && match_chunk_count(M - 1, M) == 1 && match_chunk_count(M, M) == 1 && match_chunk_count(M + 1, M) == 2);
    CHECK(match_chunk_count(0, M) == 0 && match_chunk_count(1050525, M) == 2);
    CHECK(match_chunk_pairs(9, true) == (size_t)(64 << 20) / (9 * 48) && match_chunk_pairs(1, true) == M && match_chunk_pairs(1 << 21, true) == 1);
    // lanes per shift: a power of two, at most a wave, shifts * g >= T where that can be
    CHECK(match_lanes_per_shift(1, 256) == 64 && match_lanes_per_shift(9, 256) == 32 && match_lanes_per_shift(117, 256) == 4 && match_lanes_per_shift(128, 256) == 2);
    CHECK(match_lanes_per_shift(221, 256) == 2 && match_lanes_per_shift(256, 256) == 1 && match_lanes_per_shift(713, 256) == 1);
}

static void test_sums_and_scores()
{
    // a hand-made pair, 3 wide and 2 high
    const uint8_t A[6] = {1, 2, 3, 4, 0, 6}, B[6] = {7, 8, 9, 1, 2, 3};
    // shift (0, 0): all six points
    MatchSums s = match_sums_of(A, B, 3, 2, 0, 0, false);
    CHECK(s.n == 6 && s.a == 16 && s.b == 30 && s.aa == 66 && s.bb == 208 && s.ab == 7 + 16 + 27 + 4 + 0 + 18);
    s = match_sums_of(A, B, 3, 2, 0, 0, true);      // ... without the point whose a is 0
    CHECK(s.n == 5 && s.a == 16 && s.b == 28 && s.aa == 66 && s.bb == 204 && s.ab == 72);
    // shift (1, 0): A(x, y) with B(x + 1, y), x = 0, 1: (1, 8) (2, 9) (4, 2) (0, 3)
    s = match_sums_of(A, B, 3, 2, 1, 0, false);
    CHECK(s.n == 4 && s.a == 7 && s.b == 22 && s.aa == 21 && s.bb == 158 && s.ab == 8 + 18 + 8);
    // shift (-2, 1): A(2, 0) = 3 with B(0, 1) = 1
    s = match_sums_of(A, B, 3, 2, -2, 1, false);
    CHECK(s.n == 1 && s.a == 3 && s.b == 1 && s.aa == 9 && s.bb == 1 && s.ab == 3);
    // shift (2, -1): A(0, 1) = 4 with B(2, 0) = 9
    s = match_sums_of(A, B, 3, 2, 2, -1, true);
    CHECK(s.n == 1 && s.a == 4 && s.b == 9 && s.aa == 16 && s.bb == 81 && s.ab == 36);
    const MatchOverlap o = match_overlap(9, 7, -8, 6);
    CHECK(o.x0 == 8 && o.x1 == 9 && o.y0 == 0 && o.y1 == 1);
    // the score: by hand for shift (0, 0): cov = 6 * 72 - 16 * 30 = -48, va = 6 * 66 - 256 = 140, vb = 6 * 208 - 900 = 348
    double sc = 0.0;
    s = match_sums_of(A, B, 3, 2, 0, 0, false);
    CHECK(match_score(s, 1, &sc) && same_bits(sc, (-48.0 * 48.0) / (140.0 * 348.0)) && match_score(s, 6, &sc) && !match_score(s, 7, &sc));
    // a frame against itself scores exactly 1 at shift 0, and that is the best of the range
    std::vector<uint8_t> T(20 * 13);
    for (size_t k = 0; k < T.size(); ++k) T[k] = (uint8_t)(1 + (k * 37 + k * k) % 251);
    std::vector<uint64_t> sums((size_t)match_shift_count(3, 2) * kMatchSums);
    MatchBest b = match_best_of(T.data(), T.data(), 20, 13, 3, 2, true, 8, sums.data());
    CHECK(same_bits(b.score, 1.0) && b.dx == 0 && b.dy == 0 && b.n == 260 && b.shift == (uint32_t)match_shift_index(0, 0, 3, 2));
    CHECK(sums[(size_t)kMatchSums * b.shift] == 260 && sums[0] == (uint64_t)(20 - 3) * (13 - 2));
    // a constant frame and, under skip_zero, an all-zero frame: not scored
    std::vector<uint8_t> Cn(20 * 13, 77), Z(20 * 13, 0);
    for (const MatchBest& r : {match_best_of(Cn.data(), T.data(), 20, 13, 3, 2, false, 1, nullptr), match_best_of(T.data(), Cn.data(), 20, 13, 3, 2, true, 1, nullptr),
                               match_best_of(Z.data(), T.data(), 20, 13, 3, 2, true, 1, nullptr), match_best_of(Z.data(), Z.data(), 20, 13, 0, 0, false, 1, nullptr)})
        CHECK(same_bits(r.score, -2.0) && r.dx == 0 && r.dy == 0 && r.n == 0);
    // n_min decides where the overlap shrinks to one pixel: 9 x 7 at (8, 6)
    std::vector<uint8_t> S9(63);
    for (size_t k = 0; k < 63; ++k) S9[k] = (uint8_t)(3 + (k * 29) % 200);
    b = match_best_of(S9.data(), S9.data(), 9, 7, 8, 6, false, 1, nullptr);
    CHECK(same_bits(b.score, 1.0));
    CHECK(match_sums_of(S9.data(), S9.data(), 9, 7, 8, 6, false).n == 1 && match_best_of(S9.data(), S9.data(), 9, 7, 8, 6, false, 64, nullptr).n == 0);
    // the tie goes to the lower shift index: a pattern of period 2 in x scores 1 at dx = -2, 0, 2; the first is dx = -2
    std::vector<uint8_t> Pd(8 * 4);
    for (int y = 0; y < 4; ++y)
        for (int x = 0; x < 8; ++x) Pd[y * 8 + x] = (x & 1) ? 200 : 50;
    b = match_best_of(Pd.data(), Pd.data(), 8, 4, 2, 0, false, 1, nullptr);
    CHECK(same_bits(b.score, 1.0) && b.dx == -2 && b.dy == 0 && b.shift == 0);
    CHECK(match_better(0.5, 3, true, 0.5, 4) && !match_better(0.5, 4, true, 0.5, 3) && match_better(-0.9, 9, false, 0.0, 0) && !match_better(0.4, 0, true, 0.5, 9));
}

static void test_search()
{
    // five 4 x 4 thumbnails: 0 and 4 the same bytes, 2 their mirror in value, 1 constant, 3 a frame that does not vote
    const int w = 4, h = 4;
    const size_t F = 5, S = 16;
    std::vector<uint8_t> T(F * S);
    for (size_t k = 0; k < S; ++k) {
        T[0 * S + k] = T[4 * S + k] = (uint8_t)(10 + 13 * k);
        T[1 * S + k] = 90;
        T[2 * S + k] = (uint8_t)(250 - 13 * k);
        T[3 * S + k] = (uint8_t)(10 + 13 * k);
    }
    const int32_t status[5] = {1, 2, 2, 3, 2};
    const int k = 2;
    std::vector<int32_t> partner(F * k), shift(2 * F * k);
    std::vector<double> score(F * k);
    std::vector<uint64_t> n(F * k);
    match_search_of(T.data(), F, w, h, status, 0, 0, 0, false, 1, -1.5, k, partner.data(), score.data(), shift.data(), n.data());
    // frame 0: 4 scores 1, 2 scores -1; 1 is constant (not scored), 3 does not vote
    CHECK(partner[0] == 4 && same_bits(score[0], 1.0) && partner[1] == 2 && same_bits(score[1], -1.0) && n[0] == 16);
    CHECK(partner[2] == -1 && partner[3] == -1 && same_bits(score[2], -2.0) && n[2] == 0);      // the constant frame has no partner
    CHECK(partner[4] == 0 && partner[5] == 4 && same_bits(score[4], -1.0) && same_bits(score[5], -1.0));      // frame 2: a tie, the lower index first
    CHECK(partner[6] == -1 && partner[7] == -1);      // the lost frame
    CHECK(partner[8] == 0 && partner[9] == 2);
    match_search_of(T.data(), F, w, h, nullptr, 0, 0, 3, false, 1, 0.0, k, partner.data(), score.data(), shift.data(), n.data());
    CHECK(partner[0] == 4 && partner[1] == -1 && partner[8] == 0 && partner[2] == -1 && partner[6] == -1);      // min_gap = F - 2 leaves the pair (0, 4)
    match_search_of(T.data(), F, w, h, nullptr, 0, 0, 4, false, 1, 0.0, k, partner.data(), score.data(), shift.data(), n.data());
    for (size_t o = 0; o < F * k; ++o) CHECK(partner[o] == -1);
    CHECK(match_partner_behind(0.5, 3, 0.6, 9) && match_partner_behind(0.5, 4, 0.5, 3) && !match_partner_behind(0.5, 3, 0.5, 3) && !match_partner_behind(0.7, 0, 0.5, 3));
    const uint8_t votes[4] = {1, 0, 1, 1};
    CHECK(match_candidate(votes, 0, 2, 1) && !match_candidate(votes, 0, 2, 2) && !match_candidate(votes, 1, 3, 0) && match_votes(nullptr, 7) && !match_votes(status, 3));
}

static void turn(const double* Q, const double* b, double* rb) { pair_turn(Q, b, rb); }

static void test_start()
{
    double Q[4];
    for (int l = 0; l <= 3; ++l) {
        match_start(0, 0, l, 32.0, 35.2, 31.5, 23.5, 64, 48, Q);
        CHECK(same_bits(Q[0], 0.0) && same_bits(Q[1], 0.0) && same_bits(Q[2], 0.0) && same_bits(Q[3], 1.0));
        match_start(0, 0, l, 201.7, 199.3, 117.2, 93.9, 240, 180, Q);      // (off the centre: the bearings are equal, not the axis)
        CHECK(same_bits(Q[0], 0.0) && same_bits(Q[1], 0.0) && same_bits(Q[2], 0.0) && same_bits(Q[3], 1.0));
    }
    // R(Q) b_i = b_j, a unit quaternion, zero roll: the axis is b_i x b_j
    const int shifts[5][2] = {{3, 0}, {0, -2}, {-5, 4}, {7, 5}, {-1, -1}};
    for (const auto& d : shifts)
        for (int l : {0, 2}) {
            const double fu = 32.0, fv = 35.2, cu = 31.5, cv = 23.5;
            match_start(d[0], d[1], l, fu, fv, cu, cv, 64, 48, Q);
            const double tx = (double)(1 << l) * d[0] / 2.0, ty = (double)(1 << l) * d[1] / 2.0;
            double bi[3], bj[3], rb[3];
            match_bearing(31.5 - tx, 23.5 - ty, fu, fv, cu, cv, bi);
            match_bearing(31.5 + tx, 23.5 + ty, fu, fv, cu, cv, bj);
            turn(Q, bi, rb);
            CHECK(fabs(rb[0] - bj[0]) < 1e-15 && fabs(rb[1] - bj[1]) < 1e-15 && fabs(rb[2] - bj[2]) < 1e-15);
            CHECK(fabs(Q[0] * Q[0] + Q[1] * Q[1] + Q[2] * Q[2] + Q[3] * Q[3] - 1.0) < 1e-15 && Q[3] > 0.0);
            CHECK(fabs(Q[0] * (bi[0] + bj[0]) + Q[1] * (bi[1] + bj[1]) + Q[2] * (bi[2] + bj[2])) < 1e-15);      // no turn about the bisector: zero roll
        }
    // dx > 0: the place lies left of the centre in frame i and right of it in frame j; the bearing is turned about +y
    match_start(4, 0, 2, 32.0, 32.0, 31.5, 23.5, 64, 48, Q);
    CHECK(Q[1] > 0.0 && fabs(Q[0]) < 1e-15 && fabs(Q[2]) < 1e-15);
    CHECK(match_start_ok(0, 1.0, 1.0, 0.0, 0.0, 1, 1) && !match_start_ok(8, 1.0, 1.0, 0.0, 0.0, 1, 1) && !match_start_ok(0, 0.0, 1.0, 0.0, 0.0, 1, 1));
    CHECK(!match_start_ok(0, 1.0, kNaN, 0.0, 0.0, 1, 1) && !match_start_ok(0, 1.0, 1.0, kNaN, 0.0, 1, 1) && !match_start_ok(0, 1.0, 1.0, 0.0, 0.0, 0, 1));
}

int main()
{
    test_refusals();
    test_launch_arithmetic();
    test_sums_and_scores();
    test_search();
    test_start();
    if (g_fail) { std::printf("%d checks failed\n", g_fail); return 1; }
    std::printf("OK match_rule\n");
    return 0;
}
