// emba_amd/csrc/match_rule.h — loop-closure pairs found by appearance (match_host.h, match_kernels.h), as functions of plain values: two frames' thumbnails
// (a level of pair_level_rule.h's pyramid) compared under every integer shift of a range by the zero-mean normalised correlation, formed from six exact
// integer sums; the best shift of a pair; per frame the k best partners; the rotation a matched pair starts from; the launch arithmetic (the number of shifts,
// the triangular table of pairs, the chunks) and the argument checks.  The thumbnails are pair_level_rule.h's level bytes, called here and not restated.
// emba_amd.io.match_sums / match_score / match_best / match_search / match_start / match_pairs are the same rules in numpy; include/emba_hip.h
// (emba_frames_match_eval, emba_frames_match_search, emba_match_start) states them in words.
//
// No HIP in here: plain C++17, so that tests/cpp/match_rule_test.cpp checks it on a CPU in milliseconds.  What the kernels call is compiled for the host and
// for the device; the loops over pixels and frames at the end are the host's alone, the CPU form of what the kernels do.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <cmath>
#include <vector>

#include "pair_level_rule.h"
#include "pair_rule.h"

namespace emba {

constexpr size_t kMatchMaxPixels = 16384;             // S_l of a thumbnail: 255^2 * 16384 < 2^32, so every sum fits uint32; two thumbnails are 32 KB of LDS
constexpr int kMatchMaxPerFrame = 64;                 // k: a wave's lanes
constexpr size_t kMatchChunkPairs = (size_t)1 << 20;  // workgroups of one evaluation launch: one per pair
constexpr size_t kMatchSumsChunkBytes = (size_t)64 << 20;      // ... and, where the sums of every shift are asked for, the bytes of a chunk's sums
constexpr size_t kMatchMaxTableBytes = (size_t)1 << 30;        // the triangular table of a search: 44.7 M records, F = 9 459
constexpr double kMatchUnscored = -2.0;               // the score of a pair without a scored shift: below every correlation

// ---- the shifts of a range: (2 rx + 1)(2 ry + 1), row-major: dy from -ry, then dx from -rx
EMBA_RULE_HD inline int match_shift_count(int rx, int ry) { return (2 * rx + 1) * (2 * ry + 1); }
EMBA_RULE_HD inline void match_shift_of(int s, int rx, int ry, int* dx, int* dy)
{
    (void)ry;
    *dx = s % (2 * rx + 1) - rx;
    *dy = s / (2 * rx + 1) - ry;
}
EMBA_RULE_HD inline int match_shift_index(int dx, int dy, int rx, int ry) { return (dy + ry) * (2 * rx + 1) + (dx + rx); }

// ---- the overlap of a shift d: every (x, y) with (x, y) and (x + dx, y + dy) inside [0, w) x [0, h): x in [x0, x1), y in [y0, y1)
struct MatchOverlap { int x0, x1, y0, y1; };
EMBA_RULE_HD inline MatchOverlap match_overlap(int w, int h, int dx, int dy)
{
    MatchOverlap o;
    o.x0 = dx < 0 ? -dx : 0; o.x1 = dx > 0 ? w - dx : w;
    o.y0 = dy < 0 ? -dy : 0; o.y1 = dy > 0 ? h - dy : h;
    return o;
}

// ---- the six integer sums of a shift: n, sum a, sum b, sum a^2, sum b^2, sum a b over the overlap; under skip_zero a point where either byte is 0 takes
// no part.  Every one fits uint32 at kMatchMaxPixels.
constexpr int kMatchSums = 6;
struct MatchSums { uint32_t n, a, b, aa, bb, ab; };
EMBA_RULE_HD inline void match_add(MatchSums* s, unsigned a, unsigned b, bool skip_zero)
{
    const uint32_t m = (!skip_zero || (a && b)) ? 1u : 0u;
    s->n += m;
    s->a += m * a; s->b += m * b;
    s->aa += m * a * a; s->bb += m * b * b; s->ab += m * a * b;
}

// ---- the score of a shift: the signed square of the zero-mean normalised correlation.  cov = n sab - sa sb, va = n saa - sa^2, vb likewise: exact in int64
// (below 2^53 at the pixel bound); score = (double)cov |(double)cov| / ((double)va (double)vb), in this order, no contraction.  false (not scored): n < n_min,
// va = 0 or vb = 0.
EMBA_RULE_HD inline bool match_score(const MatchSums& s, uint32_t n_min, double* score)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    if (s.n < n_min) return false;
    const int64_t n = (int64_t)s.n, sa = (int64_t)s.a, sb = (int64_t)s.b;
    const int64_t cov = n * (int64_t)s.ab - sa * sb, va = n * (int64_t)s.aa - sa * sa, vb = n * (int64_t)s.bb - sb * sb;
    if (va == 0 || vb == 0) return false;
    const double c = (double)cov;
    const double num = c * fabs(c);
    const double den = (double)va * (double)vb;
    *score = num / den;
    return true;
}

// ---- the best of a pair: the scored shift of greatest score, ties to the lowest shift index; without one: kMatchUnscored, (0, 0), n = 0
struct MatchBest { double score; int32_t dx, dy; uint32_t n, shift; };      // shift: the index (the tie rule's key; 0 where nothing is scored)
EMBA_RULE_HD inline MatchBest match_best_none() { return MatchBest{kMatchUnscored, 0, 0, 0u, 0u}; }
// is (score, shift) better than the best so far?  `have`: the best so far is a scored shift
EMBA_RULE_HD inline bool match_better(double score, uint32_t shift, bool have, double best, uint32_t best_shift)
{
    return !have || score > best || (score == best && shift < best_shift);
}

// ---- the k partners of a frame: greatest best score first among those with score >= score_min, ties to the lower partner index.  Is (score, g) behind
// (score0, g0) in that order?  (The select kernel's passes walk the order with it.)
EMBA_RULE_HD inline bool match_partner_behind(double score, int64_t g, double score0, int64_t g0) { return score < score0 || (score == score0 && g > g0); }
// a frame votes: anchor or tracked (EMBA_TRACK_ANCHOR 1, EMBA_TRACK_TRACKED 2), as io.pair_candidates has it; status NULL: every frame
EMBA_RULE_HD inline bool match_votes(const int32_t* status, size_t f) { return !status || status[f] == 1 || status[f] == 2; }
// (i, j), i < j, is a candidate: both vote and j - i > min_gap
EMBA_RULE_HD inline bool match_candidate(const uint8_t* votes, int64_t i, int64_t j, int64_t min_gap) { return j - i > min_gap && votes[i] && votes[j]; }

// ---- the triangular table of the pairs i < j of F frames, row-major: row i holds j = i + 1 ... F - 1
EMBA_RULE_HD inline uint64_t match_table_pairs(uint64_t F) { return F * (F - 1) / 2; }
EMBA_RULE_HD inline uint64_t match_table_row(uint64_t F, uint64_t i) { return i * F - i * (i + 1) / 2; }      // the index of (i, i + 1)
EMBA_RULE_HD inline uint64_t match_table_index(uint64_t F, uint64_t i, uint64_t j) { return match_table_row(F, i) + (j - i - 1); }
EMBA_RULE_HD inline void match_table_pair(uint64_t F, uint64_t p, uint64_t* i, uint64_t* j)
{
    // row i begins at i (2 F - 1 - i) / 2: the root of the quadratic in doubles, then put right in integers (F < 2^31: (2 F - 1)^2 < 2^64)
    const double b = 2.0 * (double)F - 1.0;
    double disc = b * b - 8.0 * (double)p;      // (rounded at 2^64 it may come out below zero near the last rows: zero then, and the walk below is short)
    if (!(disc > 0.0)) disc = 0.0;
    double r = (b - sqrt(disc)) * 0.5;
    if (!(r >= 0.0)) r = 0.0;
    uint64_t row = (uint64_t)r;
    if (row > F - 2) row = F - 2;
    while (row > 0 && match_table_row(F, row) > p) --row;
    while (row + 1 <= F - 2 && match_table_row(F, row + 1) <= p) ++row;
    *i = row;
    *j = row + 1 + (p - match_table_row(F, row));
}
inline size_t match_table_bytes(uint64_t F, size_t record) { return (size_t)match_table_pairs(F) * record; }
inline bool match_table_ok(uint64_t F, size_t record) { return match_table_pairs(F) <= kMatchMaxTableBytes / record; }

// ---- chunks of pairs: one workgroup per pair, at most 2^20 workgroups per launch; where the sums of every shift go out, at most kMatchSumsChunkBytes of them
inline size_t match_chunk_pairs(int shifts, bool want_sums)
{
    if (!want_sums) return kMatchChunkPairs;
    const size_t per = (size_t)shifts * kMatchSums * sizeof(uint64_t);
    const size_t fit = kMatchSumsChunkBytes / per;
    return fit < 1 ? 1 : fit < kMatchChunkPairs ? fit : kMatchChunkPairs;
}
inline size_t match_chunk_count(size_t P, size_t per) { return (P + per - 1) / per; }

// ---- lanes per shift: the workgroup's T lanes share the shifts; with fewer shifts than lanes a shift's rows are dealt to g lanes of one wave (g a power of
// two, at most 64: the smallest with shifts * g >= T), whose integer sums are added — integers, so the order does not matter
EMBA_RULE_HD inline int match_lanes_per_shift(int shifts, int T)
{
    int g = 1;
    while (g < 64 && shifts * g < T) g *= 2;
    return g;
}

// ---- the smallest level whose thumbnail fits kMatchMaxPixels (it may lie above kPairMaxLevel or below 2 x 2: the caller says so)
inline int match_smallest_level(int sw, int sh)
{
    int l = 0;
    while ((size_t)(sw >> l) * (size_t)(sh >> l) > kMatchMaxPixels) ++l;
    return l;
}

// ---- argument checks (the order the C ABI reports them in); `search`: emba_frames_match_search, else the pair list of emba_frames_match_eval
enum class MatchArgStatus { ok, frames_null, bad_frames, pairs_null, too_many_pairs, pair_out_of_range, level_out_of_range, level_too_small, too_many_pixels,
                            bad_range, n_min_zero, bad_k, bad_gap, bad_score_min, bytes, table };
struct MatchCall {
    bool have_frames; size_t F; const int32_t* pairs; size_t P; int32_t level, rx, ry; uint32_t n_min;
    bool search; int32_t k, min_gap; double score_min;
};
// *at: the first pair that is refused, where one is
inline MatchArgStatus match_args_ok(const MatchCall& a, int sw, int sh, size_t record, size_t* at)
{
    if (!a.have_frames) return MatchArgStatus::frames_null;
    if (a.F == 0 || a.F >= 0x80000000ull) return MatchArgStatus::bad_frames;
    if (!a.search) {
        if (a.P && !a.pairs) return MatchArgStatus::pairs_null;
        if (a.P >= 0x80000000ull) return MatchArgStatus::too_many_pairs;
        for (size_t p = 0; p < a.P; ++p) {
            *at = p;
            if (a.pairs[2 * p] < 0 || a.pairs[2 * p + 1] < 0 || (size_t)a.pairs[2 * p] >= a.F || (size_t)a.pairs[2 * p + 1] >= a.F) return MatchArgStatus::pair_out_of_range;
        }
    }
    if (a.level < 0 || a.level > kPairMaxLevel) return MatchArgStatus::level_out_of_range;
    if (!pair_level_size_ok(sw, sh, a.level)) return MatchArgStatus::level_too_small;
    const int w = sw >> a.level, h = sh >> a.level;
    if ((size_t)w * (size_t)h > kMatchMaxPixels) return MatchArgStatus::too_many_pixels;
    if (a.rx < 0 || a.ry < 0 || a.rx >= w || a.ry >= h) return MatchArgStatus::bad_range;
    if (a.n_min == 0) return MatchArgStatus::n_min_zero;
    if (a.search) {
        if (a.k < 1 || a.k > kMatchMaxPerFrame) return MatchArgStatus::bad_k;
        if (a.min_gap < 0) return MatchArgStatus::bad_gap;
        if (std::isnan(a.score_min)) return MatchArgStatus::bad_score_min;
    }
    if (!pair_bytes_ok(a.F, (size_t)sw * (size_t)sh)) return MatchArgStatus::bytes;
    if (a.search && !match_table_ok(a.F, record)) return MatchArgStatus::table;
    return MatchArgStatus::ok;
}

// ---- the start of a matched pair: the shift d of level l says that pixel p_i = c - t of frame i and p_j = c + t of frame j show the same place, with
// c = ((sw - 1) / 2, (sh - 1) / 2) and t = 2^l d / 2.  Pinhole bearings ((x - cu) / fu, (y - cv) / fv, 1), normalised; Q is the shortest arc from b_i to
// b_j: (b_i x b_j, 1 + b_i . b_j), normalised — R(Q) b_i = b_j, zero roll.  + - * / sqrt in the order written, no contraction: numpy gives the same bits.
EMBA_RULE_HD inline void match_bearing(double x, double y, double fu, double fv, double cu, double cv, double* b)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double bx = (x - cu) / fu, by = (y - cv) / fv;
    const double n = sqrt((bx * bx + by * by) + 1.0);
    b[0] = bx / n; b[1] = by / n; b[2] = 1.0 / n;
}
EMBA_RULE_HD inline void match_start(int dx, int dy, int l, double fu, double fv, double cu, double cv, int sw, int sh, double* Q)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double cx = ((double)sw - 1.0) / 2.0, cy = ((double)sh - 1.0) / 2.0;
    const double tx = (double)(1 << l) * (double)dx / 2.0, ty = (double)(1 << l) * (double)dy / 2.0;
    double bi[3], bj[3];
    match_bearing(cx - tx, cy - ty, fu, fv, cu, cv, bi);
    match_bearing(cx + tx, cy + ty, fu, fv, cu, cv, bj);
    const double x = bi[1] * bj[2] - bi[2] * bj[1], y = bi[2] * bj[0] - bi[0] * bj[2], z = bi[0] * bj[1] - bi[1] * bj[0];
    const double w = 1.0 + ((bi[0] * bj[0] + bi[1] * bj[1]) + bi[2] * bj[2]);
    const double n = sqrt(((x * x + y * y) + z * z) + w * w);
    Q[0] = x / n; Q[1] = y / n; Q[2] = z / n; Q[3] = w / n;
}
// what emba_match_start refuses: a level outside 0 ... kPairMaxLevel, a sensor without pixels, fu or fv not finite or not positive, cu or cv not finite
inline bool match_start_ok(int l, double fu, double fv, double cu, double cv, int sw, int sh)
{
    return l >= 0 && l <= kPairMaxLevel && sw > 0 && sh > 0 && std::isfinite(fu) && std::isfinite(fv) && fu > 0.0 && fv > 0.0 && std::isfinite(cu) && std::isfinite(cv);
}

// ======== the host's own loops: what the kernels compute, on a CPU ========
// the six sums of shift (dx, dy) of thumbnails a, b [h, w]
inline MatchSums match_sums_of(const uint8_t* a, const uint8_t* b, int w, int h, int dx, int dy, bool skip_zero)
{
    MatchSums s{0, 0, 0, 0, 0, 0};
    const MatchOverlap o = match_overlap(w, h, dx, dy);
    for (int y = o.y0; y < o.y1; ++y)
        for (int x = o.x0; x < o.x1; ++x) match_add(&s, a[(size_t)y * w + x], b[(size_t)(y + dy) * w + (x + dx)], skip_zero);
    return s;
}
// the best of a pair over the range; sums_out [shifts, 6] or nullptr
inline MatchBest match_best_of(const uint8_t* a, const uint8_t* b, int w, int h, int rx, int ry, bool skip_zero, uint32_t n_min, uint64_t* sums_out)
{
    MatchBest best = match_best_none();
    bool have = false;
    for (int s = 0; s < match_shift_count(rx, ry); ++s) {
        int dx, dy;
        match_shift_of(s, rx, ry, &dx, &dy);
        const MatchSums m = match_sums_of(a, b, w, h, dx, dy, skip_zero);
        if (sums_out) {
            uint64_t* o = sums_out + (size_t)kMatchSums * s;
            o[0] = m.n; o[1] = m.a; o[2] = m.b; o[3] = m.aa; o[4] = m.bb; o[5] = m.ab;
        }
        double score;
        if (match_score(m, n_min, &score) && match_better(score, (uint32_t)s, have, best.score, best.shift)) {
            best = MatchBest{score, dx, dy, m.n, (uint32_t)s};
            have = true;
        }
    }
    return best;
}
// the search over thumbnails [F, h, w]: per frame the k partners; partner [F, k] (-1: none), score (kMatchUnscored), shift [F, k, 2] (0), n (0)
inline void match_search_of(const uint8_t* thumbs, size_t F, int w, int h, const int32_t* status, int rx, int ry, int64_t min_gap, bool skip_zero, uint32_t n_min,
                            double score_min, int k, int32_t* partner, double* score, int32_t* shift, uint64_t* n)
{
    const size_t S = (size_t)w * h;
    std::vector<uint8_t> votes(F);
    for (size_t f = 0; f < F; ++f) votes[f] = match_votes(status, f) ? 1 : 0;
    std::vector<MatchBest> table((size_t)match_table_pairs(F));
    for (size_t i = 0; i + 1 < F; ++i)
        for (size_t j = i + 1; j < F; ++j)
            if (match_candidate(votes.data(), (int64_t)i, (int64_t)j, min_gap))
                table[(size_t)match_table_index(F, i, j)] = match_best_of(thumbs + i * S, thumbs + j * S, w, h, rx, ry, skip_zero, n_min, nullptr);
    for (size_t f = 0; f < F; ++f) {
        double s0 = 0.0;
        int64_t g0 = -1;
        for (int t = 0; t < k; ++t) {
            int64_t pick = -1;
            MatchBest pb = match_best_none();
            if (votes[f] && (t == 0 || g0 >= 0))
                for (size_t g = 0; g < F; ++g) {
                    const size_t lo = g < f ? g : f, hi = g < f ? f : g;
                    if (g == f || !match_candidate(votes.data(), (int64_t)lo, (int64_t)hi, min_gap)) continue;
                    const MatchBest& b = table[(size_t)match_table_index(F, lo, hi)];
                    if (b.n == 0 || !(b.score >= score_min)) continue;
                    if (t > 0 && !match_partner_behind(b.score, (int64_t)g, s0, g0)) continue;
                    if (pick < 0 || match_partner_behind(pb.score, pick, b.score, (int64_t)g)) { pick = (int64_t)g; pb = b; }
                }
            const size_t o = f * (size_t)k + (size_t)t;
            partner[o] = (int32_t)pick; score[o] = pb.score; shift[2 * o] = pb.dx; shift[2 * o + 1] = pb.dy; n[o] = pb.n;
            s0 = pb.score; g0 = pick;
        }
    }
}

}  // namespace emba
