// emba_amd/csrc/match_kernels.h — loop-closure pairs found by appearance (gfx950, wave64): two frames' thumbnails compared under every integer shift of a
// range, and per frame the k best partners.  The rule: match_rule.h, include/emba_hip.h (emba_frames_match_eval, emba_frames_match_search), DESIGN.md §28.
// The thumbnails are the level bytes emba_frames_pair_reduce_kernel (pair_level_kernels.h) makes, as it is.
//   * emba_frames_match_eval_kernel    one workgroup of kFrameThreads lanes per pair: both thumbnails are staged once into LDS (2 x 16 KB at the most); the
//                                      lanes share the shifts — with fewer shifts than lanes a shift's rows are dealt to g lanes of one wave
//                                      (match_lanes_per_shift) whose integer sums are added by shuffles — and a shift's six sums stay in registers; the score
//                                      is match_score; every lane keeps the best of its own shifts, the workgroup's best comes from a wave reduction and LDS
//                                      across the waves on the key (score, -shift index), and lane 0 stores the record.  The pair comes from a list, or is
//                                      an index of the search's triangular table (a pair that is no candidate leaves at once, and its record is never read).
//                                      With `sums`: the six sums of every shift go out as uint64 as well.
//   * emba_frames_match_select_kernel  one wave per frame: k passes over the frame's row and column of the table, each a wave arg-max of the partners behind
//                                      the pass before in the rule's order (match_partner_behind), so the order is the rule's whatever the lanes do.
// Integer sums, one fixed order of comparisons: the same inputs give the same bits.  No atomic, no grid-wide synchronisation, no scratch.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "frame_kernels.h"
#include "match_rule.h"

namespace emba {

struct MatchEvalParams {
    const uint8_t* thumbs;        // the level's bytes of the whole sequence [F, S]
    const int32_t* pairs;         // the chunk's (i, j) [np, 2], both below F (match_args_ok); nullptr: the pair is index p0 + blockIdx.x of the triangular table
    const uint8_t* votes;         // [F], the table form alone
    unsigned long long p0, F;
    long long min_gap;
    int w, h, S;                  // the level's
    int rx, ry, shifts;
    int g_log2;                   // log2 of match_lanes_per_shift
    int skip_zero;
    uint32_t n_min;
    MatchBest* out;               // the list form: [np]; the table form: the table
    unsigned long long* sums;     // the list form: [np, shifts, 6] or nullptr
};

// is (score, shift) of another lane better than this lane's?
__device__ inline bool match_other_better(bool have, double score, uint32_t shift, bool o_have, double o_score, uint32_t o_shift)
{
    return o_have && match_better(o_score, o_shift, have, score, shift);
}

#pragma clang fp contract(off)
__global__ __launch_bounds__(kFrameThreads) void emba_frames_match_eval_kernel(MatchEvalParams p)
{
    __shared__ __attribute__((aligned(16))) uint8_t ta[kMatchMaxPixels];
    __shared__ __attribute__((aligned(16))) uint8_t tb[kMatchMaxPixels];
    __shared__ double wv_score[kFrameWaves];
    __shared__ uint32_t wv_shift[kFrameWaves], wv_n[kFrameWaves], wv_have[kFrameWaves];
    const int tid = (int)threadIdx.x;
    size_t fi, fj, slot;
    if (p.pairs) {
        slot = blockIdx.x;
        fi = (size_t)p.pairs[2 * slot]; fj = (size_t)p.pairs[2 * slot + 1];
    } else {
        slot = (size_t)(p.p0 + blockIdx.x);
        uint64_t i, j;
        match_table_pair(p.F, slot, &i, &j);
        if (!match_candidate(p.votes, (int64_t)i, (int64_t)j, p.min_gap)) return;      // (the whole workgroup: the pair is blockIdx.x)
        fi = (size_t)i; fj = (size_t)j;
    }
    const uint8_t* ga = p.thumbs + fi * (size_t)p.S;
    const uint8_t* gb = p.thumbs + fj * (size_t)p.S;
    if ((p.S & 3) == 0) {      // (the buffer is aligned and S a multiple of 4: whole dwords)
        for (int k = tid; k < (p.S >> 2); k += kFrameThreads) {
            ((uint32_t*)ta)[k] = ((const uint32_t*)ga)[k];
            ((uint32_t*)tb)[k] = ((const uint32_t*)gb)[k];
        }
    } else {
        for (int k = tid; k < p.S; k += kFrameThreads) { ta[k] = ga[k]; tb[k] = gb[k]; }
    }
    __syncthreads();
    const int g = 1 << p.g_log2, units = p.shifts << p.g_log2;
    const bool skip = p.skip_zero != 0;
    bool have = false;
    double best = kMatchUnscored;
    uint32_t best_shift = 0, best_n = 0;
    for (int u0 = 0; u0 < units; u0 += kFrameThreads) {      // (uniform over the workgroup: every lane of a wave takes part in the shuffles)
        const int u = u0 + tid, s = u >> p.g_log2, part = u & (g - 1);
        MatchSums m{0, 0, 0, 0, 0, 0};
        if (s < p.shifts) {
            int dx, dy;
            match_shift_of(s, p.rx, p.ry, &dx, &dy);
            const MatchOverlap o = match_overlap(p.w, p.h, dx, dy);
            for (int y = o.y0 + part; y < o.y1; y += g) {
                const uint8_t* ra = ta + y * p.w;
                const uint8_t* rb = tb + (y + dy) * p.w + dx;
                for (int x = o.x0; x < o.x1; ++x) match_add(&m, ra[x], rb[x], skip);
            }
        }
        for (int off = g >> 1; off; off >>= 1) {
            m.n += __shfl_xor(m.n, off); m.a += __shfl_xor(m.a, off); m.b += __shfl_xor(m.b, off);
            m.aa += __shfl_xor(m.aa, off); m.bb += __shfl_xor(m.bb, off); m.ab += __shfl_xor(m.ab, off);
        }
        if (s < p.shifts && part == 0) {
            if (p.sums) {
                unsigned long long* o = p.sums + ((size_t)slot * (size_t)p.shifts + (size_t)s) * kMatchSums;
                o[0] = m.n; o[1] = m.a; o[2] = m.b; o[3] = m.aa; o[4] = m.bb; o[5] = m.ab;
            }
            double score;
            if (match_score(m, p.n_min, &score) && match_better(score, (uint32_t)s, have, best, best_shift)) {
                have = true; best = score; best_shift = (uint32_t)s; best_n = m.n;
            }
        }
    }
    // the workgroup's best on the key (score, -shift index): across the wave, then across the waves
    for (int off = 32; off; off >>= 1) {
        const bool o_have = __shfl_xor((int)have, off) != 0;
        const double o_score = __shfl_xor(best, off);
        const uint32_t o_shift = __shfl_xor(best_shift, off), o_n = __shfl_xor(best_n, off);
        if (match_other_better(have, best, best_shift, o_have, o_score, o_shift)) { have = true; best = o_score; best_shift = o_shift; best_n = o_n; }
    }
    if ((tid & 63) == 0) { wv_score[tid >> 6] = best; wv_shift[tid >> 6] = best_shift; wv_n[tid >> 6] = best_n; wv_have[tid >> 6] = have ? 1u : 0u; }
    __syncthreads();
    if (tid == 0) {
        for (int k = 1; k < kFrameWaves; ++k)
            if (match_other_better(have, best, best_shift, wv_have[k] != 0, wv_score[k], wv_shift[k])) { have = true; best = wv_score[k]; best_shift = wv_shift[k]; best_n = wv_n[k]; }
        MatchBest r = match_best_none();
        if (have) {
            int dx, dy;
            match_shift_of((int)best_shift, p.rx, p.ry, &dx, &dy);
            r = MatchBest{best, dx, dy, best_n, best_shift};
        }
        p.out[slot] = r;
    }
}
#pragma clang fp contract(fast)

struct MatchSelectParams {
    const MatchBest* table;       // the triangular table
    const uint8_t* votes;         // [F]
    unsigned long long F;
    long long min_gap;
    double score_min;
    int k;
    int32_t* partner;             // [F, k]
    double* score;                // [F, k]
    int32_t* shift;               // [F, k, 2]
    unsigned long long* n;        // [F, k]
};

__global__ __launch_bounds__(64) void emba_frames_match_select_kernel(MatchSelectParams p)
{
    const int64_t f = (int64_t)blockIdx.x, F = (int64_t)p.F;
    const int lane = (int)threadIdx.x;
    const bool votes = p.votes[f] != 0;
    double s0 = 0.0;
    int64_t g0 = -1;
    for (int t = 0; t < p.k; ++t) {
        int64_t pick = -1;
        double ps = kMatchUnscored;
        int32_t pdx = 0, pdy = 0;
        uint32_t pn = 0;
        if (votes && (t == 0 || g0 >= 0)) {
            for (int64_t g = lane; g < F; g += 64) {
                const int64_t lo = g < f ? g : f, hi = g < f ? f : g;
                if (g == f || !match_candidate(p.votes, lo, hi, p.min_gap)) continue;
                const MatchBest b = p.table[match_table_index(p.F, (uint64_t)lo, (uint64_t)hi)];
                if (b.n == 0 || !(b.score >= p.score_min)) continue;
                if (t > 0 && !match_partner_behind(b.score, g, s0, g0)) continue;
                if (pick < 0 || match_partner_behind(ps, pick, b.score, g)) { pick = g; ps = b.score; pdx = b.dx; pdy = b.dy; pn = b.n; }
            }
        }
        for (int off = 32; off; off >>= 1) {
            const int64_t o_pick = __shfl_xor((long long)pick, off);
            const double o_s = __shfl_xor(ps, off);
            const int32_t o_dx = __shfl_xor(pdx, off), o_dy = __shfl_xor(pdy, off);
            const uint32_t o_n = __shfl_xor(pn, off);
            if (o_pick >= 0 && (pick < 0 || match_partner_behind(ps, pick, o_s, o_pick))) { pick = o_pick; ps = o_s; pdx = o_dx; pdy = o_dy; pn = o_n; }
        }
        if (lane == 0) {
            const size_t o = (size_t)f * (size_t)p.k + (size_t)t;
            p.partner[o] = (int32_t)pick; p.score[o] = ps; p.shift[2 * o] = pdx; p.shift[2 * o + 1] = pdy; p.n[o] = pn;
        }
        s0 = ps; g0 = pick;
    }
}

}  // namespace emba
