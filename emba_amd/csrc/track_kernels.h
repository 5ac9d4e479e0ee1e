// emba_amd/csrc/track_kernels.h — intensity frames tracked against their own growing mosaic (gfx950, wave64): a frame's normal equations against a level's
// two integer sums, the vote of the tracked frames into every level, and the per-frame bookkeeping between them.
// The rules: track_rule.h, align_rule.h, mosaic_rule.h, panorama_rule.h (pano_vote), include/emba_hip.h (emba_frames_track, emba_track_eval), DESIGN.md §21;
// the bodies: frame_kernels.h.
//   * emba_frames_track_eval_kernel    frame_eval_body with track_pixel: the warp once at level 0, pm and J23 scaled by 2^-l; track_pixel forms the four
//                                      means of the level's two sums in registers; ten sums, partial[frame][workgroup][12].  The reduce and step kernels
//                                      behind it are align_kernels.h's, as they are
//   * emba_frames_track_vote_kernel    one lane per frame pixel, the frame in blockIdx.y; a frame that is neither tracked nor the anchor leaves at once (and
//                                      fills its pm with NaN); frame_warp once, then per plane pano_vote on the level's grid and frame_vote_cells;
//                                      frame_vote_counters
//   * emba_frames_track_frame_kernel   one lane per frame of a batch, by phase: the anchor; the prediction from the last two tracked frames (found by walking
//                                      the statuses back from the batch's first frame); the end of a level (its iterations, the next level's start); the
//                                      verdict.  Batches follow each other on the stream without the host reading a pose
// No grid-wide synchronisation and no flag anywhere: ordering comes from the stream.  384 B of LDS in the evaluation kernel, no scratch.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "align_kernels.h"
#include "frame_kernels.h"
#include "track_rule.h"

namespace emba {

struct TrackEvalParams {
    const double* lut;                    // bearing vector per sensor pixel [S, 3]
    const double* q;                      // the rotation each frame is evaluated at [nf, 4]
    const int32_t* status;                // [nf] or nullptr: a frame whose status is not EMBA_ALIGN_RUNNING is left out
    const uint8_t* frames;                // the batch's bytes [nf, S]
    const unsigned long long* sum_w;      // the level's planes [H_l, W_l]
    const unsigned long long* sum_v;
    int S, W, H;                          // W, H: the level's
    double scale;                         // 2^-l
    double fx, fy, cx, cy;                // the equirectangular camera of the context (level 0)
    unsigned long long min_weight;
    double huber_k;
    int skip_zero;
    double* partial;                      // [nf, gridDim.x, frame_partial(kAlignSums)]
    double* pm;                           // [nf, S, 2] or nullptr: the level's pm
    double* resid;                        // [nf, S] or nullptr
};

// Compiled without contraction: pm feeds floor(), and r is compared by its bits.
#pragma clang fp contract(off)
// the pixel rule of frame_eval_body: ten sums, pm and J23 on the level's grid, track_pixel on the level's two sums
struct TrackEvalRule {
    static constexpr int kSums = kAlignSums;
    using Term = AlignTerm;
    static __device__ __forceinline__ void level(const TrackEvalParams& p, double* pm, double* J23)
    {
        pm[0] *= p.scale; pm[1] *= p.scale;      // (a power of two: exact)
#pragma unroll
        for (int j = 0; j < 6; ++j) J23[j] *= p.scale;
    }
    static __device__ __forceinline__ int pixel(const TrackEvalParams& p, size_t, const double* pm, const double* J23, unsigned int v, AlignTerm* t)
    {
        return track_pixel(reinterpret_cast<const uint64_t*>(p.sum_w), reinterpret_cast<const uint64_t*>(p.sum_v), p.W, p.H, pm[0], pm[1], J23, v,
                           (uint64_t)p.min_weight, p.skip_zero != 0, p.huber_k, t);
    }
    static __device__ __forceinline__ void accumulate(const AlignTerm& t, double* acc) { align_accumulate(t, acc); }
};

__global__ __launch_bounds__(kFrameThreads) void emba_frames_track_eval_kernel(TrackEvalParams p) { frame_eval_body<TrackEvalRule>(p); }

struct TrackPlane { unsigned long long *sum_w, *sum_v; int W, H; double scale; };
struct TrackVoteParams {
    const double* lut;            // bearing vector per sensor pixel [S, 3]
    const double* q;              // the rotation of each frame of the batch [nf, 4]
    const int32_t* status;        // [nf]: EMBA_TRACK_*; only the anchor and the tracked frames vote
    const uint8_t* frames;        // the batch's bytes [nf, S]
    int S, n_planes;
    double fx, fy, cx, cy;
    int skip_zero;
    double* pm;                   // [nf, S, 2] or nullptr: the level-0 pm, NaN for a frame that does not vote
    unsigned long long* counters; // [0] dropped votes, [1] skipped pixels
    TrackPlane plane[kTrackMaxPlanes];
};

__global__ __launch_bounds__(kFrameThreads) void emba_frames_track_vote_kernel(TrackVoteParams p)
{
    const int s = (int)blockIdx.x * kFrameThreads + (int)threadIdx.x;
    const size_t f = blockIdx.y;
    if (!track_votes(p.status[f])) {      // (the whole workgroup)
        if (p.pm && s < p.S) { const size_t o = f * (size_t)p.S + (size_t)s; p.pm[2 * o] = p.pm[2 * o + 1] = __builtin_nan(""); }
        return;
    }
    unsigned int dropped = 0, skipped = 0;
    if (s < p.S) {
        const size_t o = f * (size_t)p.S + (size_t)s;
        const unsigned int v = p.frames[o];
        double pm[2], J23[6];
        frame_warp(p.lut, p.q + 4 * f, s, p.fx, p.fy, p.cx, p.cy, pm, J23);
        if (p.pm) { p.pm[2 * o] = pm[0]; p.pm[2 * o + 1] = pm[1]; }
        if (p.skip_zero && v == 0) skipped = 1;
        else {
#pragma unroll 1
            for (int l = 0; l < p.n_planes; ++l) {
                const TrackPlane& L = p.plane[l];      // (uniform: read from the kernel's arguments)
                frame_vote_cells(pano_vote(pm[0] * L.scale, pm[1] * L.scale, L.W, L.H), v, L.sum_w, L.sum_v, dropped);
            }
        }
    }
    frame_vote_counters(dropped, skipped, p.counters);
}
#pragma clang fp contract(fast)

// The bookkeeping of a batch's frames [f0, f0 + nf): arrays over the call's frames (t, q_all, status_all, ...) and over the batch (the members of the loop's state).
enum TrackPhase : int { kTrackAnchor = 0, kTrackPredict = 1, kTrackLevelEnd = 2, kTrackVerdict = 3 };
struct TrackFrameParams {
    int phase;
    long nf, f0;
    int n_levels, level_index, predict;
    double min_overlap;
    unsigned long long S;
    double q0[4];                         // kTrackAnchor: normalise(q0)
    const long long* t;                   // [F]
    double* q_all;                        // [F, 4]
    int32_t* status_all;                  // [F]: 0 until the frame has its verdict
    int32_t* iters_all;                   // [F, n_levels]
    double *cost_all, *overlap_all;       // [F]
    unsigned long long* counts_all;       // [F, 4]
    double *pred, *q, *q_trial;           // [nf, 4]: the prediction; the loop's accepted rotation; where the next level starts
    const double* sums;                   // [nf, 10]
    const unsigned long long* counts;     // [nf, 4]
    const int32_t *status, *iters;        // [nf]: the loop's, of the level that ended last
};

__global__ __launch_bounds__(64) void emba_frames_track_frame_kernel(TrackFrameParams p)
{
    const long i = (long)blockIdx.x * 64 + threadIdx.x;
    if (i >= p.nf) return;
    const long f = p.f0 + i;
    if (p.phase == kTrackAnchor) {
#pragma unroll
        for (int k = 0; k < 4; ++k) { p.q_all[4 * f + k] = p.q0[k]; p.counts_all[4 * f + k] = 0; }
        for (int l = 0; l < p.n_levels; ++l) p.iters_all[f * p.n_levels + l] = 0;
        p.cost_all[f] = 0.0; p.overlap_all[f] = 0.0;
        p.status_all[f] = EMBA_TRACK_ANCHOR;
    } else if (p.phase == kTrackPredict) {
        long b = p.f0 - 1;
        while (b >= 0 && !track_votes(p.status_all[b])) --b;
        long a = b - 1;
        while (a >= 0 && !track_votes(p.status_all[a])) --a;
        double qa[4] = {0.0, 0.0, 0.0, 1.0}, qb[4] = {0.0, 0.0, 0.0, 1.0}, q[4] = {0.0, 0.0, 0.0, 1.0};
        long long ta = 0, tb = 0;
        if (b >= 0) { tb = p.t[b]; for (int k = 0; k < 4; ++k) qb[k] = p.q_all[4 * b + k]; }
        if (a >= 0) { ta = p.t[a]; for (int k = 0; k < 4; ++k) qa[k] = p.q_all[4 * a + k]; }
        track_predict((b >= 0) + (a >= 0), qa, ta, qb, tb, p.t[f], p.predict != 0, q);
#pragma unroll
        for (int k = 0; k < 4; ++k) p.pred[4 * i + k] = p.q_trial[4 * i + k] = q[k];
    } else if (p.phase == kTrackLevelEnd) {
        p.iters_all[f * p.n_levels + p.level_index] = p.iters[i];
#pragma unroll
        for (int k = 0; k < 4; ++k) p.q_trial[4 * i + k] = p.q[4 * i + k];
    } else {
        const double overlap = track_overlap(p.counts[4 * i], p.counts[4 * i + 3], p.S);
        const int verdict = track_verdict(p.status[i], overlap, p.min_overlap);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            p.q_all[4 * f + k] = verdict == EMBA_TRACK_TRACKED ? p.q[4 * i + k] : p.pred[4 * i + k];
            p.counts_all[4 * f + k] = p.counts[4 * i + k];
        }
        p.cost_all[f] = p.sums[(size_t)kAlignSums * i + 9];
        p.overlap_all[f] = overlap;
        p.status_all[f] = verdict;
    }
}

}  // namespace emba
