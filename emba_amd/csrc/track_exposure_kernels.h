// emba_amd/csrc/track_exposure_kernels.h — the frame tracker with a per-frame exposure (gfx950, wave64): a frame's 5-parameter normal equations against a
// level's two integer sums, the vote of the tracked frames' compensated bytes into every level, and the per-frame bookkeeping between them.
// The rules: track_exposure_rule.h, track_rule.h, exposure_rule.h, align_rule.h, mosaic_rule.h, panorama_rule.h (pano_vote), include/emba_hip.h
// (emba_frames_track_exposure, emba_track_exposure_eval); the bodies: frame_kernels.h.
//   * emba_frames_track_exposure_eval_kernel    frame_eval_body with track_exposure_pixel: the warp once at level 0, pm and J23 scaled by 2^-l; the four means
//                                               of the level's two sums formed in registers; the frame's gain and bias; 21 sums (the butterfly is one pass
//                                               over the 21 terms), partial[frame][workgroup][23].  The reduce and step kernels behind it are
//                                               exposure_kernels.h's, as they are
//   * emba_frames_track_exposure_vote_kernel    emba_frames_track_vote_kernel with exposure_byte(v, a_f, b_f) in the place of v: a frame that is neither
//                                               tracked nor the anchor leaves at once (and fills its pm with NaN); frame_warp once, then per plane pano_vote
//                                               on the level's grid and frame_vote_cells; frame_vote_counters; skip_zero tests the raw byte
//   * emba_frames_track_exposure_frame_kernel   emba_frames_track_frame_kernel with the gain and bias carried along: the anchor (q0, 1, 0); the prediction
//                                               (the rotation from the last two tracked frames, gain and bias from the last one); the end of a level
//                                               (q, a, b to the trial arrays); the verdict (q_all, gain_all, bias_all)
// No floating-point atomic, no grid-wide synchronisation, no cooperative launch and no flag anywhere: ordering comes from the stream.  736 B of LDS in the
// evaluation kernel, no scratch.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "exposure_kernels.h"
#include "frame_kernels.h"
#include "track_exposure_rule.h"
#include "track_kernels.h"      // TrackPlane, TrackPhase

namespace emba {

// Compiled without contraction, the whole header: pm feeds floor(), r is compared by its bits, and the compensated byte is rint of a product and a sum.
#pragma clang fp contract(off)

struct TrackExposureEvalParams {
    const double* lut;                    // bearing vector per sensor pixel [S, 3]
    const double* q;                      // the rotation each frame is evaluated at [nf, 4]
    const double* gain;                   // ... and its gain and bias [nf]
    const double* bias;
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
    double* partial;                      // [nf, gridDim.x, frame_partial(kExposureSums)]
    double* pm;                           // [nf, S, 2] or nullptr: the level's pm
    double* resid;                        // [nf, S] or nullptr
};

// the pixel rule of frame_eval_body: 21 sums, pm and J23 on the level's grid, track_exposure_pixel on the level's two sums with the frame's gain and bias
struct TrackExposureEvalRule {
    static constexpr int kSums = kExposureSums;
    using Term = ExposureTerm;
    static __device__ __forceinline__ void level(const TrackExposureEvalParams& p, double* pm, double* J23)
    {
        pm[0] *= p.scale; pm[1] *= p.scale;      // (a power of two: exact)
#pragma unroll
        for (int j = 0; j < 6; ++j) J23[j] *= p.scale;
    }
    static __device__ __forceinline__ int pixel(const TrackExposureEvalParams& p, size_t f, const double* pm, const double* J23, unsigned int v, ExposureTerm* t)
    {
        return track_exposure_pixel(reinterpret_cast<const uint64_t*>(p.sum_w), reinterpret_cast<const uint64_t*>(p.sum_v), p.W, p.H, pm[0], pm[1], J23, v,
                                    (uint64_t)p.min_weight, p.gain[f], p.bias[f], p.skip_zero != 0, p.huber_k, t);
    }
    static __device__ __forceinline__ void accumulate(const ExposureTerm& t, double* acc) { exposure_accumulate(t, acc); }
};

__global__ __launch_bounds__(kFrameThreads) void emba_frames_track_exposure_eval_kernel(TrackExposureEvalParams p) { frame_eval_body<TrackExposureEvalRule>(p); }

struct TrackExposureVoteParams {
    const double* lut;            // bearing vector per sensor pixel [S, 3]
    const double* q;              // the rotation of each frame of the batch [nf, 4]
    const double* gain;           // ... and its gain and bias [nf]
    const double* bias;
    const int32_t* status;        // [nf]: EMBA_TRACK_*; only the anchor and the tracked frames vote
    const uint8_t* frames;        // the batch's bytes [nf, S]
    int S, n_planes;
    double fx, fy, cx, cy;
    int skip_zero;                // a RAW byte of 0 casts no vote and is counted
    double* pm;                   // [nf, S, 2] or nullptr: the level-0 pm, NaN for a frame that does not vote
    unsigned long long* counters; // [0] dropped votes, [1] skipped pixels
    TrackPlane plane[kTrackMaxPlanes];
};

__global__ __launch_bounds__(kFrameThreads) void emba_frames_track_exposure_vote_kernel(TrackExposureVoteParams p)
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
        const unsigned int raw = p.frames[o];
        double pm[2], J23[6];
        frame_warp(p.lut, p.q + 4 * f, s, p.fx, p.fy, p.cx, p.cy, pm, J23);
        if (p.pm) { p.pm[2 * o] = pm[0]; p.pm[2 * o + 1] = pm[1]; }
        if (p.skip_zero && raw == 0) skipped = 1;
        else {
            const unsigned int v = exposure_byte(raw, p.gain[f], p.bias[f]);
#pragma unroll 1
            for (int l = 0; l < p.n_planes; ++l) {
                const TrackPlane& L = p.plane[l];      // (uniform: read from the kernel's arguments)
                frame_vote_cells(pano_vote(pm[0] * L.scale, pm[1] * L.scale, L.W, L.H), v, L.sum_w, L.sum_v, dropped);
            }
        }
    }
    frame_vote_counters(dropped, skipped, p.counters);
}

// The bookkeeping of a batch's frames [f0, f0 + nf): TrackFrameParams' arrays, and beside each rotation its gain and bias.
struct TrackExposureFrameParams {
    int phase;                            // TrackPhase
    long nf, f0;
    int n_levels, level_index, predict;
    double min_overlap;
    unsigned long long S;
    double q0[4];                         // kTrackAnchor: normalise(q0)
    const long long* t;                   // [F]
    double *q_all, *gain_all, *bias_all;  // [F, 4], [F], [F]
    int32_t* status_all;                  // [F]: 0 until the frame has its verdict
    int32_t* iters_all;                   // [F, n_levels]
    double *cost_all, *overlap_all;       // [F]
    unsigned long long* counts_all;       // [F, 4]
    double *pred, *q, *q_trial;           // [nf, 4]: the prediction; the loop's accepted rotation; where the next level starts
    double *gain_pred, *gain, *gain_trial;      // [nf]: the same three of the gain
    double *bias_pred, *bias, *bias_trial;      // [nf]: ... and of the bias
    const double* sums;                   // [nf, 21]
    const unsigned long long* counts;     // [nf, 4]
    const int32_t *status, *iters;        // [nf]: the loop's, of the level that ended last
};

__global__ __launch_bounds__(64) void emba_frames_track_exposure_frame_kernel(TrackExposureFrameParams p)
{
    const long i = (long)blockIdx.x * 64 + threadIdx.x;
    if (i >= p.nf) return;
    const long f = p.f0 + i;
    if (p.phase == kTrackAnchor) {
#pragma unroll
        for (int k = 0; k < 4; ++k) { p.q_all[4 * f + k] = p.q0[k]; p.counts_all[4 * f + k] = 0; }
        p.gain_all[f] = 1.0; p.bias_all[f] = 0.0;
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
        double ga, gb;
        track_exposure_start(p.status_all, p.gain_all, p.bias_all, p.f0, &ga, &gb);
#pragma unroll
        for (int k = 0; k < 4; ++k) p.pred[4 * i + k] = p.q_trial[4 * i + k] = q[k];
        p.gain_pred[i] = p.gain_trial[i] = ga;
        p.bias_pred[i] = p.bias_trial[i] = gb;
    } else if (p.phase == kTrackLevelEnd) {
        p.iters_all[f * p.n_levels + p.level_index] = p.iters[i];
#pragma unroll
        for (int k = 0; k < 4; ++k) p.q_trial[4 * i + k] = p.q[4 * i + k];
        p.gain_trial[i] = p.gain[i];
        p.bias_trial[i] = p.bias[i];
    } else {
        const double overlap = track_overlap(p.counts[4 * i], p.counts[4 * i + 3], p.S);
        const int verdict = track_verdict(p.status[i], overlap, p.min_overlap);
        const bool tracked = verdict == EMBA_TRACK_TRACKED;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            p.q_all[4 * f + k] = tracked ? p.q[4 * i + k] : p.pred[4 * i + k];
            p.counts_all[4 * f + k] = p.counts[4 * i + k];
        }
        p.gain_all[f] = tracked ? p.gain[i] : p.gain_pred[i];
        p.bias_all[f] = tracked ? p.bias[i] : p.bias_pred[i];
        p.cost_all[f] = p.sums[(size_t)kExposureSums * i + kExposureCost];
        p.overlap_all[f] = overlap;
        p.status_all[f] = verdict;
    }
}
#pragma clang fp contract(fast)

}  // namespace emba
