// emba_amd/csrc/refit_kernels.h — tracked frames refitted against the mosaic of the other frames (gfx950, wave64): the vote that can be taken out again, and
// the per-frame bookkeeping of a sweep.  The evaluation, reduce and step kernels of a batch's alignment are track_exposure_kernels.h's and
// exposure_kernels.h's, as they are.
// The rules: refit_rule.h, track_exposure_rule.h, track_rule.h, exposure_rule.h, panorama_rule.h (pano_vote), include/emba_hip.h (emba_frames_refit),
// DESIGN.md §25; the bodies: frame_kernels.h.
//   * emba_frames_refit_vote_kernel     emba_frames_track_exposure_vote_kernel with a sign and a selector: one lane per pixel, the frame in blockIdx.y;
//                                       a frame the selector leaves out leaves at once (the whole workgroup); frame_warp once, then per plane pano_vote on
//                                       the level's grid and per cell two return-less 64-bit integer atomic adds of w and w * v — or, with `negate`, of
//                                       their two's complements; the two counters likewise.  `negate` is an argument of the kernel: uniform over the grid.
//                                       Vote and un-vote are this one kernel, so their pm cannot differ
//   * emba_frames_refit_frame_kernel    one lane per frame, by phase: the start of a sweep (codes and the last sweep's figures reset), the start of a batch
//                                       (own values, or the interpolation across lost frames), the end of a level, the verdict (keep-old on failure, with
//                                       the refit code)
// No floating-point atomic, no grid-wide synchronisation, no cooperative launch and no flag anywhere: ordering comes from the stream.  No LDS, no scratch.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "frame_kernels.h"
#include "refit_rule.h"
#include "track_kernels.h"      // TrackPlane

namespace emba {

// Compiled without contraction, the whole header: pm feeds floor(), and the compensated byte is rint of a product and a sum.
#pragma clang fp contract(off)

struct RefitVoteParams {
    const double* lut;            // bearing vector per sensor pixel [S, 3]
    const double* q;              // the rotation of each frame of the batch [nf, 4]
    const double* gain;           // ... and its gain and bias [nf]
    const double* bias;
    const int32_t* status;        // [nf]: EMBA_TRACK_*
    const uint8_t* frames;        // the batch's bytes [nf, S]
    int S, n_planes;
    double fx, fy, cx, cy;
    int skip_zero;                // a RAW byte of 0 casts no vote and is counted
    int select;                   // RefitSelect: the frames this launch serves
    int negate;                   // the un-vote: every added value is negated modulo 2^64
    double* pm;                   // [nf, S, 2] or nullptr (never with negate): the level-0 pm of every voting frame of the batch, NaN for one that does not vote
    unsigned long long* counters; // [0] dropped votes, [1] skipped pixels
    TrackPlane plane[kTrackMaxPlanes];
};

// frame_vote_cells with the sign: the same cells, the same weights, the same return-less adds
__device__ __forceinline__ void refit_vote_cells(const PanoVotes& pv, unsigned int v, bool negate, unsigned long long* sum_w, unsigned long long* sum_v, unsigned int& dropped)
{
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (!pv.w[k]) continue;
        if (pv.cell[k] < 0) { ++dropped; continue; }
        atomicAdd(sum_w + pv.cell[k], (unsigned long long)refit_signed((uint64_t)pv.w[k], negate));                          // (results unused: return-less adds)
        if (v) atomicAdd(sum_v + pv.cell[k], (unsigned long long)refit_signed((uint64_t)pv.w[k] * (uint64_t)v, negate));
    }
}

// frame_vote_counters with the sign; every lane of the wave calls it
__device__ __forceinline__ void refit_vote_counters(unsigned int dropped, unsigned int skipped, bool negate, unsigned long long* counters)
{
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) { dropped += __shfl_xor(dropped, o); skipped += __shfl_xor(skipped, o); }
    if ((threadIdx.x & 63) == 0) {
        if (dropped) atomicAdd(counters, (unsigned long long)refit_signed(dropped, negate));
        if (skipped) atomicAdd(counters + 1, (unsigned long long)refit_signed(skipped, negate));
    }
}

__global__ __launch_bounds__(kFrameThreads) void emba_frames_refit_vote_kernel(RefitVoteParams p)
{
    const int s = (int)blockIdx.x * kFrameThreads + (int)threadIdx.x;
    const size_t f = blockIdx.y;
    const int status = p.status[f];
    if (!refit_selected(p.select, status)) {      // (the whole workgroup)
        if (p.pm && s < p.S) {
            // an anchor of a sweep's batch stays in the planes: its pm is reported, nothing is voted
            const size_t o = f * (size_t)p.S + (size_t)s;
            double pm[2] = {__builtin_nan(""), __builtin_nan("")}, J23[6];
            if (track_votes(status)) frame_warp(p.lut, p.q + 4 * f, s, p.fx, p.fy, p.cx, p.cy, pm, J23);
            p.pm[2 * o] = pm[0]; p.pm[2 * o + 1] = pm[1];
        }
        return;
    }
    const bool negate = p.negate != 0;
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
                refit_vote_cells(pano_vote(pm[0] * L.scale, pm[1] * L.scale, L.W, L.H), v, negate, L.sum_w, L.sum_v, dropped);
            }
        }
    }
    refit_vote_counters(dropped, skipped, negate, p.counters);
}

enum RefitPhase { kRefitSweepBegin = 0, kRefitStart = 1, kRefitLevelEnd = 2, kRefitVerdict = 3 };

// The bookkeeping of the frames [f0, f0 + nf): a batch's, or (kRefitSweepBegin) all F.
struct RefitFrameParams {
    int phase;                            // RefitPhase
    long nf, f0, F;
    int n_levels, level_index, recover;
    double min_overlap;
    unsigned long long S;
    const long long* t;                   // [F]
    double *q_all, *gain_all, *bias_all;  // [F, 4], [F], [F]: every frame's current values
    int32_t* status_all;                  // [F]: EMBA_TRACK_*
    int32_t* refit_all;                   // [F]: EMBA_REFIT_* of this sweep
    int32_t* iters_all;                   // [F, n_levels]
    double *cost_all, *overlap_all;       // [F]
    unsigned long long* counts_all;       // [F, 4]
    double *q, *q_trial;                  // [nf, 4]: the loop's accepted rotation; where the next level starts
    double *gain, *gain_trial;            // [nf]: the same two of the gain
    double *bias, *bias_trial;            // [nf]: ... and of the bias
    const double* sums;                   // [nf, 21]
    const unsigned long long* counts;     // [nf, 4]
    const int32_t *status, *iters;        // [nf]: the loop's, of the level that ended last
};

__global__ __launch_bounds__(64) void emba_frames_refit_frame_kernel(RefitFrameParams p)
{
    const long i = (long)blockIdx.x * 64 + threadIdx.x;
    if (i >= p.nf) return;
    const long f = p.f0 + i;
    const int st = p.status_all[f];      // (as the frame entered the batch: only its own verdict writes it)
    if (p.phase == kRefitSweepBegin) {
        p.refit_all[f] = st == EMBA_TRACK_TRACKED ? 0 : refit_code(st, false);
        for (int l = 0; l < p.n_levels; ++l) p.iters_all[f * p.n_levels + l] = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) p.counts_all[4 * f + k] = 0;
        p.cost_all[f] = 0.0; p.overlap_all[f] = 0.0;
    } else if (p.phase == kRefitStart) {
        // a frame the sweep does not align is evaluated where it stands (or at the interpolation), and its result is dropped
        double q[4] = {0.0, 0.0, 0.0, 1.0}, a = 1.0, b = 0.0;
        refit_start(p.status_all, p.t, p.q_all, p.gain_all, p.bias_all, p.F, f, q, &a, &b);
#pragma unroll
        for (int k = 0; k < 4; ++k) p.q_trial[4 * i + k] = q[k];
        p.gain_trial[i] = a;
        p.bias_trial[i] = b;
    } else if (p.phase == kRefitLevelEnd) {
        if (refit_active(st, p.recover != 0)) p.iters_all[f * p.n_levels + p.level_index] = p.iters[i];
#pragma unroll
        for (int k = 0; k < 4; ++k) p.q_trial[4 * i + k] = p.q[4 * i + k];
        p.gain_trial[i] = p.gain[i];
        p.bias_trial[i] = p.bias[i];
    } else {
        if (!refit_active(st, p.recover != 0)) return;
        const double overlap = track_overlap(p.counts[4 * i], p.counts[4 * i + 3], p.S);
        const bool passed = track_verdict(p.status[i], overlap, p.min_overlap) == EMBA_TRACK_TRACKED;
        if (passed) {
#pragma unroll
            for (int k = 0; k < 4; ++k) p.q_all[4 * f + k] = p.q[4 * i + k];
            p.gain_all[f] = p.gain[i];
            p.bias_all[f] = p.bias[i];
            p.status_all[f] = EMBA_TRACK_TRACKED;
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) p.counts_all[4 * f + k] = p.counts[4 * i + k];
        p.cost_all[f] = p.sums[(size_t)kExposureSums * i + kExposureCost];
        p.overlap_all[f] = overlap;
        p.refit_all[f] = refit_code(st, passed);
    }
}
#pragma clang fp contract(fast)

}  // namespace emba
