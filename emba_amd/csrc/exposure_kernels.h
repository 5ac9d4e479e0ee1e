// emba_amd/csrc/exposure_kernels.h — per-frame exposure (gfx950, wave64): per frame the normal equations of the 5-parameter photometric alignment (rotation,
// gain, bias), the Levenberg-Marquardt step on them, and the vote of compensated bytes into the mosaic.
// The rules: exposure_rule.h, align_rule.h, include/emba_hip.h (emba_frames_exposure_eval, emba_frames_exposure_align, emba_mosaic_frames_exposure),
// DESIGN.md §22; the bodies: frame_kernels.h.
//   * emba_frames_exposure_eval_kernel    frame_eval_body with exposure_pixel: one lane per frame pixel, the frame in blockIdx.y; the pixel's 21 terms and
//                                         its class count summed in a fixed order (the butterfly is one pass over the 21 terms); the workgroup writes its
//                                         partial sums to partial[frame][workgroup][23]
//   * emba_frames_exposure_reduce_kernel  frame_reduce_body<21>: one lane per (frame, sum), the frame's partial sums added in workgroup order
//   * emba_frames_exposure_step_kernel    one lane per frame: exposure_step — decide on the evaluated trial, propose the next; q, a, b, lambda and the
//                                         status stay on the device between iterations
//   * emba_mosaic_exposure_vote_kernel    emba_mosaic_vote_kernel with exposure_byte(v, a_f, b_f) in the place of v: frame_warp, pano_vote,
//                                         frame_vote_cells, frame_vote_counters; skip_zero tests the raw byte
// A frame whose status is final leaves the first three at once; in the evaluation kernel that is uniform over the workgroup (the frame is blockIdx.y).
// 736 B of LDS in the evaluation kernel, no scratch.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "exposure_rule.h"
#include "frame_kernels.h"
#include "kernels.h"      // kPoseStride
#include "panorama_rule.h"

namespace emba {

struct ExposureEvalParams {
    const double* lut;            // bearing vector per sensor pixel [S, 3]
    const double* q;              // the rotation each frame is evaluated at [nf, 4]
    const double* gain;           // ... and its gain and bias [nf]
    const double* bias;
    const int32_t* status;        // [nf] or nullptr: a frame whose status is not EMBA_ALIGN_RUNNING is left out
    const uint8_t* frames;        // the chunk's bytes [nf, S]
    const double* plane;          // [H, W]
    const uint8_t* valid;         // [H, W] or nullptr
    int S, W, H;
    double fx, fy, cx, cy;        // the equirectangular camera of the context
    double lo, hi, huber_k;
    int skip_zero;
    double* partial;              // [nf, gridDim.x, frame_partial(kExposureSums)]
    double* pm;                   // [nf, S, 2] or nullptr
    double* resid;                // [nf, S] or nullptr
};

// the pixel rule of frame_eval_body: 21 sums, pm as the warp gives it, exposure_pixel on the plane with the frame's gain and bias
struct ExposureEvalRule {
    static constexpr int kSums = kExposureSums;
    using Term = ExposureTerm;
    static __device__ __forceinline__ void level(const ExposureEvalParams&, double*, double*) {}
    static __device__ __forceinline__ int pixel(const ExposureEvalParams& p, size_t f, const double* pm, const double* J23, unsigned int v, ExposureTerm* t)
    {
        return exposure_pixel(p.plane, p.valid, p.W, p.H, pm[0], pm[1], J23, v, p.lo, p.hi, p.gain[f], p.bias[f], p.skip_zero != 0, p.huber_k, t);
    }
    static __device__ __forceinline__ void accumulate(const ExposureTerm& t, double* acc) { exposure_accumulate(t, acc); }
};

__global__ __launch_bounds__(kFrameThreads) void emba_frames_exposure_eval_kernel(ExposureEvalParams p) { frame_eval_body<ExposureEvalRule>(p); }

// sums [nf, 21] and counts [nf, 4] of the frames' partial sums, added in workgroup order
__global__ __launch_bounds__(kFrameThreads) void emba_frames_exposure_reduce_kernel(const double* partial, int nb, long nf, const int32_t* status, double* sums,
                                                                                     unsigned long long* counts)
{
    frame_reduce_body<kExposureSums>(partial, nb, nf, status, sums, counts);
}

// The frames' state of the loop, one array per member of ExposureFrame (exposure_rule.h); esums / ecounts: the evaluation at the trial.
struct ExposureStepParams {
    long nf;
    int first;                    // the first step of a chunk: the state is made from the trial arrays (where the call's inputs were uploaded) and the evaluation there
    int estimate;
    emba_exposure_settings set;
    double *q, *q_trial, *gain, *bias, *gain_trial, *bias_trial, *sums, *lambda, *dnorm;
    unsigned long long* counts;
    int32_t *status, *iters, *have_trial;
    const double* esums;
    const unsigned long long* ecounts;
    double* cost0;                // [nf]: cost and n of the first evaluation
    unsigned long long* n0;
    unsigned int* running;        // [1], zeroed in front of the launch: the frames still running behind this step
};

__global__ __launch_bounds__(64) void emba_frames_exposure_step_kernel(ExposureStepParams p)
{
    const long f = (long)blockIdx.x * 64 + threadIdx.x;
    if (f >= p.nf) return;
    if (!p.first && p.status[f] != EMBA_ALIGN_RUNNING) return;
    ExposureFrame s;
    uint64_t ec[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) ec[k] = p.ecounts[4 * f + k];
    if (p.first) {
        exposure_frame_init(&s, p.q_trial + 4 * f, p.gain_trial[f], p.bias_trial[f], p.set.align.lambda0);
        p.cost0[f] = p.esums[(size_t)kExposureSums * f + kExposureCost];
        p.n0[f] = ec[0];
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) { s.q[k] = p.q[4 * f + k]; s.q_trial[k] = p.q_trial[4 * f + k]; s.counts[k] = p.counts[4 * f + k]; }
#pragma unroll
        for (int k = 0; k < kExposureSums; ++k) s.sums[k] = p.sums[(size_t)kExposureSums * f + k];
        s.gain = p.gain[f]; s.bias = p.bias[f]; s.gain_trial = p.gain_trial[f]; s.bias_trial = p.bias_trial[f];
        s.lambda = p.lambda[f]; s.dnorm = p.dnorm[f];
        s.status = p.status[f]; s.iters = p.iters[f]; s.have_trial = p.have_trial[f];
    }
    exposure_step(&s, p.esums + (size_t)kExposureSums * f, ec, p.set, p.estimate);
#pragma unroll
    for (int k = 0; k < 4; ++k) { p.q[4 * f + k] = s.q[k]; p.q_trial[4 * f + k] = s.q_trial[k]; p.counts[4 * f + k] = s.counts[k]; }
#pragma unroll
    for (int k = 0; k < kExposureSums; ++k) p.sums[(size_t)kExposureSums * f + k] = s.sums[k];
    p.gain[f] = s.gain; p.bias[f] = s.bias; p.gain_trial[f] = s.gain_trial; p.bias_trial[f] = s.bias_trial;
    p.lambda[f] = s.lambda; p.dnorm[f] = s.dnorm;
    p.status[f] = s.status; p.iters[f] = s.iters; p.have_trial[f] = s.have_trial;
    if (s.status == EMBA_ALIGN_RUNNING) atomicAdd(p.running, 1u);
}

struct ExposureVoteParams {
    const double* lut;            // bearing vector per sensor pixel [S, 3]
    const double* pose;           // pose records of the chunk's frames (kPoseStride doubles each)
    const double* gain;           // the chunk's gains and biases [nf]
    const double* bias;
    const uint8_t* frames;        // the chunk's bytes [nf, S]
    int S, W, H;
    double fx, fy, cx, cy;        // the equirectangular camera of the context
    int skip_zero;                // a RAW byte of 0 casts no vote and is counted
    unsigned long long* sum_w;    // [H, W]
    unsigned long long* sum_v;    // [H, W]
    double* pm;                   // [nf, S, 2] or nullptr
    unsigned long long* counters; // [0] dropped votes, [1] skipped pixels (zeroed on the stream in front of the first launch)
};

// Compiled without contraction: pm feeds floor(), and the compensated byte is rint of a product and a sum.
#pragma clang fp contract(off)
__global__ __launch_bounds__(kFrameThreads) void emba_mosaic_exposure_vote_kernel(ExposureVoteParams p)
{
    const int s = (int)blockIdx.x * kFrameThreads + (int)threadIdx.x;
    const size_t f = blockIdx.y;
    unsigned int dropped = 0, skipped = 0;
    if (s < p.S) {
        const size_t o = f * (size_t)p.S + (size_t)s;
        const unsigned int raw = p.frames[o];
        double pm[2], J23[6];
        frame_warp(p.lut, p.pose + (size_t)kPoseStride * f, s, p.fx, p.fy, p.cx, p.cy, pm, J23);
        if (p.pm) { p.pm[2 * o] = pm[0]; p.pm[2 * o + 1] = pm[1]; }
        if (p.skip_zero && raw == 0) skipped = 1;
        else {
            const unsigned int v = exposure_byte(raw, p.gain[f], p.bias[f]);
            frame_vote_cells(pano_vote(pm[0], pm[1], p.W, p.H), v, p.sum_w, p.sum_v, dropped);
        }
    }
    frame_vote_counters(dropped, skipped, p.counters);
}
#pragma clang fp contract(fast)

}  // namespace emba
