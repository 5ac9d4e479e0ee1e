// emba_amd/csrc/align_kernels.h — intensity frames aligned to a panorama plane (gfx950, wave64): per frame the normal equations of a 3-DoF photometric
// alignment, and the Levenberg-Marquardt step on them.
// The rules: align_rule.h, include/emba_hip.h (emba_frames_align_eval, emba_frames_align); the bodies: frame_kernels.h.
//   * emba_frames_align_eval_kernel    frame_eval_body with align_pixel: one lane per frame pixel, the frame in blockIdx.y; the pixel's ten terms and its
//                                      class count summed in a fixed order; the workgroup writes its partial sums to partial[frame][workgroup][12]
//   * emba_frames_align_reduce_kernel  frame_reduce_body<10>: one lane per (frame, sum), the frame's partial sums added in workgroup order.  The tracker
//                                      (track_kernels.h) reduces and steps with this kernel and the next, as they are
//   * emba_frames_align_step_kernel    one lane per frame: align_step — decide on the evaluated trial, propose the next
// A frame whose status is final leaves all three at once; in the evaluation kernel that is uniform over the workgroup (the frame is blockIdx.y).
// 384 B of LDS in the evaluation kernel, no scratch.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "align_rule.h"
#include "frame_kernels.h"

namespace emba {

struct AlignEvalParams {
    const double* lut;            // bearing vector per sensor pixel [S, 3]
    const double* q;              // the rotation each frame is evaluated at [nf, 4]
    const int32_t* status;        // [nf] or nullptr: a frame whose status is not EMBA_ALIGN_RUNNING is left out
    const uint8_t* frames;        // the chunk's bytes [nf, S]
    const double* plane;          // [H, W]
    const uint8_t* valid;         // [H, W] or nullptr
    int S, W, H;
    double fx, fy, cx, cy;        // the equirectangular camera of the context
    double lo, hi, huber_k;
    int skip_zero;
    double* partial;              // [nf, gridDim.x, frame_partial(kAlignSums)]
    double* pm;                   // [nf, S, 2] or nullptr
    double* resid;                // [nf, S] or nullptr
};

// the pixel rule of frame_eval_body: ten sums, pm as the warp gives it, align_pixel on the plane
struct AlignEvalRule {
    static constexpr int kSums = kAlignSums;
    using Term = AlignTerm;
    static __device__ __forceinline__ void level(const AlignEvalParams&, double*, double*) {}
    static __device__ __forceinline__ int pixel(const AlignEvalParams& p, size_t, const double* pm, const double* J23, unsigned int v, AlignTerm* t)
    {
        return align_pixel(p.plane, p.valid, p.W, p.H, pm[0], pm[1], J23, v, p.lo, p.hi, p.skip_zero != 0, p.huber_k, t);
    }
    static __device__ __forceinline__ void accumulate(const AlignTerm& t, double* acc) { align_accumulate(t, acc); }
};

__global__ __launch_bounds__(kFrameThreads) void emba_frames_align_eval_kernel(AlignEvalParams p) { frame_eval_body<AlignEvalRule>(p); }

// sums [nf, 10] and counts [nf, 4] of the frames' partial sums, added in workgroup order
__global__ __launch_bounds__(kFrameThreads) void emba_frames_align_reduce_kernel(const double* partial, int nb, long nf, const int32_t* status, double* sums,
                                                                                  unsigned long long* counts)
{
    frame_reduce_body<kAlignSums>(partial, nb, nf, status, sums, counts);
}

// The frames' state of the loop, one array per member of AlignFrame (align_rule.h); esums / ecounts: the evaluation at q_trial.
struct AlignStepParams {
    long nf;
    int first;                    // the first step of a chunk: the state is made from q_trial (where the call's q_xyzw was uploaded) and the evaluation there
    emba_align_settings set;
    double *q, *q_trial, *sums, *lambda, *dnorm;
    unsigned long long* counts;
    int32_t *status, *iters, *have_trial;
    const double* esums;
    const unsigned long long* ecounts;
    double* cost0;                // [nf]: cost and n of the first evaluation
    unsigned long long* n0;
    unsigned int* running;        // [1], zeroed in front of the launch: the frames still running behind this step
};

__global__ __launch_bounds__(64) void emba_frames_align_step_kernel(AlignStepParams p)
{
    const long f = (long)blockIdx.x * 64 + threadIdx.x;
    if (f >= p.nf) return;
    if (!p.first && p.status[f] != EMBA_ALIGN_RUNNING) return;
    AlignFrame s;
    uint64_t ec[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) ec[k] = p.ecounts[4 * f + k];
    if (p.first) {
        align_frame_init(&s, p.q_trial + 4 * f, p.set.lambda0);
        p.cost0[f] = p.esums[(size_t)kAlignSums * f + 9];
        p.n0[f] = ec[0];
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) { s.q[k] = p.q[4 * f + k]; s.q_trial[k] = p.q_trial[4 * f + k]; s.counts[k] = p.counts[4 * f + k]; }
#pragma unroll
        for (int k = 0; k < kAlignSums; ++k) s.sums[k] = p.sums[(size_t)kAlignSums * f + k];
        s.lambda = p.lambda[f]; s.dnorm = p.dnorm[f];
        s.status = p.status[f]; s.iters = p.iters[f]; s.have_trial = p.have_trial[f];
    }
    align_step(&s, p.esums + (size_t)kAlignSums * f, ec, p.set);
#pragma unroll
    for (int k = 0; k < 4; ++k) { p.q[4 * f + k] = s.q[k]; p.q_trial[4 * f + k] = s.q_trial[k]; p.counts[4 * f + k] = s.counts[k]; }
#pragma unroll
    for (int k = 0; k < kAlignSums; ++k) p.sums[(size_t)kAlignSums * f + k] = s.sums[k];
    p.lambda[f] = s.lambda; p.dnorm[f] = s.dnorm;
    p.status[f] = s.status; p.iters[f] = s.iters; p.have_trial[f] = s.have_trial;
    if (s.status == EMBA_ALIGN_RUNNING) atomicAdd(p.running, 1u);
}

}  // namespace emba
