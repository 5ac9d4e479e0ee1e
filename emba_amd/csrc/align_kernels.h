// emba_amd/csrc/align_kernels.h — intensity frames aligned to a panorama plane (gfx950, wave64): per frame the normal equations of a 3-DoF photometric
// alignment, and the Levenberg-Marquardt step on them.
// The rules: align_rule.h, include/emba_hip.h (emba_frames_align_eval, emba_frames_align), DESIGN.md §20.
//   * emba_frames_align_eval_kernel    one lane per frame pixel, the frame in blockIdx.y: the byte (coalesced), the warp of emba_view_kernel (quat_to_matrix,
//                                      the sum3 products, project_chain<false>, here with its Jacobian live), align_pixel, and the pixel's ten terms and its
//                                      class count summed over the wave by shuffles and over the workgroup's four waves in LDS, in a fixed order; the
//                                      workgroup writes its partial sums to partial[frame][workgroup][12]
//   * emba_frames_align_reduce_kernel  one lane per (frame, sum): the frame's partial sums added in workgroup order.  No floating-point atomic anywhere: the
//                                      same inputs give the same bits
//   * emba_frames_align_step_kernel    one lane per frame: align_step — decide on the evaluated trial, propose the next
// A frame whose status is final leaves all three at once; in the evaluation kernel that is uniform over the workgroup (the frame is blockIdx.y).
// 384 B of LDS in the evaluation kernel, no scratch.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "align_rule.h"
#include "device_math.h"

namespace emba {

constexpr int kAlignThreads = 256;
constexpr int kAlignWaves = kAlignThreads / 64;
constexpr int kAlignPartial = 12;      // doubles per (frame, workgroup): the ten sums, then the four class counts as uint32 in the space of two

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
    double* partial;              // [nf, gridDim.x, kAlignPartial]
    double* pm;                   // [nf, S, 2] or nullptr
    double* resid;                // [nf, S] or nullptr
};

// Compiled without contraction: pm feeds floor(), and r is compared by its bits.
#pragma clang fp contract(off)
__global__ __launch_bounds__(kAlignThreads) void emba_frames_align_eval_kernel(AlignEvalParams p)
{
    __shared__ double red[kAlignWaves][kAlignSums];
    __shared__ unsigned int redc[kAlignWaves][4];
    const size_t f = blockIdx.y;
    if (p.status && p.status[f] != EMBA_ALIGN_RUNNING) return;      // (the whole workgroup: f is blockIdx.y)
    const int s = (int)blockIdx.x * kAlignThreads + (int)threadIdx.x;
    double acc[kAlignSums];
    unsigned int cnt[4] = {0, 0, 0, 0};
#pragma unroll
    for (int k = 0; k < kAlignSums; ++k) acc[k] = 0.0;
    if (s < p.S) {
        const size_t o = f * (size_t)p.S + (size_t)s;
        const unsigned int v = p.frames[o];
        const double* Q = p.q + 4 * f;      // wave-uniform
        const double q[4] = {Q[0], Q[1], Q[2], Q[3]};
        double R[9];
        quat_to_matrix(q, R);
        const double* bv = p.lut + 3 * (size_t)s;
        const double b0 = bv[0], b1 = bv[1], b2 = bv[2];
        double rb[3], pm[2], J23[6];
#pragma unroll
        for (int r = 0; r < 3; ++r) rb[r] = sum3(R[3 * r] * b0, R[3 * r + 1] * b1, R[3 * r + 2] * b2);
        project_chain<false>(rb, p.fx, p.fy, p.cx, p.cy, pm, J23);
        if (p.pm) { p.pm[2 * o] = pm[0]; p.pm[2 * o + 1] = pm[1]; }
        AlignTerm t;
        const int cls = align_pixel(p.plane, p.valid, p.W, p.H, pm[0], pm[1], J23, v, p.lo, p.hi, p.skip_zero != 0, p.huber_k, &t);
        if (p.resid) p.resid[o] = t.r;
        if (cls == kAlignUsed) align_accumulate(t, acc);
#pragma unroll
        for (int k = 0; k < 4; ++k) cnt[k] = cls == k ? 1u : 0u;
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
#pragma unroll
        for (int k = 0; k < kAlignSums; ++k) acc[k] += __shfl_xor(acc[k], o);
#pragma unroll
        for (int k = 0; k < 4; ++k) cnt[k] += __shfl_xor(cnt[k], o);
    }
    const int wave = (int)threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int k = 0; k < kAlignSums; ++k) red[wave][k] = acc[k];
#pragma unroll
        for (int k = 0; k < 4; ++k) redc[wave][k] = cnt[k];
    }
    __syncthreads();
    double* out = p.partial + (f * (size_t)gridDim.x + (size_t)blockIdx.x) * (size_t)kAlignPartial;
    const int k = (int)threadIdx.x;
    if (k < kAlignSums) out[k] = ((red[0][k] + red[1][k]) + red[2][k]) + red[3][k];
    else if (k < kAlignSums + 4) reinterpret_cast<unsigned int*>(out + kAlignSums)[k - kAlignSums] = ((redc[0][k - kAlignSums] + redc[1][k - kAlignSums]) + redc[2][k - kAlignSums]) + redc[3][k - kAlignSums];
}
#pragma clang fp contract(fast)

// sums [nf, 10] and counts [nf, 4] of the frames' partial sums, added in workgroup order
__global__ __launch_bounds__(kAlignThreads) void emba_frames_align_reduce_kernel(const double* partial, int nb, long nf, const int32_t* status, double* sums,
                                                                                  unsigned long long* counts)
{
#pragma clang fp contract(off)
    const long i = (long)blockIdx.x * kAlignThreads + threadIdx.x;
    const long f = i / (kAlignSums + 4);
    const int k = (int)(i % (kAlignSums + 4));
    if (f >= nf || (status && status[f] != EMBA_ALIGN_RUNNING)) return;
    const double* P = partial + (size_t)f * (size_t)nb * (size_t)kAlignPartial;
    if (k < kAlignSums) {
        double a = 0.0;
        for (int b = 0; b < nb; ++b) a += P[(size_t)b * kAlignPartial + k];
        sums[(size_t)f * kAlignSums + k] = a;
    } else {
        unsigned long long a = 0;
        for (int b = 0; b < nb; ++b) a += reinterpret_cast<const unsigned int*>(P + (size_t)b * kAlignPartial + kAlignSums)[k - kAlignSums];
        counts[(size_t)f * 4 + (k - kAlignSums)] = a;
    }
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
