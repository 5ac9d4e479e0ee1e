// emba_amd/csrc/exposure_kernels.h — per-frame exposure (gfx950, wave64): per frame the normal equations of the 5-parameter photometric alignment (rotation,
// gain, bias), the Levenberg-Marquardt step on them, and the vote of compensated bytes into the mosaic.
// The rules: exposure_rule.h, align_rule.h, include/emba_hip.h (emba_frames_exposure_eval, emba_frames_exposure_align, emba_mosaic_frames_exposure),
// DESIGN.md §22.
//   * emba_frames_exposure_eval_kernel    emba_frames_align_eval_kernel's shape: one lane per frame pixel, the frame in blockIdx.y: the byte (coalesced), the
//                                         warp of emba_view_kernel with its Jacobian live, exposure_pixel, and the pixel's 21 terms and its class count summed
//                                         over the wave by the xor butterfly and over the workgroup's four waves in LDS, in wave order; the workgroup
//                                         writes its partial sums to partial[frame][workgroup][23].  The butterfly is one pass over the 21 terms
//   * emba_frames_exposure_reduce_kernel  one lane per (frame, sum): the frame's partial sums added in workgroup order.  No floating-point atomic anywhere:
//                                         the same inputs give the same bits
//   * emba_frames_exposure_step_kernel    one lane per frame: exposure_step — decide on the evaluated trial, propose the next; q, a, b, lambda and the
//                                         status stay on the device between iterations
//   * emba_mosaic_exposure_vote_kernel    emba_mosaic_vote_kernel with exposure_byte(v, a_f, b_f) in the place of v: the same warp, pano_vote and the two
//                                         return-less 64-bit integer atomics; skip_zero tests the raw byte
// A frame whose status is final leaves the first three at once; in the evaluation kernel that is uniform over the workgroup (the frame is blockIdx.y).
// 736 B of LDS in the evaluation kernel, no scratch.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "device_math.h"
#include "exposure_rule.h"
#include "kernels.h"      // kPoseStride
#include "panorama_rule.h"

namespace emba {

constexpr int kExposureThreads = 256;
constexpr int kExposureWaves = kExposureThreads / 64;
constexpr int kExposurePartial = kExposureSums + 2;      // doubles per (frame, workgroup): the 21 sums, then the four class counts as uint32 in the space of two

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
    double* partial;              // [nf, gridDim.x, kExposurePartial]
    double* pm;                   // [nf, S, 2] or nullptr
    double* resid;                // [nf, S] or nullptr
};

// Compiled without contraction: pm feeds floor(), and r is compared by its bits.
#pragma clang fp contract(off)
__global__ __launch_bounds__(kExposureThreads) void emba_frames_exposure_eval_kernel(ExposureEvalParams p)
{
    __shared__ double red[kExposureWaves][kExposureSums];
    __shared__ unsigned int redc[kExposureWaves][4];
    const size_t f = blockIdx.y;
    if (p.status && p.status[f] != EMBA_ALIGN_RUNNING) return;      // (the whole workgroup: f is blockIdx.y)
    const int s = (int)blockIdx.x * kExposureThreads + (int)threadIdx.x;
    double acc[kExposureSums];
    unsigned int cnt[4] = {0, 0, 0, 0};
#pragma unroll
    for (int k = 0; k < kExposureSums; ++k) acc[k] = 0.0;
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
        ExposureTerm t;
        const int cls = exposure_pixel(p.plane, p.valid, p.W, p.H, pm[0], pm[1], J23, v, p.lo, p.hi, p.gain[f], p.bias[f], p.skip_zero != 0, p.huber_k, &t);
        if (p.resid) p.resid[o] = t.r;
        if (cls == kAlignUsed) exposure_accumulate(t, acc);
#pragma unroll
        for (int k = 0; k < 4; ++k) cnt[k] = cls == k ? 1u : 0u;
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
#pragma unroll
        for (int k = 0; k < kExposureSums; ++k) acc[k] += __shfl_xor(acc[k], o);
#pragma unroll
        for (int k = 0; k < 4; ++k) cnt[k] += __shfl_xor(cnt[k], o);
    }
    const int wave = (int)threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int k = 0; k < kExposureSums; ++k) red[wave][k] = acc[k];
#pragma unroll
        for (int k = 0; k < 4; ++k) redc[wave][k] = cnt[k];
    }
    __syncthreads();
    double* out = p.partial + (f * (size_t)gridDim.x + (size_t)blockIdx.x) * (size_t)kExposurePartial;
    const int k = (int)threadIdx.x;
    if (k < kExposureSums) out[k] = ((red[0][k] + red[1][k]) + red[2][k]) + red[3][k];
    else if (k < kExposureSums + 4) {
        const int j = k - kExposureSums;
        reinterpret_cast<unsigned int*>(out + kExposureSums)[j] = ((redc[0][j] + redc[1][j]) + redc[2][j]) + redc[3][j];
    }
}
#pragma clang fp contract(fast)

// sums [nf, 21] and counts [nf, 4] of the frames' partial sums, added in workgroup order
__global__ __launch_bounds__(kExposureThreads) void emba_frames_exposure_reduce_kernel(const double* partial, int nb, long nf, const int32_t* status, double* sums,
                                                                                        unsigned long long* counts)
{
#pragma clang fp contract(off)
    const long i = (long)blockIdx.x * kExposureThreads + threadIdx.x;
    const long f = i / (kExposureSums + 4);
    const int k = (int)(i % (kExposureSums + 4));
    if (f >= nf || (status && status[f] != EMBA_ALIGN_RUNNING)) return;
    const double* P = partial + (size_t)f * (size_t)nb * (size_t)kExposurePartial;
    if (k < kExposureSums) {
        double a = 0.0;
        for (int b = 0; b < nb; ++b) a += P[(size_t)b * kExposurePartial + k];
        sums[(size_t)f * kExposureSums + k] = a;
    } else {
        unsigned long long a = 0;
        for (int b = 0; b < nb; ++b) a += reinterpret_cast<const unsigned int*>(P + (size_t)b * kExposurePartial + kExposureSums)[k - kExposureSums];
        counts[(size_t)f * 4 + (k - kExposureSums)] = a;
    }
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
__global__ __launch_bounds__(kExposureThreads) void emba_mosaic_exposure_vote_kernel(ExposureVoteParams p)
{
    const int s = (int)blockIdx.x * kExposureThreads + (int)threadIdx.x;
    const size_t f = blockIdx.y;
    unsigned int dropped = 0, skipped = 0;
    if (s < p.S) {
        const size_t o = f * (size_t)p.S + (size_t)s;
        const unsigned int raw = p.frames[o];
        const double* P = p.pose + (size_t)kPoseStride * f;      // wave-uniform
        const double q[4] = {P[0], P[1], P[2], P[3]};
        double R[9];
        quat_to_matrix(q, R);
        const double* bv = p.lut + 3 * (size_t)s;
        const double b0 = bv[0], b1 = bv[1], b2 = bv[2];
        double rb[3], pm[2], J23[6];
#pragma unroll
        for (int r = 0; r < 3; ++r) rb[r] = sum3(R[3 * r] * b0, R[3 * r + 1] * b1, R[3 * r + 2] * b2);
        project_chain<false>(rb, p.fx, p.fy, p.cx, p.cy, pm, J23);
        if (p.pm) { p.pm[2 * o] = pm[0]; p.pm[2 * o + 1] = pm[1]; }
        if (p.skip_zero && raw == 0) skipped = 1;
        else {
            const unsigned int v = exposure_byte(raw, p.gain[f], p.bias[f]);
            const PanoVotes pv = pano_vote(pm[0], pm[1], p.W, p.H);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (!pv.w[k]) continue;
                if (pv.cell[k] < 0) { ++dropped; continue; }
                atomicAdd(p.sum_w + pv.cell[k], (unsigned long long)pv.w[k]);                          // (results unused: return-less adds)
                if (v) atomicAdd(p.sum_v + pv.cell[k], (unsigned long long)pv.w[k] * (unsigned long long)v);
            }
        }
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) { dropped += __shfl_xor(dropped, o); skipped += __shfl_xor(skipped, o); }
    if ((threadIdx.x & 63) == 0) {
        if (dropped) atomicAdd(p.counters, (unsigned long long)dropped);
        if (skipped) atomicAdd(p.counters + 1, (unsigned long long)skipped);
    }
}
#pragma clang fp contract(fast)

}  // namespace emba
