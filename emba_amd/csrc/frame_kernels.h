// emba_amd/csrc/frame_kernels.h — what the kernels over intensity frames share (gfx950, wave64): one lane per frame pixel, the frame in blockIdx.y,
// kFrameThreads lanes per workgroup.  DESIGN.md §23.
//   * frame_warp           a sensor pixel's bearing turned by the frame's rotation and projected: quat_to_matrix, the three sum3 products,
//                          project_chain<false>.  Used by emba_view_kernel (view_kernels.h), the vote kernels emba_mosaic_vote_kernel (mosaic_kernels.h),
//                          emba_mosaic_exposure_vote_kernel (exposure_kernels.h) and emba_frames_track_vote_kernel (track_kernels.h), where the Jacobian is dead
//                          code, and by the three evaluation kernels, where it is live
//   * frame_eval_body      the evaluation kernels emba_frames_align_eval_kernel, emba_frames_track_eval_kernel and emba_frames_exposure_eval_kernel but for
//                          their pixel rule: the status gate, the byte, the warp, the pixel's N terms and its class count summed over the wave by the xor
//                          butterfly (offsets 32 ... 1) and over the workgroup's four waves in LDS in wave order; the workgroup writes
//                          partial[frame][workgroup][N + 2], the four class counts as uint32 in the space of the last two doubles
//   * frame_reduce_body    one lane per (frame, sum): the frame's partial sums added in workgroup order.  No floating-point atomic anywhere: the same
//                          inputs give the same bits
//   * frame_vote_cells, frame_vote_counters   the tail of the vote kernels: per cell of pano_vote two return-less 64-bit integer atomic adds; a wave's
//                          dropped votes and skipped pixels in one atomic each
// The kernels keep their names, parameter structs and grids; each is a call of these bodies.
// The whole header is compiled without contraction, and every helper is defined here for that reason (the pragma is lexical): pm feeds floor(), and what the
// kernels give is compared with numpy bit for bit.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "align_rule.h"         // kAlignUsed, EMBA_ALIGN_RUNNING
#include "device_math.h"
#include "panorama_rule.h"      // PanoVotes

namespace emba {

constexpr int kFrameThreads = 256;
constexpr int kFrameWaves = kFrameThreads / 64;
// doubles per (frame, workgroup) of an evaluation of `sums` sums: the sums, then the four class counts as uint32 in the space of two
constexpr int frame_partial(int sums) { return sums + 2; }

#pragma clang fp contract(off)
// pm, and its Jacobian J23 with respect to the turned bearing, of sensor pixel s under the rotation q4 (xyzw; a wave-uniform address)
__device__ __forceinline__ void frame_warp(const double* lut, const double* q4, int s, double fx, double fy, double cx, double cy, double* pm, double* J23)
{
    const double q[4] = {q4[0], q4[1], q4[2], q4[3]};
    double R[9];
    quat_to_matrix(q, R);
    const double* bv = lut + 3 * (size_t)s;
    const double b0 = bv[0], b1 = bv[1], b2 = bv[2];
    double rb[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) rb[r] = sum3(R[3 * r] * b0, R[3 * r + 1] * b1, R[3 * r + 2] * b2);
    project_chain<false>(rb, fx, fy, cx, cy, pm, J23);
}

// The tail of an evaluation kernel's body, every lane of the workgroup in it: a lane's N sums and four class counts summed over the wave by the xor butterfly
// (offsets 32 ... 1) and over the workgroup's four waves in LDS in wave order; the record partial[item][workgroup][frame_partial(N)] is written, the counts as uint32 in the space
// of the last two doubles.  frame_eval_body and the pair kernel (pair_kernels.h) end in it.
template <int N>
__device__ __forceinline__ void frame_sum_tail(double* acc, unsigned int* cnt, double* partial, size_t item)
{
    __shared__ double red[kFrameWaves][N];
    __shared__ unsigned int redc[kFrameWaves][4];
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
#pragma unroll
        for (int k = 0; k < N; ++k) acc[k] += __shfl_xor(acc[k], o);
#pragma unroll
        for (int k = 0; k < 4; ++k) cnt[k] += __shfl_xor(cnt[k], o);
    }
    const int wave = (int)threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int k = 0; k < N; ++k) red[wave][k] = acc[k];
#pragma unroll
        for (int k = 0; k < 4; ++k) redc[wave][k] = cnt[k];
    }
    __syncthreads();
    double* out = partial + (item * (size_t)gridDim.x + (size_t)blockIdx.x) * (size_t)frame_partial(N);
    const int k = (int)threadIdx.x;
    if (k < N) out[k] = ((red[0][k] + red[1][k]) + red[2][k]) + red[3][k];
    else if (k < N + 4) {
        const int j = k - N;
        reinterpret_cast<unsigned int*>(out + N)[j] = ((redc[0][j] + redc[1][j]) + redc[2][j]) + redc[3][j];
    }
}

// An evaluation kernel's body.  Params has lut, q, status, frames, S, fx, fy, cx, cy, partial, pm, resid; Rule has
//   kSums                                the number of sums N
//   Term                                 a pixel's term, with its residual r
//   level(p, pm, J23)                    what happens to pm and J23 behind the warp (nothing, or the scale of a level)
//   pixel(p, f, pm, J23, v, &t) -> class the pixel rule
//   accumulate(t, acc)                   a used pixel's term into the N sums
template <class Rule, class Params>
__device__ __forceinline__ void frame_eval_body(const Params& p)
{
    constexpr int N = Rule::kSums;
    const size_t f = blockIdx.y;
    if (p.status && p.status[f] != EMBA_ALIGN_RUNNING) return;      // (the whole workgroup: f is blockIdx.y)
    const int s = (int)blockIdx.x * kFrameThreads + (int)threadIdx.x;
    double acc[N];
    unsigned int cnt[4] = {0, 0, 0, 0};
#pragma unroll
    for (int k = 0; k < N; ++k) acc[k] = 0.0;
    if (s < p.S) {
        const size_t o = f * (size_t)p.S + (size_t)s;
        const unsigned int v = p.frames[o];
        double pm[2], J23[6];
        frame_warp(p.lut, p.q + 4 * f, s, p.fx, p.fy, p.cx, p.cy, pm, J23);
        Rule::level(p, pm, J23);
        if (p.pm) { p.pm[2 * o] = pm[0]; p.pm[2 * o + 1] = pm[1]; }
        typename Rule::Term t;
        const int cls = Rule::pixel(p, f, pm, J23, v, &t);
        if (p.resid) p.resid[o] = t.r;
        if (cls == kAlignUsed) Rule::accumulate(t, acc);
#pragma unroll
        for (int k = 0; k < 4; ++k) cnt[k] = cls == k ? 1u : 0u;
    }
    frame_sum_tail<N>(acc, cnt, p.partial, f);
}

// sums [nf, N] and counts [nf, 4] of the frames' partial sums, added in workgroup order
template <int N>
__device__ __forceinline__ void frame_reduce_body(const double* partial, int nb, long nf, const int32_t* status, double* sums, unsigned long long* counts)
{
    const long i = (long)blockIdx.x * kFrameThreads + threadIdx.x;
    const long f = i / (N + 4);
    const int k = (int)(i % (N + 4));
    if (f >= nf || (status && status[f] != EMBA_ALIGN_RUNNING)) return;
    const double* P = partial + (size_t)f * (size_t)nb * (size_t)frame_partial(N);
    if (k < N) {
        double a = 0.0;
        for (int b = 0; b < nb; ++b) a += P[(size_t)b * frame_partial(N) + k];
        sums[(size_t)f * N + k] = a;
    } else {
        unsigned long long a = 0;
        for (int b = 0; b < nb; ++b) a += reinterpret_cast<const unsigned int*>(P + (size_t)b * frame_partial(N) + N)[k - N];
        counts[(size_t)f * 4 + (k - N)] = a;
    }
}

// a pixel's votes of the byte v into the two sums of a plane; a vote whose cell lies outside the plane is counted in `dropped`
__device__ __forceinline__ void frame_vote_cells(const PanoVotes& pv, unsigned int v, unsigned long long* sum_w, unsigned long long* sum_v, unsigned int& dropped)
{
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (!pv.w[k]) continue;
        if (pv.cell[k] < 0) { ++dropped; continue; }
        atomicAdd(sum_w + pv.cell[k], (unsigned long long)pv.w[k]);                          // (results unused: return-less adds)
        if (v) atomicAdd(sum_v + pv.cell[k], (unsigned long long)pv.w[k] * (unsigned long long)v);
    }
}

// a wave's dropped votes into counters[0] and its skipped pixels into counters[1]; every lane of the wave calls it
__device__ __forceinline__ void frame_vote_counters(unsigned int dropped, unsigned int skipped, unsigned long long* counters)
{
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) { dropped += __shfl_xor(dropped, o); skipped += __shfl_xor(skipped, o); }
    if ((threadIdx.x & 63) == 0) {
        if (dropped) atomicAdd(counters, (unsigned long long)dropped);
        if (skipped) atomicAdd(counters + 1, (unsigned long long)skipped);
    }
}
#pragma clang fp contract(fast)

}  // namespace emba
