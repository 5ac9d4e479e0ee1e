// emba_amd/csrc/cmax_kernels.h — contrast maximisation on the resident event sequence (gfx950, wave64): the angular velocity of every slice of events
// from the events alone (Gallego & Scaramuzza, RA-L 2017), no counterpart in the reference.  The rule: cmax_rule.h, include/emba_hip.h, DESIGN.md §11.
//   * emba_cmax_search_kernel      one workgroup per slice; the whole compass search of the slice runs inside the launch
//   * emba_cmax_objective_kernel   one workgroup per candidate omega of one event range: J, and the image of warped events where asked for (tests)
// Both evaluate J(omega) with cmax_eval: the image of warped events lives in LDS as uint32 and is filled with LDS integer atomics, sum I^2 is reduced in
// uint64 — integer arithmetic on top of a warp that uses + - x / only and is compiled without contraction, so J and every decision of the search are
// the same numbers in emba_amd.io.cmax_objective.  No global atomics, nothing between workgroups.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cmax_rule.h"

namespace emba {

constexpr int kCmaxThreads = 1024;                 // 16 waves sweep one slice.  LDS (64 KiB + the wave slots) would let two workgroups share a compute unit; at the search kernel's
                                                   // 80 VGPRs one is resident (two need 64) — immaterial below 256 slices, one workgroup per compute unit
constexpr int kCmaxWaves = kCmaxThreads / 64;

struct CmaxParams {
    const uint16_t* x; const uint16_t* y; const int64_t* t;   // the resident sequence
    const double* lut;                                        // bearing vector per sensor pixel [S, 3]
    int sw;                                                   // sensor width (p = y sw + x; every event was checked at its upload)
    int gw, gh, shift;                                        // the vote grid (cmax_rule.h: cmax_grid); gw gh <= kCmaxMaxCells
    double f, cu, cv;                                         // the pinhole of the image plane (cmax_pinhole_fit)
};

// The warp and the vote feed integers that emba_amd.io reproduces: no contraction (device_math.h has the convention).
#pragma clang fp contract(off)

// The votes of event k at omega w, warped to t_ref: a = w dt / 2, b' = (1 + a.a) b + 2 (a x b + a x (a x b)) — the unnormalised Cayley rotation of b by
// 2 atan(|w| dt / 2) about w —, u = f b'x / b'z + cu, v likewise, cell coordinate g = u / 2^shift, bilinear weights in sixteenths.
__device__ __forceinline__ void cmax_vote(const CmaxParams& P, long k, int64_t t_ref, double w0, double w1, double w2, uint32_t* iwe)
{
    const int64_t dti = P.t[k] - t_ref;
    const double dt = (double)dti * 1e-9;
    const double hdt = dt * 0.5;
    const double a0 = w0 * hdt, a1 = w1 * hdt, a2 = w2 * hdt;
    const size_t p = (size_t)P.y[k] * (size_t)P.sw + (size_t)P.x[k];
    const double b0 = P.lut[3 * p], b1 = P.lut[3 * p + 1], b2 = P.lut[3 * p + 2];
    const double aa = (a0 * a0 + a1 * a1) + a2 * a2;
    const double c0 = a1 * b2 - a2 * b1, c1 = a2 * b0 - a0 * b2, c2 = a0 * b1 - a1 * b0;      // a x b
    const double d0 = a1 * c2 - a2 * c1, d1 = a2 * c0 - a0 * c2, d2 = a0 * c1 - a1 * c0;      // a x (a x b)
    const double s = 1.0 + aa;
    const double r0 = s * b0 + 2.0 * (c0 + d0), r1 = s * b1 + 2.0 * (c1 + d1), r2 = s * b2 + 2.0 * (c2 + d2);
    if (!(r2 > 0.0)) return;                                                                   // behind the plane (or NaN): votes nowhere
    const double u = P.f * (r0 / r2) + P.cu, v = P.f * (r1 / r2) + P.cv;
    const double inv = 1.0 / (double)(1 << P.shift);                                            // exact
    const double gx = u * inv, gy = v * inv;
    if (!(gx >= -1.0 && gx < (double)P.gw && gy >= -1.0 && gy < (double)P.gh)) return;           // no cell of the four lies inside (or NaN)
    const double fx = floor(gx), fy = floor(gy);
    const int ix = (int)fx, iy = (int)fy;                                                       // in [-1, gw - 1], [-1, gh - 1]
    const uint32_t wx = (uint32_t)((gx - fx) * 16.0), wy = (uint32_t)((gy - fy) * 16.0);       // floor(frac 16) in [0, 15]
    const bool x0 = ix >= 0, x1 = ix + 1 < P.gw, y0 = iy >= 0, y1 = iy + 1 < P.gh;
    const int base = iy * P.gw + ix;
    const uint32_t v00 = (16u - wx) * (16u - wy), v10 = wx * (16u - wy), v01 = (16u - wx) * wy, v11 = wx * wy;
    if (x0 && y0) atomicAdd(iwe + base, v00);
    if (x1 && y0 && v10) atomicAdd(iwe + base + 1, v10);
    if (x0 && y1 && v01) atomicAdd(iwe + base + P.gw, v01);
    if (x1 && y1 && v11) atomicAdd(iwe + base + P.gw + 1, v11);
}

#pragma clang fp contract(fast)

// J(w) = sum over the cells of I^2 for the events [beg, end), every thread of the workgroup gets it.  iwe: kCmaxMaxCells words of LDS, wsum: one slot per
// wave.  Every thread of the workgroup calls this with the same arguments (three barriers inside); the image stays in iwe until the next call.
__device__ __forceinline__ unsigned long long cmax_eval(const CmaxParams& P, long beg, long end, int64_t t_ref, double w0, double w1, double w2, uint32_t* iwe,
                                                        unsigned long long* wsum)
{
    const int cells = P.gw * P.gh;
    for (int i = threadIdx.x; i < cells; i += kCmaxThreads) iwe[i] = 0u;
    __syncthreads();
    for (long k = beg + threadIdx.x; k < end; k += kCmaxThreads) cmax_vote(P, k, t_ref, w0, w1, w2, iwe);
    __syncthreads();
    unsigned long long acc = 0;
    for (int i = threadIdx.x; i < cells; i += kCmaxThreads) {
        const unsigned long long I = iwe[i];
        acc += I * I;
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) acc += __shfl_xor(acc, o);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = acc;
    __syncthreads();      // (also: nobody zeroes the image for the next evaluation before everybody has summed this one)
    unsigned long long J = 0;
#pragma unroll
    for (int w = 0; w < kCmaxWaves; ++w) J += wsum[w];      // the same slots in the same order in every thread: the same J
    return J;
}

// Slice s = blockIdx.x of m events: [s m, (s + 1) m), t_ref = t[s m].  The search state (cmax_rule.h: CmaxSearch) is a function of omega_max and of the J
// values alone, and every thread reads the same J from LDS behind a barrier: every thread takes every decision itself, all of them the same one — the
// trip count of the loop and of the barriers inside cmax_eval is uniform over the workgroup without a flag to hand around.
// Out, per slice: omega [3], t_ref, J(0), J(omega), evaluations.
__global__ __launch_bounds__(kCmaxThreads) void emba_cmax_search_kernel(CmaxParams P, long n_slices, long m, double omega_max, double* __restrict__ omega_out,
                                                                        int64_t* __restrict__ t_ref_out, unsigned long long* __restrict__ j0_out,
                                                                        unsigned long long* __restrict__ j_out, int32_t* __restrict__ evals_out)
{
    __shared__ uint32_t iwe[kCmaxMaxCells];
    __shared__ unsigned long long wsum[kCmaxWaves];
    const long s = blockIdx.x;
    if (s >= n_slices) return;                                // (uniform: the whole workgroup)
    const long beg = s * m, end = beg + m;
    const int64_t t_ref = P.t[beg];
    const bool one_instant = P.t[end - 1] == t_ref;           // (uniform) a slice of one instant has no motion to find: omega = 0 after J(0)
    CmaxSearch st(omega_max, 0);
    unsigned long long J0 = 0, Jbest = 0;
    int evals = 0, best = 0;
    // one call site of cmax_eval (the code stays small and in registers): c = -1 evaluates the centre, omega = 0, once; then c = 0 ... 5 per iteration
    for (int c = -1;;) {
        double w[3] = {st.w[0], st.w[1], st.w[2]};
        if (c >= 0) st.candidate(c, w);
        const unsigned long long J = cmax_eval(P, beg, end, t_ref, w[0], w[1], w[2], iwe, wsum);
        ++evals;
        if (c < 0) {
            J0 = J; st.J = J;
            if (one_instant || !st.running()) break;
            c = 0;
            continue;
        }
        if (c == 0 || J > Jbest) { best = c; Jbest = J; }   // ties: the earlier candidate
        if (++c == 6) {
            st.advance(best, Jbest);
            if (!st.running()) break;
            c = 0;
        }
    }
    if (threadIdx.x == 0) {
        omega_out[3 * s] = st.w[0]; omega_out[3 * s + 1] = st.w[1]; omega_out[3 * s + 2] = st.w[2];
        t_ref_out[s] = t_ref;
        j0_out[s] = J0; j_out[s] = st.J; evals_out[s] = evals;
    }
}

// Candidate j = blockIdx.x of M: J(omega[j]) over the events [beg, end), beg < end, t_ref = t[beg]; iwe_out (or nullptr): its image, cells words per candidate.
__global__ __launch_bounds__(kCmaxThreads) void emba_cmax_objective_kernel(CmaxParams P, long beg, long end, const double* __restrict__ omega, long M,
                                                                           unsigned long long* __restrict__ j_out, uint32_t* __restrict__ iwe_out)
{
    __shared__ uint32_t iwe[kCmaxMaxCells];
    __shared__ unsigned long long wsum[kCmaxWaves];
    const long j = blockIdx.x;
    if (j >= M) return;
    const unsigned long long J = cmax_eval(P, beg, end, P.t[beg], omega[3 * j], omega[3 * j + 1], omega[3 * j + 2], iwe, wsum);
    if (threadIdx.x == 0) j_out[j] = J;
    if (iwe_out) {
        const int cells = P.gw * P.gh;
        for (int i = threadIdx.x; i < cells; i += kCmaxThreads) iwe_out[(size_t)j * cells + i] = iwe[i];
    }
}

}  // namespace emba
