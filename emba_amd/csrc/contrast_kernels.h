// emba_amd/csrc/contrast_kernels.h — the smooth contrast of the panorama of warped events and its gradient with respect to the control poses (gfx950,
// wave64).  The rule: contrast_rule.h, include/emba_hip.h (emba_seq_contrast_gradient), DESIGN.md §13.  Stages on one stream:
//   * pose stage                       seq_range_poses (panorama_host.h): the pose record of every batch of the range holds q, J1 and cp
//   * emba_contrast_vote_kernel        one lane per event: seq_event_warp and seq_cast_votes (panorama_kernels.h) — up to four return-less fp64 atomic adds
//                                      into the double image in HBM
//   * emba_contrast_vote_lds_kernel    the same where the image fits LDS (contrast_vote_plan): a fixed grid of persistent workgroups, each summing a
//                                      contiguous share of the events into an image in LDS (ds_add_f64) and then adding its non-zero cells to the image in HBM
//   * emba_contrast_grad_kernel        one lane per event: seq_event_warp again (the same cells), the four I gathered, ge = 2 s gp^T D; summed per
//                                      workgroup in an LDS table over the control poses the workgroup spans, then one global fp64 add per touched component
//   * emba_contrast_reduce_kernel,     J = sum I^2 in fp64 in a fixed order: per thread -> wave shuffle -> one slot per wave, then one wave adds the slots
//     emba_contrast_reduce_final_kernel
//   * emba_contrast_prior_vote_kernel  the prior: one lane per event, ONE seq_event_warp, then the votes of every level of the call into that
//                                      level's prior image in HBM (emba_seq_contrast_prior_add; its own launch, once per window)
//   * emba_contrast_prior_init_kernel  image <- prior_weight P_l in the place of the zeroing, in front of either vote kernel (emba_seq_contrast_gradient_prior)
// Levels (contrast_rule.h): every kernel exists once; it votes at pm 2^-l on the level's grid and multiplies D by 2^-l.  At level 0, and
// for the level-free entry point, both are products with 1.0: exact.
// The fp64 adds into the image and into g arrive in no fixed order: both depend on it in their last bits (compared by tolerance, never by bits).  Given the
// image, J is deterministic.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "contrast_rule.h"
#include "device_math.h"
#include "panorama_kernels.h"      // SeqEventParams, seq_event_warp, seq_cast_votes, seq_add_dropped

namespace emba {

constexpr int kContrastThreads = 256;
constexpr int kContrastReduceBlocks = 256;                                          // at the most: one round over the compute units
constexpr int kContrastReduceSlots = kContrastReduceBlocks * (kContrastThreads / 64);   // one per wave

struct ContrastParams {
    SeqEventParams ev;                                          // (panorama_kernels.h)
    int W, H, K;                                                // (W, H: the grid voted on — the level's W_l, H_l)
    double scale;                                               // 2^-level
    double* image;                                              // [H, W], zeroed on the stream in front of the vote launch
    double* grad;                                               // [3 K], zeroed likewise (gradient pass)
    double* d_out;                                              // [nn, 2, 6] or nullptr (gradient pass)
    int32_t* cp_out;                                            // [nn] or nullptr (gradient pass)
};

// Everything below is compiled without contraction: the two passes must land in the same cells, and the rule header's functions are the CPU test's.
#pragma clang fp contract(off)

// The votes of an event projected to pm: at pm 2^-level on the level's grid (pm itself stays unscaled).  The one formulation every pass calls.
__device__ __forceinline__ ContrastVotes contrast_votes_at(const ContrastParams& p, const double* pm)
{
    return contrast_vote_level(pm[0], pm[1], ContrastLevel{p.W, p.H, p.scale});
}

__global__ __launch_bounds__(kContrastThreads) void emba_contrast_vote_kernel(ContrastParams p)
{
    const long k = (long)blockIdx.x * kContrastThreads + threadIdx.x;
    unsigned int lost = 0;
    if (k < p.ev.nn) {
        double pm[2];
        seq_event_pm(p.ev, k, pm);
        lost = seq_cast_votes(p.ev, k, contrast_votes_at(p, pm), p.image);
    }
    seq_add_dropped(p.ev, lost);
}

// The votes of a level whose image fits LDS (contrast_vote_plan).  gridDim.x persistent workgroups (contrast_lds_grid: a function of the chip, not of
// nn); workgroup b zeroes the W x H cells of its LDS image, votes its share of the events (contrast_share: contiguous, so in time order a compact part of
// the panorama) into it with LDS atomics, and after the barrier adds its cells that are not zero to the image in HBM, return-less.  A workgroup with an
// empty share returns at once and adds nothing.  p.W * p.H <= kContrastLdsCells is the host's plan; contrast_vote keeps every cell index inside W x H.
__global__ __launch_bounds__(kContrastLdsThreads) void emba_contrast_vote_lds_kernel(ContrastParams p)
{
    __shared__ double img[kContrastLdsCells];
    const int cells = p.W * p.H;
    const ContrastShare sh = contrast_share(p.ev.nn, (int)gridDim.x, (int)blockIdx.x);
    if (sh.end <= sh.beg) return;      // (uniform over the workgroup: in front of every barrier)
    for (int i = threadIdx.x; i < cells; i += kContrastLdsThreads) img[i] = 0.0;
    __syncthreads();
    unsigned int lost = 0;
    for (long k = sh.beg + threadIdx.x; k < sh.end; k += kContrastLdsThreads) {
        double pm[2];
        seq_event_pm(p.ev, k, pm);
        lost += seq_cast_votes(p.ev, k, contrast_votes_at(p, pm), img);
    }
    seq_add_dropped(p.ev, lost);      // (the lanes have left the loop)
    __syncthreads();
    for (int i = threadIdx.x; i < cells; i += kContrastLdsThreads) {
        const double v = img[i];
        if (v != 0.0) atomicAdd(p.image + i, v);
    }
}

// ---- the prior (contrast_rule.h)
// The levels one emba_seq_contrast_prior_add votes at, by value: entry j is the j-th set level of the mask — its grid, its prior image P_l [H_l, W_l] in HBM
// and dropped[j], the votes of that level whose row lies outside the grid (zeroed on the stream in front of the launch).  ev.dropped and ev.pm_out are not used.
struct ContrastPriorParams {
    SeqEventParams ev;
    int n;                                                      // levels in use: 1 ... kContrastLevels
    ContrastLevel lv[kContrastLevels];
    double* image[kContrastLevels];
    unsigned long long* dropped;                                // [n]
};

// P_l += the level-l votes of every event, for every level of the call: one lane per event, seq_event_warp ONCE per event (the spline pose, the LUT and the
// projection are the expensive part), then per level the scaled vote (contrast_vote_level: what contrast_votes_at is) and seq_cast_votes into that level's
// image — return-less fp64 atomics in HBM like emba_contrast_vote_kernel's.  The level loop is uniform: every lane of the wave takes part in every level's
// count of dropped votes, one add per wave per level.
__global__ __launch_bounds__(kContrastThreads) void emba_contrast_prior_vote_kernel(ContrastPriorParams p)
{
    const long k = (long)blockIdx.x * kContrastThreads + threadIdx.x;
    const bool on = k < p.ev.nn;
    double pm[2] = {0.0, 0.0}, J23[6];
    if (on) seq_event_warp(p.ev, k, pm, J23);      // (the Jacobian is dead code)
    for (int j = 0; j < p.n; ++j) {
        unsigned int lost = 0;
        if (on) lost = seq_cast_votes(p.ev, k, contrast_vote_level(pm[0], pm[1], p.lv[j]), p.image[j]);
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) lost += __shfl_xor(lost, o);
        if ((threadIdx.x & 63) == 0 && lost) atomicAdd(p.dropped + j, (unsigned long long)lost);
    }
}

// image[c] = prior_weight * P_l[c]: what stands in the image in front of the votes of emba_seq_contrast_gradient_prior, in the place of the zeroing.
// Grid-stride, two cells (16 bytes) per lane and round; an odd last cell by one lane.  Both arrays are the heads of device allocations: 16-byte aligned.
__global__ __launch_bounds__(kContrastThreads) void emba_contrast_prior_init_kernel(const double* __restrict__ prior, double prior_weight, long cells,
                                                                                    double* __restrict__ image)
{
    const long pairs = cells >> 1;
    const double2* __restrict__ src = reinterpret_cast<const double2*>(prior);
    double2* __restrict__ dst = reinterpret_cast<double2*>(image);
    for (long i = (long)blockIdx.x * kContrastThreads + threadIdx.x; i < pairs; i += (long)gridDim.x * kContrastThreads) {
        double2 v = src[i];
        v.x = contrast_prior_cell(prior_weight, v.x);
        v.y = contrast_prior_cell(prior_weight, v.y);
        dst[i] = v;
    }
    if ((cells & 1) && blockIdx.x == 0 && threadIdx.x == 0) image[cells - 1] = contrast_prior_cell(prior_weight, prior[cells - 1]);
}

// g += the gradients of the workgroup's events.  Events are in time order, so the control-pose indices of a workgroup's 256 events are a short run
// [cp_first, cp_last]; the workgroup sums into an LDS table over [cp_first, cp_last + 1] (contrast_span), a wave whose lanes all have one cp by a shuffle
// reduction and one lane's six LDS adds, a wave across a knot boundary by LDS atomics per lane, and then adds each touched component to g once.  A span
// longer than the table (kContrastTableCps control poses): the lanes add to g in HBM directly.  A lane whose pose record holds no control-pose index in
// [0, K - 2] — a batch outside the knots leaves its record unwritten, and sets the call's status word — adds nothing anywhere.
__global__ __launch_bounds__(kContrastThreads) void emba_contrast_grad_kernel(ContrastParams p)
{
    __shared__ double tab[3 * kContrastTableCps];
    __shared__ int w_lo[kContrastThreads / 64], w_hi[kContrastThreads / 64];
    const long k = (long)blockIdx.x * kContrastThreads + threadIdx.x;
    const int wave = threadIdx.x >> 6;
    bool live = false;
    int cp = 0;
    double ge[6] = {0, 0, 0, 0, 0, 0};
    if (k < p.ev.nn) {
        double pm[2], J23[6];
        const double* P = seq_event_warp(p.ev, k, pm, J23);
        const ContrastVotes v = contrast_votes_at(p, pm);
        const double cpd = P[13];
        live = cpd >= 0.0 && cpd <= (double)(p.K - 2);      // (false for NaN)
        // dpm_ddrot_cp = J23 * [I - J1 | J1]   (the warp kernels' D, kernels.h)
        double D[12];
#pragma unroll
        for (int r = 0; r < 2; ++r)
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                double s0 = 0, s1 = 0;
#pragma unroll
                for (int j = 0; j < 3; ++j) {
                    const double j1 = P[4 + 3 * j + c];
                    const double j0 = ((j == c) ? 1.0 : 0.0) - j1;
                    s0 += J23[3 * r + j] * j0;
                    s1 += J23[3 * r + j] * j1;
                }
                D[6 * r + c] = s0;
                D[6 * r + c + 3] = s1;
            }
        if (p.d_out) {
#pragma unroll
            for (int j = 0; j < 12; ++j) p.d_out[12 * k + j] = D[j];
        }
        if (p.cp_out) p.cp_out[k] = live ? (int32_t)cpd : -1;
#pragma unroll
        for (int j = 0; j < 12; ++j) D[j] *= p.scale;      // D_l = D 2^-level (d_out above stays the unscaled D)
        if (live) {
            cp = (int)cpd;
            double I4[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) I4[i] = v.cell[i] >= 0 ? p.image[v.cell[i]] : 0.0;
            contrast_event_grad(v, I4, D, (p.ev.signed_polarity && p.ev.pol[k] == 0) ? -1.0 : 1.0, ge);
        }
    }
    // the wave's and the workgroup's run of control poses (every lane arrives here)
    int lo = live ? cp : 0x7FFFFFFF, hi = live ? cp : -1;
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) { lo = min(lo, __shfl_xor(lo, o)); hi = max(hi, __shfl_xor(hi, o)); }
    if ((threadIdx.x & 63) == 0) { w_lo[wave] = lo; w_hi[wave] = hi; }
    for (int i = threadIdx.x; i < 3 * kContrastTableCps; i += kContrastThreads) tab[i] = 0.0;
    __syncthreads();
    int b_lo = w_lo[0], b_hi = w_hi[0];
#pragma unroll
    for (int i = 1; i < kContrastThreads / 64; ++i) { b_lo = min(b_lo, w_lo[i]); b_hi = max(b_hi, w_hi[i]); }
    const ContrastSpan span = contrast_span(b_lo, b_hi);
    if (b_hi < b_lo) return;      // no event of the workgroup has a pose (uniform: after the only barrier every lane takes part in)
    if (!span.fits) {             // the fallback: every lane adds its six components to g
        if (live) {
#pragma unroll
            for (int j = 0; j < 6; ++j)
                if (ge[j] != 0.0) atomicAdd(p.grad + 3 * (size_t)cp + j, ge[j]);
        }
        return;
    }
    if (hi >= lo) {               // the wave has live lanes
        if (lo == hi) {           // all at one control pose: the butterfly, then lane 0's six LDS adds
#pragma unroll
            for (int j = 0; j < 6; ++j)
#pragma unroll
                for (int o = 32; o >= 1; o >>= 1) ge[j] += __shfl_xor(ge[j], o);
            if ((threadIdx.x & 63) == 0) {
#pragma unroll
                for (int j = 0; j < 6; ++j) atomicAdd(&tab[3 * (lo - span.first) + j], ge[j]);
            }
        } else if (live) {        // a knot boundary inside the wave
#pragma unroll
            for (int j = 0; j < 6; ++j) atomicAdd(&tab[3 * (cp - span.first) + j], ge[j]);
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < span.comps; i += kContrastThreads) {
        const double v = tab[i];
        if (v != 0.0) atomicAdd(p.grad + 3 * (size_t)span.first + i, v);
    }
}

// Slot (blockIdx.x, wave) <- sum I^2 over the cells the wave's lanes stride over: a grid-stride sweep, the butterfly, then the final kernel's order.
__global__ __launch_bounds__(kContrastThreads) void emba_contrast_reduce_kernel(const double* __restrict__ image, long cells, double* __restrict__ slots)
{
    double j = 0.0;
    for (long i = (long)blockIdx.x * kContrastThreads + threadIdx.x; i < cells; i += (long)gridDim.x * kContrastThreads) {
        const double I = image[i];
        j += I * I;
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) j += __shfl_xor(j, o);
    if ((threadIdx.x & 63) == 0) slots[(size_t)blockIdx.x * (kContrastThreads / 64) + (threadIdx.x >> 6)] = j;
}

// One wave: lane l adds the slots l, l + 64, ... in that order, the butterfly adds the lanes.
__global__ __launch_bounds__(64) void emba_contrast_reduce_final_kernel(const double* __restrict__ slots, int n_slots, double* __restrict__ out)
{
    double j = 0.0;
    for (int i = threadIdx.x; i < n_slots; i += 64) j += slots[i];
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) j += __shfl_xor(j, o);
    if (threadIdx.x == 0) out[0] = j;
}
#pragma clang fp contract(fast)

}  // namespace emba
