// emba_amd/csrc/panorama_kernels.h — the panorama of warped events along a trajectory (gfx950, wave64): every event of a range of the resident sequence
// warped through the linear SO(3) spline onto the equirectangular panorama, bilinear votes with exact integer weights, the image reduced to its contrast.
// The rule: panorama_rule.h, include/emba_hip.h (emba_seq_event_panorama), DESIGN.md §12.  Three stages on one stream:
//   * pose stage                    the batches' midpoints and rotations: emba_batch_mid_kernel (order_kernels.h) and emba_pose_kernel (kernels.h) as they
//                                   are, on the range's own batches and into the tables of seq_range_poses (panorama_host.h) — the registered window's are not touched
//   * emba_pano_vote_kernel         one lane per event: seq_event_warp (bearing, batch pose, pm by the evaluation path's own device_math.h functions),
//                                   pano_vote, seq_cast_votes (up to four return-less int32 atomic adds into the image in HBM)
//   * emba_pano_reduce_kernel,      J = sum I^2, sum I and the non-zero cells over the H W cells: per thread -> wave shuffle -> one slot per wave, then one
//     emba_pano_reduce_final_kernel wave adds the slots in a fixed order
// The atomics execute at the memory side (MI355X_MICROARCH.md, global atomics): an add leaves the XCD's L2 as an uncached 64-B request and nothing of the
// image stays there, so neither the block shape nor the placement of the workgroups changes what an add costs, and events in time order are neighbours on
// the panorama only as far as the scene makes them.  Plain 256-thread workgroups, one lane per event; measured, the kernel runs at the rate of those
// requests (23 adds per ns at 1 M events) — what an LDS-tiled form would have to beat by merging votes before they leave the chip.
// seq_event_warp, seq_cast_votes and seq_add_dropped below are also what every pass of contrast_kernels.h is made of.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "device_math.h"
#include "kernels.h"      // kPoseStride, emba_pose_kernel
#include "panorama_rule.h"

namespace emba {

constexpr int kPanoThreads = 256;
constexpr int kPanoReduceBlocks = 256;                                   // at the most: one round over the compute units
constexpr int kPanoReduceSlots = kPanoReduceBlocks * (kPanoThreads / 64);   // one per wave
constexpr int kPanoSums = 3;                                             // per slot: J, sum (two's complement), non-zero cells

// What every stage over a range of the resident sequence reads of an event and where it reports: embedded by PanoParams and by ContrastParams
// (contrast_kernels.h).
struct SeqEventParams {
    const uint16_t* x; const uint16_t* y; const uint8_t* pol;   // the resident sequence, from the range's first event
    const double* lut;                                          // bearing vector per sensor pixel [S, 3]
    const double* pose;                                         // pose table of the range's batches (kPoseStride doubles each: q[4] J1[9] cp)
    long nn;                                                    // events used: whole batches
    int sw;
    double fx, fy, cx, cy;                                      // the equirectangular camera of the context
    int signed_polarity;
    unsigned long long* dropped;                                // votes whose row lies outside the grid (zeroed on the stream in front of the vote launch)
    double* pm_out;                                             // [nn, 2] or nullptr (vote pass)
};

struct PanoParams {
    SeqEventParams ev;
    int W, H;
    int32_t* image;                                             // [H, W], zeroed on the stream in front of this launch
};

// Compiled without contraction, like everything that feeds an integer (device_math.h): the panorama and every contrast pass must land in the same cells.
#pragma clang fp contract(off)

// Event k of the range: pm = project(R(batch k / 100) * bearing) and J23 = dpm / d(rotation increment) — quat_to_matrix, the three products and two sums
// of the warp kernels (kernels.h) and project_chain.  The one place where an event of the range becomes pm; returns the batch's pose record.
__device__ __forceinline__ const double* seq_event_warp(const SeqEventParams& e, long k, double* pm, double* J23)
{
    const double* P = e.pose + (size_t)kPoseStride * (size_t)(k / (long)kPanoBatch);
    const double q[4] = {P[0], P[1], P[2], P[3]};
    double R[9];
    quat_to_matrix(q, R);
    const double* bv = e.lut + 3 * ((size_t)e.y[k] * (size_t)e.sw + (size_t)e.x[k]);      // (every event was checked at its upload: inside the LUT)
    const double b0 = bv[0], b1 = bv[1], b2 = bv[2];
    double rb[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) rb[r] = sum3(R[3 * r] * b0, R[3 * r + 1] * b1, R[3 * r + 2] * b2);
    project_chain<false>(rb, e.fx, e.fy, e.cx, e.cy, pm, J23);
    return P;
}

// The vote pass's use of it: pm alone (the Jacobian is dead code), stored where asked for.
__device__ __forceinline__ void seq_event_pm(const SeqEventParams& e, long k, double* pm)
{
    double J23[6];
    seq_event_warp(e, k, pm, J23);
    if (e.pm_out) { e.pm_out[2 * k] = pm[0]; e.pm_out[2 * k + 1] = pm[1]; }
}

// The votes v of event k (PanoVotes, ContrastVotes) added to `image` with the event's sign: up to four adds whose result is not used, so return-less atomics
// of the address space the call site shows after inlining — global_atomic_add for int32 in HBM, global_atomic_add_f64 for fp64 in HBM, ds_add_f64 for
// fp64 in LDS.  A vote of zero weight is skipped; one whose row lies outside the grid is dropped and counted: the return value.
template <typename Votes, typename Cell>
__device__ __forceinline__ unsigned int seq_cast_votes(const SeqEventParams& e, long k, const Votes& v, Cell* image)
{
    const bool neg = e.signed_polarity && e.pol[k] == 0;
    unsigned int lost = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        if (v.w[i] == 0) continue;
        if (v.cell[i] < 0) { ++lost; continue; }
        atomicAdd(image + v.cell[i], neg ? -v.w[i] : v.w[i]);
    }
    return lost;
}

// The dropped votes of the wave in one add.  Every lane of the wave arrives here.
__device__ __forceinline__ void seq_add_dropped(const SeqEventParams& e, unsigned int lost)
{
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) lost += __shfl_xor(lost, o);
    if ((threadIdx.x & 63) == 0 && lost) atomicAdd(e.dropped, (unsigned long long)lost);
}

// One lane per event: seq_event_pm, pano_vote, the integer votes into the image in HBM.
__global__ __launch_bounds__(kPanoThreads) void emba_pano_vote_kernel(PanoParams p)
{
    const long k = (long)blockIdx.x * kPanoThreads + threadIdx.x;
    unsigned int lost = 0;
    if (k < p.ev.nn) {
        double pm[2];
        seq_event_pm(p.ev, k, pm);
        lost = seq_cast_votes(p.ev, k, pano_vote(pm[0], pm[1], p.W, p.H), p.image);
    }
    seq_add_dropped(p.ev, lost);
}
#pragma clang fp contract(fast)

// Slot (blockIdx.x, wave) <- {sum I^2, sum I, cells != 0} over the cells the wave's lanes stride over.  Integers: every order gives the same sums; the order
// is fixed all the same (a grid-stride sweep, the butterfly, then the final kernel's), like the reduction of cmax_kernels.h.
__global__ __launch_bounds__(kPanoThreads) void emba_pano_reduce_kernel(const int32_t* __restrict__ image, long cells, unsigned long long* __restrict__ slots)
{
    unsigned long long j = 0, s = 0, nz = 0;
    for (long i = (long)blockIdx.x * kPanoThreads + threadIdx.x; i < cells; i += (long)gridDim.x * kPanoThreads) {
        const long long I = image[i];
        j += (unsigned long long)(I * I);
        s += (unsigned long long)I;
        nz += I != 0;
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) { j += __shfl_xor(j, o); s += __shfl_xor(s, o); nz += __shfl_xor(nz, o); }
    if ((threadIdx.x & 63) == 0) {
        unsigned long long* o = slots + (size_t)kPanoSums * ((size_t)blockIdx.x * (kPanoThreads / 64) + (threadIdx.x >> 6));
        o[0] = j; o[1] = s; o[2] = nz;
    }
}

// One wave: lane l adds the slots l, l + 64, ... in that order, the butterfly adds the lanes.  out[0..2] = J, sum, non-zero cells.
__global__ __launch_bounds__(64) void emba_pano_reduce_final_kernel(const unsigned long long* __restrict__ slots, int n_slots, unsigned long long* __restrict__ out)
{
    unsigned long long j = 0, s = 0, nz = 0;
    for (int i = threadIdx.x; i < n_slots; i += 64) { j += slots[kPanoSums * i]; s += slots[kPanoSums * i + 1]; nz += slots[kPanoSums * i + 2]; }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) { j += __shfl_xor(j, o); s += __shfl_xor(s, o); nz += __shfl_xor(nz, o); }
    if (threadIdx.x == 0) { out[0] = j; out[1] = s; out[2] = nz; }
}

}  // namespace emba
