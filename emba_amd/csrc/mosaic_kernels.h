// emba_amd/csrc/mosaic_kernels.h — the mosaic of intensity frames on the panorama (gfx950, wave64): frames -> panorama, the way back from
// emba_view_kernel, and the gradient map made from the mosaic.
// The rules: mosaic_rule.h, panorama_rule.h (pano_vote), include/emba_hip.h (emba_mosaic_frames, emba_mosaic_get, emba_mosaic_map), DESIGN.md §19.
//   * pose stage                 the rotations at the F frame times: emba_pose_kernel (kernels.h) as it is, into the pose table of mosaic_host.h
//   * emba_mosaic_vote_kernel    one lane per frame pixel, the frame in blockIdx.y: the byte (coalesced), frame_warp (frame_kernels.h), pano_vote's
//                                four cells, and per cell two return-less 64-bit integer atomic adds into sum_w and sum_v in HBM (frame_vote_cells); a
//                                wave's dropped votes and skipped pixels go up in one atomic each (frame_vote_counters)
//   * emba_mosaic_mean_kernel    one lane per cell: mosaic_mean, the covered byte, a wave's count of covered cells in one atomic
//   * emba_mosaic_log_kernel     one lane per cell: mosaic_log of the mean, the byte of the cells that stay covered
//   * emba_mosaic_map_kernel     one lane per cell: mosaic_gradient of the L and the bytes the log kernel wrote (a second pass: the neighbours' L are read,
//                                never recomputed, so Gx, Gy are the differences of the very L a caller downloads)
// No LDS, no scratch.  Integer sums do not depend on the order of the adds: whatever order the atomics land in, numpy gives the same integers.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "frame_kernels.h"
#include "kernels.h"      // kPoseStride, emba_pose_kernel
#include "mosaic_rule.h"

namespace emba {

constexpr int kMosaicThreads = kFrameThreads;      // the vote kernel's, and the per-cell kernels' below

struct MosaicVoteParams {
    const double* lut;            // bearing vector per sensor pixel [S, 3]
    const double* pose;           // pose records of the chunk's frames (kPoseStride doubles each)
    const uint8_t* frames;        // the chunk's bytes [nf, S]
    int S, W, H;
    double fx, fy, cx, cy;        // the equirectangular camera of the context
    int skip_zero;                // a byte of 0 casts no vote and is counted
    unsigned long long* sum_w;    // [H, W]
    unsigned long long* sum_v;    // [H, W]
    double* pm;                   // [nf, S, 2] or nullptr
    unsigned long long* counters; // [0] dropped votes, [1] skipped pixels (zeroed on the stream in front of the first launch)
};

// Compiled without contraction: pm feeds floor().
#pragma clang fp contract(off)
__global__ __launch_bounds__(kMosaicThreads) void emba_mosaic_vote_kernel(MosaicVoteParams p)
{
    const int s = (int)blockIdx.x * kMosaicThreads + (int)threadIdx.x;
    const size_t f = blockIdx.y;
    unsigned int dropped = 0, skipped = 0;
    if (s < p.S) {
        const size_t o = f * (size_t)p.S + (size_t)s;
        const unsigned int v = p.frames[o];
        double pm[2], J23[6];
        frame_warp(p.lut, p.pose + (size_t)kPoseStride * f, s, p.fx, p.fy, p.cx, p.cy, pm, J23);
        if (p.pm) { p.pm[2 * o] = pm[0]; p.pm[2 * o + 1] = pm[1]; }
        if (p.skip_zero && v == 0) skipped = 1;
        else frame_vote_cells(pano_vote(pm[0], pm[1], p.W, p.H), v, p.sum_w, p.sum_v, dropped);
    }
    frame_vote_counters(dropped, skipped, p.counters);
}
#pragma clang fp contract(fast)

__global__ __launch_bounds__(kMosaicThreads) void emba_mosaic_mean_kernel(const unsigned long long* sum_w, const unsigned long long* sum_v, long n,
                                                                            unsigned long long min_weight, double fill, double* mean, uint8_t* covered,
                                                                            unsigned long long* n_covered /* zeroed on the stream in front of the launch */)
{
    const long c = (long)blockIdx.x * kMosaicThreads + threadIdx.x;
    unsigned int cov = 0;
    if (c < n) {
        const unsigned long long w = sum_w[c];
        cov = mosaic_covered(w, min_weight);
        mean[c] = mosaic_mean(w, sum_v[c], min_weight, fill);
        covered[c] = (uint8_t)cov;
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) cov += __shfl_xor(cov, o);
    if ((threadIdx.x & 63) == 0 && cov) atomicAdd(n_covered, (unsigned long long)cov);
}

__global__ __launch_bounds__(kMosaicThreads) void emba_mosaic_log_kernel(const double* mean, const uint8_t* covered, long n, double lo, double hi, double eps,
                                                                           int take_log, double* L, uint8_t* covered_out)
{
    const long c = (long)blockIdx.x * kMosaicThreads + threadIdx.x;
    if (c >= n) return;
    double l = 0.0;
    const bool ok = mosaic_log(mean[c], covered[c] != 0, lo, hi, eps, take_log, &l);
    L[c] = ok ? l : 0.0;
    covered_out[c] = ok ? 1 : 0;
}

__global__ __launch_bounds__(kMosaicThreads) void emba_mosaic_map_kernel(const double* L, const uint8_t* covered, int W, int H, double* Gx, double* Gy)
{
    const long c = (long)blockIdx.x * kMosaicThreads + threadIdx.x;
    if (c >= (long)W * H) return;
    double gx, gy;
    mosaic_gradient(L, covered, W, (int)(c / W), (int)(c % W), &gx, &gy);
    Gx[c] = gx;
    Gy[c] = gy;
}

}  // namespace emba
