// emba_amd/csrc/view_kernels.h — sensor views along the trajectory (gfx950, wave64): what the camera would have seen at a frame time, sampled from a
// panorama plane, and what it reported between two frame times, counted from the resident event sequence.
// The rules: view_rule.h, include/emba_hip.h (emba_render_views, emba_seq_event_frames), DESIGN.md §17.
//   * pose stage                 the rotations at the F frame times: emba_pose_kernel (kernels.h) as it is, into the pose table of view_host.h
//   * emba_view_kernel           one lane per sensor pixel, the frame in blockIdx.y: frame_warp (frame_kernels.h, DESIGN.md §23: the bearing turned by the
//                                frame's rotation, the sum3 products of seq_event_warp, pm by project_chain<false>; the Jacobian is dead code),
//                                view_sample's four gathers, view_u8
//   * emba_event_frames_kernel   one lane per event: view_frame_of (a binary search over the edges) and one return-less int32 atomic add into the frame's
//                                pixel in HBM
// The view kernel streams: 24 B of LUT in and 8 B (+ 1) out per pixel, coalesced; the frame's pose record sits at a wave-uniform address, and the four
// gathers are plain loads — neighbouring sensor pixels land on neighbouring cells, and the patch of the panorama a view covers stays in L2.  No LDS, no
// scratch; the one atomic is a wave's count of outside pixels.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "frame_kernels.h"
#include "kernels.h"      // kPoseStride, emba_pose_kernel
#include "view_rule.h"

namespace emba {

constexpr int kViewThreads = 256;

struct ViewParams {
    const double* lut;            // bearing vector per sensor pixel [S, 3]
    const double* pose;           // pose records of the chunk's frames (kPoseStride doubles each)
    const double* plane;          // the source plane [H, W]
    int S, W, H;
    double fx, fy, cx, cy;        // the equirectangular camera of the context
    double fill, lo, scale;
    double* views;                // [nf, S] or nullptr
    uint8_t* u8;                  // [nf, S] or nullptr
    double* pm;                   // [nf, S, 2] or nullptr
    unsigned long long* outside;  // [nf], zeroed on the stream in front of the first launch
};

// Compiled without contraction: pm feeds floor(), and the sample is compared with numpy bit for bit.
#pragma clang fp contract(off)
__global__ __launch_bounds__(kViewThreads) void emba_view_kernel(ViewParams p)
{
    const int s = (int)blockIdx.x * kViewThreads + (int)threadIdx.x;
    const size_t f = blockIdx.y;
    unsigned int out = 0;
    if (s < p.S) {
        double pm[2], J23[6];
        frame_warp(p.lut, p.pose + (size_t)kPoseStride * f, s, p.fx, p.fy, p.cx, p.cy, pm, J23);
        const size_t o = f * (size_t)p.S + (size_t)s;
        if (p.pm) { p.pm[2 * o] = pm[0]; p.pm[2 * o + 1] = pm[1]; }
        double v;
        const bool inside = view_sample(p.plane, p.W, p.H, pm[0], pm[1], &v);
        out = inside ? 0u : 1u;
        if (p.views) p.views[o] = inside ? v : p.fill;
        if (p.u8) p.u8[o] = inside ? view_u8(v, p.lo, p.scale) : (uint8_t)0;
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) out += __shfl_xor(out, o);
    if ((threadIdx.x & 63) == 0 && out) atomicAdd(p.outside + f, (unsigned long long)out);
}
#pragma clang fp contract(fast)

struct EventFramesParams {
    const uint16_t* x; const uint16_t* y; const uint8_t* pol; const int64_t* t;   // the resident sequence, from the range's first event
    long n;                       // events of the range
    const int64_t* edge;          // [F + 1], strictly increasing
    long F, f0, nf;               // all frames; this launch's chunk [f0, f0 + nf)
    int sw; size_t S;
    int signed_polarity;
    int count_ends;               // this launch counts the events before edge[0] and at or after edge[F] (one launch of a call does)
    int32_t* frames;              // [nf, S], zeroed on the stream in front of this launch
    unsigned long long* ends;     // [0] before, [1] after (zeroed on the stream in front of the first launch)
};

__global__ __launch_bounds__(kViewThreads) void emba_event_frames_kernel(EventFramesParams p)
{
    const long k = (long)blockIdx.x * kViewThreads + threadIdx.x;
    unsigned int before = 0, after = 0;
    if (k < p.n) {
        const long f = view_frame_of(p.edge, p.F, p.t[k]);
        before = f < 0; after = f >= p.F;
        if (f >= p.f0 && f < p.f0 + p.nf)      // (every event was checked at its upload: inside the sensor)
            atomicAdd(p.frames + (size_t)(f - p.f0) * p.S + (size_t)p.y[k] * (size_t)p.sw + (size_t)p.x[k], (p.signed_polarity && p.pol[k] == 0) ? -1 : 1);
    }
    if (!p.count_ends) return;      // (uniform over the launch)
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) { before += __shfl_xor(before, o); after += __shfl_xor(after, o); }
    if ((threadIdx.x & 63) == 0) {
        if (before) atomicAdd(p.ends, (unsigned long long)before);
        if (after) atomicAdd(p.ends + 1, (unsigned long long)after);
    }
}

}  // namespace emba
