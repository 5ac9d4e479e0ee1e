// emba_amd/csrc/view_rule.h — sensor views along the trajectory (view_host.h, view_kernels.h), as functions of plain values: the bilinear sample of a
// panorama plane at a projected sensor pixel, its 8-bit tone, the frame an event's timestamp belongs to, and the cut of F frames into chunks.
// emba_amd.io.render_views / io.event_frames are the same rules in numpy; include/emba_hip.h (emba_render_views, emba_seq_event_frames) states them in words.
//
// No HIP in here: plain C++17, so that tests/cpp/view_rule_test.cpp checks it on a CPU in milliseconds.  view_sample, view_u8 and view_frame_of are compiled
// for the host and for the device: the kernels and the CPU test run the same functions.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <cmath>

#if !defined(EMBA_RULE_HD)
#if defined(__HIPCC__)
#define EMBA_RULE_HD __host__ __device__
#else
#define EMBA_RULE_HD
#endif
#endif

namespace emba {

// ---- chunks: the device holds the frames of one chunk at a time — at most 65 535 frames (the frame is the grid's y index) and at most 32 MiB of cells,
// but always one frame.  F itself has no limit.
constexpr size_t kViewChunkMaxFrames = 65535;
constexpr size_t kViewChunkMaxBytes = (size_t)32 << 20;
inline size_t view_chunk_frames(size_t S, size_t cell_bytes)      // frames per chunk for frames of S cells of cell_bytes each
{
    const size_t frame = S * cell_bytes, fit = frame ? kViewChunkMaxBytes / frame : kViewChunkMaxFrames;
    return fit < 1 ? 1 : (fit > kViewChunkMaxFrames ? kViewChunkMaxFrames : fit);
}
inline size_t view_chunk_count(size_t F, size_t per) { return (F + per - 1) / per; }
struct ViewChunk { size_t f0, nf; };
inline ViewChunk view_chunk(size_t F, size_t per, size_t i)       // chunk i < view_chunk_count(F, per): the frames [f0, f0 + nf)
{
    const size_t f0 = i * per;
    return ViewChunk{f0, F - f0 < per ? F - f0 : per};
}

// ---- the sample of plane P [H, W] at pm = (pm_x, pm_y): ix = floor(pm_x), ax = pm_x - ix, iy, ay likewise; the columns ix, ix + 1 wrap modulo W (the rule
// of panorama_rule.h: azimuth is periodic); iy < 0 or iy + 1 > H - 1 has no sample (false: the pixel is outside), and so has a pm that is not finite or
// |pm| >= 2^31.  Otherwise *v = (1 - ay) ((1 - ax) P[iy][ix] + ax P[iy][ix + 1]) + ay ((1 - ax) P[iy + 1][ix] + ax P[iy + 1][ix + 1]), in this order and
// without contraction: numpy gives the same bits from the same pm.
EMBA_RULE_HD inline bool view_sample(const double* P, int W, int H, double pm_x, double pm_y, double* v)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    if (!(fabs(pm_x) < 2147483648.0 && fabs(pm_y) < 2147483648.0)) return false;      // (also NaN)
    const double fx = floor(pm_x), fy = floor(pm_y);
    const int64_t ix = (int64_t)fx, iy = (int64_t)fy;
    if (iy < 0 || iy + 1 > (int64_t)H - 1) return false;
    const double ax = pm_x - fx, ay = pm_y - fy;
    int64_t c0 = ix % W;
    if (c0 < 0) c0 += W;
    const int64_t c1 = c0 + 1 == W ? 0 : c0 + 1;
    const double* r0 = P + (size_t)iy * (size_t)W;
    const double* r1 = r0 + W;
    const double top = (1.0 - ax) * r0[c0] + ax * r0[c1];
    const double bot = (1.0 - ax) * r1[c0] + ax * r1[c1];
    *v = (1.0 - ay) * top + ay * bot;
    return true;
}

// ---- the tone of emba_normalize_robust with the caller's lo / hi: u8 = sat(rint(scale (v - lo))), scale = 255 / (hi - lo), or 1 where hi == lo.  A NaN is 0.
EMBA_RULE_HD inline double view_scale(double lo, double hi) { return hi != lo ? 255.0 / (hi - lo) : 1.0; }
EMBA_RULE_HD inline uint8_t view_u8(double v, double lo, double scale)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double r = rint(scale * (v - lo));
    if (!(r > 0.0)) return 0;
    return r > 255.0 ? (uint8_t)255 : (uint8_t)r;
}

// ---- the frame of an event at time t among F frames with the edges edge[0] < ... < edge[F]: f with edge[f] <= t < edge[f + 1]; -1 before edge[0], F at or
// after edge[F].  A binary search: the number of edges <= t, less one.
EMBA_RULE_HD inline long view_frame_of(const int64_t* edge, long F, int64_t t)
{
    long lo = 0, hi = F + 1;
    while (lo < hi) {
        const long mid = lo + (hi - lo) / 2;
        if (edge[mid] <= t) lo = mid + 1; else hi = mid;
    }
    return lo - 1;
}
inline bool view_edges_ok(const int64_t* edge, size_t F)      // F + 1 edges, strictly increasing
{
    for (size_t f = 0; f < F; ++f) if (!(edge[f] < edge[f + 1])) return false;
    return true;
}

}  // namespace emba
