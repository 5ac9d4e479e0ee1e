// emba_amd/csrc/panorama_rule.h — the panorama of warped events along a trajectory (panorama_host.h, panorama_kernels.h), as functions of plain values: the
// argument checks, the batches of an event range and the four bilinear votes of one projected event on the equirectangular panorama.
// emba_amd.io.event_panorama is the same rule in numpy; include/emba_hip.h (emba_seq_event_panorama) states it in words.
//
// No HIP in here: plain C++17, so that tests/cpp/panorama_rule_test.cpp checks it on a CPU in milliseconds.  pano_vote is compiled for the host and for
// the device: the vote kernel and the CPU test run the same function.
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

// ---- batches: the model warps events in batches of 100 with one pose each (model.cpp:100-119); the tail behind the last whole batch is ignored (Q1)
constexpr size_t kPanoBatch = 100;
inline size_t pano_batch_count(size_t beg, size_t end) { return end > beg ? (end - beg) / kPanoBatch : 0; }
inline size_t pano_events_used(size_t beg, size_t end) { return pano_batch_count(beg, end) * kPanoBatch; }

// A bilinear vote is 256 units over four cells and a cell is an int32 (votes may be negative): exact for fewer than 2^23 events
// (|I| <= 256 nn < 2^31; sum I^2 <= (sum |I|)^2 < 2^62, a uint64; |sum I| < 2^31, an int64).
constexpr int kPanoVoteBits = 4;                           // weights in sixteenths: wx, wy = floor(frac * 16)
constexpr size_t kPanoMaxEvents = (size_t)1 << 23;         // nn >= this: refused

// ---- argument checks (the order the C ABI reports them in)
enum class PanoArgStatus { ok, not_a_range, too_few_knots, bad_dt, too_long };
inline PanoArgStatus pano_args_ok(size_t beg, size_t end, size_t n, int K, int64_t dt_ns)
{
    if (beg > end || end > n) return PanoArgStatus::not_a_range;
    if (K < 2) return PanoArgStatus::too_few_knots;
    if (dt_ns <= 0) return PanoArgStatus::bad_dt;
    if (pano_events_used(beg, end) >= kPanoMaxEvents) return PanoArgStatus::too_long;
    return PanoArgStatus::ok;
}

// ---- the votes of one event projected to pm = (pm_x, pm_y) on a panorama of W x H cells:
//     ix = floor(pm_x), wx = floor((pm_x - ix) * 16), iy, wy likewise; the cells (ix, iy), (ix + 1, iy), (ix, iy + 1), (ix + 1, iy + 1) get
//     (16 - wx)(16 - wy), wx (16 - wy), (16 - wx) wy, wx wy — 256 in all.
// Columns wrap modulo W (azimuth is periodic).  A row outside [0, H) has no cell: cell = -1, the weight stays (the caller counts the non-zero ones as
// dropped votes).  A pm that is not finite votes nowhere: every cell -1, every weight 0; so does |pm| >= 2^31, which no equirectangular projection gives.
struct PanoVotes {
    int32_t cell[4];      // row * W + column, or -1
    int32_t w[4];         // 0 ... 256
};
EMBA_RULE_HD inline PanoVotes pano_vote(double pm_x, double pm_y, int W, int H)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    PanoVotes v = {{-1, -1, -1, -1}, {0, 0, 0, 0}};
    if (!(fabs(pm_x) < 2147483648.0 && fabs(pm_y) < 2147483648.0)) return v;      // (also NaN)
    const double fx = floor(pm_x), fy = floor(pm_y);
    const int64_t ix = (int64_t)fx, iy = (int64_t)fy;
    const int32_t wx = (int32_t)((pm_x - fx) * 16.0), wy = (int32_t)((pm_y - fy) * 16.0);      // floor(frac 16) in [0, 15]
    int64_t c0 = ix % W;
    if (c0 < 0) c0 += W;
    const int64_t c1 = c0 + 1 == W ? 0 : c0 + 1;
    const bool r0 = iy >= 0 && iy < H, r1 = iy + 1 >= 0 && iy + 1 < H;
    v.w[0] = (16 - wx) * (16 - wy); v.w[1] = wx * (16 - wy); v.w[2] = (16 - wx) * wy; v.w[3] = wx * wy;
    if (r0) { v.cell[0] = (int32_t)(iy * W + c0); v.cell[1] = (int32_t)(iy * W + c1); }
    if (r1) { v.cell[2] = (int32_t)((iy + 1) * W + c0); v.cell[3] = (int32_t)((iy + 1) * W + c1); }
    return v;
}

}  // namespace emba
