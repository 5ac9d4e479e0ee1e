// emba_amd/csrc/contrast_rule.h — the smooth contrast of the panorama of warped events and its gradient with respect to the control poses
// (contrast_host.h, contrast_kernels.h), as functions of plain values: the argument checks, the bilinear votes of one projected event with their
// derivatives, the gradient of one event, and the span of control poses a workgroup's LDS table covers.
// emba_amd.io.contrast_votes / contrast_gradient are the same rule in numpy; include/emba_hip.h (emba_seq_contrast_gradient) states it in words.
//
// The rule, once.  Range, batches, midpoints, pm, column wrap and pole rows are those of emba_seq_event_panorama (panorama_rule.h).  Event k projected to
// pm = (pm_x, pm_y): ix = floor(pm_x), ax = pm_x - ix, iy, ay likewise.  The cells (ix, iy), (ix + 1, iy), (ix, iy + 1), (ix + 1, iy + 1) carry
//     w    = (1 - ax)(1 - ay),  ax (1 - ay),  (1 - ax) ay,  ax ay            (they sum to 1)
//     dw/dpm_x = -(1 - ay), +(1 - ay), -ay, +ay      dw/dpm_y = -(1 - ax), -ax, +(1 - ax), +ax      (each sums to 0)
// A cell whose row lies outside [0, H) has index -1: it is dropped, and counted where its weight is not zero.  A pm that is not finite votes nowhere.
//     I(c) = sum_k s_k w_kc      s_k = 1, or +-1 by polarity (signed_polarity)          J = sum_c I(c)^2
// The gradient is taken with respect to the increments of io.incremental_update, knot_i <- exp(x_i) knot_i: g has 3 K entries.  For event k of the batch
// whose spline segment begins at control pose cp:
//     gp = sum_i I(c_i) (dwx_i, dwy_i) over the kept cells          ge = 2 s_k gp^T D_k
// with D_k the 2x6 dpm_ddrot_cp of the warp kernels, J23 [I - J1 | J1]; ge[0:3] is added to g[3 cp ..], ge[3:6] to g[3 (cp + 1) ..].
//
// No HIP in here: plain C++17, so that tests/cpp/contrast_rule_test.cpp checks it on a CPU in milliseconds.  contrast_vote and contrast_event_grad are
// compiled for the host and for the device, without contraction: the kernels and the CPU test run the same functions.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <cmath>

#include "panorama_rule.h"      // kPanoBatch, pano_batch_count, pano_events_used, pano_args_ok

namespace emba {

// ---- argument checks: those of the integer panorama except its limit on the range's length (fp64 cells do not overflow)
inline PanoArgStatus contrast_args_ok(size_t beg, size_t end, size_t n, int K, int64_t dt_ns)
{
    const PanoArgStatus s = pano_args_ok(beg, end, n, K, dt_ns);
    return s == PanoArgStatus::too_long ? PanoArgStatus::ok : s;
}

// ---- the votes of one event and their derivatives in pm
struct ContrastVotes {
    int32_t cell[4];      // row * W + column, or -1
    double w[4];          // in [0, 1]
    double dwx[4], dwy[4];
};
EMBA_RULE_HD inline ContrastVotes contrast_vote(double pm_x, double pm_y, int W, int H)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    ContrastVotes v = {{-1, -1, -1, -1}, {0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}};
    if (!(fabs(pm_x) < 2147483648.0 && fabs(pm_y) < 2147483648.0)) return v;      // (also NaN)
    const double fx = floor(pm_x), fy = floor(pm_y);
    const int64_t ix = (int64_t)fx, iy = (int64_t)fy;
    const double ax = pm_x - fx, ay = pm_y - fy, bx = 1.0 - ax, by = 1.0 - ay;
    int64_t c0 = ix % W;
    if (c0 < 0) c0 += W;
    const int64_t c1 = c0 + 1 == W ? 0 : c0 + 1;
    const bool r0 = iy >= 0 && iy < H, r1 = iy + 1 >= 0 && iy + 1 < H;
    v.w[0] = bx * by; v.w[1] = ax * by; v.w[2] = bx * ay; v.w[3] = ax * ay;
    v.dwx[0] = -by; v.dwx[1] = by; v.dwx[2] = -ay; v.dwx[3] = ay;
    v.dwy[0] = -bx; v.dwy[1] = -ax; v.dwy[2] = bx; v.dwy[3] = ax;
    if (r0) { v.cell[0] = (int32_t)(iy * W + c0); v.cell[1] = (int32_t)(iy * W + c1); }
    if (r1) { v.cell[2] = (int32_t)((iy + 1) * W + c0); v.cell[3] = (int32_t)((iy + 1) * W + c1); }
    return v;
}

// ---- ge = 2 s gp^T D of one event (a component that comes out not finite is 0): I4 = the image at the event's four cells (whatever stands at a dropped one), D row-major 2x6, s = +-1
EMBA_RULE_HD inline void contrast_event_grad(const ContrastVotes& v, const double* I4, const double* D, double s, double* ge)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    double gx = 0.0, gy = 0.0;
    for (int i = 0; i < 4; ++i)
        if (v.cell[i] >= 0) { gx += I4[i] * v.dwx[i]; gy += I4[i] * v.dwy[i]; }
    const double t = 2.0 * s;
    for (int j = 0; j < 6; ++j) {
        const double e = t * (gx * D[j] + gy * D[6 + j]);
        ge[j] = fabs(e) <= 1.7976931348623157e308 ? e : 0.0;      // a component that is not finite (a pm that is not, a D at a pole) adds nothing
    }
}

// ---- the span plan of the gradient kernel.  A workgroup whose events' control-pose indices lie in [cp_first, cp_last] adds to the control poses
// [cp_first, cp_last + 1]: cp_last - cp_first + 2 of them, three components each.  They fit the workgroup's LDS table iff that is at most
// kContrastTableCps; else the workgroup's lanes add to g in HBM directly.  Component j of control pose cp stands at table[3 (cp - cp_first) + j].
constexpr int kContrastTableCps = 64;
struct ContrastSpan {
    int first;        // cp_first
    int comps;        // 3 (cp_last - cp_first + 2): table entries in use, 0 for an empty workgroup (cp_last < cp_first)
    bool fits;        // comps <= 3 kContrastTableCps
};
EMBA_RULE_HD inline ContrastSpan contrast_span(int cp_first, int cp_last)
{
    ContrastSpan s = {cp_first, 0, true};
    if (cp_last < cp_first) return s;
    const int64_t cps = (int64_t)cp_last - (int64_t)cp_first + 2;
    s.fits = cps <= kContrastTableCps;
    s.comps = s.fits ? (int)(3 * cps) : 0;
    return s;
}

}  // namespace emba
