// emba_amd/csrc/contrast_rule.h — the smooth contrast of the panorama of warped events and its gradient with respect to the control poses
// (contrast_host.h, contrast_kernels.h), as functions of plain values: the argument checks, the bilinear votes of one projected event with their
// derivatives, the gradient of one event, the span of control poses a workgroup's LDS table covers, the levels of the coarse-to-fine refinement
// (their grids, the scaled vote, the vote kernel a level takes, the shares of its persistent workgroups), and the prior (the level mask, the weight, the
// cell an image starts from).
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

// ---- levels (coarse to fine).  Level l in [0, kContrastMaxLevel] is the rule above on a grid of W_l = pano_w >> l by H_l = pano_h >> l
// cells: the vote coordinate is pm_l = pm 2^-l and the Jacobian D_l = D 2^-l (both exact scalings), everything else — floor, the four weights and their
// derivatives, the column wrap modulo W_l, rows outside [0, H_l) dropped and counted, a pm that is not finite, the polarity signs, ge and where it is
// added — is unchanged with W_l, H_l for W, H.  Level 0 is the rule above, bit for bit (a product with 1.0).  emba_amd.io.contrast_level is the numpy form.
constexpr int kContrastMaxLevel = 8;
enum class ContrastLevelStatus { ok, bad_level, not_divisible, too_few_rows };
inline ContrastLevelStatus contrast_level_ok(int pano_w, int pano_h, int level)
{
    if (level < 0 || level > kContrastMaxLevel) return ContrastLevelStatus::bad_level;
    const int m = (1 << level) - 1;
    if ((pano_w & m) || (pano_h & m)) return ContrastLevelStatus::not_divisible;
    if ((pano_h >> level) < 2) return ContrastLevelStatus::too_few_rows;
    return ContrastLevelStatus::ok;
}
struct ContrastLevel {
    int W, H;          // W_l, H_l
    double scale;      // 2^-l
};
EMBA_RULE_HD inline ContrastLevel contrast_level_grid(int pano_w, int pano_h, int level)      // (of a level contrast_level_ok accepts)
{
    return ContrastLevel{pano_w >> level, pano_h >> level, 1.0 / (double)(1 << level)};
}
// the votes of one event at a level: contrast_vote of the scaled pm on the level's grid
EMBA_RULE_HD inline ContrastVotes contrast_vote_level(double pm_x, double pm_y, const ContrastLevel& lv)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    return contrast_vote(pm_x * lv.scale, pm_y * lv.scale, lv.W, lv.H);
}

// ---- which vote kernel a level call takes.  An image of at most kContrastLdsCells cells (64 KiB of fp64: what one workgroup may declare as a static array,
// and two fifths of a compute unit's 160 KiB) is summed in LDS by a fixed grid of persistent workgroups, each over a contiguous share of the events, and
// only the non-zero cells of each workgroup's image go to HBM; a larger one takes the adds in HBM directly.  forced: option contrast_vote, -1 by the size,
// 0 always HBM, 1 LDS wherever the image fits (never where it does not).
constexpr int kContrastLdsCells = 8192;
constexpr int kContrastLdsThreads = 1024;
enum class ContrastVotePath { hbm = 0, lds = 1 };
inline ContrastVotePath contrast_vote_plan(int W_l, int H_l, int forced)
{
    const bool fits = (int64_t)W_l * (int64_t)H_l <= kContrastLdsCells;
    return fits && forced != 0 ? ContrastVotePath::lds : ContrastVotePath::hbm;
}
// the persistent grid: one workgroup per compute unit, whatever the number of events
inline int contrast_lds_grid(int compute_units) { return compute_units > 0 ? compute_units : 1; }
// the events [beg, end) of workgroup b of `blocks`: contiguous shares of ceil(nn / blocks) events, at least one round of the workgroup's lanes — any
// partition is correct (every vote is an add); a workgroup behind the last event gets an empty share and adds nothing
struct ContrastShare { long beg, end; };
EMBA_RULE_HD inline ContrastShare contrast_share(long nn, int blocks, int b)
{
    long per = (nn + blocks - 1) / blocks;
    if (per < kContrastLdsThreads) per = kContrastLdsThreads;
    const long beg = (long)b * per < nn ? (long)b * per : nn;
    const long end = beg + per < nn ? beg + per : nn;
    return ContrastShare{beg, end};
}

// ---- the prior: per level at most one image P_l [H_l, W_l] of what earlier events voted.  With one, the image of a call starts as
// prior_weight P_l instead of zero: I(c) = prior_weight P_l(c) + sum_k s_k w_kc, and J and the gradient are the rule above on that I — J = sum (lambda P + I_w)^2,
// the window's own contrast plus twice its correlation with the prior plus a constant.  Everything about the votes is unchanged.
constexpr int kContrastLevels = kContrastMaxLevel + 1;
// a cell of the image in front of the votes
EMBA_RULE_HD inline double contrast_prior_cell(double prior_weight, double p) { return prior_weight * p; }
// the weight of a call: finite and not negative (false for NaN)
inline bool contrast_prior_weight_ok(double prior_weight) { return prior_weight >= 0.0 && prior_weight <= 1.7976931348623157e308; }
// the levels of emba_seq_contrast_prior_add: bit l of the mask is level l.  Refused: no bit, a bit at kContrastLevels or above, a set level the panorama
// does not admit (*bad_level: the lowest such level; contrast_level_ok says what is wrong with it)
enum class ContrastMaskStatus { ok, empty, bad_bit, bad_level };
inline ContrastMaskStatus contrast_prior_mask_ok(int pano_w, int pano_h, uint32_t mask, int* bad_level = nullptr)
{
    if (!mask) return ContrastMaskStatus::empty;
    if (mask >> kContrastLevels) return ContrastMaskStatus::bad_bit;
    for (int l = 0; l < kContrastLevels; ++l) {
        if (!((mask >> l) & 1u) || contrast_level_ok(pano_w, pano_h, l) == ContrastLevelStatus::ok) continue;
        if (bad_level) *bad_level = l;
        return ContrastMaskStatus::bad_level;
    }
    return ContrastMaskStatus::ok;
}
// the levels of a mask in the order the vote kernel takes them (ascending): levels[0 .. n), n returned
inline int contrast_prior_levels(uint32_t mask, int* levels)
{
    int n = 0;
    for (int l = 0; l < kContrastLevels; ++l)
        if ((mask >> l) & 1u) levels[n++] = l;
    return n;
}

}  // namespace emba
