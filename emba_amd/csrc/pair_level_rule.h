// emba_amd/csrc/pair_level_rule.h — the pair alignment coarse to fine over a pyramid of the sensor frames, with the pair's exposure estimated
// (pair_level_host.h, pair_level_kernels.h), as functions of plain values: the sizes, bytes, bearings and camera of a level, the argument checks, the
// 5-parameter term of one pixel, min_pixels per level and the schedule over levels.  The projection, the cell, the sample and the term of the rotation are
// pair_rule.h's, the 21 sums, the solve and the step exposure_rule.h's: they are called here and not restated.
// emba_amd.io.pair_level_size / pair_level_bytes / pair_level_lut / pair_level_calib / pair_exposure_terms / pair_exposure_sums / pair_align_levels are the
// same rules in numpy; include/emba_hip.h (emba_frames_pair_level_eval, emba_frames_pair_align_levels) states them in words.
//
// No HIP in here: plain C++17, so that tests/cpp/pair_level_rule_test.cpp checks it on a CPU in milliseconds.  What the kernels call is compiled for the host
// and for the device; the loops over pixels at the end are the host's alone, the CPU form of what the kernels do.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <cmath>
#include <vector>

#include "exposure_rule.h"
#include "pair_rule.h"

namespace emba {

constexpr int kPairMaxLevel = 7;       // level l is the frame box-reduced by 2^l
constexpr int kPairMaxLevels = 8;      // entries of a schedule

// ---- level sizes: [sh >> l, sw >> l]; level pixel (X, Y) is the box x in [X 2^l, (X + 1) 2^l), y likewise; what is left over at the right and at the bottom
// takes no part.  A bilinear cell needs 2 x 2.
EMBA_RULE_HD inline int pair_level_dim(int n, int l) { return n >> l; }
EMBA_RULE_HD inline bool pair_level_size_ok(int sw, int sh, int l) { return l >= 0 && l <= kPairMaxLevel && (sw >> l) >= 2 && (sh >> l) >= 2; }

// ---- level bytes, formed from level 0: (sum of the box + 4^l / 2) >> 2l in integers (level 0: the byte).  Under skip_zero a box that holds a zero byte is 0:
// "no data" stays "no data", and a box without a zero gives 1 at the least.
constexpr uint32_t kPairBoxZero = 0x80000000u;      // the flag "the box holds a zero byte" beside a box sum (at most 255 * 4^7 < 2^22)
EMBA_RULE_HD inline uint32_t pair_box_of_byte(unsigned v) { return v ? (uint32_t)v : kPairBoxZero; }
// four boxes of level l - 1 into one of level l: sums of sums are exact
EMBA_RULE_HD inline uint32_t pair_box_join(uint32_t a, uint32_t b, uint32_t c, uint32_t d)
{
    const uint32_t m = kPairBoxZero - 1u;
    return (((a & m) + (b & m)) + ((c & m) + (d & m))) | ((a | b | c | d) & kPairBoxZero);
}
EMBA_RULE_HD inline unsigned pair_box_byte(uint32_t box, int l, bool skip_zero)
{
    if (skip_zero && (box & kPairBoxZero)) return 0u;
    const uint32_t sum = box & (kPairBoxZero - 1u);
    return (unsigned)((sum + (((uint32_t)1 << (2 * l)) >> 1)) >> (2 * l));
}
// the box of level pixel (X, Y) straight from the frame [sh, sw]
EMBA_RULE_HD inline uint32_t pair_box_direct(const uint8_t* frame, int sw, int X, int Y, int l)
{
    const int n = 1 << l;
    uint32_t sum = 0, zero = 0;
    for (int y = Y * n; y < (Y + 1) * n; ++y)
        for (int x = X * n; x < (X + 1) * n; ++x) {
            const unsigned v = frame[(size_t)y * (size_t)sw + (size_t)x];
            sum += v;
            if (!v) zero = kPairBoxZero;
        }
    return sum | zero;
}

// ---- level bearings from the table (x', y', 1) per pixel: level 0 is the table; for l >= 1 the centre of a box is the corner shared by its four central
// pixels, and the bearing is 0.25 ((b00 + b01) + (b10 + b11)) of those four, componentwise in this order, so z stays 1.  Behind a pinhole that is the centre's
// bearing but for rounding; behind a lens the bilinear midpoint.
EMBA_RULE_HD inline void pair_level_bearing(const double* lut, int sw, int X, int Y, int l, double* b)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    if (l == 0) {
        const double* p = lut + 3 * ((size_t)Y * (size_t)sw + (size_t)X);
        b[0] = p[0]; b[1] = p[1]; b[2] = p[2];
        return;
    }
    const int h = 1 << (l - 1);
    const size_t x = (size_t)X * (size_t)(2 * h) + (size_t)(h - 1), y = (size_t)Y * (size_t)(2 * h) + (size_t)(h - 1);
    const double* b00 = lut + 3 * (y * (size_t)sw + x);
    const double* b01 = b00 + 3;
    const double* b10 = b00 + 3 * (size_t)sw;
    const double* b11 = b10 + 3;
    for (int k = 0; k < 3; ++k) b[k] = 0.25 * ((b00[k] + b01[k]) + (b10[k] + b11[k]));
}

// ---- level camera: full-resolution u is the centre of pixel u; the centre of level pixel X is X 2^l + (2^l - 1) / 2, so u_l = (u - (2^l - 1) / 2) / 2^l:
// fu_l = fu / 2^l, cu_l = (cu - (2^l - 1) / 2) / 2^l, v likewise, D unchanged.  Level 0 is the camera bit for bit.
EMBA_RULE_HD inline PairCamera pair_level_camera(const PairCamera& c, int l)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double n = (double)(1 << l), half = ((double)(1 << l) - 1.0) / 2.0;
    PairCamera o = c;
    o.fu = c.fu / n; o.fv = c.fv / n;
    o.cu = (c.cu - half) / n; o.cv = (c.cv - half) / n;
    return o;
}

// ---- min_pixels at level l: min_pixels >> 2l, but not below the smaller of min_pixels and 8; every other setting is the same at every level
EMBA_RULE_HD inline int32_t pair_level_min_pixels(int32_t min_pixels, int l)
{
    const int32_t scaled = min_pixels >> (2 * l), floor_ = min_pixels < 8 ? min_pixels : 8;
    return scaled > floor_ ? scaled : floor_;
}
inline emba_exposure_settings pair_level_settings(const emba_exposure_settings& xs, int l)
{
    emba_exposure_settings o = xs;
    o.align.min_pixels = pair_level_min_pixels(xs.align.min_pixels, l);
    return o;
}

// ---- argument checks behind pair_args_ok (the order the C ABI reports them in); *at: the entry of the schedule that is refused
enum class PairLevelArgStatus { ok, levels_null, too_many_levels, level_out_of_range, level_too_small };
inline PairLevelArgStatus pair_levels_ok(const int32_t* levels, size_t n, int sw, int sh, size_t* at)
{
    if (!levels || !n) return PairLevelArgStatus::levels_null;
    if (n > (size_t)kPairMaxLevels) return PairLevelArgStatus::too_many_levels;
    for (size_t k = 0; k < n; ++k) {
        *at = k;
        if (levels[k] < 0 || levels[k] > kPairMaxLevel) return PairLevelArgStatus::level_out_of_range;
    }
    for (size_t k = 0; k < n; ++k) {
        *at = k;
        if (!pair_level_size_ok(sw, sh, levels[k])) return PairLevelArgStatus::level_too_small;
    }
    return PairLevelArgStatus::ok;
}
// everything emba_frames_pair_align_levels refuses, in its order: pair_args_ok's up to huber_k, the schedule, estimate, the gain bounds, the loop's settings,
// the bytes of the sequence
enum class PairLevelsCallStatus { ok, pair_args, levels, estimate, bounds, settings, bytes };
inline PairLevelsCallStatus pair_levels_call_ok(PairArgStatus args, PairLevelArgStatus lv, int32_t estimate, const emba_exposure_settings* xs, size_t F, size_t S)
{
    if (args != PairArgStatus::ok) return PairLevelsCallStatus::pair_args;
    if (lv != PairLevelArgStatus::ok) return PairLevelsCallStatus::levels;
    if (!exposure_estimate_ok(estimate)) return PairLevelsCallStatus::estimate;
    if (xs && !exposure_bounds_ok(xs->gain_min, xs->gain_max)) return PairLevelsCallStatus::bounds;
    if (align_settings_ok(xs ? &xs->align : nullptr) != AlignSetStatus::ok) return PairLevelsCallStatus::settings;
    if (!pair_bytes_ok(F, S)) return PairLevelsCallStatus::bytes;
    return PairLevelsCallStatus::ok;
}

// ---- the 5-parameter term of level pixel s of a pair: pair_term as it is on the level's table, bytes, size and camera, and from its AlignTerm and the source
// byte v the ExposureTerm with I0 = (double)v; the Jacobian row of r in (delta, a, b) is (g, -v, -1).  pair_pixel's r = val - (a v + b) is exposure_pixel's
// expression already.
EMBA_RULE_HD inline int pair_exposure_term(const double* lut, int s, const double* Q, const PairCamera& cam, const uint8_t* tgt, int sw, int sh, unsigned v, double a,
                                           double b, bool skip_zero, double huber_k, double* uv, ExposureTerm* t)
{
    AlignTerm at;
    const int cls = pair_term(lut, s, Q, cam, tgt, sw, sh, v, a, b, skip_zero, huber_k, uv, &at);
    t->r = at.r;
    if (cls != kAlignUsed) return cls;
    t->w = at.w; t->rho = at.rho;
    t->g[0] = at.g[0]; t->g[1] = at.g[1]; t->g[2] = at.g[2];
    t->I0 = (double)v;
    return cls;
}

// ---- the schedule: levels[0 ... n) in any order.  A pair starts level k + 1 from its accepted (Q, a, b) of level k; a level that ends converged, on
// iterations or stalled hands its accepted state on; a level that ends degenerate ends the pair there.
EMBA_RULE_HD inline bool pair_level_hands_on(int32_t status) { return status != EMBA_ALIGN_DEGENERATE; }

// ======== the host's own loops over pixels: what the kernels compute, on a CPU ========
// the bytes [sh_l, sw_l] of level l of one frame
inline void pair_level_bytes(const uint8_t* frame, int sw, int sh, int l, bool skip_zero, uint8_t* out)
{
    const int wl = sw >> l, hl = sh >> l;
    for (int Y = 0; Y < hl; ++Y)
        for (int X = 0; X < wl; ++X) out[(size_t)Y * wl + X] = l ? (uint8_t)pair_box_byte(pair_box_direct(frame, sw, X, Y, l), l, skip_zero) : frame[(size_t)Y * sw + X];
}
// the table [S_l, 3] of level l
inline void pair_level_lut(const double* lut, int sw, int sh, int l, double* out)
{
    const int wl = sw >> l, hl = sh >> l;
    for (int Y = 0; Y < hl; ++Y)
        for (int X = 0; X < wl; ++X) pair_level_bearing(lut, sw, X, Y, l, out + 3 * ((size_t)Y * wl + X));
}
// one evaluation of a pair at a level: the 21 sums and the four counts, summed in pixel order
inline void pair_level_evaluate(const double* lut_l, const uint8_t* src_l, const uint8_t* tgt_l, int wl, int hl, const PairCamera& cam_l, const double* Q, double a,
                                double b, bool skip_zero, double huber_k, double* sums, uint64_t* counts)
{
    for (int k = 0; k < kExposureSums; ++k) sums[k] = 0.0;
    for (int k = 0; k < 4; ++k) counts[k] = 0;
    for (int s = 0; s < wl * hl; ++s) {
        double uv[2];
        ExposureTerm t;
        const int cls = pair_exposure_term(lut_l, s, Q, cam_l, tgt_l, wl, hl, src_l[s], a, b, skip_zero, huber_k, uv, &t);
        if (cls == kAlignUsed) exposure_accumulate(t, sums);
        ++counts[cls];
    }
}
// the whole schedule of one pair (frames src, tgt [sh, sw]).  level_status / level_iters [n]: 0 where a level was not run.
struct PairLevelsResult {
    double q[4], gain, bias, sums[kExposureSums], cost0, info[6];
    uint64_t counts[4], n0;
    int32_t status, iters, level_status[kPairMaxLevels], level_iters[kPairMaxLevels];
};
inline PairLevelsResult pair_levels_align(const double* lut, const uint8_t* src, const uint8_t* tgt, int sw, int sh, const PairCamera& cam, const double* Q, double a,
                                          double b, bool skip_zero, const int32_t* levels, size_t n, int estimate, const emba_exposure_settings& xs)
{
    PairLevelsResult r{};
    double q[4] = {Q[0], Q[1], Q[2], Q[3]};
    for (size_t k = 0; k < n; ++k) {
        const int l = levels[k], wl = sw >> l, hl = sh >> l;
        std::vector<uint8_t> sb((size_t)wl * hl), tb((size_t)wl * hl);
        std::vector<double> tl(3 * (size_t)wl * hl);
        pair_level_bytes(src, sw, sh, l, skip_zero, sb.data());
        pair_level_bytes(tgt, sw, sh, l, skip_zero, tb.data());
        pair_level_lut(lut, sw, sh, l, tl.data());
        const PairCamera cl = pair_level_camera(cam, l);
        const emba_exposure_settings xl = pair_level_settings(xs, l);
        ExposureFrame f;
        exposure_frame_init(&f, q, a, b, xl.align.lambda0);
        while (f.status == EMBA_ALIGN_RUNNING) {
            double es[kExposureSums];
            uint64_t ec[4];
            pair_level_evaluate(tl.data(), sb.data(), tb.data(), wl, hl, cl, f.q_trial, f.gain_trial, f.bias_trial, skip_zero, xl.align.huber_k, es, ec);
            if (k == 0 && !f.have_trial) { r.cost0 = es[kExposureCost]; r.n0 = ec[0]; }
            exposure_step(&f, es, ec, xl, estimate);
        }
        r.level_status[k] = f.status; r.level_iters[k] = f.iters; r.iters += f.iters; r.status = f.status;
        for (int i = 0; i < 4; ++i) { r.q[i] = q[i] = f.q[i]; r.counts[i] = f.counts[i]; }
        for (int i = 0; i < kExposureSums; ++i) r.sums[i] = f.sums[i];
        r.gain = a = f.gain; r.bias = b = f.bias;
        if (!pair_level_hands_on(f.status)) break;
    }
    double ten[kAlignSums];
    exposure_shared_sums(r.sums, ten);
    pair_information(ten, r.counts[0], r.info);
    return r;
}

}  // namespace emba
