// emba_amd/csrc/align_rule.h — direct photometric alignment of intensity frames to a panorama plane (align_host.h, align_kernels.h), as functions of plain
// values: the argument checks, the cell of a projected pixel (view_sample's, shared with the mask test), the sample with its gradient, the inverse tone, the
// Huber weight, the terms one pixel adds to a frame's normal equations, and the Levenberg-Marquardt step of one frame with its accept / reject and its four
// ways to end.  The chunks are view_chunk_frames(S, 1) of view_rule.h.
// emba_amd.io.align_sample / align_terms / align_sums / align_step / align_frames are the same rules in numpy; include/emba_hip.h (emba_frames_align_eval,
// emba_frames_align) states them in words.
//
// No HIP in here: plain C++17, so that tests/cpp/align_rule_test.cpp checks it on a CPU in milliseconds.  Everything below the argument checks is compiled
// for the host and for the device: the kernels and the CPU test run the same functions.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <cmath>

#include "../../include/emba_hip.h"      // emba_align_settings, EMBA_ALIGN_*
#include "view_rule.h"

namespace emba {

// ---- argument checks (the order the C ABI reports them in)
enum class AlignArgStatus { ok, frames_null, q_null, too_many_frames, tone_not_finite, hi_not_above_lo, huber_not_finite };
inline AlignArgStatus align_args_ok(bool have_frames, bool have_q, size_t F, double lo, double hi, double huber_k)
{
    if (F && !have_frames) return AlignArgStatus::frames_null;
    if (F && !have_q) return AlignArgStatus::q_null;
    if (F > 0x7FFFFFFFull) return AlignArgStatus::too_many_frames;
    if (!(std::isfinite(lo) && std::isfinite(hi))) return AlignArgStatus::tone_not_finite;
    if (!(hi > lo)) return AlignArgStatus::hi_not_above_lo;
    if (std::isnan(huber_k)) return AlignArgStatus::huber_not_finite;
    return AlignArgStatus::ok;
}
inline bool align_q_ok(const double* q)      // finite, and not of zero norm
{
    const double n2 = q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3];
    return std::isfinite(n2) && n2 > 0.0;
}
inline size_t align_first_bad_q(const double* q_xyzw, size_t F)      // the first frame whose rotation is refused, F where there is none
{
    for (size_t f = 0; f < F; ++f) if (!align_q_ok(q_xyzw + 4 * f)) return f;
    return F;
}
enum class AlignSetStatus { ok, null, max_iters, factors, lambda0, lambda_range, tol_rot, min_pixels };
inline AlignSetStatus align_settings_ok(const emba_align_settings* s)
{
    if (!s) return AlignSetStatus::null;
    if (s->max_iters < 0) return AlignSetStatus::max_iters;
    if (!(s->lambda_up > 1.0 && s->lambda_down > 1.0 && std::isfinite(s->lambda_up) && std::isfinite(s->lambda_down))) return AlignSetStatus::factors;
    if (!(s->lambda0 > 0.0 && std::isfinite(s->lambda0))) return AlignSetStatus::lambda0;
    if (!(s->lambda_min >= 0.0 && s->lambda_max > 0.0 && s->lambda_min <= s->lambda_max)) return AlignSetStatus::lambda_range;      // (a NaN is refused)
    if (!(s->tol_rot >= 0.0)) return AlignSetStatus::tol_rot;
    if (s->min_pixels < 3) return AlignSetStatus::min_pixels;
    return AlignSetStatus::ok;
}

// ---- the cell of pm on a plane [H, W]: exactly view_sample's — ix = floor(pm_x), ax = pm_x - ix, iy, ay likewise, the columns c0 = ix mod W and c1 = c0 + 1
// wrapped, row0 = iy * W; false (outside) for iy < 0, iy + 1 > H - 1, a pm that is not finite or |pm| >= 2^31.
struct AlignCell { size_t row0; int c0, c1; double ax, ay; };
EMBA_RULE_HD inline bool align_cell(int W, int H, double pm_x, double pm_y, AlignCell* c)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    if (!(fabs(pm_x) < 2147483648.0 && fabs(pm_y) < 2147483648.0)) return false;      // (also NaN)
    const double fx = floor(pm_x), fy = floor(pm_y);
    const int64_t ix = (int64_t)fx, iy = (int64_t)fy;
    if (iy < 0 || iy + 1 > (int64_t)H - 1) return false;
    c->ax = pm_x - fx;
    c->ay = pm_y - fy;
    int64_t c0 = ix % W;
    if (c0 < 0) c0 += W;
    c->c0 = (int)c0;
    c->c1 = c0 + 1 == W ? 0 : (int)c0 + 1;
    c->row0 = (size_t)iy * (size_t)W;
    return true;
}

// ---- the sample of plane P at a cell with its gradient in pm: val is view_sample's value, operation for operation;
//     gx = (1 - ay) (P[iy][c1] - P[iy][c0]) + ay (P[iy+1][c1] - P[iy+1][c0]),  gy = (1 - ax) (P[iy+1][c0] - P[iy][c0]) + ax (P[iy+1][c1] - P[iy][c1]),
// in this order and without contraction: numpy gives the same bits from the same pm.
EMBA_RULE_HD inline void align_sample_cell(const double* P, int W, const AlignCell& c, double* val, double* gx, double* gy)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double* r0 = P + c.row0;
    const double* r1 = r0 + W;
    const double p00 = r0[c.c0], p01 = r0[c.c1], p10 = r1[c.c0], p11 = r1[c.c1];
    const double top = (1.0 - c.ax) * p00 + c.ax * p01;
    const double bot = (1.0 - c.ax) * p10 + c.ax * p11;
    *val = (1.0 - c.ay) * top + c.ay * bot;
    *gx = (1.0 - c.ay) * (p01 - p00) + c.ay * (p11 - p10);
    *gy = (1.0 - c.ax) * (p10 - p00) + c.ax * (p11 - p01);
}
EMBA_RULE_HD inline bool align_sample(const double* P, int W, int H, double pm_x, double pm_y, double* val, double* gx, double* gy)
{
    AlignCell c;
    if (!align_cell(W, H, pm_x, pm_y, &c)) return false;
    align_sample_cell(P, W, c, val, gx, gy);
    return true;
}
// masked: a `valid` plane of bytes [H, W] is given and any of the cell's four bytes is 0
EMBA_RULE_HD inline bool align_masked(const uint8_t* valid, int W, const AlignCell& c)
{
    if (!valid) return false;
    const uint8_t* r0 = valid + c.row0;
    const uint8_t* r1 = r0 + W;
    return !(r0[c.c0] && r0[c.c1] && r1[c.c0] && r1[c.c1]);
}

// ---- the frame's byte in the plane's units: I = lo + v (hi - lo) / 255, mosaic_log's order, without contraction
EMBA_RULE_HD inline double align_tone(unsigned v, double lo, double hi)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    return lo + (double)v * (hi - lo) / 255.0;
}

// ---- the weight and the cost of a residual: huber_k <= 0 quadratic (w = 1, rho = r^2); else w = 1, rho = r^2 for |r| <= k and w = k / |r|,
// rho = 2 k |r| - k^2 beyond
EMBA_RULE_HD inline void align_huber(double r, double k, double* w, double* rho)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double a = fabs(r);
    if (!(k > 0.0) || a <= k) { *w = 1.0; *rho = r * r; return; }
    *w = k / a;
    *rho = 2.0 * k * a - k * k;
}

// ---- one pixel: its class (in this precedence: outside, masked, skipped; else used) and, where used, the residual r = val - I, its weight and cost and the
// row g = gx J23[0,:] + gy J23[1,:] (J23 row-major 2 x 3: d pm / d delta for R <- exp(delta) R).  r is 0 where the pixel is not used.
enum AlignClass : int { kAlignUsed = 0, kAlignOutside = 1, kAlignMasked = 2, kAlignSkipped = 3 };
struct AlignTerm { double r, w, rho, g[3]; };
EMBA_RULE_HD inline int align_pixel(const double* P, const uint8_t* valid, int W, int H, double pm_x, double pm_y, const double* J23, unsigned v, double lo, double hi,
                                    bool skip_zero, double huber_k, AlignTerm* t)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    t->r = 0.0;
    AlignCell c;
    if (!align_cell(W, H, pm_x, pm_y, &c)) return kAlignOutside;
    if (align_masked(valid, W, c)) return kAlignMasked;
    if (skip_zero && v == 0) return kAlignSkipped;
    double val, gx, gy;
    align_sample_cell(P, W, c, &val, &gx, &gy);
    t->r = val - align_tone(v, lo, hi);
    align_huber(t->r, huber_k, &t->w, &t->rho);
    for (int j = 0; j < 3; ++j) t->g[j] = gx * J23[j] + gy * J23[3 + j];
    return kAlignUsed;
}
// ... added to the frame's ten sums: H (00 01 02 11 12 22), b (0 1 2), cost
constexpr int kAlignSums = 10;
EMBA_RULE_HD inline void align_accumulate(const AlignTerm& t, double* sums)
{
    const double w0 = t.w * t.g[0], w1 = t.w * t.g[1], w2 = t.w * t.g[2];
    sums[0] += w0 * t.g[0]; sums[1] += w0 * t.g[1]; sums[2] += w0 * t.g[2];
    sums[3] += w1 * t.g[1]; sums[4] += w1 * t.g[2]; sums[5] += w2 * t.g[2];
    sums[6] += w0 * t.r; sums[7] += w1 * t.r; sums[8] += w2 * t.r;
    sums[9] += t.rho;
}

// ---- the step: (H + lambda diag H) delta = -b by a 3 x 3 Cholesky.  false: a pivot is not positive (also a NaN), delta is left alone.
EMBA_RULE_HD inline bool align_solve(const double* sums, double lambda, double* delta)
{
    const double a00 = sums[0] + lambda * sums[0], a11 = sums[3] + lambda * sums[3], a22 = sums[5] + lambda * sums[5];
    const double a01 = sums[1], a02 = sums[2], a12 = sums[4];
    if (!(a00 > 0.0)) return false;
    const double l00 = sqrt(a00), l10 = a01 / l00, l20 = a02 / l00;
    const double d1 = a11 - l10 * l10;
    if (!(d1 > 0.0)) return false;
    const double l11 = sqrt(d1), l21 = (a12 - l20 * l10) / l11;
    const double d2 = a22 - l20 * l20 - l21 * l21;
    if (!(d2 > 0.0)) return false;
    const double l22 = sqrt(d2);
    const double y0 = -sums[6] / l00, y1 = (-sums[7] - l10 * y0) / l11, y2 = (-sums[8] - l20 * y0 - l21 * y1) / l22;
    const double x2 = y2 / l22, x1 = (y1 - l21 * x2) / l11, x0 = (y0 - l10 * x1 - l20 * x2) / l00;
    if (!(std::isfinite(x0) && std::isfinite(x1) && std::isfinite(x2))) return false;
    delta[0] = x0; delta[1] = x1; delta[2] = x2;
    return true;
}
// q' = normalise(exp(delta) (x) q), quaternions xyzw (the exponential of emba_amd.so3.exp)
EMBA_RULE_HD inline void align_apply(const double* delta, const double* q, double* out)
{
    const double th2 = delta[0] * delta[0] + delta[1] * delta[1] + delta[2] * delta[2];
    double imag, real;
    if (th2 < 1e-20) { imag = 0.5 - th2 / 48.0; real = 1.0 - th2 / 8.0; }
    else { const double th = sqrt(th2); imag = sin(0.5 * th) / th; real = cos(0.5 * th); }
    const double ax = imag * delta[0], ay = imag * delta[1], az = imag * delta[2], aw = real;
    const double bx = q[0], by = q[1], bz = q[2], bw = q[3];
    const double x = aw * bx + ax * bw + ay * bz - az * by, y = aw * by + ay * bw + az * bx - ax * bz;
    const double z = aw * bz + az * bw + ax * by - ay * bx, w = aw * bw - ax * bx - ay * by - az * bz;
    const double n = sqrt(x * x + y * y + z * z + w * w);
    out[0] = x / n; out[1] = y / n; out[2] = z / n; out[3] = w / n;
}

// ---- one frame of the loop.  q with its sums and counts is the accepted state; q_trial with |delta| = dnorm is the trial the next evaluation is taken at.
// status: EMBA_ALIGN_RUNNING until the frame ends.
struct AlignFrame {
    double q[4], q_trial[4], sums[kAlignSums], lambda, dnorm;
    uint64_t counts[4];
    int32_t status, iters, have_trial;
};
EMBA_RULE_HD inline void align_frame_init(AlignFrame* s, const double* q, double lambda0)
{
    for (int k = 0; k < 4; ++k) { s->q[k] = s->q_trial[k] = q[k]; s->counts[k] = 0; }
    for (int k = 0; k < kAlignSums; ++k) s->sums[k] = 0.0;
    s->lambda = lambda0; s->dnorm = 0.0;
    s->status = EMBA_ALIGN_RUNNING; s->iters = 0; s->have_trial = 0;
}
// align_step: takes the evaluation (esums, ecounts) that was made at s->q_trial (at s->q itself while there is no trial yet) and moves the frame on —
//   decide    the trial is accepted when n' >= min_pixels and cost' / n' < cost / n: q <- q', the trial's sums become the frame's, lambda <-
//             max(lambda / lambda_down, lambda_min), and the frame has converged when |delta| < tol_rot; rejected: lambda <- lambda lambda_up, and the frame
//             has stalled when lambda > lambda_max.  Either way one iteration is counted.
//   propose   a frame still running is degenerate when n < min_pixels or a pivot is not positive; has used its iterations when iters == max_iters; otherwise
//             delta is solved and q_trial = normalise(exp(delta) q) is the next trial.
// A frame whose status is final is left alone.
EMBA_RULE_HD inline void align_step(AlignFrame* s, const double* esums, const uint64_t* ecounts, const emba_align_settings& set)
{
    if (s->status != EMBA_ALIGN_RUNNING) return;
    bool take = !s->have_trial;
    if (s->have_trial) {
        ++s->iters;
        const uint64_t n1 = ecounts[0], n0 = s->counts[0];
        take = n1 >= (uint64_t)set.min_pixels && esums[9] / (double)n1 < s->sums[9] / (double)n0;
    }
    if (take) {
        for (int k = 0; k < kAlignSums; ++k) s->sums[k] = esums[k];
        for (int k = 0; k < 4; ++k) s->counts[k] = ecounts[k];
    }
    if (s->have_trial) {
        if (take) {
            for (int k = 0; k < 4; ++k) s->q[k] = s->q_trial[k];
            const double down = s->lambda / set.lambda_down;
            s->lambda = down > set.lambda_min ? down : set.lambda_min;
            if (s->dnorm < set.tol_rot) { s->status = EMBA_ALIGN_CONVERGED; return; }
        } else {
            s->lambda *= set.lambda_up;
            if (s->lambda > set.lambda_max) { s->status = EMBA_ALIGN_STALLED; return; }
        }
    }
    double delta[3];
    if (s->counts[0] < (uint64_t)set.min_pixels || !align_solve(s->sums, s->lambda, delta)) { s->status = EMBA_ALIGN_DEGENERATE; return; }
    if (s->iters >= set.max_iters) { s->status = EMBA_ALIGN_ITERATIONS; return; }
    align_apply(delta, s->q, s->q_trial);
    s->dnorm = sqrt(delta[0] * delta[0] + delta[1] * delta[1] + delta[2] * delta[2]);
    s->have_trial = 1;
}

}  // namespace emba
