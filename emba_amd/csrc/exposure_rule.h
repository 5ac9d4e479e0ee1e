// emba_amd/csrc/exposure_rule.h — the photometric half of the frame alignment (exposure_host.h, exposure_kernels.h), as functions of plain values: a frame
// carries, beside its rotation, a gain and a bias, I = a * I0 + b, which are estimated with the rotation and applied when the frame is stitched.  Here are
// the argument checks, the terms one pixel adds to a frame's 5-parameter normal equations, the Levenberg-Marquardt step on the active rows with its accept /
// reject and its four ways to end, the compensated byte a frame votes into the mosaic, and the gauge of a set of frames aligned to their own mosaic.
// The warp, the cell, the sample with its gradient, the inverse tone, the Huber weight, the classes and the rotation's trial are align_rule.h's: they are
// called here, not restated.
// emba_amd.io.exposure_terms / exposure_sums / exposure_step / align_frames_exposure / exposure_bytes / exposure_gauge are the same rules in numpy;
// include/emba_hip.h (emba_frames_exposure_eval, emba_frames_exposure_align, emba_mosaic_frames_exposure) states them in words.
//
// No HIP in here: plain C++17, so that tests/cpp/exposure_rule_test.cpp checks it on a CPU in milliseconds.  Everything below the argument checks but the
// gauge is compiled for the host and for the device: the kernels and the CPU test run the same functions.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <cmath>

#include "../../include/emba_hip.h"      // emba_exposure_settings, EMBA_EXPOSURE_*
#include "align_rule.h"

namespace emba {

// ---- argument checks (behind align_rule.h's, in the order the C ABI reports them in)
enum class ExposureArgStatus { ok, gain_null, bias_null, gain_not_finite, gain_not_positive, bias_not_finite };
// *bad: the first frame whose gain or bias is refused
inline ExposureArgStatus exposure_args_ok(const double* gain, const double* bias, size_t F, size_t* bad)
{
    if (F && !gain) return ExposureArgStatus::gain_null;
    if (F && !bias) return ExposureArgStatus::bias_null;
    for (size_t f = 0; f < F; ++f) {
        *bad = f;
        if (!std::isfinite(gain[f])) return ExposureArgStatus::gain_not_finite;
        if (!(gain[f] > 0.0)) return ExposureArgStatus::gain_not_positive;
        if (!std::isfinite(bias[f])) return ExposureArgStatus::bias_not_finite;
    }
    return ExposureArgStatus::ok;
}
inline bool exposure_estimate_ok(int32_t estimate) { return estimate >= 0 && estimate <= 3; }
// the two bounds of the gain: finite, 0 < gain_min <= 1 <= gain_max
inline bool exposure_bounds_ok(double gain_min, double gain_max)
{
    return std::isfinite(gain_min) && std::isfinite(gain_max) && gain_min > 0.0 && gain_min <= 1.0 && gain_max >= 1.0;
}

// ---- one pixel: align_pixel's classes in align_pixel's precedence (skipped tests the raw byte) and, where used, I0 = align_tone(v), the compensated
// intensity I = a * I0 + b (multiply, then add, without contraction), r = val - I, its weight and cost, and g.  The Jacobian row of r in (delta, a, b) is
// (g, -I0, -1).  With a = 1, b = 0, I is I0 exactly and every member is align_pixel's.
struct ExposureTerm { double r, w, rho, g[3], I0; };
EMBA_RULE_HD inline int exposure_pixel(const double* P, const uint8_t* valid, int W, int H, double pm_x, double pm_y, const double* J23, unsigned v, double lo, double hi,
                                       double gain, double bias, bool skip_zero, double huber_k, ExposureTerm* t)
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
    t->I0 = align_tone(v, lo, hi);
    const double scaled = gain * t->I0;
    t->r = val - (scaled + bias);
    align_huber(t->r, huber_k, &t->w, &t->rho);
    for (int j = 0; j < 3; ++j) t->g[j] = gx * J23[j] + gy * J23[3 + j];
    return kAlignUsed;
}

// ---- the frame's 21 sums: H = sum w J^T J as the upper triangle in row-major order over (delta0, delta1, delta2, a, b) — 00 01 02 03 04 11 12 13 14 22 23
// 24 33 34 44 —, then b = sum w J^T r (five), then cost = sum rho.  The ten of them that align_accumulate forms are formed by the same operations.
constexpr int kExposureParams = 5;
constexpr int kExposureSums = 21, kExposureRhs = 15, kExposureCost = 20;
EMBA_RULE_HD constexpr int exposure_h_index(int i, int j) { return i * kExposureParams - i * (i - 1) / 2 + (j - i); }      // i <= j
// where align_rule.h's ten sums lie among the 21
EMBA_RULE_HD constexpr int exposure_shared_index(int k)
{
    return k == 0 ? 0 : k == 1 ? 1 : k == 2 ? 2 : k == 3 ? 5 : k == 4 ? 6 : k == 5 ? 9 : k < 9 ? kExposureRhs + (k - 6) : kExposureCost;
}
EMBA_RULE_HD inline void exposure_accumulate(const ExposureTerm& t, double* sums)
{
    const double ja = -t.I0, jb = -1.0;
    const double w0 = t.w * t.g[0], w1 = t.w * t.g[1], w2 = t.w * t.g[2], wa = t.w * ja, wb = t.w * jb;
    sums[0] += w0 * t.g[0]; sums[1] += w0 * t.g[1]; sums[2] += w0 * t.g[2]; sums[3] += w0 * ja; sums[4] += w0 * jb;
    sums[5] += w1 * t.g[1]; sums[6] += w1 * t.g[2]; sums[7] += w1 * ja; sums[8] += w1 * jb;
    sums[9] += w2 * t.g[2]; sums[10] += w2 * ja; sums[11] += w2 * jb;
    sums[12] += wa * ja; sums[13] += wa * jb;
    sums[14] += wb * jb;
    sums[15] += w0 * t.r; sums[16] += w1 * t.r; sums[17] += w2 * t.r; sums[18] += wa * t.r; sums[19] += wb * t.r;
    sums[20] += t.rho;
}
// the ten sums of align_rule.h out of the 21
EMBA_RULE_HD inline void exposure_shared_sums(const double* sums, double* ten)
{
    for (int k = 0; k < kAlignSums; ++k) ten[k] = sums[exposure_shared_index(k)];
}

// ---- the step.  `estimate`: bit 0 the gain, bit 1 the bias; a parameter that is not estimated has no row or column.  The rotation always has its three.
constexpr int kExposureGain = 1, kExposureBias = 2;
// (A + lambda diag A) x = rhs for the N x N symmetric A (row-major, the upper triangle is read) by a Cholesky: align_solve's operations in align_solve's
// order on the leading 3 x 3 block.  false: a pivot is not positive (also a NaN) or x is not finite; x is left alone.
template <int N>
EMBA_RULE_HD inline bool exposure_cholesky(const double* A, const double* rhs, double lambda, double* x)
{
    double L[N][N], y[N], z[N];
#if defined(__clang__)
#pragma unroll
#endif
    for (int j = 0; j < N; ++j) {
        double d = A[j * N + j] + lambda * A[j * N + j];
#if defined(__clang__)
#pragma unroll
#endif
        for (int k = 0; k < j; ++k) d = d - L[j][k] * L[j][k];
        if (!(d > 0.0)) return false;
        L[j][j] = sqrt(d);
#if defined(__clang__)
#pragma unroll
#endif
        for (int i = j + 1; i < N; ++i) {
            double s = A[j * N + i];
#if defined(__clang__)
#pragma unroll
#endif
            for (int k = 0; k < j; ++k) s = s - L[i][k] * L[j][k];
            L[i][j] = s / L[j][j];
        }
    }
#if defined(__clang__)
#pragma unroll
#endif
    for (int i = 0; i < N; ++i) {
        double s = rhs[i];
#if defined(__clang__)
#pragma unroll
#endif
        for (int k = 0; k < i; ++k) s = s - L[i][k] * y[k];
        y[i] = s / L[i][i];
    }
#if defined(__clang__)
#pragma unroll
#endif
    for (int i = N - 1; i >= 0; --i) {
        double s = y[i];
#if defined(__clang__)
#pragma unroll
#endif
        for (int k = i + 1; k < N; ++k) s = s - L[k][i] * z[k];
        z[i] = s / L[i][i];
    }
    bool finite = true;
    for (int i = 0; i < N; ++i) finite = finite && std::isfinite(z[i]);
    if (!finite) return false;
    for (int i = 0; i < N; ++i) x[i] = z[i];
    return true;
}
// the rows i3, i4 (3: gain, 4: bias; -1: none) beside the rotation's three, gathered out of the 21 sums
template <int N>
EMBA_RULE_HD inline bool exposure_solve_rows(const double* sums, double lambda, int i3, int i4, double* x)
{
    const int idx[5] = {0, 1, 2, i3, i4};
    double A[N * N], rhs[N];
    for (int i = 0; i < N; ++i) {
        for (int j = i; j < N; ++j) A[i * N + j] = A[j * N + i] = sums[exposure_h_index(idx[i], idx[j])];
        rhs[i] = -sums[kExposureRhs + idx[i]];
    }
    return exposure_cholesky<N>(A, rhs, lambda, x);
}
// Collinear: with gain and bias both estimated, their columns -I0 and -1 are collinear when every used byte is the same.  The damping lambda diag H keeps
// every pivot of such a system positive, so the Cholesky does not see it; the undamped 2 x 2 block of the two does: its second pivot H44 - H34^2 / H33 is
// sum w (1 - mean(I0)^2 / mean(I0^2)), zero but for rounding.  A frame whose pivot is at most kExposureCollinear of H44 is degenerate.  Rounding leaves
// about n * 2^-53 of H44 at the worst, 1e-10 for a million pixels; one byte of a million that differs from the rest by one step leaves 1.5e-11 and is
// degenerate too: such a frame does not tell a gain from a bias.
constexpr double kExposureCollinear = 1e-9;
EMBA_RULE_HD inline bool exposure_collinear(const double* sums)
{
    const double h33 = sums[12], h34 = sums[13], h44 = sums[14];
    if (!(h33 > 0.0) || !(h44 > 0.0)) return true;      // (a NaN too; no weight at all, or every I0 zero)
    return !(h44 - h34 * h34 / h33 > kExposureCollinear * h44);
}
// x [5] = (delta, x_a, x_b), zero where a parameter is not estimated.  estimate = 0: the system is align_solve's, and align_solve is called.  false: the frame
// is degenerate, x is left alone.
EMBA_RULE_HD inline bool exposure_solve(const double* sums, double lambda, int estimate, double* x)
{
    double s[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    bool ok = false;
    if (estimate == 0) {
        double ten[kAlignSums];
        exposure_shared_sums(sums, ten);
        ok = align_solve(ten, lambda, s);
    } else if (estimate == kExposureGain) {
        double y[4];
        ok = exposure_solve_rows<4>(sums, lambda, 3, -1, y);
        if (ok) { s[0] = y[0]; s[1] = y[1]; s[2] = y[2]; s[3] = y[3]; }
    } else if (estimate == kExposureBias) {
        double y[4];
        ok = exposure_solve_rows<4>(sums, lambda, 4, -1, y);
        if (ok) { s[0] = y[0]; s[1] = y[1]; s[2] = y[2]; s[4] = y[3]; }
    } else {
        ok = !exposure_collinear(sums) && exposure_solve_rows<5>(sums, lambda, 3, 4, s);
    }
    if (!ok) return false;
    for (int k = 0; k < 5; ++k) x[k] = s[k];
    return true;
}

// ---- one frame of the loop: align_rule.h's AlignFrame with (a, b) beside q and 21 sums.  (q, gain, bias) with its sums and counts is the accepted state;
// (q_trial, gain_trial, bias_trial) is the trial the next evaluation is taken at.
struct ExposureFrame {
    double q[4], q_trial[4], gain, bias, gain_trial, bias_trial, sums[kExposureSums], lambda, dnorm;
    uint64_t counts[4];
    int32_t status, iters, have_trial;
};
EMBA_RULE_HD inline void exposure_frame_init(ExposureFrame* s, const double* q, double gain, double bias, double lambda0)
{
    for (int k = 0; k < 4; ++k) { s->q[k] = s->q_trial[k] = q[k]; s->counts[k] = 0; }
    for (int k = 0; k < kExposureSums; ++k) s->sums[k] = 0.0;
    s->gain = s->gain_trial = gain; s->bias = s->bias_trial = bias;
    s->lambda = lambda0; s->dnorm = 0.0;
    s->status = EMBA_ALIGN_RUNNING; s->iters = 0; s->have_trial = 0;
}
// exposure_step: align_step with the two parameters more —
//   decide    as align_step decides, and a trial whose gain was estimated and lies outside [gain_min, gain_max] is rejected like one that raises the mean
//             cost.  Accepted: (q, a, b) <- the trial's; converged tests |delta| < tol_rot, the rotation alone.
//   propose   degenerate when n < min_pixels or exposure_solve fails; otherwise q_trial = normalise(exp(delta) q) by align_apply, a_trial = a + x_a,
//             b_trial = b + x_b.
// With estimate = 0 every operation on q, lambda and the ten shared sums is align_step's.
EMBA_RULE_HD inline void exposure_step(ExposureFrame* s, const double* esums, const uint64_t* ecounts, const emba_exposure_settings& xs, int estimate)
{
    const emba_align_settings& set = xs.align;
    if (s->status != EMBA_ALIGN_RUNNING) return;
    bool take = !s->have_trial;
    if (s->have_trial) {
        ++s->iters;
        const uint64_t n1 = ecounts[0], n0 = s->counts[0];
        take = n1 >= (uint64_t)set.min_pixels && esums[kExposureCost] / (double)n1 < s->sums[kExposureCost] / (double)n0;
        if ((estimate & kExposureGain) && !(s->gain_trial >= xs.gain_min && s->gain_trial <= xs.gain_max)) take = false;
    }
    if (take) {
        for (int k = 0; k < kExposureSums; ++k) s->sums[k] = esums[k];
        for (int k = 0; k < 4; ++k) s->counts[k] = ecounts[k];
    }
    if (s->have_trial) {
        if (take) {
            for (int k = 0; k < 4; ++k) s->q[k] = s->q_trial[k];
            s->gain = s->gain_trial; s->bias = s->bias_trial;
            const double down = s->lambda / set.lambda_down;
            s->lambda = down > set.lambda_min ? down : set.lambda_min;
            if (s->dnorm < set.tol_rot) { s->status = EMBA_ALIGN_CONVERGED; return; }
        } else {
            s->lambda *= set.lambda_up;
            if (s->lambda > set.lambda_max) { s->status = EMBA_ALIGN_STALLED; return; }
        }
    }
    double x[5];
    if (s->counts[0] < (uint64_t)set.min_pixels || !exposure_solve(s->sums, s->lambda, estimate, x)) { s->status = EMBA_ALIGN_DEGENERATE; return; }
    if (s->iters >= set.max_iters) { s->status = EMBA_ALIGN_ITERATIONS; return; }
    align_apply(x, s->q, s->q_trial);
    s->gain_trial = s->gain + x[3];
    s->bias_trial = s->bias + x[4];
    s->dnorm = sqrt(x[0] * x[0] + x[1] * x[1] + x[2] * x[2]);
    s->have_trial = 1;
}

// ---- the byte a compensated frame votes into the mosaic: clamp(rint(a * v + b), 0, 255), ties to even, in fp64 without contraction.  The bias is in byte
// units here: the mosaic's plane is (lo = 0, hi = 255, I0 = v).
EMBA_RULE_HD inline unsigned exposure_byte(unsigned v, double gain, double bias)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double scaled = gain * (double)v;
    const double r = rint(scaled + bias);
    return r <= 0.0 ? 0u : r >= 255.0 ? 255u : (unsigned)r;
}

// ---- the gauge of F frames aligned to their own mosaic: the common affine tone is free, and is fixed by alpha = mean a, beta = mean b over the frames with
// ok != 0: a <- a / alpha, b <- (b - beta) / alpha, for every frame.  false (nothing is changed): no frame is ok, or alpha is not positive and finite.
inline bool exposure_gauge(double* gain, double* bias, const uint8_t* ok, size_t F)
{
    double sa = 0.0, sb = 0.0;
    size_t n = 0;
    for (size_t f = 0; f < F; ++f) if (!ok || ok[f]) { sa += gain[f]; sb += bias[f]; ++n; }
    if (!n) return false;
    const double alpha = sa / (double)n, beta = sb / (double)n;
    if (!(alpha > 0.0 && std::isfinite(alpha) && std::isfinite(beta))) return false;
    for (size_t f = 0; f < F; ++f) { gain[f] = gain[f] / alpha; bias[f] = (bias[f] - beta) / alpha; }
    return true;
}

}  // namespace emba
