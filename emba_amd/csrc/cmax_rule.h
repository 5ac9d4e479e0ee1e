// emba_amd/csrc/cmax_rule.h — contrast maximisation on the resident event sequence (cmax_host.h, cmax_kernels.h), as functions of plain values: the vote
// grid of a sensor, the pinhole behind the image of warped events, the slices, the compass search's step schedule and the argument checks.
// emba_amd.io (cmax_grid, cmax_pinhole_fit, cmax_objective, estimate_angular_velocity) is the same rule in numpy; include/emba_hip.h states it in words.
//
// No HIP in here: plain C++17, so that tests/cpp/cmax_rule_test.cpp checks it on a CPU in milliseconds.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <cmath>

// (the search's step is taken by the kernel and by the host alike; step_rule.h defines the same macro the same way)
#if !defined(EMBA_RULE_HD)
#if defined(__HIPCC__)
#define EMBA_RULE_HD __host__ __device__
#else
#define EMBA_RULE_HD
#endif
#endif

namespace emba {

// ---- the vote grid: cells of 2^shift sensor pixels, shift the smallest for which ceil(w / 2^shift) x ceil(h / 2^shift) uint32 cells fit 64 KiB (the LDS
// of a compute unit, 160 KiB, has room for two such workgroups; how many are resident is the kernel's register count's to say: cmax_kernels.h).  240x180: shift 1, 120x90 (43 200 B); 64x48: shift 0.
constexpr size_t kCmaxGridBytes = (size_t)64 << 10;
constexpr size_t kCmaxMaxCells = kCmaxGridBytes / sizeof(uint32_t);
struct CmaxGrid {
    int shift, w, h;
    size_t cells() const { return (size_t)w * (size_t)h; }
};
inline CmaxGrid cmax_grid(int sensor_w, int sensor_h)
{
    for (int s = 0;; ++s) {
        const long gw = ((long)sensor_w + (1L << s) - 1) >> s, gh = ((long)sensor_h + (1L << s) - 1) >> s;
        if ((size_t)gw * (size_t)gh <= kCmaxMaxCells) return {s, (int)gw, (int)gh};
    }
}

// ---- the plane of the image of warped events: an ideal pinhole u = f b'x / b'z + cu, v = f b'y / b'z + cv fitted to the bearing LUT alone, so that an
// unrotated event lands within about a pixel of its sensor position.  Least squares of x over b.x / b.z along the centre row (y = h / 2) and of y over
// b.y / b.z along the centre column (x = w / 2), entries with b.z > 0 only:
//     mx = (sum x) / n, mr = (sum r) / n, sxr = sum (x - mx)(r - mr), srr = sum (r - mr)^2, slope = sxr / srr
// every sum in index order and every operation rounded on its own (no contraction), f = (slope_row + slope_col) / 2 (one of them where the other
// direction has fewer than two entries or srr = 0), cu = mx - f mr of the row, cv likewise of the column.
struct CmaxPinhole {
    double f = 0, cu = 0, cv = 0;
    bool ok = false;
};
struct CmaxLine { double m_pos = 0, m_ratio = 0, slope = 0; bool ok = false; };
// one line of the LUT: entries first, first + stride, ... (count of them) of lut [.., 3]; comp: 0 = x, 1 = y
inline CmaxLine cmax_fit_line(const double* lut, size_t first, size_t stride, int count, int comp)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    CmaxLine l;
    double sp = 0.0, sr = 0.0;
    int n = 0;
    for (int i = 0; i < count; ++i) {
        const double* b = lut + 3 * (first + (size_t)i * stride);
        if (!(b[2] > 0.0)) continue;
        const double r = b[comp] / b[2];
        sp = sp + (double)i;
        sr = sr + r;
        ++n;
    }
    if (!n) return l;
    l.m_pos = sp / (double)n;
    l.m_ratio = sr / (double)n;
    double spr = 0.0, srr = 0.0;
    for (int i = 0; i < count; ++i) {
        const double* b = lut + 3 * (first + (size_t)i * stride);
        if (!(b[2] > 0.0)) continue;
        const double r = b[comp] / b[2];
        const double dp = (double)i - l.m_pos, dr = r - l.m_ratio;
        const double pr = dp * dr, rr = dr * dr;
        spr = spr + pr;
        srr = srr + rr;
    }
    if (n < 2 || !(srr > 0.0)) return l;
    l.slope = spr / srr;
    l.ok = std::isfinite(l.slope) && l.slope > 0.0;
    return l;
}
inline CmaxPinhole cmax_pinhole_fit(const double* lut, int sensor_w, int sensor_h)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const CmaxLine row = cmax_fit_line(lut, (size_t)(sensor_h / 2) * (size_t)sensor_w, 1, sensor_w, 0);
    const CmaxLine col = cmax_fit_line(lut, (size_t)(sensor_w / 2), (size_t)sensor_w, sensor_h, 1);
    CmaxPinhole p;
    if (!row.ok && !col.ok) return p;
    if (row.ok && col.ok) {
        const double s = row.slope + col.slope;
        p.f = s * 0.5;
    } else {
        p.f = row.ok ? row.slope : col.slope;
    }
    const double fu = p.f * row.m_ratio, fv = p.f * col.m_ratio;
    p.cu = row.m_pos - fu;
    p.cv = col.m_pos - fv;
    p.ok = std::isfinite(p.f) && std::isfinite(p.cu) && std::isfinite(p.cv);
    return p;
}

// ---- slices: slice s of m = slice_events events is [s m, (s + 1) m) of the sequence; the tail behind the last whole slice is not estimated
inline size_t cmax_slice_count(size_t n, int64_t slice_events) { return slice_events >= 1 ? n / (size_t)slice_events : 0; }

// A bilinear vote is 256 units over four cells, a cell is a uint32 and the objective sum I^2 a uint64: exact for ranges of fewer than 2^24 events
// (I <= 256 m < 2^32, sum I^2 <= (sum I)^2 < 2^64).
constexpr int kCmaxVoteBits = 4;                          // weights in sixteenths: wx, wy = floor(frac * 16)
constexpr size_t kCmaxMaxRange = ((size_t)1 << 24) - 1;

// ---- the compass search of one slice, from omega = 0: the step starts at omega_max / 2; an iteration evaluates the six points omega +- step e_i in the
// order +x -x +y -y +z -z and moves to the best of them (ties: the earlier) iff its J is strictly greater than the centre's, else halves the step; it
// stops when step < omega_max 2^-12, or after 64 iterations.  Halving and the scale by 2^-12 are exact, and so is every omega the search visits.
constexpr int kCmaxMaxIter = 64;
constexpr int kCmaxEvalCap = 1 + 6 * kCmaxMaxIter;         // J(0) and six per iteration
EMBA_RULE_HD inline double cmax_first_step(double omega_max) { return omega_max * 0.5; }
EMBA_RULE_HD inline double cmax_min_step(double omega_max) { return omega_max * (1.0 / 4096.0); }
// the candidate c in [0, 6) of an iteration: axis c / 2, sign + for even c
EMBA_RULE_HD inline int cmax_axis(int c) { return c >> 1; }
EMBA_RULE_HD inline double cmax_sign(int c) { return (c & 1) ? -1.0 : 1.0; }

// The state of one slice's search as the kernel and the host take it: while running(), the six candidates of the iteration, then advance() with the first
// of them that has the largest J.
struct CmaxSearch {
    double w[3] = {0, 0, 0}, step = 0, min_step = 0;
    uint64_t J = 0;
    int iter = 0;
    EMBA_RULE_HD CmaxSearch(double omega_max, uint64_t J0) : step(cmax_first_step(omega_max)), min_step(cmax_min_step(omega_max)), J(J0) {}
    EMBA_RULE_HD bool running() const { return iter < kCmaxMaxIter && !(step < min_step); }
    // candidate c of the iteration (selects, no indexing by a run-time value: the kernel keeps all of this in registers)
    EMBA_RULE_HD void candidate(int c, double* out) const
    {
        const double d = cmax_sign(c) * step;
        const int a = cmax_axis(c);
        out[0] = a == 0 ? w[0] + d : w[0];
        out[1] = a == 1 ? w[1] + d : w[1];
        out[2] = a == 2 ? w[2] + d : w[2];
    }
    // the iteration's verdict: `best`, the first of the candidates with the largest J, and that J
    EMBA_RULE_HD void advance(int best, uint64_t Jbest)
    {
        if (Jbest > J) {
            double to[3];
            candidate(best, to);
            w[0] = to[0]; w[1] = to[1]; w[2] = to[2];
            J = Jbest;
        } else {
            step = step * 0.5;
        }
        ++iter;
    }
};

// ---- argument checks
enum class CmaxArgStatus { ok, bad_slice, bad_omega_max, slice_too_long };
inline CmaxArgStatus cmax_args_ok(int64_t slice_events, double omega_max)
{
    if (slice_events < 1) return CmaxArgStatus::bad_slice;
    if (!std::isfinite(omega_max) || !(omega_max > 0.0)) return CmaxArgStatus::bad_omega_max;
    if ((uint64_t)slice_events > kCmaxMaxRange) return CmaxArgStatus::slice_too_long;
    return CmaxArgStatus::ok;
}
enum class CmaxRangeStatus { ok, not_a_range, too_long };
inline CmaxRangeStatus cmax_range_ok(size_t beg, size_t end, size_t n)
{
    if (beg > end || end > n) return CmaxRangeStatus::not_a_range;
    if (end - beg > kCmaxMaxRange) return CmaxRangeStatus::too_long;
    return CmaxRangeStatus::ok;
}

}  // namespace emba
