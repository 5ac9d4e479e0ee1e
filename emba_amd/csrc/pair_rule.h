// emba_amd/csrc/pair_rule.h — direct photometric alignment of one intensity frame to another (pair_host.h, pair_kernels.h), as functions of plain values:
// the argument checks, the projection of a turned bearing into the other frame through the plumb_bob model with its Jacobian, the bilinear sample of that
// frame's bytes with its gradient, the classes of a pixel, the term it adds to the pair's normal equations, and the information of a finished pair.  The
// weight, the ten sums, the solve and the Levenberg-Marquardt step are align_rule.h's, called here and not restated: the perturbation is the same left one,
// Q <- exp(delta) Q.
// emba_amd.io.pair_start / pair_project / pair_terms / pair_sums / pair_align / pair_information are the same rules in numpy; include/emba_hip.h
// (emba_frames_pair_eval, emba_frames_pair_align) states them in words.
//
// No HIP in here: plain C++17, so that tests/cpp/pair_rule_test.cpp checks it on a CPU in milliseconds.  Everything below the argument checks is compiled
// for the host and for the device: the kernel and the CPU test run the same functions.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <cmath>

#include "align_rule.h"

namespace emba {

// ---- the bound on the sequence: all F frames lie in one device buffer for the whole call, so F * S bytes are bounded — at 1 GiB, 24 000 frames of 240 x 180,
// far past what a candidate search of O(F^2) on the host serves, and a tenth of what the other resident stages leave free on the card
constexpr size_t kPairMaxBytes = (size_t)1 << 30;
// pairs per launch: the pair is the grid's y index (view_rule.h: kViewChunkMaxFrames), and a chunk's scratch is bounded as a chunk of frames is
inline size_t pair_chunk_pairs(size_t S) { return view_chunk_frames(S, 1); }

// ---- argument checks (the order the C ABI reports them in)
enum class PairArgStatus { ok, frames_null, pairs_null, q_null, too_many_pairs, pair_out_of_range, bad_q, bad_exposure, bad_focal, bad_centre, bad_distortion,
                           huber_not_finite };
// *at: the first pair that is refused, where one is
inline PairArgStatus pair_args_ok(bool have_frames, size_t F, const int32_t* pairs, size_t P, const double* Q, const double* gain, const double* bias, double fu,
                                  double fv, double cu, double cv, const double* D, double huber_k, size_t* at)
{
    if (P && !have_frames) return PairArgStatus::frames_null;
    if (P && !pairs) return PairArgStatus::pairs_null;
    if (P && !Q) return PairArgStatus::q_null;
    if (P > 0x7FFFFFFFull) return PairArgStatus::too_many_pairs;
    for (size_t p = 0; p < P; ++p) {
        *at = p;
        if (pairs[2 * p] < 0 || pairs[2 * p + 1] < 0 || (size_t)pairs[2 * p] >= F || (size_t)pairs[2 * p + 1] >= F) return PairArgStatus::pair_out_of_range;
    }
    for (size_t p = 0; p < P; ++p) {
        *at = p;
        if (!align_q_ok(Q + 4 * p)) return PairArgStatus::bad_q;
    }
    for (size_t p = 0; p < P; ++p) {
        *at = p;
        if (gain && !(std::isfinite(gain[p]) && gain[p] > 0.0)) return PairArgStatus::bad_exposure;
        if (bias && !std::isfinite(bias[p])) return PairArgStatus::bad_exposure;
    }
    if (!(std::isfinite(fu) && std::isfinite(fv) && fu > 0.0 && fv > 0.0)) return PairArgStatus::bad_focal;
    if (!(std::isfinite(cu) && std::isfinite(cv))) return PairArgStatus::bad_centre;
    if (D) for (int k = 0; k < 5; ++k) if (!std::isfinite(D[k])) return PairArgStatus::bad_distortion;
    if (std::isnan(huber_k)) return PairArgStatus::huber_not_finite;
    return PairArgStatus::ok;
}
// (behind the loop's settings, align_settings_ok) the sequence fits its buffer
inline bool pair_bytes_ok(size_t F, size_t S) { return !S || F <= kPairMaxBytes / S; }

// ---- the camera of the target frame: u = fu x' + cu, v = fv y' + cv on the plumb_bob point (x', y') of (x, y); D = k1 k2 p1 p2 k3, the order of
// io.bearing_lut_from_calibration; all zero is the pinhole
struct PairCamera { double fu, fv, cu, cv, D[5]; };
EMBA_RULE_HD inline PairCamera pair_camera(double fu, double fv, double cu, double cv, const double* D)
{
    PairCamera c{fu, fv, cu, cv, {0.0, 0.0, 0.0, 0.0, 0.0}};
    if (D) for (int k = 0; k < 5; ++k) c.D[k] = D[k];
    return c;
}

// ---- rb = R(Q) b: the matrix of device_math.h's quat_to_matrix and the three sum3 products of frame_warp, operation for operation, without contraction
EMBA_RULE_HD inline void pair_turn(const double* Q, const double* b, double* rb)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double x = Q[0], y = Q[1], z = Q[2], w = Q[3];
    const double tx = 2 * x, ty = 2 * y, tz = 2 * z;
    const double twx = tx * w, twy = ty * w, twz = tz * w;
    const double txx = tx * x, txy = ty * x, txz = tz * x;
    const double tyy = ty * y, tyz = tz * y, tzz = tz * z;
    const double R[9] = {1 - (tyy + tzz), txy - twz, txz + twy, txy + twz, 1 - (txx + tzz), tyz - twx, txz - twy, tyz + twx, 1 - (txx + tyy)};
    for (int r = 0; r < 3; ++r) rb[r] = R[3 * r] * b[0] + (R[3 * r + 1] * b[1] + R[3 * r + 2] * b[2]);
}

// ---- the projection of rb into the target frame: false (outside) for rb_z <= 0 (also a NaN); else uv and J23 = d(u, v) / d rb, row-major 2 x 3, analytic.
// uv feeds floor(): no contraction.
EMBA_RULE_HD inline bool pair_project(const PairCamera& c, const double* rb, double* uv, double* J23)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double z = rb[2];
    if (!(z > 0.0)) return false;
    const double x = rb[0] / z, y = rb[1] / z;
    const double k1 = c.D[0], k2 = c.D[1], p1 = c.D[2], p2 = c.D[3], k3 = c.D[4];
    const double r2 = x * x + y * y;
    const double radial = 1.0 + ((k3 * r2 + k2) * r2 + k1) * r2;
    const double xd = x * radial + (2.0 * p1 * x * y + p2 * (r2 + 2.0 * x * x));
    const double yd = y * radial + (p1 * (r2 + 2.0 * y * y) + 2.0 * p2 * x * y);
    uv[0] = c.fu * xd + c.cu;
    uv[1] = c.fv * yd + c.cv;
    // d(x', y') / d(x, y), with rd = d radial / d r2
    const double rd = (3.0 * k3 * r2 + 2.0 * k2) * r2 + k1;
    const double cross = 2.0 * x * y * rd + 2.0 * p1 * x + 2.0 * p2 * y;
    const double axx = radial + 2.0 * x * x * rd + 2.0 * p1 * y + 6.0 * p2 * x;
    const double ayy = radial + 2.0 * y * y * rd + 6.0 * p1 * y + 2.0 * p2 * x;
    // d(x, y) / d rb = [1/z 0 -x/z; 0 1/z -y/z]
    const double iz = 1.0 / z;
    J23[0] = c.fu * axx * iz; J23[1] = c.fu * cross * iz; J23[2] = -c.fu * (axx * x + cross * y) * iz;
    J23[3] = c.fv * cross * iz; J23[4] = c.fv * ayy * iz; J23[5] = -c.fv * (cross * x + ayy * y) * iz;
    return true;
}
// Ju = J23 (-[rb]x), row-major 2 x 3: d(u, v) / d delta for Q <- exp(delta) Q
EMBA_RULE_HD inline void pair_left_jacobian(const double* J23, const double* rb, double* Ju)
{
    const double x = rb[0], y = rb[1], z = rb[2];
    for (int r = 0; r < 2; ++r) {
        const double j0 = J23[3 * r], j1 = J23[3 * r + 1], j2 = J23[3 * r + 2];
        Ju[3 * r] = j2 * y - j1 * z;
        Ju[3 * r + 1] = j0 * z - j2 * x;
        Ju[3 * r + 2] = j1 * x - j0 * y;
    }
}

// ---- the cell of (u, v) in a frame [sh, sw]: ix = floor(u), iy = floor(v), ax = u - ix, ay = v - iy; false (outside) for ix < 0, ix + 1 > sw - 1, iy < 0,
// iy + 1 > sh - 1, a point that is not finite or |.| >= 2^31.  A frame does not wrap.
struct PairCell { size_t o00; double ax, ay; };      // o00: the offset of byte (iy, ix) in the frame
EMBA_RULE_HD inline bool pair_cell(int sw, int sh, double u, double v, PairCell* c)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    if (!(fabs(u) < 2147483648.0 && fabs(v) < 2147483648.0)) return false;      // (also NaN)
    const double fx = floor(u), fy = floor(v);
    const int64_t ix = (int64_t)fx, iy = (int64_t)fy;
    if (ix < 0 || ix + 1 > (int64_t)sw - 1 || iy < 0 || iy + 1 > (int64_t)sh - 1) return false;
    c->ax = u - fx;
    c->ay = v - fy;
    c->o00 = (size_t)iy * (size_t)sw + (size_t)ix;
    return true;
}
// val, gx, gy of the four bytes of a cell as doubles: align_sample_cell's expressions, operation for operation
EMBA_RULE_HD inline void pair_sample_cell(double p00, double p01, double p10, double p11, double ax, double ay, double* val, double* gx, double* gy)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double top = (1.0 - ax) * p00 + ax * p01;
    const double bot = (1.0 - ax) * p10 + ax * p11;
    *val = (1.0 - ay) * top + ay * bot;
    *gx = (1.0 - ay) * (p01 - p00) + ay * (p11 - p10);
    *gy = (1.0 - ax) * (p10 - p00) + ax * (p11 - p01);
}

// ---- one source pixel of byte v against the target frame `tgt` [sh, sw], given where it lands: its class (align_rule.h's four, in its precedence: outside;
// masked: skip_zero and any of the cell's four bytes is 0; skipped: skip_zero and v is 0; else used) and, where used, r = val - (a v + b) in byte units, its
// weight and cost and the row g = gx Ju[0,:] + gy Ju[1,:].  r is 0 where the pixel is not used.  `projected`: pair_project's answer.
EMBA_RULE_HD inline int pair_pixel(const uint8_t* tgt, int sw, int sh, bool projected, const double* uv, const double* Ju, unsigned v, double a, double b,
                                   bool skip_zero, double huber_k, AlignTerm* t)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    t->r = 0.0;
    PairCell c;
    if (!projected || !pair_cell(sw, sh, uv[0], uv[1], &c)) return kAlignOutside;
    const uint8_t* r0 = tgt + c.o00;
    const uint8_t* r1 = r0 + sw;
    const unsigned b00 = r0[0], b01 = r0[1], b10 = r1[0], b11 = r1[1];
    if (skip_zero && !(b00 && b01 && b10 && b11)) return kAlignMasked;
    if (skip_zero && v == 0) return kAlignSkipped;
    double val, gx, gy;
    pair_sample_cell((double)b00, (double)b01, (double)b10, (double)b11, c.ax, c.ay, &val, &gx, &gy);
    t->r = val - (a * (double)v + b);
    align_huber(t->r, huber_k, &t->w, &t->rho);
    for (int j = 0; j < 3; ++j) t->g[j] = gx * Ju[j] + gy * Ju[3 + j];
    return kAlignUsed;
}
// the whole of it for source pixel s of a pair: turn, project, Jacobian, pixel.  uv is NaN where the projection has no point.
EMBA_RULE_HD inline int pair_term(const double* lut, int s, const double* Q, const PairCamera& cam, const uint8_t* tgt, int sw, int sh, unsigned v, double a, double b,
                                  bool skip_zero, double huber_k, double* uv, AlignTerm* t)
{
    double rb[3], J23[6], Ju[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    pair_turn(Q, lut + 3 * (size_t)s, rb);
    const bool projected = pair_project(cam, rb, uv, J23);
    if (projected) pair_left_jacobian(J23, rb, Ju);
    else uv[0] = uv[1] = NAN;
    return pair_pixel(tgt, sw, sh, projected, uv, Ju, v, a, b, skip_zero, huber_k, t);
}

// ---- the information of a finished pair about its rotation, in the target camera's coordinates: Lambda = H / s^2 with s^2 = cost / max(n - 3, 1), the six
// entries 00 01 02 11 12 22 of the sums' H
inline void pair_information(const double* sums, uint64_t n, double* info)
{
    const double dof = n > 3 ? (double)(n - 3) : 1.0;
    const double s2 = sums[9] / dof;
    for (int k = 0; k < 6; ++k) info[k] = sums[k] / s2;
}

// ---- the pair of two frames' values (camera to world rotations q_i, q_j; exposures a, b): Q = q_j^-1 (x) q_i normalised, a = a_i / a_j, b = (b_i - b_j) / a_j
inline void pair_start(const double* qi, const double* qj, double ai, double bi, double aj, double bj, double* Q, double* a, double* b)
{
    const double ax = -qj[0], ay = -qj[1], az = -qj[2], aw = qj[3];
    const double bx = qi[0], by = qi[1], bz = qi[2], bw = qi[3];
    const double x = aw * bx + ax * bw + ay * bz - az * by, y = aw * by + ay * bw + az * bx - ax * bz;
    const double z = aw * bz + az * bw + ax * by - ay * bx, w = aw * bw - ax * bx - ay * by - az * bz;
    const double n = sqrt(x * x + y * y + z * z + w * w);
    Q[0] = x / n; Q[1] = y / n; Q[2] = z / n; Q[3] = w / n;
    *a = ai / aj;
    *b = (bi - bj) / aj;
}

}  // namespace emba
