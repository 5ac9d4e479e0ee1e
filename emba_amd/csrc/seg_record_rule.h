// emba_amd/csrc/seg_record_rule.h — the segment record {p0, delta, r1, k, r2} of a pair of neighbouring control poses, and the SO(3) leaves it is formed from:
// ONE definition for the device (device_math.h includes this file; the prep launch, the in-kernel producer and every per-event pose use these functions) and for
// the host (step_host.h forms the K - 1 records of a steady step itself, option step_prep = 2; tests/cpp/seg_record_rule_test.cpp checks them on a CPU).
//
// No HIP in here: `__host__ __device__` under hipcc, plain C++ otherwise.  Everything below feeds an INTEGER the reference computes (the rounded panorama pixel),
// so every function body switches floating-point contraction off for itself (device_math.h says why) — per body, so that including this file changes nothing
// for the code behind it.  A compiler that does not know the pragma must be told on its command line (-ffp-contract=off).  What remains between the two sides
// is libm: sqrt and the divisions are correctly rounded on both, atan / sin / cos are ocml's on the device and the host C library's on the host.
#pragma once
#include <math.h>
#include <stddef.h>

#if defined(__HIPCC__)
#define EMBA_SEG_HD __host__ __device__ __forceinline__
#else
#define EMBA_SEG_HD inline
#endif
#if defined(__clang__)
#define EMBA_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#if defined(__FP_FAST_FMA) && !defined(EMBA_FP_CONTRACT_OFF)
#error "seg_record_rule.h: compile with -ffp-contract=off -DEMBA_FP_CONTRACT_OFF (the target has a fused multiply-add and this compiler may contract)"
#endif
#define EMBA_NO_CONTRACT
#endif

namespace emba {

constexpr double kSophusEps = 1e-10;  // Sophus::Constants<double>::epsilon(), sophus/common.hpp:94
constexpr double kPi = 3.14159265358979323846;

EMBA_SEG_HD double sqn3(double a, double b, double c) { EMBA_NO_CONTRACT return (a + b) + c; }

// SO3Base::normalize (sophus/so3.hpp:297-303); (x,y,z,w) storage.
// (round 6, measured and dropped: the four quotients by the same n with the reciprocal's refinement shared — the compiler's own fdiv expansion written out once,
// bit-identical in every parity test — saves ~35 of the tiled kernel's ~1100 VALU instructions per event: warp kernel -1.4 % at config 3, -1 % at 3 M, +1 us at 1 M;
// profiles/r06_shared_rcp_ab.txt.  Not worth a second path to the rounded pixel.)
EMBA_SEG_HD void quat_normalize(double* q)
{
    EMBA_NO_CONTRACT
    const double n2 = (q[0] * q[0] + q[2] * q[2]) + (q[1] * q[1] + q[3] * q[3]);
    const double n = sqrt(n2);
    q[0] /= n; q[1] /= n; q[2] /= n; q[3] /= n;
}

// SO3Base::operator* (so3.hpp:324-339) followed by the normalizing SO3(Quaternion) ctor (:481-487).
EMBA_SEG_HD void so3_mul(const double* a, const double* b, double* out)
{
    EMBA_NO_CONTRACT
    const double ax = a[0], ay = a[1], az = a[2], aw = a[3];
    const double bx = b[0], by = b[1], bz = b[2], bw = b[3];
    double r[4];
    r[3] = aw * bw - ax * bx - ay * by - az * bz;
    r[0] = aw * bx + ax * bw + ay * bz - az * by;
    r[1] = aw * by + ay * bw + az * bx - ax * bz;
    r[2] = aw * bz + az * bw + ax * by - ay * bx;
    quat_normalize(r);
    out[0] = r[0]; out[1] = r[1]; out[2] = r[2]; out[3] = r[3];
}

// Eigen QuaternionBase::toRotationMatrix via SO3Base::matrix() (so3.hpp:310-312); row-major.
EMBA_SEG_HD void quat_to_matrix(const double* q, double* R)
{
    EMBA_NO_CONTRACT
    const double x = q[0], y = q[1], z = q[2], w = q[3];
    const double tx = 2 * x, ty = 2 * y, tz = 2 * z;
    const double twx = tx * w, twy = ty * w, twz = tz * w;
    const double txx = tx * x, txy = ty * x, txz = tz * x;
    const double tyy = ty * y, tyz = tz * y, tzz = tz * z;
    R[0] = 1 - (tyy + tzz); R[1] = txy - twz;       R[2] = txz + twy;
    R[3] = txy + twz;       R[4] = 1 - (txx + tzz); R[5] = tyz - twx;
    R[6] = txz - twy;       R[7] = tyz + twx;       R[8] = 1 - (txx + tyy);
}

// Sophus::SO3Base::logAndTheta (so3.hpp:247-290)
EMBA_SEG_HD void so3_log(const double* q, double* w)
{
    EMBA_NO_CONTRACT
    const double squared_n = sqn3(q[0] * q[0], q[1] * q[1], q[2] * q[2]);
    const double qw = q[3];
    double f;
    if (squared_n < kSophusEps * kSophusEps) {
        const double squared_w = qw * qw;
        f = 2.0 / qw - (2.0 / 3.0) * (squared_n) / (qw * squared_w);
    } else {
        const double n = sqrt(squared_n);
        if (fabs(qw) < kSophusEps) f = (qw > 0.0) ? kPi / n : -kPi / n;
        else f = 2.0 * atan(n / qw) / n;
    }
    w[0] = f * q[0]; w[1] = f * q[1]; w[2] = f * q[2];
}

// Tile order, and pixel order with the pose per event: the pose of an event is evaluated PER EVENT from per-SEGMENT constants, so the warp kernel gathers nothing per batch.
// (At 100 M events the batch table is 1 M records: every event pulled its own 128-B line from HBM — 13.6 GB per launch, 43 % of the
// kernel's traffic by the counters — while the VALU was a third busy.)  The K-1 segment records (96 B each) stay in cache.
//   seg[12] = { p0[4], delta[3], r1, k[3], r2 }   with delta = log(p0^-1 p1), theta = |delta|, k = R0 delta/theta (world-frame axis),
//   r1 = -theta/2, r2 = theta^2 c(theta): the coefficients of Jl^-1(delta) = I + r1 A + r2 A^2 in A = hat(delta/theta)
//   (sophus_utils.hpp:372-414, incl. its small-angle and near-pi branches).
// Value: q = p0 * exp(u delta), the SAME calls in the same order as So3Spline<2>::evaluate (so3_spline.h:233-247) — bit-identical to the
// per-batch evaluation, which is what round(pm) needs.  Jacobian: Jl(u delta) = I + p1 A + p2 A^2 (sophus_utils.hpp:332-362) commutes with
// Jl^-1(delta) and R0 A R0^T = hat(k), hence J1 = u R0 Jl Jl^-1 R0^T = u (I + alpha hat(k) + gamma hat(k)^2) (so3_spline.h:261-270) with
// alpha = p1 + r1 - p1 r2 - p2 r1, gamma = p2 + r2 + p1 r1 - p2 r2 (A^3 = -A): the reference's J1 to rounding (Jacobian tolerance only).
constexpr int kSegRecordDoubles = 12;
EMBA_SEG_HD void segment_consts(const double* p0, const double* p1, double* seg)
{
    EMBA_NO_CONTRACT
    double p0inv[4] = {-p0[0], -p0[1], -p0[2], p0[3]};
    quat_normalize(p0inv);
    double r01[4], delta[3], R0[9];
    so3_mul(p0inv, p1, r01);
    so3_log(r01, delta);
    const double n2 = sqn3(delta[0] * delta[0], delta[1] * delta[1], delta[2] * delta[2]);
    const double th = sqrt(n2);
    double k[3] = {0, 0, 0}, r2;
    if (th > 0.0) {
        quat_to_matrix(p0, R0);
        const double a0 = delta[0] / th, a1 = delta[1] / th, a2 = delta[2] / th;
#if defined(__clang__)
#pragma unroll
#endif
        for (int r = 0; r < 3; ++r) k[r] = R0[3 * r] * a0 + R0[3 * r + 1] * a1 + R0[3 * r + 2] * a2;
    }
    if (n2 > kSophusEps) {
        if (th < kPi - sqrt(kSophusEps)) r2 = 1.0 - th * (1.0 + cos(th)) / (2.0 * sin(th));
        else r2 = n2 / (kPi * kPi);
    } else {
        r2 = n2 / 12.0;
    }
    seg[0] = p0[0]; seg[1] = p0[1]; seg[2] = p0[2]; seg[3] = p0[3];
    seg[4] = delta[0]; seg[5] = delta[1]; seg[6] = delta[2]; seg[7] = -0.5 * th;
    seg[8] = k[0]; seg[9] = k[1]; seg[10] = k[2]; seg[11] = r2;
}

// The K - 1 records of K control poses (x,y,z,w each), record s from poses s and s + 1: what the host forms for a steady step (step_host.h)
inline void segment_records(const double* knots, int K, double* seg)
{
    for (int s = 0; s + 1 < K; ++s) segment_consts(knots + 4 * s, knots + 4 * (s + 1), seg + (size_t)kSegRecordDoubles * s);
}

}  // namespace emba
