// emba_amd/csrc/device_math.h — gfx950 device functions for the geometry leaves of the EMBA hot path.
// All IEEE double, written from the formulas of the reference (file:line cited per function); the
// evaluation order follows the reference where that is cheap, but only the integer results
// (control-pose index, rounded panorama pixel) are required to be bit-exact (BASELINE north_star).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "seg_record_rule.h"   // sqn3, quat_normalize, so3_mul, quat_to_matrix, so3_log, segment_consts: shared with the host

namespace emba {

// Everything in this header up to the "Jacobian only" part of project_chain feeds an INTEGER the reference computes — the
// control-pose index and the rounded panorama pixel round(pm) (model.cpp:209-211) — so it is compiled WITHOUT floating-point
// contraction: the oracle is built -ffp-contract=off (oracle/Makefile) and a fused multiply-add here would make the two
// disagree in the last bit of pm, i.e. leave bit-exact indexing to luck.  With contraction off every operation below is the
// same IEEE operation in the same order as in the oracle; what remains is libm (ocml vs glibc atan2/asin/sin/cos/atan).
#pragma clang fp contract(off)

__device__ __forceinline__ double sum3(double a, double b, double c) { return a + (b + c); }

// C = A*B, row-major 3x3 (same summation pattern as Eigen's 3x3 lazy product into a Matrix3d:
// rows 0-1 ((t0+t1)+t2), row 2 (t0+(t1+t2)) — see oracle/emba_oracle.c mat3_mul_seq).
__device__ __forceinline__ void mat3_mul(const double* A, const double* B, double* C)
{
    double T[9];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const double t0 = A[3 * i + 0] * B[0 + j], t1 = A[3 * i + 1] * B[3 + j], t2 = A[3 * i + 2] * B[6 + j];
            T[3 * i + j] = (i < 2) ? (t0 + t1) + t2 : t0 + (t1 + t2);
        }
#pragma unroll
    for (int i = 0; i < 9; ++i) C[i] = T[i];
}

__device__ __forceinline__ void hat3(const double* p, double* M)
{   // Sophus::SO3::hat
    M[0] = 0;     M[1] = -p[2]; M[2] = p[1];
    M[3] = p[2];  M[4] = 0;     M[5] = -p[0];
    M[6] = -p[1]; M[7] = p[0];  M[8] = 0;
}

// sin and cos of the half rotation angle.  Between neighbouring control poses it is far below pi/4, where the two polynomial kernels
// of fdlibm (k_sin.c / k_cos.c, |x| <= pi/4, < 1 ulp) need no argument reduction and no quadrant selection: a third of the instructions
// of the general sin() + cos(), which stay as the fallback.  (The oracle calls the host libm; neither device form is bit-identical to it,
// both are within an ulp — scripts/flip_rate.py measures what that does to round(pm).)
__device__ __forceinline__ void sin_cos_half(double x, double& sn, double& cs)
{
    if (fabs(x) <= 0x1.921fb54442d18p-1) {
        // (explicit fma: the same instructions wherever this is inlined, whatever the contraction mode)
        const double z = x * x;
        const double rs = fma(z, fma(z, fma(z, fma(z, 1.58969099521155010221e-10, -2.50507602534068634195e-08), 2.75573137070700676789e-06),
                                     -1.98412698298579493134e-04), 8.33333333332248946124e-03);
        sn = fma(z * x, fma(z, rs, -1.66666666666666324348e-01), x);
        const double rc = z * fma(z, fma(z, fma(z, fma(z, fma(z, -1.13596475577881948265e-11, 2.08757232129817482790e-09), -2.75573143513906633035e-07),
                                              2.48015872894767294178e-05), -1.38888888888741095749e-03), 4.16666666666666019037e-02);
        const double hz = 0.5 * z, w = 1.0 - hz;
        cs = w + fma(z, rc, (1.0 - w) - hz);
    } else {
        sn = sin(x); cs = cos(x);
    }
}

// Jacobian-only reciprocal: v_rcp_f64 and two Newton steps (about an ulp) instead of the IEEE division's ~14 instructions.  Never
// used for anything an integer result depends on; its arguments here are O(1) (no scaling for denormal or huge values needed).
__device__ __forceinline__ double rcp_nr(double x)
{
    double r = __builtin_amdgcn_rcp(x);
    double e = fma(-x, r, 1.0);
    r = fma(r, e, r);
    e = fma(-x, r, 1.0);
    return fma(r, e, r);
}

// Sophus::SO3::expAndTheta (so3.hpp:583-619)
__device__ __forceinline__ void so3_exp(const double* w, double* q)
{
    const double theta_sq = sqn3(w[0] * w[0], w[1] * w[1], w[2] * w[2]);
    double imag, real;
    if (theta_sq < kSophusEps * kSophusEps) {
        const double theta_po4 = theta_sq * theta_sq;
        imag = 0.5 - (1.0 / 48.0) * theta_sq + (1.0 / 3840.0) * theta_po4;
        real = 1.0 - (1.0 / 8.0) * theta_sq + (1.0 / 384.0) * theta_po4;
    } else {
        const double theta = sqrt(theta_sq);
        const double half = 0.5 * theta;
        double sn, cs;
        sin_cos_half(half, sn, cs);
        imag = sn / theta;
        real = cs;
    }
    q[0] = imag * w[0]; q[1] = imag * w[1]; q[2] = imag * w[2]; q[3] = real;
}

// Sophus::leftJacobianSO3 (basalt/utils/sophus_utils.hpp:332-362)
__device__ __forceinline__ void left_jacobian(const double* phi, double* J)
{
    const double n2 = sqn3(phi[0] * phi[0], phi[1] * phi[1], phi[2] * phi[2]);
    double H[9], H2[9];
    hat3(phi, H);
    mat3_mul(H, H, H2);
#pragma unroll
    for (int i = 0; i < 9; ++i) J[i] = (i % 4 == 0) ? 1.0 : 0.0;
    if (n2 > kSophusEps) {
        const double n = sqrt(n2);
        const double n3 = n2 * n;
        const double c1 = 1 - cos(n), c2 = n - sin(n);
#pragma unroll
        for (int i = 0; i < 9; ++i) J[i] += H[i] * c1 / n2;
#pragma unroll
        for (int i = 0; i < 9; ++i) J[i] += H2[i] * c2 / n3;
    } else {
#pragma unroll
        for (int i = 0; i < 9; ++i) J[i] += H[i] / 2;
#pragma unroll
        for (int i = 0; i < 9; ++i) J[i] += H2[i] / 6;
    }
}

// Sophus::leftJacobianInvSO3 (basalt/utils/sophus_utils.hpp:372-414)
__device__ __forceinline__ void left_jacobian_inv(const double* phi, double* J)
{
    const double n2 = sqn3(phi[0] * phi[0], phi[1] * phi[1], phi[2] * phi[2]);
    double H[9], H2[9];
    hat3(phi, H);
    mat3_mul(H, H, H2);
#pragma unroll
    for (int i = 0; i < 9; ++i) J[i] = ((i % 4 == 0) ? 1.0 : 0.0) - H[i] / 2;
    if (n2 > kSophusEps) {
        const double n = sqrt(n2);
        if (n < kPi - sqrt(kSophusEps)) {
            const double c = 1 / n2 - (1 + cos(n)) / (2 * n * sin(n));
#pragma unroll
            for (int i = 0; i < 9; ++i) J[i] += H2[i] * c;
        } else {
#pragma unroll
            for (int i = 0; i < 9; ++i) J[i] += H2[i] / (kPi * kPi);
        }
    } else {
#pragma unroll
        for (int i = 0; i < 9; ++i) J[i] += H2[i] / 12;
    }
}

// basalt::So3Spline<2>::evaluate (so3_spline.h:218-274) for one query; knots (x,y,z,w).
// Outputs the value as unit quaternion q (x,y,z,w) and J1 = d_val_d_knot[1] (row-major); d_val_d_knot[0] = I - J1.
__device__ __forceinline__ void spline2_eval(const double* p0, const double* p1, double u, double* q_out, double* J1)
{
    double p0inv[4] = {-p0[0], -p0[1], -p0[2], p0[3]};
    quat_normalize(p0inv);                       // SO3::inverse -> SO3(conjugate) normalizes
    double r01[4], delta[3], kdelta[3];
    so3_mul(p0inv, p1, r01);
    so3_log(r01, delta);
#pragma unroll
    for (int i = 0; i < 3; ++i) kdelta[i] = delta[i] * u;
    double Jli[9], Jlk[9], T[9], R0[9], R0inv[9];
    left_jacobian_inv(delta, Jli);
    left_jacobian(kdelta, Jlk);
    quat_to_matrix(p0, R0);
#pragma unroll
    for (int i = 0; i < 9; ++i) T[i] = u * R0[i];
    mat3_mul(T, Jlk, T);
    mat3_mul(T, Jli, T);
    quat_to_matrix(p0inv, R0inv);
    mat3_mul(T, R0inv, J1);
    double e[4], res[4];
    so3_exp(kdelta, e);
    so3_mul(p0, e, res);
    q_out[0] = res[0]; q_out[1] = res[1]; q_out[2] = res[2]; q_out[3] = res[3];
}

__device__ __forceinline__ void project_jacobian(const double* rb, double fx, double fy, double* J23);

// J1 = u I + a1 hat(k) + a2 (k k^T - (k.k) I)
__device__ __forceinline__ void rebuild_j1(double u, double a1, double a2, const double* k, double* J1)
{
    const double kk = k[0] * k[0] + k[1] * k[1] + k[2] * k[2];
    const double d = u - a2 * kk;
    J1[0] = d + a2 * k[0] * k[0]; J1[1] = a2 * k[0] * k[1] - a1 * k[2]; J1[2] = a2 * k[0] * k[2] + a1 * k[1];
    J1[3] = a2 * k[1] * k[0] + a1 * k[2]; J1[4] = d + a2 * k[1] * k[1]; J1[5] = a2 * k[1] * k[2] - a1 * k[0];
    J1[6] = a2 * k[2] * k[0] - a1 * k[1]; J1[7] = a2 * k[2] * k[1] + a1 * k[0]; J1[8] = d + a2 * k[2] * k[2];
}

// sin and cos of the half angle behind a REAL call (see project_angles_call below: fp64 polynomial constants hoisted out of the tiled kernel's loop)
__device__ __attribute__((noinline)) double2 sin_cos_call(double x)
{
    double sn, cs;
    sin_cos_half(x, sn, cs);
    return make_double2(sn, cs);
}

template <bool CALL>
__device__ __forceinline__ void spline2_event(const double* seg, double u, double* q_out, double* J1)
{
    // value: kdelta = delta * u; exp; p0 * exp  (the tail of spline2_eval, operation for operation)
    const double kd[3] = {seg[4] * u, seg[5] * u, seg[6] * u};
    const double theta_sq = sqn3(kd[0] * kd[0], kd[1] * kd[1], kd[2] * kd[2]);
    double imag, real, p1c, p2c;            // p1c, p2c: coefficients of Jl(u delta) (only the Jacobian uses them)
    if (theta_sq < kSophusEps * kSophusEps) {                          // so3.hpp:594
        const double theta_po4 = theta_sq * theta_sq;
        imag = 0.5 - (1.0 / 48.0) * theta_sq + (1.0 / 3840.0) * theta_po4;
        real = 1.0 - (1.0 / 8.0) * theta_sq + (1.0 / 384.0) * theta_po4;
        const double n = sqrt(theta_sq);
        p1c = 0.5 * n; p2c = theta_sq * (1.0 / 6.0);
    } else {
        const double theta = sqrt(theta_sq);
        const double half = 0.5 * theta;
        double sh, ch;
        if (CALL) { const double2 sc = sin_cos_call(half); sh = sc.x; ch = sc.y; }
        else sin_cos_half(half, sh, ch);
        imag = sh / theta;
        real = ch;
        if (theta_sq > kSophusEps) { const double it2 = 2.0 * rcp_nr(theta); p1c = sh * sh * it2; p2c = 1.0 - sh * ch * it2; }     // (1 - cos n)/n, (n - sin n)/n
        else { p1c = 0.5 * theta; p2c = theta_sq * (1.0 / 6.0); }                                                    // sophus_utils.hpp:351 small branch
    }
    const double e[4] = {imag * kd[0], imag * kd[1], imag * kd[2], real};
    so3_mul(seg, e, q_out);
    const double r1 = seg[7], r2 = seg[11];
    const double alpha = p1c + r1 - p1c * r2 - p2c * r1, gamma = p2c + r2 + p1c * r1 - p2c * r2;
    rebuild_j1(u, u * alpha, u * gamma, seg + 8, J1);
}

__device__ __forceinline__ void project_jacobian(const double* rb, double fx, double fy, double* J23);

// EquirectangularCamera::projectToImage (include/utils/equirectangular_camera.h:18-45) chained with
// -[rb]x (event_pano_warper.cpp:62-65): pm (2) and J23 = dpm_drb * drb_ddrot (row-major 2x3).
// The projection alone, as a REAL function (noinline): its atan2 / asin carry ~40 fp64 polynomial constants, which the compiler
// hoists out of a loop and keeps in registers for the loop's whole life (fp64 literals cannot be encoded in VALU instructions
// on gfx9: the tiled warp kernel, whose waves loop over event groups, went from 88 to 190 VGPRs that way).  Behind a call the
// constants are materialised per call and die at the return.  Same expressions, same results as the inline form.
// (results by value: out-pointers to the caller's locals would travel through scratch memory)
__device__ __attribute__((noinline)) double2 project_angles_call(double x, double y, double z)
{
    const double phi = atan2(x, z);
    const double r2 = x * x + y * y + z * z;
    return make_double2(phi, asin(y / sqrt(r2)));
}


template <bool CALL = false>
__device__ __forceinline__ void project_chain(const double* rb, double fx, double fy, double cx, double cy,
                                              double* pm, double* J23)
{
    if (CALL) {
        const double2 a = project_angles_call(rb[0], rb[1], rb[2]);
        pm[0] = cx + a.x * fx;
        pm[1] = cy + a.y * fy;
        project_jacobian(rb, fx, fy, J23);
        return;
    }
    const double x = rb[0], y = rb[1], z = rb[2];
    const double phi = atan2(x, z);
    const double r2 = x * x + y * y + z * z;
    const double theta = asin(y / sqrt(r2));
    pm[0] = cx + phi * fx;
    pm[1] = cy + theta * fy;
    project_jacobian(rb, fx, fy, J23);
}

// Jacobian only from here on: contraction is allowed again (last-bit differences, tolerance 1e-5 relative in the north star).
#pragma clang fp contract(fast)
__device__ __forceinline__ void project_jacobian(const double* rb, double fx, double fy, double* J23)
{
    const double x = rb[0], y = rb[1], z = rb[2];
    // The Jacobian row formulas of equirectangular_camera.h:28-41 with their seven divisions folded into three reciprocals
    // (fp64 division is ~25 VALU instructions here and this kernel's arithmetic is not free):
    //   tmp1 = fx / ((1 + (x/z)^2) z) = fx z / (x^2 + z^2),   tmp1 * (x/z) = fx x / (x^2 + z^2),
    //   tmp2 = -fy / sqrt(1 - (y/rho)^2),  tmp3 = (y/rho) / rho^2  with 1/rho taken once.
    // Only the Jacobian is affected (last-bit differences); phi and theta — the rounded pixel — use the reference's expressions.
    // (round 2: the reciprocals are rcp_nr, and sqrt(1 - (y/rho)^2) = sqrt(x^2 + z^2) / rho shares 1/(x^2 + z^2) with the first row)
    const double d2 = x * x + z * z;
    const double rho = sqrt(d2 + y * y);
    const double inv_rho = rcp_nr(rho);
    const double Ydivrho = y * inv_rho;
    const double inv_d2 = rcp_nr(d2);
    const double inv_d = fx * inv_d2;
    const double tmp2 = -fy * rho * (sqrt(d2) * inv_d2);
    const double tmp3 = Ydivrho * inv_rho * inv_rho;
    const double Jp[6] = {z * inv_d, 0.0, -x * inv_d, tmp2 * tmp3 * x, tmp2 * (tmp3 * y - inv_rho), tmp2 * tmp3 * z};
    const double M[9] = {0, rb[2], -rb[1], -rb[2], 0, rb[0], rb[1], -rb[0], 0};
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            double s = 0;
#pragma unroll
            for (int k = 0; k < 3; ++k) s += Jp[3 * i + k] * M[3 * k + j];
            J23[3 * i + j] = s;
        }
}

}  // namespace emba
