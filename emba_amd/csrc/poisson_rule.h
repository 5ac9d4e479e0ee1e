// emba_amd/csrc/poisson_rule.h — the boundary rules of the intensity panorama (render_host.h, poisson_kernels.h) as functions of plain values: the boundary
// argument's check, the smallest width a wrapped panorama may have, the divergence of a panorama whose columns wrap, and the closing step of the cyclic
// systems along W.  tests/poisson_wrap_ref.py is the same rule in numpy (its spectral form); include/emba_hip.h (EMBA_POISSON_WRAP_X) states it in words.
//
// The rule, once.  Boundary 0 is the reference's: zero Dirichlet values all round (poisson_kernels.h).  Boundary 1 wraps in x and keeps the zero rows beyond
// the poles:
//     F[i][j] = Gx[i][(j+1) mod W] - Gx[i][j] + Gy[i+1][j] - Gy[i][j]      (i < H-1, every j; row H-1 is 0)
//     M[i-1][j] + M[i+1][j] + M[i][(j-1) mod W] + M[i][(j+1) mod W] - 4 M[i][j] = F[i][j],      M[-1][:] = M[H][:] = 0
// After the DST-I along H the equation is, per H-frequency i, the cyclic system (C_W + lambda1[i] I) x = g with C_W the circulant second difference:
// x[j-1] + beta x[j] + x[j+1] = g[j], indices mod W, beta = -2 + lambda1[i] < -2.  Condensed on the last unknown t = x[W-1], the other W-1 unknowns solve the
// constant-diagonal tridiagonal system T_{W-1} = tridiag(1, beta, 1) the Dirichlet rule already solves:
//     T_{W-1} x[0:W-1] = g[0:W-1] - t (e_0 + e_{W-2})        =>   x[0:W-1] = p - t q,   p = T^-1 g[0:W-1],   q = T^-1 (e_0 + e_{W-2})
//     row W-1:  x[W-2] + beta t + x[0] = g[W-1]              =>   t = (g[W-1] - p[0] - p[W-2]) / (beta - q[0] - q[W-2])
// The denominator is the Schur complement of a non-singular matrix (every eigenvalue lambda1[i] - 4 sin^2(pi k / W) of the cyclic system is negative), so it
// does not vanish.  W = 3 is the smallest width at which column j has two different neighbours: below it the 5-point equation is not the one above.
//
// No HIP in here: plain C++17, so that tests/cpp/poisson_rule_test.cpp checks it on a CPU in milliseconds.  The arithmetic is compiled for the host and for
// the device, without contraction: the kernels and the CPU test run the same functions.
#pragma once

#if !defined(EMBA_RULE_HD)
#if defined(__HIPCC__)
#define EMBA_RULE_HD __host__ __device__
#else
#define EMBA_RULE_HD
#endif
#endif

namespace emba {

// ---- the boundary argument (the values of EMBA_POISSON_DIRICHLET / EMBA_POISSON_WRAP_X in include/emba_hip.h)
constexpr int kPoissonDirichlet = 0, kPoissonWrapX = 1;
constexpr int kPoissonWrapMinW = 3;
enum class PoissonBoundaryStatus { ok, unknown, too_narrow };
inline PoissonBoundaryStatus poisson_boundary_ok(int boundary, int pano_w)
{
    if (boundary != kPoissonDirichlet && boundary != kPoissonWrapX) return PoissonBoundaryStatus::unknown;
    if (boundary == kPoissonWrapX && pano_w < kPoissonWrapMinW) return PoissonBoundaryStatus::too_narrow;
    return PoissonBoundaryStatus::ok;
}

// ---- the wrapped divergence: the column to the right of j, and F from the four values it reads (the reference's association, left to right)
EMBA_RULE_HD inline int poisson_wrap_right(int j, int W) { return j + 1 == W ? 0 : j + 1; }
EMBA_RULE_HD inline double poisson_divergence(double gx_right, double gx, double gy_below, double gy) { return gx_right - gx + gy_below - gy; }

// ---- the closing step of one cyclic system: t from the three gathered values, then every other unknown
EMBA_RULE_HD inline double poisson_wrap_pivot(double g_last, double p_first, double p_last, double beta, double q_first, double q_last)
{
    return (g_last - p_first - p_last) / (beta - q_first - q_last);
}
EMBA_RULE_HD inline double poisson_wrap_close(double p, double t, double q)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    return p - t * q;
}

}  // namespace emba
