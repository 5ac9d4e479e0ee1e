// tests/cpp/poisson_rule_test.cpp — emba_amd/csrc/poisson_rule.h (plain C++17, no HIP): the boundary argument's check, the wrapped column and divergence, and
// the closing step of the cyclic systems (C_W + (beta + 2) I) x = g — Thomas sweeps of T_{W-1} by the recurrence the kernels use (c_j = 1 / (beta - c_{j-1})),
// then poisson_wrap_pivot and poisson_wrap_close — against dense Gaussian elimination with partial pivoting.
// Built and run by tests/test_poisson_wrap_cpu.py.
//
// The bound.  The cyclic matrix is symmetric with eigenvalues beta + 2 cos(2 pi k / W), all in [beta - 2, beta + 2] and negative: its condition number is at
// most cond = (|beta| + 2) / (|beta| - 2).  Elimination with pivoting and the condensed Thomas solve are each backward stable to a few W eps on these
// diagonally dominant systems, so each solution is within 8 W eps cond of the true one, relative to its largest entry: the two differ by at most
// 16 W eps cond.  The residual of the rule's own solution does not see cond: at most 8 W eps (|beta| + 2) max|x|.
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../emba_amd/csrc/poisson_rule.h"

using namespace emba;

static int g_fail = 0;
#define CHECK(x) do { if (!(x)) { std::printf("FAIL %s:%d  %s\n", __FILE__, __LINE__, #x); ++g_fail; } } while (0)

// x = T_n^-1 g, T_n = tridiag(1, beta, 1): emba_thomas_coef_kernel's factors and emba_tridiag_sweep_kernel's two recurrences
static std::vector<double> thomas(double beta, const std::vector<double>& g)
{
    const int n = (int)g.size();
    std::vector<double> cp(n), x(n);
    double c = 0.0, y = 0.0;
    for (int j = 0; j < n; ++j) { c = 1.0 / (beta - c); cp[j] = c; y = c * (g[j] - y); x[j] = y; }
    double nx = 0.0;
    for (int j = n - 1; j >= 0; --j) { nx = x[j] - cp[j] * nx; x[j] = nx; }
    return x;
}

// the cyclic system by the rule
static std::vector<double> solve_by_rule(double beta, const std::vector<double>& g, double* denominator)
{
    const int W = (int)g.size();
    std::vector<double> e(W - 1, 0.0);
    e[0] += 1.0; e[W - 2] += 1.0;                 // e_0 + e_{W-2}: at W - 1 >= 2 two different entries (kPoissonWrapMinW)
    const std::vector<double> q = thomas(beta, e), p = thomas(beta, std::vector<double>(g.begin(), g.end() - 1));
    *denominator = beta - q[0] - q[W - 2];
    const double t = poisson_wrap_pivot(g[W - 1], p[0], p[W - 2], beta, q[0], q[W - 2]);
    std::vector<double> x(W);
    for (int j = 0; j < W - 1; ++j) x[j] = poisson_wrap_close(p[j], t, q[j]);
    x[W - 1] = t;
    return x;
}

// the same system, dense, by elimination with partial pivoting
static std::vector<double> solve_dense(double beta, const std::vector<double>& g)
{
    const int W = (int)g.size();
    std::vector<double> A((size_t)W * W, 0.0), b = g;
    for (int j = 0; j < W; ++j) {
        A[(size_t)j * W + j] += beta;
        A[(size_t)j * W + (j + 1) % W] += 1.0;
        A[(size_t)j * W + (j + W - 1) % W] += 1.0;
    }
    for (int k = 0; k < W; ++k) {
        int piv = k;
        for (int r = k + 1; r < W; ++r) if (std::fabs(A[(size_t)r * W + k]) > std::fabs(A[(size_t)piv * W + k])) piv = r;
        if (piv != k) { for (int cidx = 0; cidx < W; ++cidx) std::swap(A[(size_t)k * W + cidx], A[(size_t)piv * W + cidx]); std::swap(b[k], b[piv]); }
        for (int r = k + 1; r < W; ++r) {
            const double f = A[(size_t)r * W + k] / A[(size_t)k * W + k];
            if (f == 0.0) continue;
            for (int cidx = k; cidx < W; ++cidx) A[(size_t)r * W + cidx] -= f * A[(size_t)k * W + cidx];
            b[r] -= f * b[k];
        }
    }
    std::vector<double> x(W);
    for (int k = W - 1; k >= 0; --k) {
        double s = b[k];
        for (int cidx = k + 1; cidx < W; ++cidx) s -= A[(size_t)k * W + cidx] * x[cidx];
        x[k] = s / A[(size_t)k * W + k];
    }
    return x;
}

static double max_abs(const std::vector<double>& v) { double m = 0.0; for (double a : v) m = std::fmax(m, std::fabs(a)); return m; }

int main()
{
    // ---- the boundary argument
    CHECK(kPoissonDirichlet == 0 && kPoissonWrapX == 1 && kPoissonWrapMinW == 3);
    for (int W : {1, 2, 3, 4, 2048}) {
        CHECK(poisson_boundary_ok(kPoissonDirichlet, W) == PoissonBoundaryStatus::ok);
        CHECK(poisson_boundary_ok(kPoissonWrapX, W) == (W >= 3 ? PoissonBoundaryStatus::ok : PoissonBoundaryStatus::too_narrow));
        for (int b : {-1, 2, 3, 1 << 30, INT32_MIN}) CHECK(poisson_boundary_ok(b, W) == PoissonBoundaryStatus::unknown);
    }

    // ---- the wrapped column and the divergence's association
    for (int W : {3, 4, 129}) {
        for (int j = 0; j + 1 < W; ++j) CHECK(poisson_wrap_right(j, W) == j + 1);
        CHECK(poisson_wrap_right(W - 1, W) == 0);
    }
    CHECK(poisson_divergence(1e16, 1e16, 1.0, 0.25) == 0.75 && poisson_divergence(0.1, 0.2, 0.3, 0.4) == ((0.1 - 0.2) + 0.3) - 0.4);

    // ---- the closing rule against dense elimination
    uint64_t lcg = 12345;
    auto rnd = [&]() { lcg = lcg * 6364136223846793005ull + 1442695040888963407ull; return (double)(int64_t)(lcg >> 11) / (double)(1ull << 52) - 1.0; };      // [-1, 1)
    for (int W : {3, 4, 5, 129, 130})
        for (double beta : {-2.0 - 1e-6, -2.0 - 1e-3, -2.1, -3.0, -4.0, -6.0}) {
            const double cond = (std::fabs(beta) + 2.0) / (std::fabs(beta) - 2.0);
            double worst = 0.0, worst_res = 0.0, min_den = 1e300;
            for (int trial = 0; trial < 6; ++trial) {
                std::vector<double> g(W, 0.0);
                if (trial == 0) g[0] = 1.0;                         // the unit vectors at the three places the condensation treats differently
                else if (trial == 1) g[W - 2] = 1.0;
                else if (trial == 2) g[W - 1] = 1.0;
                else if (trial == 3) for (double& v : g) v = 1.0;   // the constant: x = 1 / (beta + 2), the worst-conditioned direction
                else for (double& v : g) v = rnd();
                double den = 0.0;
                const std::vector<double> x = solve_by_rule(beta, g, &den), xd = solve_dense(beta, g);
                min_den = std::fmin(min_den, std::fabs(den));
                CHECK(den < 0.0);                                    // the Schur complement of a negative definite matrix
                const double scale = max_abs(xd);
                double d = 0.0, res = 0.0;
                for (int j = 0; j < W; ++j) {
                    d = std::fmax(d, std::fabs(x[j] - xd[j]));
                    res = std::fmax(res, std::fabs(x[(j + W - 1) % W] + beta * x[j] + x[(j + 1) % W] - g[j]));
                }
                worst = std::fmax(worst, d / scale);
                worst_res = std::fmax(worst_res, res / ((std::fabs(beta) + 2.0) * max_abs(x)));
                if (trial == 3) CHECK(std::fabs(x[W / 2] * (beta + 2.0) - 1.0) <= 8.0 * W * DBL_EPSILON * cond);
            }
            std::printf("W=%d beta=%.17g  |rule - dense| / max|x| = %.3e (bound %.3e)  residual %.3e (bound %.3e)  min|denominator| = %.3e\n", W, beta, worst,
                        16.0 * W * DBL_EPSILON * cond, worst_res, 8.0 * W * DBL_EPSILON, min_den);
            CHECK(worst <= 16.0 * W * DBL_EPSILON * cond);
            CHECK(worst_res <= 8.0 * W * DBL_EPSILON);
        }

    if (g_fail) { std::printf("%d checks failed\n", g_fail); return 1; }
    std::printf("OK poisson_rule\n");
    return 0;
}
