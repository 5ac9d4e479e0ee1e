// tests/cpp/poisson_rule_test.cpp — emba_amd/csrc/poisson_rule.h (plain C++17, no HIP): the boundary argument's check, the wrapped column and divergence, and
// the closing step of the cyclic systems (C_W + (beta + 2) I) x = g — Thomas sweeps of T_{W-1} by the recurrence the kernels use (c_j = 1 / (beta - c_{j-1})),
// then poisson_wrap_pivot and poisson_wrap_close — against dense Gaussian elimination with partial pivoting.
// Built and run by tests/test_poisson_wrap_cpu.py.  Also the launch plan at its thresholds (the fold, the GEMM kernel and its loads, the sweeps' chunks
// and replay), and, with the argument `plan`, the plan of every case on stdin: tests/test_poisson_edge_cases_cpu.py compares it with its Python statement,
// as it does the GEMM forms' tile table, printed with the argument `tiles`.
//
// The bound.  The cyclic matrix is symmetric with eigenvalues beta + 2 cos(2 pi k / W), all in [beta - 2, beta + 2] and negative: its condition number is at
// most cond = (|beta| + 2) / (|beta| - 2).  Elimination with pivoting and the condensed Thomas solve are each backward stable to a few W eps on these
// diagonally dominant systems, so each solution is within 8 W eps cond of the true one, relative to its largest entry: the two differ by at most
// 16 W eps cond.  The residual of the rule's own solution does not see cond: at most 8 W eps (|beta| + 2) max|x|.
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <string>
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

static const char* form_name(GemmForm f) { return f == GemmForm::k128x128 ? "k128x128" : f == GemmForm::k64x128 ? "k64x128" : "k64x64"; }

// `plan`: lines of `H W n_cu gemm64 poisson boundary` on stdin -> the launch plan of each: the fold decision, every product as `M N K lda stride vec form`,
// and the sweeps as `Wt q replay` (the dense form has none).  tests/poisson_edge_cases.py prints the same from its own statement of the rule.
static int print_plans()
{
    int H, W, n_cu, gemm64, poisson, boundary;
    while (std::scanf("%d %d %d %d %d %d", &H, &W, &n_cu, &gemm64, &poisson, &boundary) == 6) {
        std::printf("case %d %d %d %d %d %d\nfold %d\n", H, W, n_cu, gemm64, poisson, boundary, poisson_folds(H, poisson) ? 1 : 0);
        PoissonProduct pr[4];
        const int n = poisson_products(H, W, poisson, pr);
        for (int k = 0; k < n; ++k)
            std::printf("product %d %d %d %ld %d %d %s\n", pr[k].M, pr[k].N, pr[k].K, pr[k].lda, pr[k].a_kstride, gemm_vec(pr[k].K, pr[k].N),
                        form_name(gemm_form(pr[k].M, pr[k].N, n_cu, gemm64)));
        if (poisson == 1) std::printf("sweep none\n");
        else {
            const int Wt = boundary == kPoissonWrapX ? W - 1 : W;
            std::printf("sweep %d %d %s\n", Wt, tri_chunk_len(Wt), tri_replay_from_table(Wt) ? "table" : "registers");
        }
    }
    return 0;
}

// `tiles`: per GEMM form `name block_rows block_columns threads b_doubles_per_thread`, from the one table the kernel's instantiations, gemm_form and
// gemm_tiles read.  tests/test_poisson_edge_cases_cpu.py compares it with TILE and THREAD_COLS of tests/poisson_edge_cases.py.
static int print_tiles()
{
    for (GemmForm f : {GemmForm::k64x64, GemmForm::k64x128, GemmForm::k128x128}) {
        const GemmTile t = gemm_tile(f);
        std::printf("%s %d %d %d %d\n", form_name(f), t.bm, t.bn, t.threads, t.b_per_thread);
    }
    return 0;
}

// ---- the launch plan at its thresholds
static void check_plan()
{
    // the fold: even H from 64, option poisson 0 only
    CHECK(!poisson_folds(62, 0) && !poisson_folds(63, 0) && poisson_folds(64, 0) && !poisson_folds(65, 0) && poisson_folds(66, 0) && poisson_folds(2048, 0));
    for (int H : {62, 63, 64, 66}) CHECK(!poisson_folds(H, 1) && !poisson_folds(H, 2));
    PoissonProduct pr[4];
    CHECK(poisson_products(66, 131, 0, pr) == 4 && pr[3].M == 131 && pr[3].N == 33 && pr[3].K == 33 && pr[3].lda == 66 && pr[3].a_kstride == 2);
    CHECK(poisson_products(62, 125, 0, pr) == 2 && pr[1].M == 125 && pr[1].N == 62 && pr[1].K == 62 && pr[1].lda == 62 && pr[1].a_kstride == 1);
    CHECK(poisson_products(66, 131, 2, pr) == 2 && pr[0].N == 66 && pr[0].a_kstride == 1);
    CHECK(poisson_products(66, 131, 1, pr) == 4 && pr[0].M == 66 && pr[0].N == 131 && pr[0].K == 131 && pr[0].lda == 131 && pr[1].K == 66 && pr[1].lda == 66);

    // 16-byte loads: K and N both even
    CHECK(gemm_vec(50, 50) == 1 && gemm_vec(33, 33) == 0 && gemm_vec(66, 131) == 0 && gemm_vec(131, 66) == 0 && gemm_vec(1026, 1026) == 1);

    // the kernel: tile counts either side of n_cu (128 x 128 tiles) and of 2 n_cu (64 x 128 tiles)
    for (int n_cu : {256, 304, 64}) {
        const int tn = 16, N = 128 * tn;                        // 16 tile columns of 128
        const int tm = n_cu / tn;                               // tm * tn = n_cu tiles of 128 x 128
        CHECK(tm * tn == n_cu);
        CHECK(gemm_form(128 * (tm - 1) + 1, N, n_cu, 0) == GemmForm::k128x128 && gemm_tiles(128 * (tm - 1) + 1, N, GemmForm::k128x128) == n_cu);
        CHECK(gemm_form(128 * (tm - 1), N, n_cu, 0) == GemmForm::k64x64);                     // n_cu - 16 tiles: one short, and the 64 x 128 count 2 (n_cu - 16) too
        CHECK(gemm_form(128 * tm, N - 128 + 1, n_cu, 0) == GemmForm::k128x128 && gemm_form(128 * tm, N - 128, n_cu, 0) == GemmForm::k64x64);
        const int tm2 = 2 * n_cu / tn;                          // tm2 * tn = 2 n_cu tiles of 64 x 128
        CHECK(gemm_form(64 * (tm2 - 1) + 1, N, n_cu, 1) == GemmForm::k64x128 && gemm_tiles(64 * (tm2 - 1) + 1, N, GemmForm::k64x128) == 2 * n_cu);
        CHECK(gemm_form(64 * (tm2 - 1), N, n_cu, 1) == GemmForm::k64x64 && gemm_tiles(64 * (tm2 - 1), N, GemmForm::k64x64) == 2L * (tm2 - 1) * tn);
        CHECK(gemm_form(64 * tm2, N - 128 + 1, n_cu, 1) == GemmForm::k64x128 && gemm_form(64 * tm2, N - 128, n_cu, 1) == GemmForm::k64x64);
        CHECK(gemm_form(1 << 20, 1 << 10, n_cu, 1) == GemmForm::k64x128);                      // option gemm64 never takes the 128-row kernel
        // ceil(M/64) <= 2 ceil(M/128): wherever the 64 x 128 count reaches 2 n_cu the 128 x 128 count reaches n_cu, so without the option the 64 x 128
        // kernel is never chosen
        for (int M = 1; M <= 8192; M += 61)
            for (int Nn = 1; Nn <= 8192; Nn += 67) CHECK(gemm_form(M, Nn, n_cu, 0) != GemmForm::k64x128);
    }
    CHECK(gemm_tiles(4097, 1025, GemmForm::k128x128) == 33 * 9 && gemm_tiles(4097, 1025, GemmForm::k64x128) == 65 * 9 && gemm_tiles(131, 33, GemmForm::k64x64) == 3);

    // the sweeps: chunk lengths, and the backward replay from registers up to W = 4096
    CHECK(kTriSys == 8 && kTriChunks == 128 && kTriMaxQ == 32);
    CHECK(tri_chunk_len(1) == 1 && tri_chunk_len(2) == 1 && tri_chunk_len(128) == 1 && tri_chunk_len(129) == 2 && tri_chunk_len(4096) == 32 && tri_chunk_len(4097) == 33);
    CHECK(tri_chunk_len(4224) == 33 && tri_chunk_len(4225) == 34 && tri_chunk_len(8192) == 64);
    CHECK(!tri_replay_from_table(2) && !tri_replay_from_table(4095) && !tri_replay_from_table(4096) && tri_replay_from_table(4097) && tri_replay_from_table(8192));
    // every row is in exactly one chunk, and the chunk index stays below kTriChunks
    for (int W : {2, 3, 47, 4096, 4097, 4224, 4225, 8192}) { const int q = tri_chunk_len(W); CHECK((long)q * kTriChunks >= W && (W - 1) / q < kTriChunks); }
}

int main(int argc, char** argv)
{
    if (argc > 1 && std::string(argv[1]) == "plan") return print_plans();
    if (argc > 1 && std::string(argv[1]) == "tiles") return print_tiles();
    check_plan();

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
