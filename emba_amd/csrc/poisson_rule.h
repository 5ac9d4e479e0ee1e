// emba_amd/csrc/poisson_rule.h — the boundary rules of the intensity panorama (poisson_host.h, poisson_kernels.h) as functions of plain values: the boundary
// argument's check, the smallest width a wrapped panorama may have, the divergence of a panorama whose columns wrap, and the closing step of the cyclic
// systems along W.  tests/poisson_wrap_ref.py is the same rule in numpy (its spectral form); include/emba_hip.h (EMBA_POISSON_WRAP_X) states it in words.
// Below them the launch plan of the solve: the fold of the DST, the GEMM kernel of a product and its loads, the chunks of the Thomas sweeps.
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

// ---- the launch plan of the Fourier form (poisson_host.h): whether the DST along H folds, which GEMM kernel a product runs on and how it loads its
// operands, how the Thomas sweeps cut the W direction and how the backward sweep replays a chunk.  tests/poisson_edge_cases.py states the same in Python.

// The DST-I of even length H as two half-size products and a butterfly (poisson_kernels.h, emba_sine_folded_kernel).  Option poisson: 1 dense sine
// transforms on both axes, 2 no folding (comparison forms).
constexpr int kPoissonFoldMinH = 64;
inline bool poisson_folds(int H, int opt_poisson)
{
    const bool dense = opt_poisson == 1;
    return !dense && (H % 2 == 0) && H >= kPoissonFoldMinH && opt_poisson != 2;
}

// The three forms of the fp64 MFMA GEMM kernel (poisson_kernels.h, emba_dgemm_kernel<BM, BN, THREADS>) and the block tile of each, stated here once:
// the kernel's instantiations, the choice of a form and the grid all read gemm_tile.  The k-tile is 16 for all; a thread stages 16 BN / THREADS doubles of B.
constexpr int kGemmBK = 16;
enum class GemmForm { k64x64, k64x128, k128x128 };
struct GemmTile { int bm, bn, threads, b_per_thread; };      // block rows, block columns, threads, B doubles a thread stages per k-tile
constexpr GemmTile gemm_tile_of(int bm, int bn, int threads) { return GemmTile{bm, bn, threads, kGemmBK * bn / threads}; }
constexpr GemmTile gemm_tile(GemmForm f)
{
    return f == GemmForm::k128x128 ? gemm_tile_of(128, 128, 512) : f == GemmForm::k64x128 ? gemm_tile_of(64, 128, 256) : gemm_tile_of(64, 64, 256);
}
// tiles a form's launch covers (the grid is this, rounded up to the 8 XCDs)
inline long gemm_tiles(int M, int N, GemmForm f)
{
    const GemmTile t = gemm_tile(f);
    return (long)((M + t.bm - 1) / t.bm) * ((N + t.bn - 1) / t.bn);
}
// The 128 x 128 form where the output gives every CU a tile of that size (a third less operand traffic per flop); else the 64 x 128 form where it
// gives every CU two; else twice the blocks of 64 x 64.  Option gemm64 keeps the 64-row forms (comparison form).
inline GemmForm gemm_form(int M, int N, int n_cu, int opt_gemm64)
{
    if (gemm_tiles(M, N, GemmForm::k128x128) >= (long)n_cu && !opt_gemm64) return GemmForm::k128x128;
    if (gemm_tiles(M, N, GemmForm::k64x128) >= 2L * n_cu) return GemmForm::k64x128;
    return GemmForm::k64x64;
}
// 16-B operand loads on interior tiles: every row of A (lda = K or an even multiple of it) and of B (ldb = N) then starts 16-B aligned
inline int gemm_vec(int K, int N) { return ((K & 1) == 0 && (N & 1) == 0) ? 1 : 0; }

// The products of one solve in launch order, as poisson_host.h writes them out with their operands: C (M x N) = A (M x K) B (K x N), A's rows lda apart and
// its reduction index reading every a_kstride-th column.  Dense: S_H and S_W products on the plane itself.  Otherwise everything runs on the transposed
// plane (W x H): two DSTs along H, each one product, or folded two half-size products on the even- and odd-indexed columns.  Returns how many.
struct PoissonProduct { int M, N, K; long lda; int a_kstride; };
inline int poisson_products(int H, int W, int opt_poisson, PoissonProduct out[4])
{
    if (opt_poisson == 1) {
        out[0] = out[2] = PoissonProduct{H, W, W, W, 1};
        out[1] = out[3] = PoissonProduct{H, W, H, H, 1};
        return 4;
    }
    if (poisson_folds(H, opt_poisson)) {
        for (int k = 0; k < 4; ++k) out[k] = PoissonProduct{W, H / 2, H / 2, H, 2};
        return 4;
    }
    out[0] = out[1] = PoissonProduct{W, H, H, H, 1};
    return 2;
}

// The Thomas sweeps: a workgroup takes kTriSys systems and cuts the W rows into kTriChunks chunks of tri_chunk_len(W) (the last live one ragged, those
// beyond it empty).  The backward sweep replays a chunk with its factors kept in registers, up to kTriMaxQ of them; longer chunks read the factor table.
constexpr int kTriSys = 8, kTriChunks = 128;
constexpr int kTriMaxQ = 32;    // W <= kTriChunks * kTriMaxQ = 4096 replays from registers
EMBA_RULE_HD inline int tri_chunk_len(int W) { return (W + kTriChunks - 1) / kTriChunks; }
EMBA_RULE_HD inline bool tri_replay_from_table(int W) { return tri_chunk_len(W) > kTriMaxQ; }

}  // namespace emba
