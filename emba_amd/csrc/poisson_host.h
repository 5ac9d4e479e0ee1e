// emba_amd/csrc/poisson_host.h — f3, the intensity panorama from the gradient map, as host code over the kernels of poisson_kernels.h:
// emba_reconstruct_intensity[_bc], the phases of the solve — the once-per-context tables, the planes' upload, the product launcher, the DST along H, the
// dense form, the Fourier form with its wrapped closing — and poisson_solve, which runs them and says where the panorama lies on the device: the public
// entry, the record_data images (render_host.h) and the sensor views (view_host.h) all go through it, and nothing outside this file names the plane's
// buffer.  What is plain arithmetic — the boundary rule, whether the DST folds, the GEMM form of a product and its tile, the sweeps' chunks — is decided in
// poisson_rule.h; here are the buffers (emba_ctx::poisson), the launches and the C ABI.
// Part of emba_hip.hip's translation unit, included by it below solve_host.h (the device code keeps the order of first use) and above render_host.h.
#pragma once
#include "context.h"

using namespace emba;

namespace {

#define POISSON_TRY(call) do { if (const emba_status st_ = (call)) return st_; } while (0)

// the boundary argument of the _bc entry points (poisson_rule.h): refused before anything is allocated, launched or written
emba_status poisson_boundary_check(emba_ctx* c, int boundary)
{
    switch (poisson_boundary_ok(boundary, c->W)) {
    case PoissonBoundaryStatus::unknown:
        return fail(c, EMBA_ERR_INVALID_ARG, "boundary=%d: EMBA_POISSON_DIRICHLET (%d) or EMBA_POISSON_WRAP_X (%d)", boundary, EMBA_POISSON_DIRICHLET, EMBA_POISSON_WRAP_X);
    case PoissonBoundaryStatus::too_narrow:
        return fail(c, EMBA_ERR_INVALID_ARG, "boundary EMBA_POISSON_WRAP_X needs pano_w >= %d (pano_w=%d)", kPoissonWrapMinW, c->W);
    case PoissonBoundaryStatus::ok: break;
    }
    if (boundary == EMBA_POISSON_WRAP_X && c->opt_poisson == 1)
        return fail(c, EMBA_ERR_STATE, "boundary EMBA_POISSON_WRAP_X with option poisson = 1: the dense sine transforms along W have no wrapped form");
    return EMBA_OK;
}

// The form of one solve.  dense (option poisson = 1): both axes by sine-matrix products, four GEMMs — the round-1/2 form, kept for comparison.  Otherwise
// the Fourier form: analysis along H only and tridiagonal solves along W (poisson_kernels.h) — a third of the arithmetic, same solution to rounding —
// with the DST folded or not (poisson_rule.h: poisson_folds), under either boundary (wrap: never dense, poisson_boundary_check).
struct PoissonForm { bool wrap, dense, fold; };

// the two Thomas sweeps over the first Wt rows of a transposed plane, in place: (T_Wt + lambda1[i] I) x = v[:, i] for every H-frequency i
void poisson_sweeps(emba_ctx* c, double* v, int Wt)
{
    const PoissonBuffers& B = c->poisson;
    const dim3 grid((unsigned)((c->H + kTriSys - 1) / kTriSys)), block(kTriSys * kTriChunks);
    hipLaunchKernelGGL(emba_tridiag_sweep_kernel<false>, grid, block, 0, c->stream, B.thomas.as<double>(), B.lamH.as<double>(), v, c->H, Wt);
    hipLaunchKernelGGL(emba_tridiag_sweep_kernel<true>, grid, block, 0, c->stream, B.thomas.as<double>(), B.lamH.as<double>(), v, c->H, Wt);
}

// The two scratch planes every form needs and the once-per-context tables this form needs, each table made when the buffer it lies in is new.
emba_status poisson_tables(emba_ctx* c, PoissonForm f)
{
    hipStream_t s = c->stream;
    PoissonBuffers& B = c->poisson;
    const int H = c->H, W = c->W;
    const size_t npix = c->npix;
    bool fresh = false;
    // S_H and its eigenvalues
    POISSON_TRY(ensure<double>(c, B.lamH, (size_t)H));
    POISSON_TRY(ensure<double>(c, B.F, npix));
    POISSON_TRY(ensure<double>(c, B.T, npix));
    POISSON_TRY(ensure<double>(c, B.SH, (size_t)H * H, &fresh));
    if (fresh) {
        hipLaunchKernelGGL(emba_sine_matrix_kernel, dim3((unsigned)(((size_t)H * H + 255) / 256)), dim3(256), 0, s, H, B.SH.as<double>());
        hipLaunchKernelGGL(emba_dirichlet_eigen_kernel, dim3((H + 255) / 256), dim3(256), 0, s, H, B.lamH.as<double>());
    }
    if (f.dense) {      // S_W and its eigenvalues
        POISSON_TRY(ensure<double>(c, B.lamW, (size_t)W));
        POISSON_TRY(ensure<double>(c, B.SW, (size_t)W * W, &fresh));
        if (fresh) {
            hipLaunchKernelGGL(emba_sine_matrix_kernel, dim3((unsigned)(((size_t)W * W + 255) / 256)), dim3(256), 0, s, W, B.SW.as<double>());
            hipLaunchKernelGGL(emba_dirichlet_eigen_kernel, dim3((W + 255) / 256), dim3(256), 0, s, W, B.lamW.as<double>());
        }
    } else {            // Thomas factors of T_W + lambda1[i] I for every H-frequency i: W x H doubles
        POISSON_TRY(ensure<double>(c, B.thomas, npix, &fresh));
        if (fresh) hipLaunchKernelGGL(emba_thomas_coef_kernel, dim3((H + 63) / 64), dim3(64), 0, s, B.lamH.as<double>(), H, W, B.thomas.as<double>());
    }
    if (f.wrap) {       // q = T_{W-1}^-1 (e_0 + e_{W-2}) for every H-frequency i (W x H doubles) by the sweeps of the solve itself
        POISSON_TRY(ensure<double>(c, B.wrapq, npix, &fresh));
        if (fresh) {
            hipLaunchKernelGGL(emba_wrap_unit_kernel, dim3(nblocks(npix)), dim3(256), 0, s, H, W, B.wrapq.as<double>());
            poisson_sweeps(c, B.wrapq.as<double>(), W - 1);
        }
    }
    if (f.fold) {       // S_H folded by its symmetry
        POISSON_TRY(ensure<double>(c, B.Sfold, (size_t)H * H / 2, &fresh));
        if (fresh) hipLaunchKernelGGL(emba_sine_folded_kernel, dim3((unsigned)(((size_t)H * H / 2 + 255) / 256)), dim3(256), 0, s, H, B.Sfold.as<double>());
    }
    return EMBA_OK;
}

// the gradient planes of a solve: the resident map's, or the caller's, uploaded
emba_status poisson_planes(emba_ctx* c, const double* Gx_host, const double* Gy_host, const double*& gx, const double*& gy)
{
    gx = c->map.Gx(); gy = c->map.Gy();
    if (!Gx_host) return EMBA_OK;
    PoissonBuffers& B = c->poisson;
    POISSON_TRY(ensure<double>(c, B.Gx, c->npix));
    POISSON_TRY(ensure<double>(c, B.Gy, c->npix));
    HIP_TRY(c, hipMemcpyAsync(B.Gx.as<double>(), Gx_host, c->npix * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(B.Gy.as<double>(), Gy_host, c->npix * sizeof(double), hipMemcpyHostToDevice, c->stream));
    gx = B.Gx.as<double>(); gy = B.Gy.as<double>();
    return EMBA_OK;
}

// one form of the GEMM kernel on its tile (poisson_rule.h: gemm_tile)
template <GemmForm F>
void launch_gemm(const GemmParams& p, unsigned grid, hipStream_t s)
{
    constexpr GemmTile t = gemm_tile(F);
    hipLaunchKernelGGL((emba_dgemm_kernel<t.bm, t.bn, t.threads>), dim3(grid), dim3(t.threads), 0, s, p);
}

// C (M x N) = A (M x K) B (K x N) with an epilogue (GemmParams): the form, the grid and the loads by poisson_rule.h.  lda = 0: K
void poisson_gemm(emba_ctx* c, const double* A, const double* B, double* C, int M, int N, int K, int epilogue, double inv_norm, long lda = 0, int a_kstride = 1,
                  int a_koff = 0)
{
    GemmParams p{};
    p.A = A; p.B = B; p.C = C; p.M = M; p.N = N; p.K = K; p.lda = lda ? lda : K; p.ldb = N; p.ldc = N;
    p.a_kstride = a_kstride; p.a_koff = a_koff;
    p.epilogue = epilogue; p.inv_norm = inv_norm;
    p.lam1 = c->poisson.lamH.as<double>(); p.lam2 = c->poisson.lamW.as<double>();
    p.vec = gemm_vec(K, N);
    const GemmForm form = gemm_form(M, N, c->n_cu, c->opt_gemm64);
    const unsigned grid = (unsigned)grid8(gemm_tiles(M, N, form));
    switch (form) {
    case GemmForm::k128x128: launch_gemm<GemmForm::k128x128>(p, grid, c->stream); break;
    case GemmForm::k64x128: launch_gemm<GemmForm::k64x128>(p, grid, c->stream); break;
    case GemmForm::k64x64: launch_gemm<GemmForm::k64x64>(p, grid, c->stream); break;
    }
}

// DST-I along H of every row of a transposed plane: src (W x H) -> dst, times scale.  Unfolded: one product with S_H.  Folded: two half-size products on
// the even- and odd-indexed inputs, [E | O] (W x H/2 each) in the EO plane, and a butterfly — which writes dst as W x H, or with transposed_out TRANSPOSED
// (H x W), saving the solve its last transpose pass.  Unfolded, dst is W x H whatever is asked.
void poisson_dst_rows(emba_ctx* c, PoissonForm f, const double* src, double* dst, double scale, bool transposed_out)
{
    const PoissonBuffers& B = c->poisson;
    const int H = c->H, W = c->W;
    if (!f.fold) { poisson_gemm(c, src, B.SH.as<double>(), dst, W, H, H, 2, scale); return; }
    const int h = H / 2;
    double* E = B.EO.as<double>(); double* O = E + (size_t)W * h;
    poisson_gemm(c, src, B.Sfold.as<double>(), E, W, h, h, 0, 1.0, H, 2, 0);
    poisson_gemm(c, src, B.Sfold.as<double>() + (size_t)h * h, O, W, h, h, 0, 1.0, H, 2, 1);
    if (transposed_out) hipLaunchKernelGGL(emba_dst_butterfly_T_kernel, dim3((h + 31) / 32, (W + 31) / 32), dim3(256), 0, c->stream, E, O, W, H, scale, dst);
    else hipLaunchKernelGGL(emba_dst_butterfly_kernel, dim3((unsigned)(((size_t)W * h + 255) / 256)), dim3(256), 0, c->stream, E, O, W, H, scale, dst);
}

// The dense form: rhs -> eigenvector space, solve, back (laplace.cpp:633-758):  M = S_H ((S_H F S_W) o C) S_W, left in the F plane
void poisson_dense(emba_ctx* c, const double* gx, const double* gy)
{
    const PoissonBuffers& B = c->poisson;
    const int H = c->H, W = c->W;
    double *F = B.F.as<double>(), *T = B.T.as<double>();
    hipLaunchKernelGGL(emba_divergence_kernel, dim3((unsigned)((c->npix + 255) / 256)), dim3(256), 0, c->stream, gx, gy, H, W, F);
    const double inv_norm = 1.0 / (4.0 * ((double)(H + 1) * (double)(W + 1)));   // fft_norm, laplace.cpp:648
    poisson_gemm(c, F, B.SW.as<double>(), T, H, W, W, 0, 1.0);            // T = F S_W
    poisson_gemm(c, B.SH.as<double>(), T, F, H, W, H, 1, inv_norm);       // U = (S_H T / fft_norm) / (lambda1 + lambda2)
    poisson_gemm(c, F, B.SW.as<double>(), T, H, W, W, 0, 1.0);            // T = U S_W
    poisson_gemm(c, B.SH.as<double>(), T, F, H, W, H, 0, 1.0);            // M = S_H T
}

// The Fourier form, on the transposed plane (W x H):  F^T -> (S_H F)^T -> per H-frequency i the systems along W -> M^T = X^T S_H / (2 (H+1)) -> M, left in the
// F plane.  Wrapped: the cyclic systems condensed on x[W-1] (poisson_rule.h) — the same sweeps over the first W-1 rows give p, then t per system and
// x = p - t q.
emba_status poisson_fourier(emba_ctx* c, PoissonForm f, const double* gx, const double* gy)
{
    hipStream_t s = c->stream;
    PoissonBuffers& B = c->poisson;
    const int H = c->H, W = c->W;
    if (f.fold) POISSON_TRY(ensure<double>(c, B.EO, c->npix));
    double *F = B.F.as<double>(), *T = B.T.as<double>();
    const dim3 tg((W + 31) / 32, (H + 31) / 32), tgT((H + 31) / 32, (W + 31) / 32);
    if (f.wrap) hipLaunchKernelGGL(emba_divergence_T_kernel<true>, tg, dim3(256), 0, s, gx, gy, H, W, T);      // F^T (W x H), straight from the gradient maps
    else hipLaunchKernelGGL(emba_divergence_T_kernel<false>, tg, dim3(256), 0, s, gx, gy, H, W, T);
    poisson_dst_rows(c, f, T, F, 1.0, false);                                                                  // (S_H F)^T = F^T S_H
    poisson_sweeps(c, F, f.wrap ? W - 1 : W);                                                                  // (T_W + lambda1[i] I) x = g, per i
    if (f.wrap) {
        hipLaunchKernelGGL(emba_wrap_pivot_kernel, dim3((H + 255) / 256), dim3(256), 0, s, (const double*)B.wrapq.as<double>(), (const double*)B.lamH.as<double>(), F, H, W);
        hipLaunchKernelGGL(emba_wrap_close_kernel, dim3(nblocks((size_t)H * (W - 1))), dim3(256), 0, s, (const double*)B.wrapq.as<double>(), F, H, W);
    }
    // M^T = X^T S_H / (2 (H+1)).  Folded: the butterfly writes M itself into the F plane (its input X^T is dead once E and O exist)
    const double scale = 1.0 / (2.0 * (double)(H + 1));
    if (f.fold) poisson_dst_rows(c, f, F, F, scale, true);
    else {
        poisson_dst_rows(c, f, F, T, scale, false);
        hipLaunchKernelGGL(emba_transpose_kernel, tgT, dim3(256), 0, s, (const double*)T, W, H, F);             // M
    }
    return EMBA_OK;
}

// One solve: the checks of the public entry, the phases above, the copy to M_host where asked for, one wait for the stream.  *M_dev (where asked for): the
// panorama on the device (H x W), valid until the next solve on this context.
emba_status poisson_solve(emba_ctx* c, const double* Gx_host, const double* Gy_host, double* M_host, int boundary, const double** M_dev)
{
    POISSON_TRY(poisson_boundary_check(c, boundary));
    if ((Gx_host == nullptr) != (Gy_host == nullptr)) return fail(c, EMBA_ERR_INVALID_ARG, "pass both Gx and Gy, or neither");
    if (!Gx_host && !c->map.state().resident()) return fail(c, EMBA_ERR_STATE, "no map resident");
    HIP_TRY(c, hipSetDevice(c->device));
    const PoissonForm f{boundary == EMBA_POISSON_WRAP_X, c->opt_poisson == 1, poisson_folds(c->H, c->opt_poisson)};
    POISSON_TRY(poisson_tables(c, f));
    const double *gx = nullptr, *gy = nullptr;
    POISSON_TRY(poisson_planes(c, Gx_host, Gy_host, gx, gy));
    if (f.dense) poisson_dense(c, gx, gy);
    else POISSON_TRY(poisson_fourier(c, f, gx, gy));
    HIP_TRY(c, hipGetLastError());
    const double* M = c->poisson.F.as<double>();
    if (M_host) HIP_TRY(c, hipMemcpyAsync(M_host, M, c->npix * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    c->spun = false; c->knots_in_flight = false;
    if (M_dev) *M_dev = M;
    return EMBA_OK;
}

}  // namespace

extern "C" emba_status emba_reconstruct_intensity_bc(emba_ctx* c, const double* Gx_host, const double* Gy_host, double* M_host, int boundary)
{
    if (!c) return EMBA_ERR_INVALID_ARG;
    return poisson_solve(c, Gx_host, Gy_host, M_host, boundary, nullptr);
}

extern "C" emba_status emba_reconstruct_intensity(emba_ctx* c, const double* Gx_host, const double* Gy_host, double* M_host)
{
    return emba_reconstruct_intensity_bc(c, Gx_host, Gy_host, M_host, EMBA_POISSON_DIRICHLET);
}
