// emba_amd/csrc/render_host.h — f3, the intensity panorama from the gradient map (poisson_kernels.h), and the reference's record_data map images
// (render_kernels.h): emba_reconstruct_intensity[_bc], emba_render_map_images[_bc], emba_normalize_robust.  The boundary rule: poisson_rule.h.
// Part of emba_hip.hip's translation unit, included below solve_host.h (the device code keeps the order of first use) and transfer_host.h (d2h_pageable).
#pragma once
#include "context.h"

using namespace emba;

// ---- f3: intensity panorama from the gradient map ---------------------------------------------------------------------------
namespace {

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

}  // namespace

extern "C" emba_status emba_reconstruct_intensity_bc(emba_ctx* c, const double* Gx_host, const double* Gy_host, double* M_host, int boundary)
{
    if (!c) return EMBA_ERR_INVALID_ARG;
    emba_status st;
    if ((st = poisson_boundary_check(c, boundary))) return st;
    const bool wrap = boundary == EMBA_POISSON_WRAP_X;
    if ((Gx_host == nullptr) != (Gy_host == nullptr)) return fail(c, EMBA_ERR_INVALID_ARG, "pass both Gx and Gy, or neither");
    if (!Gx_host && !c->map.state().resident()) return fail(c, EMBA_ERR_STATE, "no map resident");
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t s = c->stream;
    const int H = c->H, W = c->W;
    const size_t npix = c->npix;
    // option poisson = 1 (dense): both axes by sine-matrix products (four GEMMs: the round-1/2 form, kept for comparison); default: Fourier analysis
    // along H only + tridiagonal solves along W (poisson_kernels.h) — a third of the arithmetic, same solution to rounding.
    const bool dense = c->opt_poisson == 1;      // option poisson: 1 dense sine transforms, 2 no folding (comparison forms)
    // first use: S_H, its eigenvalues, two scratch planes (each set of constants is computed when the buffer it ends with is new)
    bool fresh = false;
    if ((st = ensure<double>(c, c->d_lamH, (size_t)H)) || (st = ensure<double>(c, c->d_pF, npix)) || (st = ensure<double>(c, c->d_pT, npix)) ||
        (st = ensure<double>(c, c->d_SH, (size_t)H * H, &fresh)))
        return st;
    if (fresh) {
        hipLaunchKernelGGL(emba_sine_matrix_kernel, dim3((unsigned)(((size_t)H * H + 255) / 256)), dim3(256), 0, s, H, c->d_SH.as<double>());
        hipLaunchKernelGGL(emba_dirichlet_eigen_kernel, dim3((H + 255) / 256), dim3(256), 0, s, H, c->d_lamH.as<double>());
    }
    if (dense && ((st = ensure<double>(c, c->d_lamW, (size_t)W)) || (st = ensure<double>(c, c->d_SW, (size_t)W * W, &fresh)))) return st;
    if (dense && fresh) {
        hipLaunchKernelGGL(emba_sine_matrix_kernel, dim3((unsigned)(((size_t)W * W + 255) / 256)), dim3(256), 0, s, W, c->d_SW.as<double>());
        hipLaunchKernelGGL(emba_dirichlet_eigen_kernel, dim3((W + 255) / 256), dim3(256), 0, s, W, c->d_lamW.as<double>());
    }
    if (!dense && (st = ensure<double>(c, c->d_thomas, npix, &fresh))) return st;
    if (!dense && fresh) {   // Thomas factors of T_W + lambda1[i] I for every H-frequency i: W x H doubles, once
        hipLaunchKernelGGL(emba_thomas_coef_kernel, dim3((H + 63) / 64), dim3(64), 0, s, c->d_lamH.as<double>(), H, W, c->d_thomas.as<double>());
    }
    // boundary EMBA_POISSON_WRAP_X: q = T_{W-1}^-1 (e_0 + e_{W-2}) for every H-frequency i (W x H doubles, once) by the sweeps of the solve itself
    if (wrap && (st = ensure<double>(c, c->d_wrapq, npix, &fresh))) return st;
    if (wrap && fresh) {
        const unsigned tb = (unsigned)((H + kTriSys - 1) / kTriSys);
        hipLaunchKernelGGL(emba_wrap_unit_kernel, dim3(nblocks(npix)), dim3(256), 0, s, H, W, c->d_wrapq.as<double>());
        hipLaunchKernelGGL(emba_tridiag_sweep_kernel<false>, dim3(tb), dim3(kTriSys * kTriChunks), 0, s, c->d_thomas.as<double>(), c->d_lamH.as<double>(), c->d_wrapq.as<double>(), H, W - 1);
        hipLaunchKernelGGL(emba_tridiag_sweep_kernel<true>, dim3(tb), dim3(kTriSys * kTriChunks), 0, s, c->d_thomas.as<double>(), c->d_lamH.as<double>(), c->d_wrapq.as<double>(), H, W - 1);
    }
    const bool fold = poisson_folds(H, c->opt_poisson);      // poisson_rule.h
    if (fold && (st = ensure<double>(c, c->d_Sfold, (size_t)H * H / 2, &fresh))) return st;
    if (fold && fresh) {
        hipLaunchKernelGGL(emba_sine_folded_kernel, dim3((unsigned)(((size_t)H * H / 2 + 255) / 256)), dim3(256), 0, s, H, c->d_Sfold.as<double>());
    }
    const double *gx = c->map.Gx(), *gy = c->map.Gy();
    if (Gx_host) {
        if ((st = ensure<double>(c, c->d_pGx, npix)) || (st = ensure<double>(c, c->d_pGy, npix))) return st;
        HIP_TRY(c, hipMemcpyAsync(c->d_pGx.as<double>(), Gx_host, npix * sizeof(double), hipMemcpyHostToDevice, s));
        HIP_TRY(c, hipMemcpyAsync(c->d_pGy.as<double>(), Gy_host, npix * sizeof(double), hipMemcpyHostToDevice, s));
        gx = c->d_pGx.as<double>(); gy = c->d_pGy.as<double>();
    }
    if (dense) hipLaunchKernelGGL(emba_divergence_kernel, dim3((unsigned)((npix + 255) / 256)), dim3(256), 0, s, gx, gy, H, W, c->d_pF.as<double>());
    auto gemm = [&](const double* A, const double* B, double* C, int M, int N, int K, int epilogue, double inv_norm, long lda = 0, int a_kstride = 1, int a_koff = 0) {
        GemmParams p{};
        p.A = A; p.B = B; p.C = C; p.M = M; p.N = N; p.K = K; p.lda = lda ? lda : K; p.ldb = N; p.ldc = N;
        p.a_kstride = a_kstride; p.a_koff = a_koff;
        p.epilogue = epilogue; p.inv_norm = inv_norm;
        p.lam1 = c->d_lamH.as<double>(); p.lam2 = c->d_lamW.as<double>();
        p.vec = gemm_vec(K, N);
        const GemmForm form = gemm_form(M, N, c->n_cu, c->opt_gemm64);      // poisson_rule.h
        const dim3 grid((unsigned)grid8(gemm_tiles(M, N, form)));
        switch (form) {
        case GemmForm::k128x128: hipLaunchKernelGGL(emba_dgemm128_kernel, grid, dim3(512), 0, s, p); break;
        case GemmForm::k64x128: hipLaunchKernelGGL(emba_dgemm_kernel<128>, grid, dim3(256), 0, s, p); break;
        case GemmForm::k64x64: hipLaunchKernelGGL(emba_dgemm_kernel<64>, grid, dim3(256), 0, s, p); break;
        }
    };
    if (dense) {
        // rhs -> eigenvector space, solve, back (laplace.cpp:633-758):  M = S_H ((S_H F S_W) o C) S_W
        const double inv_norm = 1.0 / (4.0 * ((double)(H + 1) * (double)(W + 1)));   // fft_norm, laplace.cpp:648
        gemm(c->d_pF.as<double>(), c->d_SW.as<double>(), c->d_pT.as<double>(), H, W, W, 0, 1.0);            // T = F S_W
        gemm(c->d_SH.as<double>(), c->d_pT.as<double>(), c->d_pF.as<double>(), H, W, H, 1, inv_norm);       // U = (S_H T / fft_norm) / (lambda1 + lambda2)
        gemm(c->d_pF.as<double>(), c->d_SW.as<double>(), c->d_pT.as<double>(), H, W, W, 0, 1.0);            // T = U S_W
        gemm(c->d_SH.as<double>(), c->d_pT.as<double>(), c->d_pF.as<double>(), H, W, H, 0, 1.0);            // M = S_H T
    } else {
        const dim3 tg((W + 31) / 32, (H + 31) / 32), tgT((H + 31) / 32, (W + 31) / 32);
        // DST-I along H of every row of the transposed plane: src (W x H) -> dst (W x H), times scale.  Folded (even H): two half-size products on
        // the even- and odd-indexed inputs + a butterfly; tmp holds [E | O] (W x H/2 each).
        // transposed_out: dst receives the result TRANSPOSED (H x W) — the folded form's butterfly writes it that way, saving the last transpose pass
        auto dst_rows = [&](const double* src, double* dst, double* tmp, double scale, bool transposed_out) -> bool {
            if (!fold) { gemm(src, c->d_SH.as<double>(), dst, W, H, H, 2, scale); return false; }
            const int h = H / 2;
            double* E = tmp; double* O = tmp + (size_t)W * h;
            gemm(src, c->d_Sfold.as<double>(), E, W, h, h, 0, 1.0, H, 2, 0);
            gemm(src, c->d_Sfold.as<double>() + (size_t)h * h, O, W, h, h, 0, 1.0, H, 2, 1);
            if (transposed_out) hipLaunchKernelGGL(emba_dst_butterfly_T_kernel, dim3((h + 31) / 32, (W + 31) / 32), dim3(256), 0, s, E, O, W, H, scale, dst);
            else hipLaunchKernelGGL(emba_dst_butterfly_kernel, dim3((unsigned)(((size_t)W * h + 255) / 256)), dim3(256), 0, s, E, O, W, H, scale, dst);
            return transposed_out;
        };
        if (fold && (st = ensure<double>(c, c->d_pE, npix))) return st;
        if (wrap) hipLaunchKernelGGL(emba_divergence_T_wrap_kernel, tg, dim3(256), 0, s, gx, gy, H, W, c->d_pT.as<double>());      // F^T with the wrapped column
        else hipLaunchKernelGGL(emba_divergence_T_kernel, tg, dim3(256), 0, s, gx, gy, H, W, c->d_pT.as<double>());                // F^T  (W x H), straight from the gradient maps
        dst_rows(c->d_pT.as<double>(), c->d_pF.as<double>(), c->d_pE.as<double>(), 1.0, false);                                                                 // (S_H F)^T = F^T S_H
        const unsigned tb = (unsigned)((H + kTriSys - 1) / kTriSys);
        // wrapped: the cyclic systems condensed on x[W-1] (poisson_rule.h) — the same sweeps over the first W-1 rows give p, then t per system and x = p - t q
        const int Wt = wrap ? W - 1 : W;
        hipLaunchKernelGGL(emba_tridiag_sweep_kernel<false>, dim3(tb), dim3(kTriSys * kTriChunks), 0, s, c->d_thomas.as<double>(), c->d_lamH.as<double>(), c->d_pF.as<double>(), H, Wt);   // (T_W + lambda1[i] I) x = g, per i
        hipLaunchKernelGGL(emba_tridiag_sweep_kernel<true>, dim3(tb), dim3(kTriSys * kTriChunks), 0, s, c->d_thomas.as<double>(), c->d_lamH.as<double>(), c->d_pF.as<double>(), H, Wt);
        if (wrap) {
            hipLaunchKernelGGL(emba_wrap_pivot_kernel, dim3((H + 255) / 256), dim3(256), 0, s, (const double*)c->d_wrapq.as<double>(), (const double*)c->d_lamH.as<double>(), c->d_pF.as<double>(), H, W);
            hipLaunchKernelGGL(emba_wrap_close_kernel, dim3(nblocks((size_t)H * (W - 1))), dim3(256), 0, s, (const double*)c->d_wrapq.as<double>(), c->d_pF.as<double>(), H, W);
        }
        // M^T = X^T S_H / (2 (H+1)).  Folded: the butterfly writes M itself into d_pF (its input X^T is dead once E and O exist)
        if (fold) dst_rows(c->d_pF.as<double>(), c->d_pF.as<double>(), c->d_pE.as<double>(), 1.0 / (2.0 * (double)(H + 1)), true);
        else {
            dst_rows(c->d_pF.as<double>(), c->d_pT.as<double>(), c->d_pE.as<double>(), 1.0 / (2.0 * (double)(H + 1)), false);
            hipLaunchKernelGGL(emba_transpose_kernel, tgT, dim3(256), 0, s, c->d_pT.as<double>(), W, H, c->d_pF.as<double>());                  // M
        }
    }
    HIP_TRY(c, hipGetLastError());
    if (M_host) HIP_TRY(c, hipMemcpyAsync(M_host, c->d_pF.as<double>(), npix * sizeof(double), hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipStreamSynchronize(s));
    c->spun = false; c->knots_in_flight = false;
    return EMBA_OK;
}

extern "C" emba_status emba_reconstruct_intensity(emba_ctx* c, const double* Gx_host, const double* Gy_host, double* M_host)
{
    return emba_reconstruct_intensity_bc(c, Gx_host, Gy_host, M_host, EMBA_POISSON_DIRICHLET);
}

// ---- record_data map images (render_kernels.h) --------------------------------------------------------------------------------
namespace {

// The ranks of image_util::minMaxLocRobust (image_utils.cpp:22-23) in float32 index arithmetic, as emba_amd/io.normalize_robust states them
// (for the panorama sizes of this project the reference's double form gives the same ranks: tests/test_record_cpu.py).
void robust_ranks(size_t n, double pct, unsigned int k[2])
{
    const float q = 0.5f * (float)pct / 100.f;
    const size_t i_min = (size_t)(q * (float)n), i_max = (size_t)((1.f - q) * (float)n);
    k[0] = (unsigned int)std::min(i_min, n - 1);
    k[1] = (unsigned int)std::min(i_max, n - 1);
}

// rmin / rmax of every plane (n values each, device memory) by the radix select of render_kernels.h — 6 launches, no host round trip; with hsv
// (planes = Gx, Gy) also the min / max of 0.5*angle and of the magnitude.  Results stay in c->d_rstate.as<RenderState>().
emba_status robust_select(emba_ctx* c, const double* const* planes, int nplanes, size_t n, double pct, bool hsv)
{
    hipStream_t s = c->stream;
    emba_status st;
    bool fresh_st = false, fresh_h = false;
    if ((st = ensure<RenderState>(c, c->d_rstate, 1, &fresh_st)) || (st = ensure<unsigned int>(c, c->d_rhist, (size_t)kRselSlots * kRselBins, &fresh_h)) ||
        (st = ensure<unsigned long long>(c, c->d_rcand, (size_t)nplanes * n)))
        return st;
    if (fresh_st) {
        RenderState init{};
        init.mm[0] = init.mm[2] = ~0ull;
        HIP_TRY(c, hipMemcpyAsync(c->d_rstate.as<RenderState>(), &init, sizeof init, hipMemcpyHostToDevice, s));
    }
    if (fresh_h) HIP_TRY(c, hipMemsetAsync(c->d_rhist.as<unsigned int>(), 0, (size_t)kRselSlots * kRselBins * sizeof(unsigned int), s));
    RselParams p{};
    p.src[0] = planes[0]; p.src[1] = nplanes > 1 ? planes[1] : nullptr;
    p.n = (unsigned int)n; p.nplanes = nplanes; p.hsv = hsv ? 1 : 0;
    robust_ranks(n, pct, p.k);
    p.hist = c->d_rhist.as<unsigned int>(); p.cand = c->d_rcand.as<unsigned long long>(); p.st = c->d_rstate.as<RenderState>();
    const unsigned g_full = (unsigned)std::min<size_t>(nblocks(n, kRselThreads * 8), 1024);
    hipLaunchKernelGGL(emba_rsel_stats_kernel, dim3(g_full), dim3(kRselThreads), 0, s, p);
    hipLaunchKernelGGL(emba_rsel_compact_kernel, dim3((unsigned)std::min<size_t>(nblocks(n, 256 * 8), 2048)), dim3(256), 0, s, p);
    const unsigned g_round = (unsigned)std::min<size_t>(nblocks(n, kRselThreads * 32), 128);
    for (int r = 1; r <= kRselRounds; ++r)
        hipLaunchKernelGGL(emba_rsel_round_kernel, dim3(g_round, 2 * nplanes), dim3(kRselThreads), 0, s, p, r);
    HIP_TRY(c, hipGetLastError());
    return EMBA_OK;
}

inline size_t img_off(size_t bytes) { return (bytes + 255) & ~(size_t)255; }

}  // namespace

// Device layout of the images in c->d_img.as<uint8_t>(): [Gx_u8 | Gy_u8 | RGB (3 n) | Poisson_u8], each part 256-byte aligned.
extern "C" emba_status emba_render_map_images_bc(emba_ctx* c, double pct_discard, uint8_t* gx_u8, uint8_t* gy_u8, uint8_t* rgb_u8, uint8_t* poisson_u8, int boundary)
{
    if (!c) return EMBA_ERR_INVALID_ARG;
    emba_status st;
    if ((st = poisson_boundary_check(c, boundary))) return st;      // (before the first image is written)
    if (!(pct_discard >= 0.0 && pct_discard <= 100.0)) return fail(c, EMBA_ERR_INVALID_ARG, "pct_discard=%g outside [0, 100]", pct_discard);
    if (!c->map.state().resident()) return fail(c, EMBA_ERR_STATE, "no map resident");
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t s = c->stream;
    const size_t n = c->npix, o1 = img_off(n), o2 = o1 + img_off(n), o3 = o2 + img_off(3 * n);
    if (n >= ((size_t)1 << 31)) return fail(c, EMBA_ERR_CAPACITY, "%zu pixels: the select counts in 32 bits", n);
    if ((st = ensure<uint8_t>(c, c->d_img, o3 + img_off(n)))) return st;
    if (gx_u8 || gy_u8 || rgb_u8) {
        const double* planes[2] = {c->map.Gx(), c->map.Gy()};
        if ((st = robust_select(c, planes, 2, n, pct_discard, rgb_u8 != nullptr))) return st;
        const int vec = (((uintptr_t)c->map.Gx() | (uintptr_t)c->map.Gy()) & 15) == 0;
        hipLaunchKernelGGL(emba_render_kernel, dim3(nblocks(n, 1024)), dim3(256), 0, s, c->map.Gx(), c->map.Gy(), (unsigned int)n, (const RenderState*)c->d_rstate.as<RenderState>(),
                           gx_u8 ? c->d_img.as<uint8_t>() : nullptr, gy_u8 ? c->d_img.as<uint8_t>() + o1 : nullptr, rgb_u8 ? c->d_img.as<uint8_t>() + o2 : nullptr, vec);
        HIP_TRY(c, hipGetLastError());
        HIP_TRY(c, hipStreamSynchronize(s));
        if (gx_u8 && (st = d2h_pageable(c, gx_u8, c->d_img.as<uint8_t>(), n))) return st;
        if (gy_u8 && (st = d2h_pageable(c, gy_u8, c->d_img.as<uint8_t>() + o1, n))) return st;
        if (rgb_u8 && (st = d2h_pageable(c, rgb_u8, c->d_img.as<uint8_t>() + o2, 3 * n))) return st;
    }
    if (poisson_u8) {
        if ((st = emba_reconstruct_intensity_bc(c, nullptr, nullptr, nullptr, boundary))) return st;      // M stays in c->d_pF.as<double>()
        const double* planes[1] = {c->d_pF.as<double>()};
        if ((st = robust_select(c, planes, 1, n, pct_discard, false))) return st;
        hipLaunchKernelGGL(emba_robust_u8_kernel, dim3((unsigned)std::min<size_t>(nblocks(n), 4096)), dim3(256), 0, s, (const double*)c->d_pF.as<double>(), (unsigned int)n,
                           (const RenderState*)c->d_rstate.as<RenderState>(), 0, c->d_img.as<uint8_t>() + o3);
        HIP_TRY(c, hipGetLastError());
        HIP_TRY(c, hipStreamSynchronize(s));
        if ((st = d2h_pageable(c, poisson_u8, c->d_img.as<uint8_t>() + o3, n))) return st;
    }
    c->spun = false; c->knots_in_flight = false;
    return EMBA_OK;
}

extern "C" emba_status emba_render_map_images(emba_ctx* c, double pct_discard, uint8_t* gx_u8, uint8_t* gy_u8, uint8_t* rgb_u8, uint8_t* poisson_u8)
{
    return emba_render_map_images_bc(c, pct_discard, gx_u8, gy_u8, rgb_u8, poisson_u8, EMBA_POISSON_DIRICHLET);
}

extern "C" emba_status emba_normalize_robust(emba_ctx* c, const double* src_host, size_t n, double pct_discard, uint8_t* dst_host, double* rmin, double* rmax)
{
    if (!c) return EMBA_ERR_INVALID_ARG;
    if (!src_host || n == 0) return fail(c, EMBA_ERR_INVALID_ARG, "src_host NULL or n = 0");
    if (n >= ((size_t)1 << 31)) return fail(c, EMBA_ERR_CAPACITY, "n=%zu: the select counts in 32 bits", n);
    if (!(pct_discard >= 0.0 && pct_discard <= 100.0)) return fail(c, EMBA_ERR_INVALID_ARG, "pct_discard=%g outside [0, 100]", pct_discard);
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t s = c->stream;
    emba_status st;
    if ((st = ensure<double>(c, c->d_nsrc, n)) || (st = ensure<uint8_t>(c, c->d_img, img_off(n)))) return st;
    HIP_TRY(c, hipMemcpyAsync(c->d_nsrc.as<double>(), src_host, n * sizeof(double), hipMemcpyHostToDevice, s));
    const double* planes[1] = {c->d_nsrc.as<double>()};
    if ((st = robust_select(c, planes, 1, n, pct_discard, false))) return st;
    if (dst_host) {
        hipLaunchKernelGGL(emba_robust_u8_kernel, dim3((unsigned)std::min<size_t>(nblocks(n), 4096)), dim3(256), 0, s, (const double*)c->d_nsrc.as<double>(), (unsigned int)n,
                           (const RenderState*)c->d_rstate.as<RenderState>(), 0, c->d_img.as<uint8_t>());
        HIP_TRY(c, hipGetLastError());
    }
    double r[2];
    HIP_TRY(c, hipMemcpyAsync(&r[0], &c->d_rstate.as<RenderState>()->slot[0].value, sizeof(double), hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipMemcpyAsync(&r[1], &c->d_rstate.as<RenderState>()->slot[1].value, sizeof(double), hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipStreamSynchronize(s));
    if (dst_host && (st = d2h_pageable(c, dst_host, c->d_img.as<uint8_t>(), n))) return st;
    if (rmin) *rmin = r[0];
    if (rmax) *rmax = r[1];
    c->spun = false; c->knots_in_flight = false;
    return EMBA_OK;
}
