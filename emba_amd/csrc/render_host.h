// emba_amd/csrc/render_host.h — the reference's record_data map images (render_kernels.h): emba_render_map_images[_bc], emba_normalize_robust.
// Part of emba_hip.hip's translation unit, included below poisson_host.h (poisson_boundary_check; poisson_solve, whose panorama is the fourth image) and
// transfer_host.h (d2h_pageable).
#pragma once
#include "context.h"

using namespace emba;

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
        const double* planes[1] = {nullptr};
        if ((st = poisson_solve(c, nullptr, nullptr, nullptr, boundary, &planes[0]))) return st;      // the panorama of the resident map, on the device
        if ((st = robust_select(c, planes, 1, n, pct_discard, false))) return st;
        hipLaunchKernelGGL(emba_robust_u8_kernel, dim3((unsigned)std::min<size_t>(nblocks(n), 4096)), dim3(256), 0, s, planes[0], (unsigned int)n,
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
