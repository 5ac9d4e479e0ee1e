// emba_amd/csrc/readback_host.h — what the host reads back of an evaluation and of the normal equations: the compacted residual vector and the inlier numbers
// behind it (emba_compact_ep, emba_get_ep, the inlier pixels, their starts, ep by pixel), the sparse A12 factors, emba_dump_state (the reference's per-event
// intermediates, re-indexed to time order), emba_last_counts and emba_sync.  Each resolves the counters the step left pending first (step_host.h: resolve_pending).
// Part of emba_hip.hip's translation unit, included below step_host.h (resolve_pending, ensure_inl_idx, ensure_compact, warp_params) and transfer_host.h
// (d2h_pageable, d2h_chunks).
#pragma once
#include "context.h"

using namespace emba;

extern "C" {

emba_status emba_get_A12_sparse(emba_ctx* c, int32_t* cp_c, int32_t* cp_p, int32_t* pix, double* w, double* jc, double* jp, double* dp)
{
    if (!c) return EMBA_ERR_INVALID_ARG;
    if (!c->eq.accum_done) return fail(c, EMBA_ERR_STATE, "no normal equations formed yet");
    HIP_TRY(c, hipSetDevice(c->device));
    { emba_status st0 = resolve_pending(c); if (st0) return st0; }
    const size_t M = c->win.n_cand;
    if (!M) return EMBA_OK;
    DevBuf b_c, b_p, b_x, b_w, b_jc, b_jp, b_dp;      // (per call)
    emba_status st;
    if ((st = ensure<int32_t>(c, b_c, M)) || (st = ensure<int32_t>(c, b_p, M)) || (st = ensure<int32_t>(c, b_x, M)) || (st = ensure<double>(c, b_w, M)) ||
        (st = ensure<double>(c, b_jc, 6 * M)) || (st = ensure<double>(c, b_jp, 6 * M)) || (st = ensure<double>(c, b_dp, 2 * M)) || (st = ensure_compact(c)))
        return st;
    int32_t *d_c = b_c.as<int32_t>(), *d_p = b_p.as<int32_t>(), *d_x = b_x.as<int32_t>();
    double *d_w = b_w.as<double>(), *d_jc = b_jc.as<double>(), *d_jp = b_jp.as<double>(), *d_dp = b_dp.as<double>();
    hipStream_t s = c->stream;
    hipLaunchKernelGGL(emba_export_a12_kernel, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, s, c->work.rec.as<double>(), c->d_slot_key.as<uint32_t>(), (long)M,
                       c->d_count, c->d_compact.as<int32_t>(), c->eq.thres, c->eq.irls, c->eq.eta, d_c, d_p, d_x, d_w, d_jc, d_jp, d_dp, c->work.stamp);
    if (cp_c) (void)hipMemcpyAsync(cp_c, d_c, M * 4, hipMemcpyDeviceToHost, s);
    if (cp_p) (void)hipMemcpyAsync(cp_p, d_p, M * 4, hipMemcpyDeviceToHost, s);
    if (pix) (void)hipMemcpyAsync(pix, d_x, M * 4, hipMemcpyDeviceToHost, s);
    if (w) (void)hipMemcpyAsync(w, d_w, M * 8, hipMemcpyDeviceToHost, s);
    if (jc) (void)hipMemcpyAsync(jc, d_jc, 6 * M * 8, hipMemcpyDeviceToHost, s);
    if (jp) (void)hipMemcpyAsync(jp, d_jp, 6 * M * 8, hipMemcpyDeviceToHost, s);
    if (dp) (void)hipMemcpyAsync(dp, d_dp, 2 * M * 8, hipMemcpyDeviceToHost, s);
    hipError_t e = hipStreamSynchronize(s);
    if (e != hipSuccess) return fail(c, EMBA_ERR_HIP, "get_A12_sparse: %s", hipGetErrorString(e));
    return EMBA_OK;
}

emba_status emba_compact_ep(emba_ctx* c)
{
    if (!c) return EMBA_ERR_INVALID_ARG;
    if (!c->ev.launched) return fail(c, EMBA_ERR_STATE, "no evaluateDataError state");
    HIP_TRY(c, hipSetDevice(c->device));
    if (c->ev.ep_valid) return EMBA_OK;      // (the resident step's Gram launch has produced it already)
    c->ev.inl_idx_valid = false;      // (asked for explicitly: produce it for THIS call)
    return ensure_inl_idx(c);
}

emba_status emba_get_ep(emba_ctx* c, double* ep_host, size_t cap, size_t* n_inliers)
{
    if (!c || (!ep_host && cap)) return c ? fail(c, EMBA_ERR_INVALID_ARG, "ep_host NULL") : EMBA_ERR_INVALID_ARG;
    if (!c->ev.readable()) return fail(c, EMBA_ERR_STATE, "no evaluateDataError state");
    HIP_TRY(c, hipSetDevice(c->device));
    emba_status st;
    if ((st = resolve_pending(c))) return st;
    if (!c->ev.ep_valid && (st = ensure_inl_idx(c))) return st;      // (not produced by a resident step: the stand-alone compaction)
    if (n_inliers) *n_inliers = c->n_inliers;
    if (cap < c->n_inliers) return fail(c, EMBA_ERR_CAPACITY, "cap=%zu < inliers=%zu", cap, c->n_inliers);
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (c->n_inliers && (st = d2h_pageable(c, ep_host, c->d_ep.as<double>(), c->n_inliers * sizeof(double)))) return st;
    return EMBA_OK;
}

emba_status emba_get_inlier_pixels(emba_ctx* c, uint32_t* pix_host)
{
    if (!c || !pix_host) return c ? fail(c, EMBA_ERR_INVALID_ARG, "pix_host NULL") : EMBA_ERR_INVALID_ARG;
    if (!c->ev.readable()) return fail(c, EMBA_ERR_STATE, "no evaluateDataError state");
    HIP_TRY(c, hipSetDevice(c->device));
    emba_status st;
    if ((st = resolve_pending(c)) || (st = ensure_inl_idx(c))) return st;
    if (!c->n_inliers) return EMBA_OK;
    if ((st = ensure<uint32_t>(c, c->dl.out, c->n_inliers))) return st;
    uint32_t* d_out = c->dl.out.as<uint32_t>();
    hipLaunchKernelGGL(emba_inlier_pix_kernel, dim3(nblocks(c->win.n_pm)), dim3(256), 0, c->stream, c->d_pm_pix.as<uint32_t>(), c->d_flag.as<uint8_t>(), c->d_inl_idx.as<int32_t>(), (long)c->win.n_pm, d_out);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(pix_host, d_out, c->n_inliers * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return EMBA_OK;
}

emba_status emba_get_inlier_pixel_starts(emba_ctx* c, uint32_t* starts_host)
{
    if (!c || !starts_host) return c ? fail(c, EMBA_ERR_INVALID_ARG, "starts_host NULL") : EMBA_ERR_INVALID_ARG;
    if (!c->ev.readable()) return fail(c, EMBA_ERR_STATE, "no evaluateDataError state");
    HIP_TRY(c, hipSetDevice(c->device));
    emba_status st;
    if ((st = resolve_pending(c)) || (st = ensure_inl_idx(c))) return st;
    const uint32_t S = (uint32_t)((size_t)c->sw * c->sh);
    if ((st = ensure<uint32_t>(c, c->dl.out, std::max<size_t>(c->n_inliers, 1))) || (st = ensure<uint32_t>(c, c->dl.pix_starts, (size_t)S + 1))) return st;
    uint32_t *d_px = c->dl.out.as<uint32_t>(), *d_starts = c->dl.pix_starts.as<uint32_t>();
    if (c->n_inliers) hipLaunchKernelGGL(emba_inlier_pix_kernel, dim3(nblocks(c->win.n_pm)), dim3(256), 0, c->stream, c->d_pm_pix.as<uint32_t>(), c->d_flag.as<uint8_t>(), c->d_inl_idx.as<int32_t>(), (long)c->win.n_pm, d_px);
    hipLaunchKernelGGL(emba_pix_starts_kernel, dim3(nblocks(c->n_inliers + 1)), dim3(256), 0, c->stream, d_px, (long)c->n_inliers, S, d_starts);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(starts_host, d_starts, ((size_t)S + 1) * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    c->h_pix_starts.assign(starts_host, starts_host + S + 1);
    c->ev.pix_starts_valid = true;
    return EMBA_OK;
}

emba_status emba_get_ep_by_pixel(emba_ctx* c, double* ep_out, const uint64_t* dst)
{
    if (!c || !ep_out || !dst) return c ? fail(c, EMBA_ERR_INVALID_ARG, "ep_out / dst NULL") : EMBA_ERR_INVALID_ARG;
    if (!c->ev.readable()) return fail(c, EMBA_ERR_STATE, "no evaluateDataError state");
    HIP_TRY(c, hipSetDevice(c->device));
    emba_status st;
    if ((st = resolve_pending(c))) return st;
    const size_t S = (size_t)c->sw * c->sh;
    if (!c->ev.pix_starts_valid || c->h_pix_starts.size() != S + 1) {
        std::vector<uint32_t> tmp(S + 1);
        if ((st = emba_get_inlier_pixel_starts(c, tmp.data()))) return st;
    }
    if (!c->ev.ep_valid && (st = ensure_inl_idx(c))) return st;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    const uint32_t* starts = c->h_pix_starts.data();
    if ((size_t)starts[S] != c->n_inliers) return fail(c, EMBA_ERR_STATE, "the pixel starts do not belong to this evaluation (%u residuals there, %zu here)", starts[S], c->n_inliers);
    size_t p = 0;      // the pixel cursor only moves forward: the chunks arrive in ep order
    return d2h_chunks(c, c->d_ep.as<double>(), c->n_inliers * sizeof(double), [&](const void* chunk, size_t off, size_t len) {
        const size_t a = off / sizeof(double), b = (off + len) / sizeof(double);
        while (p < S && (size_t)starts[p + 1] <= a) ++p;
        for (size_t q = p; q < S && (size_t)starts[q] < b; ++q) {
            const size_t lo = std::max<size_t>(starts[q], a), hi = std::min<size_t>(starts[q + 1], b);
            if (hi > lo) std::memcpy(ep_out + dst[q] + (lo - starts[q]), (const double*)chunk + (lo - a), (hi - lo) * sizeof(double));
        }
    });
}

emba_status emba_dump_state(emba_ctx* c, double* pm, double* D, int32_t* cp_idx, int32_t* inlier_idx, int32_t* pm_int, double* dp,
                            double* Gpm, double* temp)
{
    if (!c) return EMBA_ERR_INVALID_ARG;
    if (!c->ev.readable()) return fail(c, EMBA_ERR_STATE, "no evaluateDataError state to dump");
    HIP_TRY(c, hipSetDevice(c->device));
    { emba_status st0 = resolve_pending(c); if (st0) return st0; }
    if (inlier_idx) { emba_status st0 = ensure_inl_idx(c); if (st0) return st0; }
    const size_t ns = c->win.n_sorted, n = c->win.n_in;
    if (!ns) return EMBA_OK;
    hipStream_t s = c->stream;
    // device and host staging only for what was asked for (a 100 M-event pm dump is 1.6 GB, the full state 17 GB)
    const bool w_pm = pm, w_D = D, w_dp = dp, w_G = Gpm, w_t = temp, w_pi = pm_int, w_inl = inlier_idx, w_flag = inlier_idx || pm_int || Gpm || temp;
    DevBuf b_pm, b_D, b_dp, b_G, b_t, b_pi;      // (per call)
    emba_status st = EMBA_OK;
    if ((w_pm && (st = ensure<double>(c, b_pm, 2 * ns))) || (w_D && (st = ensure<double>(c, b_D, 12 * ns))) || (w_dp && (st = ensure<double>(c, b_dp, 2 * ns))) ||
        (w_G && (st = ensure<double>(c, b_G, 2 * ns))) || (w_t && (st = ensure<double>(c, b_t, 2 * ns))) || (w_pi && (st = ensure<int32_t>(c, b_pi, 2 * ns))))
        return st;
    double *d_pm = b_pm.as<double>(), *d_D = b_D.as<double>(), *d_dp = b_dp.as<double>(), *d_G = b_G.as<double>(), *d_t = b_t.as<double>();
    int32_t* d_pi = b_pi.as<int32_t>();
    if (w_dp) (void)hipMemsetAsync(d_dp, 0, 2 * ns * 8, s);
    if (w_G) (void)hipMemsetAsync(d_G, 0, 2 * ns * 8, s);
    if (w_t) (void)hipMemsetAsync(d_t, 0, 2 * ns * 8, s);
    if (w_pi) (void)hipMemsetAsync(d_pi, 0xFF, 2 * ns * 4, s);
    // (a dump launch packs no texels, writes no tags and has no status word, cost, stamp or chunk list: those fields stay zero)
    WarpParams p = warp_params(c);
    p.d_pm = d_pm; p.d_D = d_D; p.d_dp = d_dp; p.d_Gpm = d_G; p.d_temp = d_t; p.d_pm_int = d_pi;
    if (c->order.tile_order) hipLaunchKernelGGL((emba_warp_residual_kernel<true, true>), dim3((unsigned)grid8(c->win.nblk)), dim3(kWarpBlock), 0, s, p);
    else if (c->ev.segpose) hipLaunchKernelGGL((emba_warp_residual_kernel<true, false, true>), dim3((unsigned)grid8(c->win.nblk)), dim3(kWarpBlock), 0, s, p);   // (the last evaluation left segment records, not a pose table)
    else hipLaunchKernelGGL((emba_warp_residual_kernel<true, false>), dim3((unsigned)grid8(c->win.nblk)), dim3(kWarpBlock), 0, s, p);
    std::vector<double> h_pm(w_pm ? 2 * ns : 0), h_D(w_D ? 12 * ns : 0), h_dp(w_dp ? 2 * ns : 0), h_G(w_G ? 2 * ns : 0), h_t(w_t ? 2 * ns : 0);
    std::vector<uint16_t> h_cp(cp_idx ? c->win.n_batch : 0);
    std::vector<int32_t> h_pi(w_pi ? 2 * ns : 0), h_inl(w_inl ? c->win.n_pm : 0);     // (inlier numbers and flags are indexed in pm-order)
    std::vector<uint8_t> h_flag(w_flag ? c->win.n_pm : 0);
    if (w_pm) (void)hipMemcpyAsync(h_pm.data(), d_pm, 2 * ns * 8, hipMemcpyDeviceToHost, s);
    if (w_D) (void)hipMemcpyAsync(h_D.data(), d_D, 12 * ns * 8, hipMemcpyDeviceToHost, s);
    if (w_dp) (void)hipMemcpyAsync(h_dp.data(), d_dp, 2 * ns * 8, hipMemcpyDeviceToHost, s);
    if (w_G) (void)hipMemcpyAsync(h_G.data(), d_G, 2 * ns * 8, hipMemcpyDeviceToHost, s);
    if (w_t) (void)hipMemcpyAsync(h_t.data(), d_t, 2 * ns * 8, hipMemcpyDeviceToHost, s);
    if (w_pi) (void)hipMemcpyAsync(h_pi.data(), d_pi, 2 * ns * 4, hipMemcpyDeviceToHost, s);
    if (w_inl) (void)hipMemcpyAsync(h_inl.data(), c->d_inl_idx.as<int32_t>(), c->win.n_pm * 4, hipMemcpyDeviceToHost, s);
    if (w_flag) (void)hipMemcpyAsync(h_flag.data(), c->d_flag.as<uint8_t>(), c->win.n_pm, hipMemcpyDeviceToHost, s);
    if (cp_idx) (void)hipMemcpyAsync(h_cp.data(), c->d_cp.as<uint16_t>(), h_cp.size() * 2, hipMemcpyDeviceToHost, s);
    hipError_t e = hipStreamSynchronize(s);
    if (e != hipSuccess) return fail(c, EMBA_ERR_HIP, "dump_state: %s", hipGetErrorString(e));
    // pure re-indexing (pixel-major -> original time order); no arithmetic on the host
    if (cp_idx) for (size_t k = 0; k < n; ++k) cp_idx[k] = -1;
    if (inlier_idx) for (size_t k = 0; k < n; ++k) inlier_idx[k] = -2;
    if (pm_int) for (size_t k = 0; k < 2 * n; ++k) pm_int[k] = -1;
    if (pm) memset(pm, 0, 2 * n * 8);
    if (D) memset(D, 0, 12 * n * 8);
    if (dp) memset(dp, 0, 2 * n * 8);
    if (Gpm) memset(Gpm, 0, 2 * n * 8);
    if (temp) memset(temp, 0, 2 * n * 8);
    // entry of the device order -> pm-order index -> original event (lead-in copies and halo entries map to nothing)
    std::vector<uint32_t> h_evpix(ns), h_evbatch(cp_idx ? ns : 0), h_evpm(c->order.have_ev_pm ? ns : 0), h_pmorig(c->win.n_pm);
    HIP_TRY(c, hipMemcpy(h_evpix.data(), c->order.d_ev_pix, ns * 4, hipMemcpyDeviceToHost));
    if (cp_idx) HIP_TRY(c, hipMemcpy(h_evbatch.data(), c->order.d_ev_batch, ns * 4, hipMemcpyDeviceToHost));
    if (c->order.have_ev_pm) HIP_TRY(c, hipMemcpy(h_evpm.data(), c->d_ev_pm.as<uint32_t>(), ns * 4, hipMemcpyDeviceToHost));
    HIP_TRY(c, hipMemcpy(h_pmorig.data(), c->d_pm_orig.as<uint32_t>(), c->win.n_pm * 4, hipMemcpyDeviceToHost));
    for (size_t i = 0; i < ns; ++i) {
        if (h_evpix[i] & kEvLead) continue;                        // lead-in copy / halo
        const size_t f = c->order.have_ev_pm ? h_evpm[i] : i;           // pm-order index: where flag / inlier number of this entry live
        const uint32_t k = h_pmorig[f];
        if (k == 0xFFFFFFFFu) continue;
        const bool cand = (h_evpix[i] & kEvHasPred) != 0;
        if (pm) { pm[2 * k] = h_pm[2 * i]; pm[2 * k + 1] = h_pm[2 * i + 1]; }
        if (D) memcpy(D + 12 * (size_t)k, &h_D[12 * i], 12 * 8);
        if (cp_idx) cp_idx[k] = (int32_t)h_cp[h_evbatch[i]];
        if (inlier_idx) inlier_idx[k] = cand ? (h_flag[f] ? h_inl[f] : -1) : -2;
        if (pm_int && h_flag[f]) { pm_int[2 * k] = h_pi[2 * i]; pm_int[2 * k + 1] = h_pi[2 * i + 1]; }
        if (dp && cand) { dp[2 * k] = h_dp[2 * i]; dp[2 * k + 1] = h_dp[2 * i + 1]; }
        if (Gpm && h_flag[f]) { Gpm[2 * k] = h_G[2 * i]; Gpm[2 * k + 1] = h_G[2 * i + 1]; }
        if (temp && h_flag[f]) { temp[2 * k] = h_t[2 * i]; temp[2 * k + 1] = h_t[2 * i + 1]; }
    }
    return EMBA_OK;
}

// The segment records of the last evaluation as they stand in d_seg, whoever wrote them there (the launch in front of the warp kernel, its workgroup 0 from its
// own chain, or its workgroup 0 from the host's records): a plain copy behind the stream, no kernel.
emba_status emba_dump_segments(emba_ctx* c, double* seg, size_t cap, size_t* n_seg)
{
    if (!c) return EMBA_ERR_INVALID_ARG;
    if (!c->ev.readable()) return fail(c, EMBA_ERR_STATE, "no evaluateDataError state to dump");
    HIP_TRY(c, hipSetDevice(c->device));
    { emba_status st0 = resolve_pending(c); if (st0) return st0; }
    const size_t n = (size_t)c->ev.n_seg;
    if (n_seg) *n_seg = n;
    if (!seg || !n) return EMBA_OK;
    if (cap < n) return fail(c, EMBA_ERR_CAPACITY, "dump_segments: room for %zu records, the evaluation left %zu", cap, n);
    HIP_TRY(c, hipMemcpyAsync(seg, c->d_seg.as<double>(), n * kSegStride * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return EMBA_OK;
}

emba_status emba_last_counts(emba_ctx* c, size_t* n_inliers, size_t* P)
{
    if (!c) return EMBA_ERR_INVALID_ARG;
    HIP_TRY(c, hipSetDevice(c->device));
    emba_status st = resolve_pending(c, true);
    if (st) return st;
    if (n_inliers) *n_inliers = c->n_inliers;
    if (P) *P = c->eq.P;
    return EMBA_OK;
}

emba_status emba_sync(emba_ctx* c)
{
    if (!c) return EMBA_ERR_INVALID_ARG;
    HIP_TRY(c, hipSetDevice(c->device));
    emba_status st = resolve_pending(c);
    if (st) return st;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    c->spun = false;
    return EMBA_OK;
}

}  // extern "C"
