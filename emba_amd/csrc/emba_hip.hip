// emba_amd/csrc/emba_hip.hip — the translation unit behind the C ABI of include/emba_hip.h.  Here: create and destroy, the downloads and costs that wait on the
// step's counters, emba_dump_state, the option tables, the timers and probes, f3 and the record_data images.  Every path with state of its own is a host header
// with a HIP-free rule header beside it: the context is context.h, copies into the caller's pageable memory transfer_host.h, the window and its order
// order_host.h / order_rule.h, the step path (the evaluation and the normal equations) step_host.h / step_rule.h, the map map_host.h / map_rule.h, the solvers
// (f1) solve_host.h / solve_rule.h, the resident event sequence sequence_host.h / sequence_rule.h, contrast maximisation on it
// cmax_host.h / cmax_rule.h, the panorama of warped events panorama_host.h / panorama_rule.h and its smooth contrast and gradient
// contrast_host.h / contrast_rule.h, the multi-GPU group group.h: all one translation unit.
// Host code is C++17; every per-event / per-pixel computation runs in the HIP kernels of kernels.h.
// There is no CPU compute path in this file: the host only sorts indices once per window
// (emba_set_events: pose-independent structure), launches kernels and moves bytes.
#include "../../include/emba_hip.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "kernels.h"
#include "order_kernels.h"
#include "solve_kernels.h"
#include "poisson_kernels.h"
#include "render_kernels.h"
#include "sequence_kernels.h"
#include "context.h"
#include "sequence_rule.h"

using namespace emba;

#include "transfer_host.h"   // device -> pageable host memory: the copy pool, the staging buffers, d2h_chunks / d2h_pageable
#include "order_host.h"      // the window and its device order: emba_set_events[_dev], dev_scan / dev_sort, prepare_order, free_window

extern "C" {

int emba_abi_version(void) { return EMBA_ABI_VERSION; }

const char* emba_build_info(void)
{
#ifdef EMBA_DIAG
    return "emba_hip: HIP/gfx950 (CDNA4, wave64) kernels, fp64, DIAGNOSTICS build (EMBA_ABLATE honoured: results may be wrong), built " __DATE__ " " __TIME__;
#else
    return "emba_hip: HIP/gfx950 (CDNA4, wave64) kernels, fp64, built " __DATE__ " " __TIME__;
#endif
}

const char* emba_last_error(const emba_ctx* ctx) { return ctx ? ctx->err.c_str() : g_create_error.c_str(); }

emba_status emba_create(const emba_cfg* cfg, emba_ctx** out)
{
    if (!out) return fail(nullptr, EMBA_ERR_INVALID_ARG, "out is NULL");
    *out = nullptr;
    if (!cfg || !cfg->bearing_lut) return fail(nullptr, EMBA_ERR_INVALID_ARG, "cfg or bearing_lut is NULL");
    if (cfg->sensor_w <= 0 || cfg->sensor_h <= 0 || cfg->pano_w <= 0 || cfg->pano_h <= 0 ||
        (size_t)cfg->sensor_w * cfg->sensor_h >= 0x7FFFFFFFull || (size_t)cfg->pano_w * cfg->pano_h >= 0x7FFFFFFFull)
        return fail(nullptr, EMBA_ERR_INVALID_ARG, "bad sensor/pano size");
    if (cfg->event_batch != 0 && cfg->event_batch != 100)
        return fail(nullptr, EMBA_ERR_INVALID_ARG, "event_batch must be 100 (reference hard-codes it, model.cpp:78)");
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0)
        return fail(nullptr, EMBA_ERR_NO_DEVICE, "no HIP device (%s); this library has no CPU path", hipGetErrorString(e));
    if (cfg->device < 0 || cfg->device >= ndev)
        return fail(nullptr, EMBA_ERR_NO_DEVICE, "device ordinal %d not present (%d devices)", cfg->device, ndev);

    emba_ctx* c = new emba_ctx();
    c->cfg = *cfg;
    c->device = cfg->device;
    c->sw = cfg->sensor_w; c->sh = cfg->sensor_h; c->W = cfg->pano_w; c->H = cfg->pano_h;
    c->S = (size_t)c->sw * c->sh; c->npix = (size_t)c->W * c->H;
    c->C_th = cfg->C_th;
    c->outlier_px = cfg->outlier_px > 0 ? cfg->outlier_px : 10.0;
    // focalFromFOV(imageSize, 360, 180), equirectangular_camera.h:64-67
    c->fx = (double)((c->W / 360.0) * 180.0 / M_PI);
    c->fy = (double)((c->H / 180.0) * 180.0 / M_PI);
    c->cx = (double)c->W / 2.0; c->cy = (double)c->H / 2.0;
#ifdef EMBA_DIAG
    if (const char* ab = getenv("EMBA_ABLATE")) { c->ablate = atoi(ab); if (c->ablate) fprintf(stderr, "emba_hip: DIAGNOSTICS build, EMBA_ABLATE=%d: results are WRONG\n", c->ablate); }
#endif
    { int ncu = 0; if (hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, c->device) == hipSuccess && ncu > 0) c->n_cu = ncu; }
    // (the A/B switches of rounds 1-4 — EMBA_ORDER, EMBA_STEP_FAST, EMBA_STEP_GATHER, EMBA_SEGPOSE, EMBA_GRAM_TAGS, ... — are options now: emba_set_option)

#define CREATE_TRY(call)                                                                                  \
    do {                                                                                                  \
        hipError_t e2_ = (call);                                                                          \
        if (e2_ != hipSuccess) {                                                                          \
            fail(nullptr, EMBA_ERR_HIP, "%s failed: %s", #call, hipGetErrorString(e2_));                  \
            emba_destroy(c);                                                                              \
            return EMBA_ERR_HIP;                                                                          \
        }                                                                                                 \
    } while (0)

    CREATE_TRY(hipSetDevice(c->device));
    if (cfg->stream) { c->stream = (hipStream_t)cfg->stream; c->own_stream = false; }
    else { CREATE_TRY(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking)); c->own_stream = true; }
    CREATE_TRY(c->d_lut.ensure(c->S * 3 * sizeof(double)));
    CREATE_TRY(hipMemcpy(c->d_lut.as<double>(), cfg->bearing_lut, c->S * 3 * sizeof(double), hipMemcpyHostToDevice));
    {   // the sensor's field of view from the bearing vectors (x / z, y / z extents): what schur_accumulate estimates the band of U with
        double x0 = 1e300, x1 = -1e300, y0 = 1e300, y1 = -1e300;
        for (size_t i = 0; i < c->S; ++i) {
            const double z = cfg->bearing_lut[3 * i + 2];
            if (!(z > 0.0)) continue;
            const double ax = atan(cfg->bearing_lut[3 * i] / z), ay = atan(cfg->bearing_lut[3 * i + 1] / z);
            x0 = std::min(x0, ax); x1 = std::max(x1, ax); y0 = std::min(y0, ay); y1 = std::max(y1, ay);
        }
        c->fov_x = x1 > x0 ? x1 - x0 : M_PI; c->fov_y = y1 > y0 ? y1 - y0 : M_PI;
    }
    c->cmax_pin = cmax_pinhole_fit(cfg->bearing_lut, c->sw, c->sh);   // the image plane of contrast maximisation (cmax_rule.h); asked for by emba_seq_cmax* only
    c->cfg.bearing_lut = nullptr;  // not retained
    CREATE_TRY(c->d_texel.ensure(c->npix * kTexelStride * sizeof(double)));
    CREATE_TRY(c->d_count_own.ensure(c->npix * sizeof(int32_t)));
    c->d_count = c->d_count_own.as<int32_t>();
    CREATE_TRY(c->d_pixacc.ensure(c->npix * kPixAccStride * sizeof(double)));
    CREATE_TRY(c->d_compact.ensure(c->npix * sizeof(int32_t)));
    CREATE_TRY(c->d_active_bits.ensure((c->npix + 31) / 32 * 4 + 8));
    CREATE_TRY(c->d_active.ensure(c->npix * sizeof(uint32_t)));
    c->n_ablk = (c->npix + kActivePix - 1) / kActivePix;
    CREATE_TRY(c->d_seg_act.ensure(c->n_ablk * kActivePix * sizeof(uint16_t)));
    CREATE_TRY(c->d_ablk_cnt.ensure(c->n_ablk * sizeof(uint32_t)));
    CREATE_TRY(c->d_ablk_off.ensure(c->n_ablk * sizeof(uint32_t)));
    CREATE_TRY(c->d_err2.ensure(2 * sizeof(int)));
    CREATE_TRY(hipMemset(c->d_err2.as<int>(), 0, 2 * sizeof(int)));
    c->d_err = c->d_err2.as<int>();
    CREATE_TRY(c->d_rect.ensure(8 * sizeof(int)));
    { const int init[8] = {0x7FFFFFFF, 0x7FFFFFFF, -1, -1, 0x7FFFFFFF, 0x7FFFFFFF, -1, -1}; CREATE_TRY(hipMemcpy(c->d_rect.as<int>(), init, sizeof init, hipMemcpyHostToDevice)); }
    CREATE_TRY(c->d_seg_flag.ensure(256));
    CREATE_TRY(hipMemset(c->d_seg_flag.as<unsigned>(), 0, 256));
    CREATE_TRY(c->d_blk_rect.ensure(c->n_ablk * 4 * sizeof(int)));   // per active-count block: box of the touched pixels
    CREATE_TRY(c->d_total.ensure(4 * sizeof(uint32_t)));   // [0] inliers [1] P [2] scratch total
    CREATE_TRY(c->d_scalar.ensure(2 * sizeof(double)));
    CREATE_TRY(hipHostMalloc((void**)&c->h_pinned, 64, hipHostMallocMapped));
    memset(c->h_pinned, 0, 64);
    CREATE_TRY(hipHostGetDevicePointer((void**)&c->h_pinned_dev, c->h_pinned, 0));
    for (int i = 0; i < 8; ++i) { CREATE_TRY(hipEventCreate(&c->ev_start[i])); CREATE_TRY(hipEventCreate(&c->ev_stop[i])); }
    // every slot of the kernel-timing events up front: creating one later can stall the calling thread for tens of milliseconds (round 4: a 38-51 ms
    // pause inside bench.py's timed loop, once per process, at the first use of a new slot — the runtime growing its signal pool)
    for (int k = 0; k < 16; ++k) for (int i = 0; i < 5; ++i) CREATE_TRY(hipEventCreate(&c->kt_sets[k][i]));
    for (int i = 0; i < 2; ++i) CREATE_TRY(hipEventCreate(&c->cal_ev[i]));
    CREATE_TRY(c->d_probe.ensure(8 * sizeof(unsigned long long)));
    CREATE_TRY(hipEventCreateWithFlags(&c->knots_copied, hipEventDisableTiming));
    CREATE_TRY(hipDeviceSynchronize());      // (the memsets above ran on the default stream, which does not order the context's non-blocking stream behind it)
#undef CREATE_TRY
    *out = c;
    return EMBA_OK;
}

void emba_destroy(emba_ctx* c)
{
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    free_window(c);
    if (c->h_pinned) (void)hipHostFree(c->h_pinned);
    if (c->h_cost) (void)hipHostFree(c->h_cost);
    if (c->h_knots) (void)hipHostFree(c->h_knots);
    for (int k = 0; k < 2; ++k) { if (c->h_stage[k]) (void)hipHostFree(c->h_stage[k]); if (c->stage_ev[k]) (void)hipEventDestroy(c->stage_ev[k]); }
    if (c->knots_copied) (void)hipEventDestroy(c->knots_copied);
    for (int i = 0; i < 8; ++i) { if (c->ev_start[i]) (void)hipEventDestroy(c->ev_start[i]); if (c->ev_stop[i]) (void)hipEventDestroy(c->ev_stop[i]); }
    for (int k = 0; k < 16; ++k) for (int i = 0; i < 5; ++i) if (c->kt_sets[k][i]) (void)hipEventDestroy(c->kt_sets[k][i]);
    for (int i = 0; i < 2; ++i) if (c->cal_ev[i]) (void)hipEventDestroy(c->cal_ev[i]);
    const hipStream_t own = c->own_stream ? c->stream : nullptr;
    delete c;      // (its device buffers go with it: after the stream has drained, before the stream itself)
    if (own) (void)hipStreamDestroy(own);
}

}  // extern "C"

// evaluateDataError + formNormalEq + applyL2Reg: the step path.  Here, above the map calls and the downloads that wait for its counters — and above emba_dump_state:
// kernel templates are emitted in the order of their first use, and the device code keeps its order when the step's warp and Gram forms come first.
#include "step_host.h"

#include "map_host.h"   // upload, bind, updateMap, accept / reject, the map downloads, the median blur (needs resolve_pending, ensure_compact)

extern "C" {

emba_status emba_trial_reject(emba_ctx* c)
{
    if (!c) return EMBA_ERR_INVALID_ARG;
    if (!c->eq_in_alt) return EMBA_OK;     // nothing was evaluated since the equations were formed (or they have been re-formed)
    HIP_TRY(c, hipSetDevice(c->device));
    // (a trial that was only launched: its compacted residual vector and inlier numbers will never be asked for — nothing to resolve)
    if (c->ev.ep_deferred && !c->ev.P_pending && !c->ev.inl_pending) c->ev.ep_deferred = false;
    else if (c->ev.P_pending || c->ev.inl_pending || c->ev.ep_deferred) { emba_status st = resolve_pending(c); if (st) return st; }
    std::swap(c->work, c->alt);
    c->eq = c->eq_saved;
    c->eq_in_alt = false;
    // the per-event residuals, the count map and the per-pixel sums are the rejected trial's: formNormalEq needs a new evaluation
    begin_evaluation(c);
    return EMBA_OK;
}

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

emba_status emba_data_cost(emba_ctx* c, int32_t irls, double eta, double* cost)
{
    if (!c || !cost) return EMBA_ERR_INVALID_ARG;
    if (!c->ev.readable()) return fail(c, EMBA_ERR_STATE, "no residuals yet");
    HIP_TRY(c, hipSetDevice(c->device));
    { emba_status st0 = resolve_pending(c); if (st0) return st0; }
    hipStream_t s = c->stream;
    HIP_TRY(c, hipMemsetAsync(c->d_scalar.as<double>(), 0, sizeof(double), s));
    if (c->win.n_sorted) {
        const unsigned grid = (unsigned)std::min<size_t>((c->win.n_pm + 255) / 256, 2048);
        hipLaunchKernelGGL(emba_data_cost_kernel, dim3(grid), dim3(256), 0, s, c->d_e_sorted.as<double>(), c->d_flag.as<uint8_t>(), (long)c->win.n_pm, (int)irls, eta,
                           c->d_scalar.as<double>());
    }
    double v = 0;
    HIP_TRY(c, hipMemcpyAsync(&v, c->d_scalar.as<double>(), sizeof(double), hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipStreamSynchronize(s));
    if (irls == 0) v *= 0.5;
    else if (irls == 2) v *= 0.5 / eta;
    *cost = v;
    return EMBA_OK;
}

// Both cost terms of a trial point (solver.cpp:88-91, 265-268) in ONE launch (emba_costs_kernel: its last block writes the two sums, the step's status word and a
// sequence number to pinned host memory; the host spins on the number — no memset, no copies, no stream synchronise: 159 -> 130 us per LM iteration at the BASELINE
// shape, most of it the evaluation it waits for).  emba_costs_launch / _finish split it so that a group can enqueue every rank before it waits for any.
emba_status emba_costs_launch(emba_ctx* c, int32_t irls, double eta, int32_t with_reg)
{
    if (!c) return EMBA_ERR_INVALID_ARG;
    if (!c->ev.readable()) return fail(c, EMBA_ERR_STATE, "no residuals yet");
    if (with_reg && !c->map.state().resident()) return fail(c, EMBA_ERR_STATE, "no map");
    HIP_TRY(c, hipSetDevice(c->device));
    // An evaluation that has only been launched stays that way: the reductions read the per-event residuals and flags the warp kernel wrote,
    // not the compacted vector — so the formNormalEq that follows an accepted trial still finds the post-warp work fused (emba_form_active), and
    // a rejected trial never pays for a residual vector nobody asks for.  The step's status word comes back with the sums (emba_costs_finish).
    if (!c->ev.ep_deferred) { emba_status st0 = resolve_pending(c); if (st0) return st0; }
    if (!c->h_cost) {
        HIP_TRY(c, hipHostMalloc((void**)&c->h_cost, 4 * sizeof(double), hipHostMallocDefault));
        memset(c->h_cost, 0, 4 * sizeof(double));
        HIP_TRY(c, hipHostGetDevicePointer((void**)&c->h_cost_dev, c->h_cost, 0));
        if (emba_status st = ensure<double>(c, c->d_cost_acc, 4)) return st;
        HIP_TRY(c, hipMemsetAsync(c->d_cost_acc.as<double>(), 0, 4 * sizeof(double), c->stream));      // (on the kernels' stream: a hipMemset on the default stream is not ordered in front of them)
    }
    hipStream_t s = c->stream;
    CostsParams p{};
    p.e_sorted = c->d_e_sorted.as<double>(); p.flag = c->d_flag.as<uint8_t>(); p.n_pm = c->win.n_sorted ? (long)c->win.n_pm : 0L; p.irls = (int)irls; p.eta = eta;
    p.Gx = c->map.Gx(); p.Gy = c->map.Gy(); p.npix = with_reg ? (long)c->npix : 0L;
    // (a few hundred blocks: every block ends with two same-address atomics — its sum and its ticket —, and 4096 of them on one word serialise for longer than the sums take)
    p.nb_data = (int)std::max<size_t>(1, std::min<size_t>(((size_t)p.n_pm + 255) / 256, (size_t)c->n_cu));
    p.nb_reg = with_reg ? (int)std::max<size_t>(1, std::min<size_t>((c->npix + 255) / 256, (size_t)2 * c->n_cu)) : 0;
    p.acc = c->d_cost_acc.as<double>(); p.ticket = reinterpret_cast<unsigned int*>(c->d_cost_acc.as<double>() + 2); p.err_dev = c->d_err;
    p.host_out = c->h_cost_dev; p.seq = ++c->cost_seq;
    hipLaunchKernelGGL(emba_costs_kernel, dim3((unsigned)(p.nb_data + p.nb_reg)), dim3(256), 0, s, p);
    HIP_TRY(c, hipGetLastError());
    return EMBA_OK;
}
emba_status emba_costs_finish(emba_ctx* c, int32_t irls, double eta, double alpha, double* data_cost, double* reg_cost)
{
    if (!c || !c->h_cost) return EMBA_ERR_INVALID_ARG;
    HIP_TRY(c, hipSetDevice(c->device));
    {   // the kernel's last block publishes the sequence number behind the sums: spin on it (a stream synchronise costs tens of microseconds); bounded — a faulted
        // kernel never publishes — with the stream as the fallback
        volatile int* w = reinterpret_cast<volatile int*>(c->h_cost + 3);
        bool polled = false;
        for (long spin = 0; spin < 50000000L; ++spin) { if (w[0] == c->cost_seq) { polled = true; break; } __builtin_ia32_pause(); }
        if (polled) { std::atomic_thread_fence(std::memory_order_acquire); c->spun = true; }
        else { HIP_TRY(c, hipStreamSynchronize(c->stream)); c->spun = false; }
    }
    { int w = 0; memcpy(&w, c->h_cost + 2, sizeof(int)); if (w & 1) return fail(c, EMBA_ERR_TIME_RANGE, "a batch midpoint lies outside the spline's knots"); }
    double v = c->h_cost[0];
    if (irls == 0) v *= 0.5;
    else if (irls == 2) v *= 0.5 / eta;
    if (data_cost) *data_cost = v;
    if (reg_cost) *reg_cost = 0.5 * alpha * c->h_cost[1];
    return EMBA_OK;
}
emba_status emba_costs(emba_ctx* c, int32_t irls, double eta, double alpha, double* data_cost, double* reg_cost)
{
    emba_status st = emba_costs_launch(c, irls, eta, reg_cost ? 1 : 0);
    if (st) return st;
    return emba_costs_finish(c, irls, eta, alpha, data_cost, reg_cost);
}

emba_status emba_reg_cost(emba_ctx* c, double alpha, double* cost)
{
    if (!c || !cost) return EMBA_ERR_INVALID_ARG;
    if (!c->map.state().resident()) return fail(c, EMBA_ERR_STATE, "no map");
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t s = c->stream;
    HIP_TRY(c, hipMemsetAsync(c->d_scalar.as<double>() + 1, 0, sizeof(double), s));
    const unsigned grid = (unsigned)std::min<size_t>((c->npix + 255) / 256, 2048);
    hipLaunchKernelGGL(emba_reg_cost_kernel, dim3(grid), dim3(256), 0, s, c->map.Gx(), c->map.Gy(), (long)c->npix, c->d_scalar.as<double>() + 1);
    double v = 0;
    HIP_TRY(c, hipMemcpyAsync(&v, c->d_scalar.as<double>() + 1, sizeof(double), hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipStreamSynchronize(s));
    *cost = 0.5 * alpha * v;
    return EMBA_OK;
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
    WarpParams p{};
    p.ev_pix = c->order.d_ev_pix; p.ev_batch = c->order.d_ev_batch; p.ev_slot = c->d_ev_slot.as<uint32_t>(); p.ev_pm = c->order.tile_order ? c->d_ev_pm.as<uint32_t>() : nullptr; p.n_sorted = (long)ns; p.nblk = c->win.nblk;
    p.ev_u = c->d_ev_u.as<double>(); p.ev_seg = c->d_ev_seg.as<uint16_t>();
    p.pose = c->d_pose.as<double>(); p.seg = c->d_seg.as<double>(); p.lut = c->d_lut.as<double>(); p.texel = nullptr; p.rect_acc = nullptr; p.Gx = c->map.Gx(); p.Gy = c->map.Gy(); p.pixacc = c->d_pixacc.as<double>();
    p.W = c->W; p.H = c->H; p.fx = c->fx; p.fy = c->fy; p.cx = c->cx;
    p.cy = c->cy; p.C_th = c->C_th; p.outlier_px = c->outlier_px; p.count = c->d_count; p.rec = c->work.rec.as<double>(); p.e_sorted = c->d_e_sorted.as<double>();
    p.flag = c->d_flag.as<uint8_t>(); p.d_pm = d_pm; p.d_D = d_D; p.d_dp = d_dp; p.d_Gpm = d_G; p.d_temp = d_t; p.d_pm_int = d_pi;
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

// ---- tuning and A/B switches (documented, versioned by EMBA_ABI_VERSION; not environment variables) ----------------------------
namespace {
struct OptionRef { const char* name; int emba_ctx::*field; int lo, hi; };
const OptionRef kOptions[] = {
    {"step_ep", &emba_ctx::step_ep, 0, 2},
    {"step_fast", &emba_ctx::step_fast, 0, 1},
    {"step_gather", &emba_ctx::step_gather, 0, 3},
    {"step_one_set", &emba_ctx::step_one_set, 0, 1},
    {"gram_tags", &emba_ctx::use_tags, 0, 1},
    {"segpose", &emba_ctx::segpose_mode, 0, 2},
    {"order", &emba_ctx::order_mode, 0, 2},
    {"texel", &emba_ctx::texel_mode, 0, 3},
    {"solve_perm", &emba_ctx::solve_perm_mode, -1, 1},
    {"gather_waves", &emba_ctx::opt_gather_waves, 0, 4},
    {"chunk_order_bin", &emba_ctx::opt_chunk_order_bin, 0, 1},
    {"poison", &emba_ctx::opt_poison, 0, 1},
    {"tile_reserve", &emba_ctx::opt_tile_reserve, 0, 5},
    {"tile_shape", &emba_ctx::opt_tile_shape, -1, kNumTileShapes - 1},
    {"tile_fine", &emba_ctx::opt_tile_fine, -1, 1},
    {"tile_min_events", &emba_ctx::opt_tile_min_events, 0, 2000000000},
    {"tile_chunk", &emba_ctx::opt_tile_chunk, 0, 1 << 20},
    {"solve_counts", &emba_ctx::opt_solve_counts, -1, 2},
    {"syrk_dense", &emba_ctx::opt_syrk_dense, 0, 1},
    {"syrk_lists", &emba_ctx::opt_syrk_lists, 0, 2},
    {"gram_sparse", &emba_ctx::opt_gram_sparse, -1, 1},
    {"gram_sparse_chunk", &emba_ctx::opt_gram_sparse_chunk, 1, 8},
    {"syrk_min_cols", &emba_ctx::opt_syrk_min_cols, 64, 4096},
    {"syrk_item_cap", &emba_ctx::opt_syrk_item_cap, 1, 65536},
    {"solve_debug", &emba_ctx::opt_solve_debug, 0, 1},
    {"poisson", &emba_ctx::opt_poisson, 0, 2},
    {"gemm64", &emba_ctx::opt_gemm64, 0, 1},
};
// the hand-off of the segment records inside the warp launch (step_rule.h: prep_inside_warp); tests/test_gpu_step_prep.py runs every value that selects a branch
// (tests/test_step_prep_rule_cpu.py checks that it does)
const OptionRef kStepPrepOptions[] = {
    {"step_prep", &emba_ctx::step_prep, 0, 1},
    {"step_prep_polls", &emba_ctx::step_prep_polls, 0, 1 << 16},
};
// the vote kernel of emba_seq_contrast_gradient_level (contrast_rule.h: contrast_vote_plan); tests/test_gpu_contrast_pyramid.py runs every value at a level
// whose image fits LDS and at one whose image does not
const OptionRef kContrastOptions[] = {
    {"contrast_vote", &emba_ctx::opt_contrast_vote, -1, 1},
};
// the form of the dense pixel-order Gram launch (step_rule.h: gram_paired); tests/test_gpu_gram_paired.py runs both values and asserts which form ran
const OptionRef kGramOptions[] = {
    {"gram_multikey", &emba_ctx::opt_gram_multikey, 0, 1},
};
}  // namespace

emba_status emba_set_option(emba_ctx* c, const char* name, int32_t value)
{
    if (!c || !name) return EMBA_ERR_INVALID_ARG;
    for (const OptionRef& o : kOptions)
        if (!strcmp(o.name, name)) {
            if (value < o.lo || value > o.hi) return fail(c, EMBA_ERR_INVALID_ARG, "option %s: %d outside [%d, %d]", name, (int)value, o.lo, o.hi);
            c->*(o.field) = (int)value;
            if (!strcmp(name, "order") || !strcmp(name, "chunk_order_bin") || !strncmp(name, "tile_", 5)) c->order.keys_ready = false;      // the device order is rebuilt at the next evaluation
            return EMBA_OK;
        }
    for (const OptionRef& o : kStepPrepOptions)
        if (!strcmp(o.name, name)) {
            if (value < o.lo || value > o.hi) return fail(c, EMBA_ERR_INVALID_ARG, "option %s: %d outside [%d, %d]", name, (int)value, o.lo, o.hi);
            c->*(o.field) = (int)value;
            return EMBA_OK;
        }
    for (const OptionRef& o : kContrastOptions)
        if (!strcmp(o.name, name)) {
            if (value < o.lo || value > o.hi) return fail(c, EMBA_ERR_INVALID_ARG, "option %s: %d outside [%d, %d]", name, (int)value, o.lo, o.hi);
            c->*(o.field) = (int)value;
            return EMBA_OK;
        }
    for (const OptionRef& o : kGramOptions)
        if (!strcmp(o.name, name)) {
            if (value < o.lo || value > o.hi) return fail(c, EMBA_ERR_INVALID_ARG, "option %s: %d outside [%d, %d]", name, (int)value, o.lo, o.hi);
            c->*(o.field) = (int)value;
            return EMBA_OK;
        }
    return fail(c, EMBA_ERR_INVALID_ARG, "unknown option '%s'", name);
}

emba_status emba_get_option(emba_ctx* c, const char* name, int32_t* value)
{
    if (!c || !name || !value) return EMBA_ERR_INVALID_ARG;
    // read-only, the last evaluation: no launch in front of its warp kernel; that launch carried texel blocks; waves that formed their segment records themselves
    // (all evaluations of the context; drains the stream)
    if (!strcmp(name, "prep_in_warp")) { *value = c->ev.prep_in_warp ? 1 : 0; return EMBA_OK; }
    if (!strcmp(name, "texels_packed")) { *value = c->ev.texels_packed ? 1 : 0; return EMBA_OK; }
    if (!strcmp(name, "step_prep_fallbacks")) {
        unsigned n = 0;
        HIP_TRY(c, hipSetDevice(c->device));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        c->spun = false; c->knots_in_flight = false;
        HIP_TRY(c, hipMemcpy(&n, c->d_seg_flag.as<unsigned>() + 32, sizeof n, hipMemcpyDeviceToHost));
        *value = (int32_t)std::min<unsigned>(n, 0x7FFFFFFFu);
        return EMBA_OK;
    }
    if (!strcmp(name, "ep_valid")) { *value = c->ev.ep_valid ? 1 : 0; return EMBA_OK; }      // read-only: the device holds the last evaluation's ep (a step produced it, or a compaction)
    for (const OptionRef& o : kOptions)
        if (!strcmp(o.name, name)) { *value = c->*(o.field); return EMBA_OK; }
    for (const OptionRef& o : kStepPrepOptions)
        if (!strcmp(o.name, name)) { *value = c->*(o.field); return EMBA_OK; }
    if (!strcmp(name, "contrast_vote_path")) { *value = c->contrast_vote_path; return EMBA_OK; }      // read-only: the vote kernel of the last contrast call — 0 HBM, 1 LDS, -1 none yet
    for (const OptionRef& o : kContrastOptions)
        if (!strcmp(o.name, name)) { *value = c->*(o.field); return EMBA_OK; }
    if (!strcmp(name, "gram_paired")) { *value = c->last_gram_paired ? 1 : 0; return EMBA_OK; }      // read-only: the last Gram launch took the pair-aligned form
    for (const OptionRef& o : kGramOptions)
        if (!strcmp(o.name, name)) { *value = c->*(o.field); return EMBA_OK; }
    return fail(c, EMBA_ERR_INVALID_ARG, "unknown option '%s'", name);
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

emba_status emba_timer_start(emba_ctx* c, int32_t slot)
{
    if (!c || slot < 0 || slot >= 8) return EMBA_ERR_INVALID_ARG;
    HIP_TRY(c, hipEventRecord(c->ev_start[slot], c->stream));
    return EMBA_OK;
}

emba_status emba_timer_stop(emba_ctx* c, int32_t slot)
{
    if (!c || slot < 0 || slot >= 8) return EMBA_ERR_INVALID_ARG;
    HIP_TRY(c, hipEventRecord(c->ev_stop[slot], c->stream));
    return EMBA_OK;
}

emba_status emba_timer_elapsed_ms(emba_ctx* c, int32_t slot, float* ms)
{
    if (!c || !ms || slot < 0 || slot >= 8) return EMBA_ERR_INVALID_ARG;
    HIP_TRY(c, hipEventSynchronize(c->ev_stop[slot]));
    HIP_TRY(c, hipEventElapsedTime(ms, c->ev_start[slot], c->ev_stop[slot]));
    return EMBA_OK;
}

emba_status emba_enable_kernel_timing(emba_ctx* c, int32_t on)
{
    if (!c || on < 0 || on > 16) return EMBA_ERR_INVALID_ARG;
    c->kernel_timing = on != 0;
    if (on) {       // on = 1 + slot: the next evaluation / form record their events in that slot, to be read later (emba_kernel_ms_slot)
        const int slot = on - 1;
        for (int i = 0; i < 5; ++i) if (!c->kt_sets[slot][i]) HIP_TRY(c, hipEventCreate(&c->kt_sets[slot][i]));
        c->kt = c->kt_sets[slot]; c->kt_slot = slot;
        c->kt_valid[slot][0] = c->kt_valid[slot][1] = c->kt_valid[slot][2] = false;
    }
    c->kt_warp_valid = c->kt_accum_valid = false;
    return EMBA_OK;
}

emba_status emba_kernel_ms_slot(emba_ctx* c, int32_t slot, float* warp_ms, float* accum_ms)
{
    if (!c || slot < 0 || slot >= 16) return EMBA_ERR_INVALID_ARG;
    hipEvent_t* k = c->kt_sets[slot];
    if (warp_ms) {
        *warp_ms = -1.f;
        if (c->kt_valid[slot][0]) { HIP_TRY(c, hipEventSynchronize(k[1])); HIP_TRY(c, hipEventElapsedTime(warp_ms, k[0], k[1])); }
    }
    if (accum_ms) {
        *accum_ms = -1.f;
        if (c->kt_valid[slot][1]) { HIP_TRY(c, hipEventSynchronize(k[3])); HIP_TRY(c, hipEventElapsedTime(accum_ms, k[2], k[3])); }
    }
    return EMBA_OK;
}

emba_status emba_last_kernel_ms(emba_ctx* c, float* warp_ms, float* accum_ms)
{
    if (!c) return EMBA_ERR_INVALID_ARG;
    return emba_kernel_ms_slot(c, c->kt_slot, warp_ms, accum_ms);
}

emba_status emba_kernel_timing_all(emba_ctx* c, int32_t on)
{
    if (!c) return EMBA_ERR_INVALID_ARG;
    c->kt_all = on != 0;
    return EMBA_OK;
}

emba_status emba_kernel_ms_all(emba_ctx* c, int32_t slot, float* ms4)
{
    if (!c || !ms4 || slot < 0 || slot >= 16) return EMBA_ERR_INVALID_ARG;
    hipEvent_t* k = c->kt_sets[slot];
    for (int i = 0; i < 4; ++i) ms4[i] = -1.f;
    if (!(c->kt_valid[slot][0] && c->kt_valid[slot][1] && c->kt_valid[slot][2])) return EMBA_OK;
    HIP_TRY(c, hipEventSynchronize(k[3]));
    HIP_TRY(c, hipEventElapsedTime(ms4 + 0, k[4], k[0]));     // prep || pose || texel (+ the full texel pack where it is used)
    HIP_TRY(c, hipEventElapsedTime(ms4 + 1, k[0], k[1]));     // warp kernel
    HIP_TRY(c, hipEventElapsedTime(ms4 + 2, k[1], k[2]));     // launch A (+ the sweeping active write where it is a launch of its own)
    HIP_TRY(c, hipEventElapsedTime(ms4 + 3, k[2], k[3]));     // Gram kernel (with the gather inside)
    return EMBA_OK;
}

emba_status emba_bracket_overhead_us(emba_ctx* c, int32_t reps, float* us)
{
    if (!c || !us || reps < 1 || reps > 1000) return EMBA_ERR_INVALID_ARG;
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t s = c->stream;
    double sum = 0.0;
    for (int r = 0; r < reps; ++r) {
        // the bracket sits BEHIND queued work, like the brackets of a step: a busy kernel first, then event | empty kernel | event
        hipLaunchKernelGGL(emba_clock_probe_kernel, dim3(1), dim3(64), 0, s, c->d_probe.as<unsigned long long>() + 4, 256);
        HIP_TRY(c, hipEventRecord(c->cal_ev[0], s));
        hipLaunchKernelGGL(emba_empty_kernel, dim3(1), dim3(64), 0, s);
        HIP_TRY(c, hipEventRecord(c->cal_ev[1], s));
        HIP_TRY(c, hipEventSynchronize(c->cal_ev[1]));
        float ms = 0.f;
        HIP_TRY(c, hipEventElapsedTime(&ms, c->cal_ev[0], c->cal_ev[1]));
        sum += ms;
    }
    HIP_TRY(c, hipGetLastError());
    *us = (float)(sum / reps * 1e3);
    return EMBA_OK;
}

emba_status emba_clock_probe(emba_ctx* c, double* sclk_mhz_est, double* probe_us, double* memtime_per_realtime, int32_t* clock_rate_khz,
                             int32_t* mem_clock_rate_khz, int32_t* wall_clock_rate_khz)
{
    if (!c) return EMBA_ERR_INVALID_ARG;
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t s = c->stream;
    int v = 0;
    if (clock_rate_khz) { *clock_rate_khz = 0; if (hipDeviceGetAttribute(&v, hipDeviceAttributeClockRate, c->device) == hipSuccess) *clock_rate_khz = v; }
    if (mem_clock_rate_khz) { *mem_clock_rate_khz = 0; if (hipDeviceGetAttribute(&v, hipDeviceAttributeMemoryClockRate, c->device) == hipSuccess) *mem_clock_rate_khz = v; }
    int wall_khz = 100000;
    if (hipDeviceGetAttribute(&v, hipDeviceAttributeWallClockRate, c->device) == hipSuccess && v > 0) wall_khz = v;
    if (wall_clock_rate_khz) *wall_clock_rate_khz = wall_khz;
    // every SIMD of the chip busy with one wave's dependent chain of kClockProbeOps fp32 adds (4 cycles each on a 16-lane SIMD, issued back to back)
    const int loops = 1024;
    HIP_TRY(c, hipEventRecord(c->cal_ev[0], s));
    hipLaunchKernelGGL(emba_clock_probe_kernel, dim3((unsigned)c->n_cu), dim3(256), 0, s, c->d_probe.as<unsigned long long>(), loops);
    HIP_TRY(c, hipEventRecord(c->cal_ev[1], s));
    HIP_TRY(c, hipGetLastError());
    unsigned long long h[4] = {0, 0, 0, 0};
    HIP_TRY(c, hipMemcpyAsync(h, c->d_probe.as<unsigned long long>(), sizeof h, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipStreamSynchronize(s));
    c->spun = false;
    float ms = 0.f;
    HIP_TRY(c, hipEventElapsedTime(&ms, c->cal_ev[0], c->cal_ev[1]));
    const double wall_s = (double)h[1] / ((double)wall_khz * 1e3);      // the wave's own constant-rate clock around its chain
    if (probe_us) *probe_us = wall_s * 1e6;
    // s_memtime counts shader cycles (measured, round 5: 8.08 ticks per dependent v_add_f32 of the chain, the pipeline's 8-cycle dependent-issue
    // cadence; its ratio to the 100-MHz counter moves with the power state), so ticks(s_memtime) / seconds(s_memrealtime) IS the shader clock
    if (sclk_mhz_est) *sclk_mhz_est = wall_s > 0 ? (double)h[0] / wall_s * 1e-6 : 0.0;
    if (memtime_per_realtime) *memtime_per_realtime = h[1] ? (double)h[0] / ((double)kClockProbeUnroll * loops) : 0.0;
    (void)ms;
    return EMBA_OK;
}

emba_status emba_device_pci_bus_id(emba_ctx* c, char* buf, size_t len)
{
    if (!c || !buf || len < 16) return EMBA_ERR_INVALID_ARG;
    HIP_TRY(c, hipDeviceGetPCIBusId(buf, (int)len, c->device));
    return EMBA_OK;
}

}  // extern "C"

#include "solve_host.h"   // f1: the solvers

// ---- f3: intensity panorama from the gradient map ---------------------------------------------------------------------------
extern "C" emba_status emba_reconstruct_intensity(emba_ctx* c, const double* Gx_host, const double* Gy_host, double* M_host)
{
    if (!c) return EMBA_ERR_INVALID_ARG;
    if ((Gx_host == nullptr) != (Gy_host == nullptr)) return fail(c, EMBA_ERR_INVALID_ARG, "pass both Gx and Gy, or neither");
    if (!Gx_host && !c->map.state().resident()) return fail(c, EMBA_ERR_STATE, "no map resident");
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t s = c->stream;
    const int H = c->H, W = c->W;
    const size_t npix = c->npix;
    emba_status st;
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
    const bool fold = !dense && (H % 2 == 0) && H >= 64 && c->opt_poisson != 2;
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
        p.vec = ((K & 1) == 0 && (N & 1) == 0) ? 1 : 0;
        const long tm = (M + kGemmBM - 1) / kGemmBM, wide = tm * ((N + 127) / 128), narrow = tm * ((N + 63) / 64);
        const long big = ((M + kGemmBM2 - 1) / kGemmBM2) * ((N + kGemmBN2 - 1) / kGemmBN2);
        const bool use_big = big >= (long)c->n_cu && !c->opt_gemm64;
        if (use_big) hipLaunchKernelGGL(emba_dgemm128_kernel, dim3((unsigned)grid8(big)), dim3(512), 0, s, p);
        else if (wide >= 2L * c->n_cu) hipLaunchKernelGGL(emba_dgemm_kernel<128>, dim3((unsigned)grid8(wide)), dim3(256), 0, s, p);
        else hipLaunchKernelGGL(emba_dgemm_kernel<64>, dim3((unsigned)grid8(narrow)), dim3(256), 0, s, p);
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
        hipLaunchKernelGGL(emba_divergence_T_kernel, tg, dim3(256), 0, s, gx, gy, H, W, c->d_pT.as<double>());                     // F^T  (W x H), straight from the gradient maps
        dst_rows(c->d_pT.as<double>(), c->d_pF.as<double>(), c->d_pE.as<double>(), 1.0, false);                                                                 // (S_H F)^T = F^T S_H
        const unsigned tb = (unsigned)((H + kTriSys - 1) / kTriSys);
        hipLaunchKernelGGL(emba_tridiag_sweep_kernel<false>, dim3(tb), dim3(kTriSys * kTriChunks), 0, s, c->d_thomas.as<double>(), c->d_lamH.as<double>(), c->d_pF.as<double>(), H, W);   // (T_W + lambda1[i] I) x = g, per i
        hipLaunchKernelGGL(emba_tridiag_sweep_kernel<true>, dim3(tb), dim3(kTriSys * kTriChunks), 0, s, c->d_thomas.as<double>(), c->d_lamH.as<double>(), c->d_pF.as<double>(), H, W);
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
extern "C" emba_status emba_render_map_images(emba_ctx* c, double pct_discard, uint8_t* gx_u8, uint8_t* gy_u8, uint8_t* rgb_u8, uint8_t* poisson_u8)
{
    if (!c) return EMBA_ERR_INVALID_ARG;
    if (!(pct_discard >= 0.0 && pct_discard <= 100.0)) return fail(c, EMBA_ERR_INVALID_ARG, "pct_discard=%g outside [0, 100]", pct_discard);
    if (!c->map.state().resident()) return fail(c, EMBA_ERR_STATE, "no map resident");
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t s = c->stream;
    const size_t n = c->npix, o1 = img_off(n), o2 = o1 + img_off(n), o3 = o2 + img_off(3 * n);
    if (n >= ((size_t)1 << 31)) return fail(c, EMBA_ERR_CAPACITY, "%zu pixels: the select counts in 32 bits", n);
    emba_status st;
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
        if ((st = emba_reconstruct_intensity(c, nullptr, nullptr, nullptr))) return st;      // M stays in c->d_pF.as<double>()
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

#include "sequence_host.h"   // the resident event sequence of a sliding-window run: upload, windows, time shards and their halos, noise filters
#include "cmax_host.h"       // contrast maximisation on it: the angular velocity of every slice of events, from the events alone
#include "panorama_host.h"   // the panorama of warped events along a trajectory, and its contrast
#include "contrast_host.h"   // the smooth (fp64) contrast of that panorama and its gradient with respect to the control poses

// ---- single-process multi-GPU host (emba_group_*) ----------------------------------------------------------------------------
#include "group.h"
