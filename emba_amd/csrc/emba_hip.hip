// emba_amd/csrc/emba_hip.hip — the translation unit behind the C ABI of include/emba_hip.h.  Here: the includes in dependency order, emba_abi_version,
// emba_build_info, emba_last_error, emba_create and emba_destroy.  Everything else is a host header, where it has arithmetic of its own with a HIP-free rule
// header beside it: the context is context.h, copies into the caller's pageable memory transfer_host.h, the window and its order order_host.h / order_rule.h,
// the step path (the evaluation and the normal equations) step_host.h / step_rule.h, the map map_host.h / map_rule.h, the downloads that wait on the step's
// counters and emba_dump_state readback_host.h, the costs cost_host.h / cost_rule.h, the options options_host.h, the timers and probes timing_host.h, the
// solvers (f1) solve_host.h / solve_rule.h, f3 poisson_host.h / poisson_rule.h, the record_data images render_host.h, the resident event sequence sequence_host.h / sequence_rule.h,
// contrast maximisation on it cmax_host.h / cmax_rule.h, the panorama of warped events panorama_host.h / panorama_rule.h and its smooth contrast and gradient
// contrast_host.h / contrast_rule.h, the sensor views along the trajectory view_host.h / view_rule.h, the mosaic of intensity frames mosaic_host.h / mosaic_rule.h, the event simulator
// sim_host.h / sim_rule.h, the stages over intensity frames frame_host.h (what they share) and align_host.h / align_rule.h, track_host.h / track_rule.h,
// exposure_host.h / exposure_rule.h, track_exposure_host.h / track_exposure_rule.h, refit_host.h / refit_rule.h, pair_host.h / pair_rule.h / graph_rule.h, pair_level_host.h / pair_level_rule.h, match_host.h / match_rule.h, the multi-GPU group group.h: all one translation unit.
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
#include "cost_kernels.h"
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

#include "map_host.h"        // upload, bind, updateMap, accept / reject, the map downloads, the median blur (needs resolve_pending, ensure_compact)
#include "readback_host.h"   // ep, the inlier numbers and pixels, the sparse A12 factors, emba_dump_state, emba_last_counts, emba_sync
#include "cost_host.h"       // dataCost and regCost: one launch, one wait
#include "options_host.h"    // emba_set_option / emba_get_option: the one table
#include "timing_host.h"     // the timers, kernel timing, the bracket overhead, the clock probe
#include "solve_host.h"      // f1: the solvers
#include "poisson_host.h"    // f3: the intensity panorama from the gradient map
#include "render_host.h"     // the record_data map images (the panorama among them)
#include "sequence_host.h"   // the resident event sequence of a sliding-window run: upload, windows, time shards and their halos, noise filters
#include "cmax_host.h"       // contrast maximisation on it: the angular velocity of every slice of events, from the events alone
#include "panorama_host.h"   // the panorama of warped events along a trajectory, and its contrast
#include "contrast_host.h"   // the smooth (fp64) contrast of that panorama and its gradient with respect to the control poses
#include "view_host.h"       // sensor views along the trajectory: the frames the camera would have seen, the event counts it reported
#include "mosaic_host.h"     // the way back: intensity frames stitched into the panorama along the trajectory, and the gradient map made from the mosaic
#include "sim_host.h"        // the event simulator: a recording from a panorama plane and a trajectory, and its way into the resident sequence
#include "frame_host.h"      // what the stages over intensity frames below share: the buffers of a chunk, one evaluation, the chunked evaluation, the per-frame loop
#include "align_host.h"      // poses from frames: each intensity frame's rotation aligned to a panorama plane (the mosaic's mean, or a caller's)
#include "track_host.h"      // poses from the frames alone: each frame aligned to the growing mosaic of the frames before it, then voted into it
#include "exposure_host.h"   // per-frame exposure: a gain and a bias estimated with each frame's rotation, and applied when the frames are stitched
#include "track_exposure_host.h"   // the tracker with exposure: gain and bias estimated with the rotation at every level, compensated bytes voted
#include "refit_host.h"      // tracked frames refitted: each batch taken out of the integer planes, aligned to the mosaic of the others, voted back
#include "pair_host.h"       // loops closed among tracked frames: one frame aligned to another, pair by pair, and the rotation graph over all of them (host)
#include "pair_level_host.h" // ... coarse to fine over a pyramid of the sensor frames, with the pair's exposure estimated
#include "match_host.h"      // loop-closure pairs found by appearance: thumbnails compared under every shift of a range, per frame the k best partners

// ---- single-process multi-GPU host (emba_group_*) ----------------------------------------------------------------------------
#include "group.h"

