// emba_amd/csrc/map_host.h — the calls that change, rebind or read the map planes: upload, bind, the trial update (updateMap) with accept / reject, the
// downloads, and the 3x3 median blur of the initial map.  What the host knows about the planes is MapState (map_rule.h, tested on the CPU); the buffers and
// pointers are emba_ctx::map (context.h: MapPlanes), whose functions move the pointers and the state together — no call here assigns either.
// Part of emba_hip.hip's translation unit, included by it below step_host.h (resolve_pending, ensure_compact) and transfer_host.h (d2h_pageable), above the
// solvers, which leave their x2 for updateMap through keep_x2.
#pragma once
#include "context.h"

using namespace emba;

extern "C" {

emba_status emba_upload_map(emba_ctx* c, const double* Gx, const double* Gy)
{
    if (!c || !Gx || !Gy) return c ? fail(c, EMBA_ERR_INVALID_ARG, "Gx/Gy NULL") : EMBA_ERR_INVALID_ARG;
    HIP_TRY(c, hipSetDevice(c->device));
    emba_status st;
    if ((st = ensure<double>(c, c->map.own_x, c->npix)) || (st = ensure<double>(c, c->map.own_y, c->npix))) return st;
    HIP_TRY(c, hipMemcpyAsync(c->map.own_x.as<double>(), Gx, c->npix * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(c->map.own_y.as<double>(), Gy, c->npix * sizeof(double), hipMemcpyHostToDevice, c->stream));
    c->map.uploaded();      // (a pending trial map is dropped)
    return EMBA_OK;
}

emba_status emba_bind_map_dev(emba_ctx* c, const double* Gx_dev, const double* Gy_dev)
{
    if (!c || !Gx_dev || !Gy_dev) return c ? fail(c, EMBA_ERR_INVALID_ARG, "Gx/Gy NULL") : EMBA_ERR_INVALID_ARG;
    c->map.bound(Gx_dev, Gy_dev);      // (a pending trial map is dropped; nothing touches the device: no hipSetDevice)
    return EMBA_OK;
}

}  // extern "C"

namespace {
emba_status ensure_x2(emba_ctx* c, size_t P)
{
    return ensure<double>(c, c->d_x2, std::max<size_t>(2 * P, 2));
}
// src_kind: 0 host pointer, 1 device pointer, 2 the x2 the last solve left in d_x2
emba_status update_map_impl(emba_ctx* c, const double* x2, int src_kind, double damping)
{
    if (!c) return EMBA_ERR_INVALID_ARG;
    if (!c->map.state().resident()) return fail(c, EMBA_ERR_STATE, "no map resident");
    if (!c->eq.active_done && !c->ev.P_pending) return fail(c, EMBA_ERR_STATE, "updateMap needs the active set of formNormalEq");
    HIP_TRY(c, hipSetDevice(c->device));
    emba_status st = resolve_pending(c);
    if (st) return st;
    if (src_kind == 2 && c->eq.P && c->solve.x2_resident_P != c->eq.P) return fail(c, EMBA_ERR_STATE, "x2 NULL: no solve of the current normal equations has left its x2 on the device");
    if (src_kind != 2 && c->eq.P && !x2) return fail(c, EMBA_ERR_INVALID_ARG, "x2 NULL");
    if ((st = ensure<double>(c, c->map.trial_x, c->npix)) || (st = ensure<double>(c, c->map.trial_y, c->npix))) return st;
    if ((st = ensure_x2(c, c->eq.P))) return st;
    hipStream_t s = c->stream;
    if ((st = ensure_compact(c))) return st;
    if (c->eq.P && src_kind != 2) {
        HIP_TRY(c, hipMemcpyAsync(c->d_x2.as<double>(), x2, 2 * c->eq.P * sizeof(double), src_kind == 0 ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, s));
        c->solve.x2_resident_P = (size_t)-1;      // (whatever a solve left there is overwritten)
    }
    // (from the CURRENT planes: a second update before an accept replaces the first trial, it does not build on it)
    hipLaunchKernelGGL(emba_update_map_kernel, dim3((unsigned)((c->npix + 255) / 256)), dim3(256), 0, s, c->map.cur_Gx(), c->map.cur_Gy(), c->d_compact.as<int32_t>(),
                       c->d_x2.as<double>(), damping, (long)c->npix, c->map.trial_x.as<double>(), c->map.trial_y.as<double>());
    HIP_TRY(c, hipGetLastError());
    if (src_kind == 0) HIP_TRY(c, hipStreamSynchronize(s));   // x2_host may be freed by the caller
    c->map.trial_built();
    return EMBA_OK;
}
// the solvers leave their x2 in d_x2 (device to device: 2P doubles), so that updateMap needs no trip through the host
emba_status keep_x2(emba_ctx* c, const double* d_src, size_t P)
{
    emba_status st = ensure_x2(c, P);
    if (st) return st;
    if (P) HIP_TRY(c, hipMemcpyAsync(c->d_x2.as<double>(), d_src, 2 * P * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
    c->solve.x2_resident_P = P;
    return EMBA_OK;
}
}  // namespace

extern "C" {

emba_status emba_update_map(emba_ctx* c, const double* x2_host, double damping) { return update_map_impl(c, x2_host, x2_host ? 0 : 2, damping); }
emba_status emba_update_map_dev(emba_ctx* c, const double* x2_dev, double damping) { return update_map_impl(c, x2_dev, x2_dev ? 1 : 2, damping); }

emba_status emba_map_accept(emba_ctx* c)
{
    if (!c) return EMBA_ERR_INVALID_ARG;
    if (!c->map.state().trial_pending()) return fail(c, EMBA_ERR_STATE, "no trial map (call emba_update_map first)");
    c->map.accepted();      // (the own and trial buffers swap; the version counts it although values and addresses are the trial's: map_rule.h)
    return EMBA_OK;
}

emba_status emba_map_reject(emba_ctx* c)
{
    if (!c) return EMBA_ERR_INVALID_ARG;
    // (no trial map: a step that moved the poses only — emba_solve_poses_only, no emba_update_map — was rejected; the map stays and its version with it, the
    // equations come back)
    c->map.rejected();
    return emba_trial_reject(c);           // and the normal equations the trial evaluation set aside are current again
}

emba_status emba_download_map(emba_ctx* c, double* Gx_host, double* Gy_host)
{
    if (!c || !Gx_host || !Gy_host) return c ? fail(c, EMBA_ERR_INVALID_ARG, "Gx/Gy NULL") : EMBA_ERR_INVALID_ARG;
    if (!c->map.state().resident()) return fail(c, EMBA_ERR_STATE, "no map resident");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipMemcpy(Gx_host, c->map.Gx(), c->npix * sizeof(double), hipMemcpyDeviceToHost));
    HIP_TRY(c, hipMemcpy(Gy_host, c->map.Gy(), c->npix * sizeof(double), hipMemcpyDeviceToHost));
    return EMBA_OK;
}

emba_status emba_get_map_active(emba_ctx* c, double* gxy_host, size_t cap_P)
{
    if (!c || !gxy_host) return c ? fail(c, EMBA_ERR_INVALID_ARG, "gxy_host NULL") : EMBA_ERR_INVALID_ARG;
    if (!c->map.state().resident()) return fail(c, EMBA_ERR_STATE, "no map resident");
    if (!c->eq.active_done && !c->ev.P_pending) return fail(c, EMBA_ERR_STATE, "no active set (formNormalEq) yet");
    // (only a trial map — emba_update_map's output — is zero outside the active set it was built from; an uploaded or accepted map is not)
    if (!c->map.state().trial_pending()) return fail(c, EMBA_ERR_STATE, "emba_get_map_active returns the trial map emba_update_map built; no trial map is resident");
    HIP_TRY(c, hipSetDevice(c->device));
    emba_status st = resolve_pending(c);
    if (st) return st;
    if (cap_P < c->eq.P) return fail(c, EMBA_ERR_CAPACITY, "cap_P=%zu < P=%zu", cap_P, c->eq.P);
    if (!c->eq.P) return EMBA_OK;
    if ((st = ensure<double>(c, c->dl.out, 2 * c->eq.P))) return st;
    double* d_out = c->dl.out.as<double>();
    hipLaunchKernelGGL(emba_map_active_kernel, dim3(nblocks(c->eq.P)), dim3(256), 0, c->stream, c->map.Gx(), c->map.Gy(), c->d_active.as<uint32_t>(), (long)c->eq.P, d_out);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(gxy_host, d_out, 2 * c->eq.P * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return EMBA_OK;
}

}  // extern "C"

// ---- 3x3 median blur of the initial map (emba.cpp:357-364) -----------------------------------------------------------------------
namespace {
void launch_median3(emba_ctx* c, const double* src, int h, int w, double* dst)
{
    hipLaunchKernelGGL(emba_median3_kernel, dim3((unsigned)((w + 63) / 64), (unsigned)((h + 3) / 4)), dim3(256), 0, c->stream, src, h, w, dst);
}
}  // namespace

extern "C" emba_status emba_median_blur3_map(emba_ctx* c)
{
    if (!c) return EMBA_ERR_INVALID_ARG;
    if (!c->map.state().resident()) return fail(c, EMBA_ERR_STATE, "no map resident");
    if (c->map.state().trial_pending()) return fail(c, EMBA_ERR_STATE, "a trial map is pending (emba_map_accept / emba_map_reject first)");
    HIP_TRY(c, hipSetDevice(c->device));
    emba_status st;
    if ((st = ensure<double>(c, c->d_blur, c->npix))) return st;
    // a map the caller bound (emba_bind_map_dev) is the caller's memory: the blurred map then becomes the context's own
    if (!c->map.state().current_is_own() && ((st = ensure<double>(c, c->map.own_x, c->npix)) || (st = ensure<double>(c, c->map.own_y, c->npix)))) return st;
    const double* src[2] = {c->map.cur_Gx(), c->map.cur_Gy()};
    double* dst[2] = {c->map.own_x.as<double>(), c->map.own_y.as<double>()};
    for (int k = 0; k < 2; ++k) {
        launch_median3(c, src[k], c->H, c->W, c->d_blur.as<double>());
        HIP_TRY(c, hipGetLastError());
        HIP_TRY(c, hipMemcpyAsync(dst[k], c->d_blur.as<double>(), c->npix * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
    }
    c->map.blurred();
    return EMBA_OK;
}

extern "C" emba_status emba_median_blur3(emba_ctx* c, const double* src_host, int32_t h, int32_t w, double* dst_host)
{
    if (!c) return EMBA_ERR_INVALID_ARG;
    if (!src_host || !dst_host || h <= 0 || w <= 0 || h > 4 * 65535 || (size_t)h * (size_t)w >= 0x7FFFFFFFull) return fail(c, EMBA_ERR_INVALID_ARG, "src / dst NULL or bad size %d x %d", h, w);
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t s = c->stream;
    const size_t n = (size_t)h * (size_t)w;
    emba_status st;
    if ((st = ensure<double>(c, c->d_nsrc, n)) || (st = ensure<double>(c, c->d_blur, n))) return st;
    HIP_TRY(c, hipMemcpyAsync(c->d_nsrc.as<double>(), src_host, n * sizeof(double), hipMemcpyHostToDevice, s));
    launch_median3(c, c->d_nsrc.as<double>(), h, w, c->d_blur.as<double>());
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipStreamSynchronize(s));
    return d2h_pageable(c, dst_host, c->d_blur.as<double>(), n * sizeof(double));
}
