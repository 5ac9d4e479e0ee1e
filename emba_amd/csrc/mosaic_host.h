// emba_amd/csrc/mosaic_host.h — the mosaic of intensity frames on the panorama, as host code over the kernels of mosaic_kernels.h: frames voted into two
// integer sums per cell along a trajectory (emba_mosaic_frames), their mean and coverage (emba_mosaic_get), the log-intensity plane and its backward
// differences as a gradient map, on request the context's resident map (emba_mosaic_map), and emba_mosaic_clear.  What is plain arithmetic — the argument
// checks, the 2^36 bound, the mean, the tone's inverse, the differences — is decided in mosaic_rule.h; here are the buffers (emba_ctx::mosaic), the launches
// and the C ABI.
// Part of emba_hip.hip's translation unit, included by it below view_host.h; it uses sequence_host.h (SEQ_TRY), transfer_host.h (d2h_pageable) and
// panorama_host.h (kSeqStageTimerSlot).  mosaic_vote_frames is emba_mosaic_frames_exposure's as well (exposure_host.h): with gains and biases it launches the
// vote kernel of exposure_kernels.h and keeps them in emba_ctx::exposure (vote_gain, vote_bias).  Nothing of the registered window, of the resident sequence or of any other stage's buffers is read or written; with
// make_resident the map planes take the transition of emba_upload_map (map_rule.h: MapState::uploaded), and nothing else.
#pragma once
#include "context.h"
#include "exposure_kernels.h"
#include "mosaic_kernels.h"
#include "mosaic_rule.h"

using namespace emba;

namespace {
emba_status mosaic_zero_sums(emba_ctx* c)      // both sums exist and are zero (on the stream); nothing is accumulated
{
    MosaicBuffers& B = c->mosaic;
    SEQ_TRY(ensure<unsigned long long>(c, B.sum_w, c->npix));
    SEQ_TRY(ensure<unsigned long long>(c, B.sum_v, c->npix));
    HIP_TRY(c, hipMemsetAsync(B.sum_w.p, 0, c->npix * sizeof(unsigned long long), c->stream));
    HIP_TRY(c, hipMemsetAsync(B.sum_v.p, 0, c->npix * sizeof(unsigned long long), c->stream));
    B.votes = 0;
    return EMBA_OK;
}
// the mean, the covered bytes and their number of the sums as they stand, into B.mean / B.covered / B.counters[2]
emba_status mosaic_launch_mean(emba_ctx* c, uint64_t min_weight, double fill)
{
    MosaicBuffers& B = c->mosaic;
    SEQ_TRY(ensure<double>(c, B.mean, c->npix));
    SEQ_TRY(ensure<uint8_t>(c, B.covered, c->npix));
    SEQ_TRY(ensure<unsigned long long>(c, B.counters, 4));
    HIP_TRY(c, hipMemsetAsync(B.counters.as<unsigned long long>() + 2, 0, sizeof(unsigned long long), c->stream));
    hipLaunchKernelGGL(emba_mosaic_mean_kernel, dim3(nblocks(c->npix, kMosaicThreads)), dim3(kMosaicThreads), 0, c->stream, (const unsigned long long*)B.sum_w.as<unsigned long long>(),
                       (const unsigned long long*)B.sum_v.as<unsigned long long>(), (long)c->npix, (unsigned long long)min_weight, fill, B.mean.as<double>(), B.covered.as<uint8_t>(),
                       B.counters.as<unsigned long long>() + 2);
    HIP_TRY(c, hipGetLastError());
    return EMBA_OK;
}

// what emba_mosaic_frames and emba_mosaic_frames_exposure take, as the C ABI hands it over
struct MosaicCall {
    const uint8_t* frames; const int64_t* frame_t_ns; size_t F; const double* knots_xyzw; int32_t K; int64_t t0_ns, dt_ns; int32_t skip_zero, accumulate;
    uint64_t *dropped_out, *skipped_out; double* pm_out;
};

emba_status mosaic_refusals(emba_ctx* c, const MosaicCall& m)
{
    const size_t S = c->S, F = m.F;
    const uint64_t have = m.accumulate ? c->mosaic.votes : 0;
    switch (mosaic_args_ok(m.frames != nullptr, m.frame_t_ns != nullptr, m.knots_xyzw != nullptr, F, S, have, m.K, m.dt_ns)) {
    case MosaicArgStatus::ok: break;
    case MosaicArgStatus::frames_null: return fail(c, EMBA_ERR_INVALID_ARG, "frames NULL");
    case MosaicArgStatus::times_null: return fail(c, EMBA_ERR_INVALID_ARG, "frame_t_ns NULL");
    case MosaicArgStatus::knots_null: return fail(c, EMBA_ERR_INVALID_ARG, "knots NULL");
    case MosaicArgStatus::too_few_knots: return fail(c, EMBA_ERR_INVALID_ARG, "K = %d: a linear spline has at least two control poses", (int)m.K);
    case MosaicArgStatus::bad_dt: return fail(c, EMBA_ERR_INVALID_ARG, "dt_ns = %lld: the knot spacing must be positive", (long long)m.dt_ns);
    case MosaicArgStatus::too_many_frames: return fail(c, EMBA_ERR_INVALID_ARG, "F = %zu: the pose stage counts its frames in 31 bits", F);
    case MosaicArgStatus::too_many_votes:
        return fail(c, EMBA_ERR_INVALID_ARG, "%llu votes accumulated and %zu frames of %zu pixels more: the sums are exact below 2^36 votes", (unsigned long long)have, F, S);
    }
    return EMBA_OK;
}

// The frames of a call that has passed its refusals, voted into the two sums: the pose stage, then chunk by chunk the bytes up and the vote kernel.  gain, bias:
// nullptr (emba_mosaic_vote_kernel), or the F gains and biases the bytes are compensated with (emba_mosaic_exposure_vote_kernel).  Every buffer of the call is
// allocated before anything is written.
emba_status mosaic_vote_frames(emba_ctx* c, const MosaicCall& m, const double* gain, const double* bias)
{
    MosaicBuffers& B = c->mosaic;
    ExposureBuffers& X = c->exposure;
    const size_t S = c->S, F = m.F;
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t s = c->stream;
    if (!F) {      // no frame: nothing is voted; without `accumulate` the sums are zeroed all the same
        if (!m.accumulate) { SEQ_TRY(mosaic_zero_sums(c)); HIP_TRY(c, hipStreamSynchronize(s)); }
        if (m.dropped_out) *m.dropped_out = 0;
        if (m.skipped_out) *m.skipped_out = 0;
        return EMBA_OK;
    }
    const size_t per = view_chunk_frames(S, 1), chunks = view_chunk_count(F, per), cap = std::min(per, F) * S;
    SEQ_TRY(ensure<int64_t>(c, B.t, F));
    SEQ_TRY(ensure<double>(c, B.pose, F * (size_t)kPoseStride));
    SEQ_TRY(ensure<double>(c, B.knots, 4 * (size_t)m.K));
    SEQ_TRY(ensure<uint64_t>(c, B.head, 1));
    SEQ_TRY(ensure<unsigned long long>(c, B.counters, 4));
    SEQ_TRY(ensure<unsigned long long>(c, B.sum_w, c->npix));
    SEQ_TRY(ensure<unsigned long long>(c, B.sum_v, c->npix));
    SEQ_TRY(ensure<uint8_t>(c, B.frames, cap));
    if (m.pm_out) SEQ_TRY(ensure<double>(c, B.pm, 2 * cap));
    if (gain) { SEQ_TRY(ensure<double>(c, X.vote_gain, F)); SEQ_TRY(ensure<double>(c, X.vote_bias, F)); }
    // pose stage: every frame time at once, into this stage's own table; the status word as emba_render_views keeps it
    HIP_TRY(c, hipMemcpyAsync(B.knots.p, m.knots_xyzw, (size_t)m.K * 32, hipMemcpyHostToDevice, s));
    HIP_TRY(c, hipMemcpyAsync(B.t.p, m.frame_t_ns, F * sizeof(int64_t), hipMemcpyHostToDevice, s));
    if (gain) {
        HIP_TRY(c, hipMemcpyAsync(X.vote_gain.p, gain, F * sizeof(double), hipMemcpyHostToDevice, s));
        HIP_TRY(c, hipMemcpyAsync(X.vote_bias.p, bias, F * sizeof(double), hipMemcpyHostToDevice, s));
    }
    HIP_TRY(c, hipMemsetAsync(B.head.p, 0, 8, s));
    HIP_TRY(c, hipMemsetAsync(B.counters.p, 0, 2 * sizeof(unsigned long long), s));
    hipLaunchKernelGGL(emba_pose_kernel, dim3(nblocks(F, 64)), dim3(64), 0, s, (const int64_t*)B.t.as<int64_t>(), (int)F, (const double*)B.knots.as<double>(), (int)m.K, m.t0_ns,
                       m.dt_ns, B.pose.as<double>(), reinterpret_cast<int*>(B.head.as<uint64_t>()));
    HIP_TRY(c, hipGetLastError());
    uint64_t word = 0;
    HIP_TRY(c, hipMemcpyAsync(&word, B.head.p, 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipStreamSynchronize(s));      // (the caller's arrays have been read; a frame outside the knots is refused before anything is voted)
    if ((int)(word & 0xFFFFFFFFull) & 1) return fail(c, EMBA_ERR_TIME_RANGE, "a frame time lies outside the spline's knots");
    if (!m.accumulate || !B.votes) SEQ_TRY(mosaic_zero_sums(c));      // the sums: zero without `accumulate` (and where nothing is accumulated yet)

    // frames, chunk by chunk: the bytes go up, the votes stay on the device
    for (size_t i = 0; i < chunks; ++i) {
        const ViewChunk ch = view_chunk(F, per, i);
        const size_t cells = ch.nf * S, off = ch.f0 * S;
        const bool timed = c->kernel_timing && i == 0;      // (emba_enable_kernel_timing: slot 7 is the first chunk's vote kernel)
        const dim3 grid(nblocks(S, kMosaicThreads), (unsigned)ch.nf);
        HIP_TRY(c, hipMemcpyAsync(B.frames.p, m.frames + off, cells, hipMemcpyHostToDevice, s));
        const MosaicVoteParams P{c->d_lut.as<double>(), B.pose.as<double>() + (size_t)kPoseStride * ch.f0, B.frames.as<uint8_t>(), (int)S, c->W, c->H, c->fx, c->fy, c->cx, c->cy,
                                 m.skip_zero != 0, B.sum_w.as<unsigned long long>(), B.sum_v.as<unsigned long long>(), m.pm_out ? B.pm.as<double>() : nullptr,
                                 B.counters.as<unsigned long long>()};
        if (timed) HIP_TRY(c, hipEventRecord(c->ev_start[kSeqStageTimerSlot], s));
        if (!gain) hipLaunchKernelGGL(emba_mosaic_vote_kernel, grid, dim3(kMosaicThreads), 0, s, P);
        else {
            const ExposureVoteParams PX{P.lut, P.pose, X.vote_gain.as<double>() + ch.f0, X.vote_bias.as<double>() + ch.f0, P.frames, P.S, P.W, P.H, P.fx, P.fy, P.cx, P.cy,
                                        P.skip_zero, P.sum_w, P.sum_v, P.pm, P.counters};
            hipLaunchKernelGGL(emba_mosaic_exposure_vote_kernel, grid, dim3(kMosaicThreads), 0, s, PX);
        }
        if (timed) HIP_TRY(c, hipEventRecord(c->ev_stop[kSeqStageTimerSlot], s));
        HIP_TRY(c, hipGetLastError());
        HIP_TRY(c, hipStreamSynchronize(s));      // (the chunk's bytes have been read: the next chunk overwrites them)
        B.votes += cells;
        if (m.pm_out) SEQ_TRY(d2h_pageable(c, m.pm_out + 2 * off, B.pm.p, 2 * cells * sizeof(double)));
    }
    unsigned long long cnt[2] = {0, 0};
    HIP_TRY(c, hipMemcpy(cnt, B.counters.p, sizeof cnt, hipMemcpyDeviceToHost));
    if (m.dropped_out) *m.dropped_out = cnt[0];
    if (m.skipped_out) *m.skipped_out = cnt[1];
    return EMBA_OK;
}
}  // namespace

extern "C" emba_status emba_mosaic_clear(emba_ctx* c)
{
    if (!c) return EMBA_ERR_INVALID_ARG;
    HIP_TRY(c, hipSetDevice(c->device));
    SEQ_TRY(mosaic_zero_sums(c));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return EMBA_OK;
}

extern "C" emba_status emba_mosaic_frames(emba_ctx* c, const uint8_t* frames, const int64_t* frame_t_ns, size_t F, const double* knots_xyzw, int32_t K, int64_t t0_ns,
                                          int64_t dt_ns, int32_t skip_zero, int32_t accumulate, uint64_t* dropped_out, uint64_t* skipped_out, double* pm_out)
{
    if (!c) return EMBA_ERR_INVALID_ARG;
    const MosaicCall m{frames, frame_t_ns, F, knots_xyzw, K, t0_ns, dt_ns, skip_zero, accumulate, dropped_out, skipped_out, pm_out};
    SEQ_TRY(mosaic_refusals(c, m));
    return mosaic_vote_frames(c, m, nullptr, nullptr);
}

extern "C" emba_status emba_mosaic_get(emba_ctx* c, uint64_t min_weight, double fill, uint64_t* sum_w_out, uint64_t* sum_v_out, double* mean_out, uint8_t* covered_out,
                                       uint64_t* n_covered_out)
{
    if (!c) return EMBA_ERR_INVALID_ARG;
    switch (mosaic_get_args_ok(min_weight, fill)) {
    case MosaicToneStatus::ok: break;
    case MosaicToneStatus::bad_min_weight: return fail(c, EMBA_ERR_INVALID_ARG, "min_weight = 0: a covered cell has a weight of 1 at the least");
    default: return fail(c, EMBA_ERR_INVALID_ARG, "fill = %g is not finite", fill);
    }
    MosaicBuffers& B = c->mosaic;
    if (!B.votes) return fail(c, EMBA_ERR_STATE, "nothing accumulated (emba_mosaic_frames first)");
    HIP_TRY(c, hipSetDevice(c->device));
    if (mean_out || covered_out || n_covered_out) SEQ_TRY(mosaic_launch_mean(c, min_weight, fill));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (sum_w_out) SEQ_TRY(d2h_pageable(c, sum_w_out, B.sum_w.p, c->npix * sizeof(uint64_t)));
    if (sum_v_out) SEQ_TRY(d2h_pageable(c, sum_v_out, B.sum_v.p, c->npix * sizeof(uint64_t)));
    if (mean_out) SEQ_TRY(d2h_pageable(c, mean_out, B.mean.p, c->npix * sizeof(double)));
    if (covered_out) SEQ_TRY(d2h_pageable(c, covered_out, B.covered.p, c->npix));
    if (n_covered_out) {
        unsigned long long n = 0;
        HIP_TRY(c, hipMemcpy(&n, B.counters.as<unsigned long long>() + 2, sizeof n, hipMemcpyDeviceToHost));
        *n_covered_out = n;
    }
    return EMBA_OK;
}

extern "C" emba_status emba_mosaic_map(emba_ctx* c, uint64_t min_weight, double lo, double hi, double eps, int32_t take_log, double* L_out, double* Gx_out, double* Gy_out,
                                       int32_t make_resident)
{
    if (!c) return EMBA_ERR_INVALID_ARG;
    switch (mosaic_map_args_ok(min_weight, lo, hi, eps)) {
    case MosaicToneStatus::ok: break;
    case MosaicToneStatus::bad_min_weight: return fail(c, EMBA_ERR_INVALID_ARG, "min_weight = 0: a covered cell has a weight of 1 at the least");
    case MosaicToneStatus::not_finite: return fail(c, EMBA_ERR_INVALID_ARG, "lo = %g, hi = %g, eps = %g: the tone needs finite values", lo, hi, eps);
    case MosaicToneStatus::hi_not_above_lo: return fail(c, EMBA_ERR_INVALID_ARG, "hi = %g is not above lo = %g", hi, lo);
    }
    MosaicBuffers& B = c->mosaic;
    if (!B.votes) return fail(c, EMBA_ERR_STATE, "nothing accumulated (emba_mosaic_frames first)");
    if (!L_out && !Gx_out && !Gy_out && !make_resident) return EMBA_OK;      // nothing asked for: nothing launched
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t s = c->stream;
    const size_t n = c->npix;
    SEQ_TRY(mosaic_launch_mean(c, min_weight, 0.0));
    SEQ_TRY(ensure<double>(c, B.L, n));
    SEQ_TRY(ensure<uint8_t>(c, B.covered_log, n));
    SEQ_TRY(ensure<double>(c, B.gx, n));
    SEQ_TRY(ensure<double>(c, B.gy, n));
    if (make_resident) { SEQ_TRY(ensure<double>(c, c->map.own_x, n)); SEQ_TRY(ensure<double>(c, c->map.own_y, n)); }
    hipLaunchKernelGGL(emba_mosaic_log_kernel, dim3(nblocks(n, kMosaicThreads)), dim3(kMosaicThreads), 0, s, (const double*)B.mean.as<double>(), (const uint8_t*)B.covered.as<uint8_t>(),
                       (long)n, lo, hi, eps, (int)(take_log != 0), B.L.as<double>(), B.covered_log.as<uint8_t>());
    HIP_TRY(c, hipGetLastError());
    hipLaunchKernelGGL(emba_mosaic_map_kernel, dim3(nblocks(n, kMosaicThreads)), dim3(kMosaicThreads), 0, s, (const double*)B.L.as<double>(), (const uint8_t*)B.covered_log.as<uint8_t>(),
                       c->W, c->H, B.gx.as<double>(), B.gy.as<double>());
    HIP_TRY(c, hipGetLastError());
    if (make_resident) {      // device to device into the context's own planes: the transition of emba_upload_map (a pending trial map is dropped)
        HIP_TRY(c, hipMemcpyAsync(c->map.own_x.as<double>(), B.gx.p, n * sizeof(double), hipMemcpyDeviceToDevice, s));
        HIP_TRY(c, hipMemcpyAsync(c->map.own_y.as<double>(), B.gy.p, n * sizeof(double), hipMemcpyDeviceToDevice, s));
        c->map.uploaded();
    }
    HIP_TRY(c, hipStreamSynchronize(s));
    if (L_out) SEQ_TRY(d2h_pageable(c, L_out, B.L.p, n * sizeof(double)));
    if (Gx_out) SEQ_TRY(d2h_pageable(c, Gx_out, B.gx.p, n * sizeof(double)));
    if (Gy_out) SEQ_TRY(d2h_pageable(c, Gy_out, B.gy.p, n * sizeof(double)));
    return EMBA_OK;
}
