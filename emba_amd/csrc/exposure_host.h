// emba_amd/csrc/exposure_host.h — per-frame exposure, as host code over the kernels of exposure_kernels.h: one evaluation of every frame's 5-parameter normal
// equations (emba_frames_exposure_eval), the per-frame Levenberg-Marquardt loop on them (emba_frames_exposure_align), and the mosaic of compensated frames
// (emba_mosaic_frames_exposure).  What is plain arithmetic is decided in exposure_rule.h and align_rule.h; here are the buffers (emba_ctx::exposure), the
// launches and the C ABI.
// Part of emba_hip.hip's translation unit, included by it below track_host.h; it uses align_host.h (AlignCall, align_refusals, align_load_plane: the plane
// and its mask live in emba_ctx::align, scratch there as here), mosaic_host.h (mosaic_zero_sums, mosaic_launch_mean; the pose table, the chunk of bytes and
// the counters of the vote are emba_ctx::mosaic's scratch), sequence_host.h (SEQ_TRY), transfer_host.h (d2h_pageable) and panorama_host.h
// (kSeqStageTimerSlot).  Every buffer of a call is allocated before anything is written.  Nothing of the registered window, of the resident sequence or of
// the resident map is written; the mosaic's sums are written by emba_mosaic_frames_exposure alone.
#pragma once
#include "align_host.h"
#include "context.h"
#include "exposure_kernels.h"
#include "exposure_rule.h"
#include "mosaic_host.h"

using namespace emba;

namespace {
// the refusals of the gains and biases, behind the original's
emba_status exposure_refusals(emba_ctx* c, const double* gain, const double* bias, size_t F)
{
    size_t bad = 0;
    switch (exposure_args_ok(gain, bias, F, &bad)) {
    case ExposureArgStatus::ok: break;
    case ExposureArgStatus::gain_null: return fail(c, EMBA_ERR_INVALID_ARG, "gain NULL");
    case ExposureArgStatus::bias_null: return fail(c, EMBA_ERR_INVALID_ARG, "bias NULL");
    case ExposureArgStatus::gain_not_finite: return fail(c, EMBA_ERR_INVALID_ARG, "gain[%zu] is not finite", bad);
    case ExposureArgStatus::gain_not_positive: return fail(c, EMBA_ERR_INVALID_ARG, "gain[%zu] = %g is not positive", bad, gain[bad]);
    case ExposureArgStatus::bias_not_finite: return fail(c, EMBA_ERR_INVALID_ARG, "bias[%zu] is not finite", bad);
    }
    return EMBA_OK;
}

// every buffer of a call over chunks of at most `nf` frames, the plane's and the mosaic's mean among them; `loop`: the frames' state as well
emba_status exposure_ensure(emba_ctx* c, const AlignCall& a, size_t nf, bool want_pm, bool want_resid, bool loop)
{
    ExposureBuffers& B = c->exposure;
    const size_t S = c->S, nb = nblocks(S, kExposureThreads), n = c->npix;
    SEQ_TRY(ensure<double>(c, c->align.plane, n));
    if (!a.plane_host || a.valid_host) SEQ_TRY(ensure<uint8_t>(c, c->align.valid, n));
    if (!a.plane_host) {
        SEQ_TRY(ensure<double>(c, c->mosaic.mean, n));
        SEQ_TRY(ensure<uint8_t>(c, c->mosaic.covered, n));
        SEQ_TRY(ensure<unsigned long long>(c, c->mosaic.counters, 4));
    }
    SEQ_TRY(ensure<uint8_t>(c, B.frames, nf * S));
    if (want_pm) SEQ_TRY(ensure<double>(c, B.pm, 2 * nf * S));
    if (want_resid) SEQ_TRY(ensure<double>(c, B.resid, nf * S));
    SEQ_TRY(ensure<double>(c, B.partial, nf * nb * (size_t)kExposurePartial));
    SEQ_TRY(ensure<double>(c, B.q_trial, 4 * nf));
    SEQ_TRY(ensure<double>(c, B.gain_trial, nf));
    SEQ_TRY(ensure<double>(c, B.bias_trial, nf));
    SEQ_TRY(ensure<double>(c, B.esums, (size_t)kExposureSums * nf));
    SEQ_TRY(ensure<unsigned long long>(c, B.ecounts, 4 * nf));
    if (!loop) return EMBA_OK;
    SEQ_TRY(ensure<double>(c, B.q, 4 * nf));
    SEQ_TRY(ensure<double>(c, B.gain, nf));
    SEQ_TRY(ensure<double>(c, B.bias, nf));
    SEQ_TRY(ensure<double>(c, B.sums, (size_t)kExposureSums * nf));
    SEQ_TRY(ensure<unsigned long long>(c, B.counts, 4 * nf));
    SEQ_TRY(ensure<double>(c, B.lambda, nf));
    SEQ_TRY(ensure<double>(c, B.dnorm, nf));
    SEQ_TRY(ensure<int32_t>(c, B.status, nf));
    SEQ_TRY(ensure<int32_t>(c, B.iters, nf));
    SEQ_TRY(ensure<int32_t>(c, B.have_trial, nf));
    SEQ_TRY(ensure<double>(c, B.cost0, nf));
    SEQ_TRY(ensure<unsigned long long>(c, B.n0, nf));
    SEQ_TRY(ensure<unsigned int>(c, B.running, 1));
    return EMBA_OK;
}

// a chunk's bytes, rotations, gains and biases into the buffers every frame is evaluated from
emba_status exposure_upload_chunk(emba_ctx* c, const AlignCall& a, const double* gain, const double* bias, const ViewChunk& ch)
{
    ExposureBuffers& B = c->exposure;
    hipStream_t s = c->stream;
    const size_t S = c->S;
    HIP_TRY(c, hipMemcpyAsync(B.frames.p, a.frames + ch.f0 * S, ch.nf * S, hipMemcpyHostToDevice, s));
    HIP_TRY(c, hipMemcpyAsync(B.q_trial.p, a.q_xyzw + 4 * ch.f0, 4 * ch.nf * sizeof(double), hipMemcpyHostToDevice, s));
    HIP_TRY(c, hipMemcpyAsync(B.gain_trial.p, gain + ch.f0, ch.nf * sizeof(double), hipMemcpyHostToDevice, s));
    HIP_TRY(c, hipMemcpyAsync(B.bias_trial.p, bias + ch.f0, ch.nf * sizeof(double), hipMemcpyHostToDevice, s));
    return EMBA_OK;
}

// one evaluation of the chunk's nf frames at the trial arrays into B.esums / B.ecounts: the evaluation kernel and the reduction of its partial sums.
// `status`: the frames' status words, or nullptr (every frame is evaluated); `timed`: timer slot 7 around the evaluation kernel
emba_status exposure_launch_eval(emba_ctx* c, const AlignCall& a, const uint8_t* valid, size_t nf, const int32_t* status, bool want_pm, bool want_resid, bool timed)
{
    ExposureBuffers& B = c->exposure;
    hipStream_t s = c->stream;
    const unsigned nb = nblocks(c->S, kExposureThreads);
    ExposureEvalParams P{c->d_lut.as<double>(), B.q_trial.as<double>(), B.gain_trial.as<double>(), B.bias_trial.as<double>(), status, B.frames.as<uint8_t>(),
                         c->align.plane.as<double>(), valid, (int)c->S, c->W, c->H, c->fx, c->fy, c->cx, c->cy, a.lo, a.hi, a.huber_k, a.skip_zero != 0,
                         B.partial.as<double>(), want_pm ? B.pm.as<double>() : nullptr, want_resid ? B.resid.as<double>() : nullptr};
    if (timed) HIP_TRY(c, hipEventRecord(c->ev_start[kSeqStageTimerSlot], s));
    hipLaunchKernelGGL(emba_frames_exposure_eval_kernel, dim3(nb, (unsigned)nf), dim3(kExposureThreads), 0, s, P);
    if (timed) HIP_TRY(c, hipEventRecord(c->ev_stop[kSeqStageTimerSlot], s));
    HIP_TRY(c, hipGetLastError());
    hipLaunchKernelGGL(emba_frames_exposure_reduce_kernel, dim3(nblocks(nf * (size_t)(kExposureSums + 4), kExposureThreads)), dim3(kExposureThreads), 0, s,
                       (const double*)B.partial.as<double>(), (int)nb, (long)nf, status, B.esums.as<double>(), B.ecounts.as<unsigned long long>());
    HIP_TRY(c, hipGetLastError());
    return EMBA_OK;
}
}  // namespace

extern "C" emba_status emba_frames_exposure_eval(emba_ctx* c, const uint8_t* frames, size_t F, const double* q_xyzw, const double* gain, const double* bias,
                                                 const double* plane_host, const uint8_t* valid_host, int32_t use_mosaic, uint64_t min_weight, double fill, double lo,
                                                 double hi, int32_t skip_zero, double huber_k, double* sums_out, uint64_t* counts_out, double* pm_out, double* resid_out)
{
    if (!c) return EMBA_ERR_INVALID_ARG;
    const AlignCall a{frames, F, q_xyzw, plane_host, valid_host, use_mosaic, min_weight, fill, lo, hi, skip_zero, huber_k};
    SEQ_TRY(align_refusals(c, a));
    SEQ_TRY(exposure_refusals(c, gain, bias, F));
    if (!F) return EMBA_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t s = c->stream;
    ExposureBuffers& B = c->exposure;
    const size_t S = c->S, per = view_chunk_frames(S, 1), chunks = view_chunk_count(F, per);
    SEQ_TRY(exposure_ensure(c, a, std::min(per, F), pm_out != nullptr, resid_out != nullptr, false));
    const uint8_t* valid = nullptr;
    SEQ_TRY(align_load_plane(c, a, &valid));
    for (size_t i = 0; i < chunks; ++i) {
        const ViewChunk ch = view_chunk(F, per, i);
        const size_t cells = ch.nf * S, off = ch.f0 * S;
        SEQ_TRY(exposure_upload_chunk(c, a, gain, bias, ch));
        SEQ_TRY(exposure_launch_eval(c, a, valid, ch.nf, nullptr, pm_out != nullptr, resid_out != nullptr, c->kernel_timing && i == 0));
        HIP_TRY(c, hipStreamSynchronize(s));      // (the chunk's bytes have been read: the next chunk overwrites them)
        if (sums_out) SEQ_TRY(d2h_pageable(c, sums_out + (size_t)kExposureSums * ch.f0, B.esums.p, (size_t)kExposureSums * ch.nf * sizeof(double)));
        if (counts_out) SEQ_TRY(d2h_pageable(c, counts_out + 4 * ch.f0, B.ecounts.p, 4 * ch.nf * sizeof(uint64_t)));
        if (pm_out) SEQ_TRY(d2h_pageable(c, pm_out + 2 * off, B.pm.p, 2 * cells * sizeof(double)));
        if (resid_out) SEQ_TRY(d2h_pageable(c, resid_out + off, B.resid.p, cells * sizeof(double)));
    }
    return EMBA_OK;
}

extern "C" emba_status emba_frames_exposure_align(emba_ctx* c, const uint8_t* frames, size_t F, const double* q_xyzw, const double* gain_in, const double* bias_in,
                                                  int32_t estimate, const double* plane_host, const uint8_t* valid_host, int32_t use_mosaic, uint64_t min_weight, double fill,
                                                  double lo, double hi, int32_t skip_zero, const emba_exposure_settings* xs, double* q_out, double* gain_out, double* bias_out,
                                                  double* sums_out, uint64_t* counts_out, int32_t* status_out, int32_t* iters_out, double* cost0_out, uint64_t* n0_out)
{
    if (!c) return EMBA_ERR_INVALID_ARG;
    const emba_align_settings* set = xs ? &xs->align : nullptr;
    switch (align_settings_ok(set)) {
    case AlignSetStatus::ok: break;
    case AlignSetStatus::null: return fail(c, EMBA_ERR_INVALID_ARG, "settings NULL");
    case AlignSetStatus::max_iters: return fail(c, EMBA_ERR_INVALID_ARG, "max_iters = %d is negative", (int)set->max_iters);
    case AlignSetStatus::factors: return fail(c, EMBA_ERR_INVALID_ARG, "lambda_up = %g, lambda_down = %g: both factors are above 1", set->lambda_up, set->lambda_down);
    case AlignSetStatus::lambda0: return fail(c, EMBA_ERR_INVALID_ARG, "lambda0 = %g is not positive", set->lambda0);
    case AlignSetStatus::lambda_range: return fail(c, EMBA_ERR_INVALID_ARG, "lambda_min = %g, lambda_max = %g: 0 <= lambda_min <= lambda_max", set->lambda_min, set->lambda_max);
    case AlignSetStatus::tol_rot: return fail(c, EMBA_ERR_INVALID_ARG, "tol_rot = %g is negative", set->tol_rot);
    case AlignSetStatus::min_pixels: return fail(c, EMBA_ERR_INVALID_ARG, "min_pixels = %d: three unknowns need three pixels at the least", (int)set->min_pixels);
    }
    if (!exposure_bounds_ok(xs->gain_min, xs->gain_max))
        return fail(c, EMBA_ERR_INVALID_ARG, "gain_min = %g, gain_max = %g: finite, 0 < gain_min <= 1 <= gain_max", xs->gain_min, xs->gain_max);
    if (!exposure_estimate_ok(estimate)) return fail(c, EMBA_ERR_INVALID_ARG, "estimate = %d: a mask of gain (1) and bias (2)", (int)estimate);
    const AlignCall a{frames, F, q_xyzw, plane_host, valid_host, use_mosaic, min_weight, fill, lo, hi, skip_zero, set->huber_k};
    SEQ_TRY(align_refusals(c, a));
    SEQ_TRY(exposure_refusals(c, gain_in, bias_in, F));
    if (!F) return EMBA_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t s = c->stream;
    ExposureBuffers& B = c->exposure;
    const size_t S = c->S, per = view_chunk_frames(S, 1), chunks = view_chunk_count(F, per);
    SEQ_TRY(exposure_ensure(c, a, std::min(per, F), false, false, true));
    const uint8_t* valid = nullptr;
    SEQ_TRY(align_load_plane(c, a, &valid));
    for (size_t i = 0; i < chunks; ++i) {
        const ViewChunk ch = view_chunk(F, per, i);
        SEQ_TRY(exposure_upload_chunk(c, a, gain_in, bias_in, ch));
        ExposureStepParams P{(long)ch.nf, 1, (int)estimate, *xs, B.q.as<double>(), B.q_trial.as<double>(), B.gain.as<double>(), B.bias.as<double>(),
                             B.gain_trial.as<double>(), B.bias_trial.as<double>(), B.sums.as<double>(), B.lambda.as<double>(), B.dnorm.as<double>(),
                             B.counts.as<unsigned long long>(), B.status.as<int32_t>(), B.iters.as<int32_t>(), B.have_trial.as<int32_t>(), B.esums.as<double>(),
                             B.ecounts.as<unsigned long long>(), B.cost0.as<double>(), B.n0.as<unsigned long long>(), B.running.as<unsigned int>()};
        // evaluation 0 at the given state, then per iteration: step (decide on the evaluated trial, propose the next), evaluation of the frames still running
        for (int32_t it = 0;; ++it) {
            SEQ_TRY(exposure_launch_eval(c, a, valid, ch.nf, it ? B.status.as<int32_t>() : nullptr, false, false, c->kernel_timing && i == 0 && it == 0));
            P.first = it == 0;
            HIP_TRY(c, hipMemsetAsync(B.running.p, 0, sizeof(unsigned int), s));
            hipLaunchKernelGGL(emba_frames_exposure_step_kernel, dim3(nblocks(ch.nf, 64)), dim3(64), 0, s, P);
            HIP_TRY(c, hipGetLastError());
            unsigned int running = 0;
            HIP_TRY(c, hipMemcpyAsync(&running, B.running.p, sizeof running, hipMemcpyDeviceToHost, s));
            HIP_TRY(c, hipStreamSynchronize(s));
            if (!running) break;      // (after max_iters trials no frame is running: exposure_step)
        }
        const size_t f0 = ch.f0, nf = ch.nf;
        if (q_out) SEQ_TRY(d2h_pageable(c, q_out + 4 * f0, B.q.p, 4 * nf * sizeof(double)));
        if (gain_out) SEQ_TRY(d2h_pageable(c, gain_out + f0, B.gain.p, nf * sizeof(double)));
        if (bias_out) SEQ_TRY(d2h_pageable(c, bias_out + f0, B.bias.p, nf * sizeof(double)));
        if (sums_out) SEQ_TRY(d2h_pageable(c, sums_out + (size_t)kExposureSums * f0, B.sums.p, (size_t)kExposureSums * nf * sizeof(double)));
        if (counts_out) SEQ_TRY(d2h_pageable(c, counts_out + 4 * f0, B.counts.p, 4 * nf * sizeof(uint64_t)));
        if (status_out) SEQ_TRY(d2h_pageable(c, status_out + f0, B.status.p, nf * sizeof(int32_t)));
        if (iters_out) SEQ_TRY(d2h_pageable(c, iters_out + f0, B.iters.p, nf * sizeof(int32_t)));
        if (cost0_out) SEQ_TRY(d2h_pageable(c, cost0_out + f0, B.cost0.p, nf * sizeof(double)));
        if (n0_out) SEQ_TRY(d2h_pageable(c, n0_out + f0, B.n0.p, nf * sizeof(uint64_t)));
    }
    return EMBA_OK;
}

extern "C" emba_status emba_mosaic_frames_exposure(emba_ctx* c, const uint8_t* frames, const int64_t* frame_t_ns, size_t F, const double* gain, const double* bias,
                                                   const double* knots_xyzw, int32_t K, int64_t t0_ns, int64_t dt_ns, int32_t skip_zero, int32_t accumulate,
                                                   uint64_t* dropped_out, uint64_t* skipped_out, double* pm_out)
{
    if (!c) return EMBA_ERR_INVALID_ARG;
    MosaicBuffers& B = c->mosaic;
    ExposureBuffers& X = c->exposure;
    const size_t S = c->S;
    const uint64_t have = accumulate ? B.votes : 0;
    switch (mosaic_args_ok(frames != nullptr, frame_t_ns != nullptr, knots_xyzw != nullptr, F, S, have, K, dt_ns)) {
    case MosaicArgStatus::ok: break;
    case MosaicArgStatus::frames_null: return fail(c, EMBA_ERR_INVALID_ARG, "frames NULL");
    case MosaicArgStatus::times_null: return fail(c, EMBA_ERR_INVALID_ARG, "frame_t_ns NULL");
    case MosaicArgStatus::knots_null: return fail(c, EMBA_ERR_INVALID_ARG, "knots NULL");
    case MosaicArgStatus::too_few_knots: return fail(c, EMBA_ERR_INVALID_ARG, "K = %d: a linear spline has at least two control poses", (int)K);
    case MosaicArgStatus::bad_dt: return fail(c, EMBA_ERR_INVALID_ARG, "dt_ns = %lld: the knot spacing must be positive", (long long)dt_ns);
    case MosaicArgStatus::too_many_frames: return fail(c, EMBA_ERR_INVALID_ARG, "F = %zu: the pose stage counts its frames in 31 bits", F);
    case MosaicArgStatus::too_many_votes:
        return fail(c, EMBA_ERR_INVALID_ARG, "%llu votes accumulated and %zu frames of %zu pixels more: the sums are exact below 2^36 votes", (unsigned long long)have, F, S);
    }
    SEQ_TRY(exposure_refusals(c, gain, bias, F));
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t s = c->stream;
    if (!F) {      // no frame: nothing is voted; without `accumulate` the sums are zeroed all the same
        if (!accumulate) { SEQ_TRY(mosaic_zero_sums(c)); HIP_TRY(c, hipStreamSynchronize(s)); }
        if (dropped_out) *dropped_out = 0;
        if (skipped_out) *skipped_out = 0;
        return EMBA_OK;
    }
    // every buffer of the call, before anything is written
    const size_t per = view_chunk_frames(S, 1), chunks = view_chunk_count(F, per), cap = std::min(per, F) * S;
    SEQ_TRY(ensure<int64_t>(c, B.t, F));
    SEQ_TRY(ensure<double>(c, B.pose, F * (size_t)kPoseStride));
    SEQ_TRY(ensure<double>(c, B.knots, 4 * (size_t)K));
    SEQ_TRY(ensure<uint64_t>(c, B.head, 1));
    SEQ_TRY(ensure<unsigned long long>(c, B.counters, 4));
    SEQ_TRY(ensure<unsigned long long>(c, B.sum_w, c->npix));
    SEQ_TRY(ensure<unsigned long long>(c, B.sum_v, c->npix));
    SEQ_TRY(ensure<uint8_t>(c, B.frames, cap));
    if (pm_out) SEQ_TRY(ensure<double>(c, B.pm, 2 * cap));
    SEQ_TRY(ensure<double>(c, X.vote_gain, F));
    SEQ_TRY(ensure<double>(c, X.vote_bias, F));
    // pose stage: every frame time at once, as emba_mosaic_frames runs it
    HIP_TRY(c, hipMemcpyAsync(B.knots.p, knots_xyzw, (size_t)K * 32, hipMemcpyHostToDevice, s));
    HIP_TRY(c, hipMemcpyAsync(B.t.p, frame_t_ns, F * sizeof(int64_t), hipMemcpyHostToDevice, s));
    HIP_TRY(c, hipMemcpyAsync(X.vote_gain.p, gain, F * sizeof(double), hipMemcpyHostToDevice, s));
    HIP_TRY(c, hipMemcpyAsync(X.vote_bias.p, bias, F * sizeof(double), hipMemcpyHostToDevice, s));
    HIP_TRY(c, hipMemsetAsync(B.head.p, 0, 8, s));
    HIP_TRY(c, hipMemsetAsync(B.counters.p, 0, 2 * sizeof(unsigned long long), s));
    hipLaunchKernelGGL(emba_pose_kernel, dim3(nblocks(F, 64)), dim3(64), 0, s, (const int64_t*)B.t.as<int64_t>(), (int)F, (const double*)B.knots.as<double>(), (int)K, t0_ns, dt_ns,
                       B.pose.as<double>(), reinterpret_cast<int*>(B.head.as<uint64_t>()));
    HIP_TRY(c, hipGetLastError());
    uint64_t word = 0;
    HIP_TRY(c, hipMemcpyAsync(&word, B.head.p, 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipStreamSynchronize(s));      // (the caller's arrays have been read; a frame outside the knots is refused before anything is voted)
    if ((int)(word & 0xFFFFFFFFull) & 1) return fail(c, EMBA_ERR_TIME_RANGE, "a frame time lies outside the spline's knots");
    if (!accumulate || !B.votes) SEQ_TRY(mosaic_zero_sums(c));

    for (size_t i = 0; i < chunks; ++i) {
        const ViewChunk ch = view_chunk(F, per, i);
        const size_t cells = ch.nf * S, off = ch.f0 * S;
        HIP_TRY(c, hipMemcpyAsync(B.frames.p, frames + off, cells, hipMemcpyHostToDevice, s));
        ExposureVoteParams P{c->d_lut.as<double>(), B.pose.as<double>() + (size_t)kPoseStride * ch.f0, X.vote_gain.as<double>() + ch.f0, X.vote_bias.as<double>() + ch.f0,
                             B.frames.as<uint8_t>(), (int)S, c->W, c->H, c->fx, c->fy, c->cx, c->cy, skip_zero != 0, B.sum_w.as<unsigned long long>(),
                             B.sum_v.as<unsigned long long>(), pm_out ? B.pm.as<double>() : nullptr, B.counters.as<unsigned long long>()};
        if (c->kernel_timing && i == 0) HIP_TRY(c, hipEventRecord(c->ev_start[kSeqStageTimerSlot], s));
        hipLaunchKernelGGL(emba_mosaic_exposure_vote_kernel, dim3(nblocks(S, kExposureThreads), (unsigned)ch.nf), dim3(kExposureThreads), 0, s, P);
        if (c->kernel_timing && i == 0) HIP_TRY(c, hipEventRecord(c->ev_stop[kSeqStageTimerSlot], s));
        HIP_TRY(c, hipGetLastError());
        HIP_TRY(c, hipStreamSynchronize(s));      // (the chunk's bytes have been read: the next chunk overwrites them)
        B.votes += cells;
        if (pm_out) SEQ_TRY(d2h_pageable(c, pm_out + 2 * off, B.pm.p, 2 * cells * sizeof(double)));
    }
    unsigned long long cnt[2] = {0, 0};
    HIP_TRY(c, hipMemcpy(cnt, B.counters.p, sizeof cnt, hipMemcpyDeviceToHost));
    if (dropped_out) *dropped_out = cnt[0];
    if (skipped_out) *skipped_out = cnt[1];
    return EMBA_OK;
}
