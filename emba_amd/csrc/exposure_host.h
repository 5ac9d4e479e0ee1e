// emba_amd/csrc/exposure_host.h — per-frame exposure, as host code over the kernels of exposure_kernels.h: one evaluation of every frame's 5-parameter normal
// equations (emba_frames_exposure_eval), the per-frame Levenberg-Marquardt loop on them (emba_frames_exposure_align), and the mosaic of compensated frames
// (emba_mosaic_frames_exposure).  What is plain arithmetic is decided in exposure_rule.h and align_rule.h; here are the buffers (emba_ctx::exposure), the
// launches and the C ABI.
// Part of emba_hip.hip's translation unit, included by it below track_host.h; it uses frame_host.h (the buffers of a chunk, one evaluation, the chunked
// evaluation, the loop and its read-back: DESIGN.md §23), align_host.h (AlignCall, align_refusals, align_settings_refusal, align_load_plane: the plane and its
// mask live in emba_ctx::align, scratch there as here), mosaic_host.h (mosaic_refusals, mosaic_vote_frames, which votes the compensated bytes where it is given
// gains and biases; mosaic_launch_mean), sequence_host.h (SEQ_TRY) and transfer_host.h (d2h_pageable).  Every buffer of a call is allocated
// before anything is written.  Nothing of the registered window, of the resident sequence or of the resident map is written; the mosaic's sums are written
// by emba_mosaic_frames_exposure alone.
#pragma once
#include "align_host.h"
#include "context.h"
#include "exposure_kernels.h"
#include "exposure_rule.h"
#include "frame_host.h"
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
    ExposureBuffers& X = c->exposure;
    const size_t n = c->npix;
    SEQ_TRY(ensure<double>(c, c->align.plane, n));
    if (!a.plane_host || a.valid_host) SEQ_TRY(ensure<uint8_t>(c, c->align.valid, n));
    if (!a.plane_host) {
        SEQ_TRY(ensure<double>(c, c->mosaic.mean, n));
        SEQ_TRY(ensure<uint8_t>(c, c->mosaic.covered, n));
        SEQ_TRY(ensure<unsigned long long>(c, c->mosaic.counters, 4));
    }
    SEQ_TRY(frame_ensure(c, X.loop, kExposureSums, nf, want_pm, want_resid, loop));
    SEQ_TRY(ensure<double>(c, X.gain_trial, nf));
    SEQ_TRY(ensure<double>(c, X.bias_trial, nf));
    if (!loop) return EMBA_OK;
    SEQ_TRY(ensure<double>(c, X.gain, nf));
    SEQ_TRY(ensure<double>(c, X.bias, nf));
    return EMBA_OK;
}

// a chunk's gains and biases beside its bytes and rotations (frame_upload_chunk)
emba_status exposure_upload_more(emba_ctx* c, const double* gain, const double* bias, const ViewChunk& ch)
{
    HIP_TRY(c, hipMemcpyAsync(c->exposure.gain_trial.p, gain + ch.f0, ch.nf * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(c->exposure.bias_trial.p, bias + ch.f0, ch.nf * sizeof(double), hipMemcpyHostToDevice, c->stream));
    return EMBA_OK;
}

// one evaluation of the chunk's nf frames at the trial arrays into B.esums / B.ecounts.  `status`: the frames' status words, or nullptr (every frame is
// evaluated); `timed`: timer slot 7 around the evaluation kernel
emba_status exposure_launch_eval(emba_ctx* c, const AlignCall& a, const uint8_t* valid, size_t nf, const int32_t* status, bool want_pm, bool want_resid, bool timed)
{
    ExposureBuffers& X = c->exposure;
    FrameLoopBuffers& B = X.loop;
    const ExposureEvalParams P{c->d_lut.as<double>(), B.q_trial.as<double>(), X.gain_trial.as<double>(), X.bias_trial.as<double>(), status, B.frames.as<uint8_t>(),
                               c->align.plane.as<double>(), valid, (int)c->S, c->W, c->H, c->fx, c->fy, c->cx, c->cy, a.lo, a.hi, a.huber_k, a.skip_zero != 0,
                               B.partial.as<double>(), want_pm ? B.pm.as<double>() : nullptr, want_resid ? B.resid.as<double>() : nullptr};
    return frame_launch_eval(c, B, emba_frames_exposure_eval_kernel, P, emba_frames_exposure_reduce_kernel, kExposureSums, nf, timed);
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
    SEQ_TRY(exposure_ensure(c, a, std::min(view_chunk_frames(c->S, 1), F), pm_out != nullptr, resid_out != nullptr, false));
    const uint8_t* valid = nullptr;
    SEQ_TRY(align_load_plane(c, a, &valid));
    return frame_eval_chunks(
        c, c->exposure.loop, kExposureSums, frames, q_xyzw, F, [&](const ViewChunk& ch) { return exposure_upload_more(c, gain, bias, ch); },
        [&](size_t nf, bool timed) { return exposure_launch_eval(c, a, valid, nf, nullptr, pm_out != nullptr, resid_out != nullptr, timed); }, sums_out, counts_out,
        pm_out, resid_out);
}

extern "C" emba_status emba_frames_exposure_align(emba_ctx* c, const uint8_t* frames, size_t F, const double* q_xyzw, const double* gain_in, const double* bias_in,
                                                  int32_t estimate, const double* plane_host, const uint8_t* valid_host, int32_t use_mosaic, uint64_t min_weight, double fill,
                                                  double lo, double hi, int32_t skip_zero, const emba_exposure_settings* xs, double* q_out, double* gain_out, double* bias_out,
                                                  double* sums_out, uint64_t* counts_out, int32_t* status_out, int32_t* iters_out, double* cost0_out, uint64_t* n0_out)
{
    if (!c) return EMBA_ERR_INVALID_ARG;
    const emba_align_settings* set = xs ? &xs->align : nullptr;
    SEQ_TRY(align_settings_refusal(c, set));
    if (!exposure_bounds_ok(xs->gain_min, xs->gain_max))
        return fail(c, EMBA_ERR_INVALID_ARG, "gain_min = %g, gain_max = %g: finite, 0 < gain_min <= 1 <= gain_max", xs->gain_min, xs->gain_max);
    if (!exposure_estimate_ok(estimate)) return fail(c, EMBA_ERR_INVALID_ARG, "estimate = %d: a mask of gain (1) and bias (2)", (int)estimate);
    const AlignCall a{frames, F, q_xyzw, plane_host, valid_host, use_mosaic, min_weight, fill, lo, hi, skip_zero, set->huber_k};
    SEQ_TRY(align_refusals(c, a));
    SEQ_TRY(exposure_refusals(c, gain_in, bias_in, F));
    if (!F) return EMBA_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    ExposureBuffers& X = c->exposure;
    FrameLoopBuffers& B = X.loop;
    const size_t per = view_chunk_frames(c->S, 1), chunks = view_chunk_count(F, per);
    SEQ_TRY(exposure_ensure(c, a, std::min(per, F), false, false, true));
    const uint8_t* valid = nullptr;
    SEQ_TRY(align_load_plane(c, a, &valid));
    for (size_t i = 0; i < chunks; ++i) {
        const ViewChunk ch = view_chunk(F, per, i);
        SEQ_TRY(frame_upload_chunk(c, B, frames, q_xyzw, ch));
        SEQ_TRY(exposure_upload_more(c, gain_in, bias_in, ch));
        ExposureStepParams P{(long)ch.nf, 1, (int)estimate, *xs, B.q.as<double>(), B.q_trial.as<double>(), X.gain.as<double>(), X.bias.as<double>(),
                             X.gain_trial.as<double>(), X.bias_trial.as<double>(), B.sums.as<double>(), B.lambda.as<double>(), B.dnorm.as<double>(),
                             B.counts.as<unsigned long long>(), B.status.as<int32_t>(), B.iters.as<int32_t>(), B.have_trial.as<int32_t>(), B.esums.as<double>(),
                             B.ecounts.as<unsigned long long>(), B.cost0.as<double>(), B.n0.as<unsigned long long>(), B.running.as<unsigned int>()};
        SEQ_TRY(frame_lm_loop(
            c, B, [&](const int32_t* status, bool first) { return exposure_launch_eval(c, a, valid, ch.nf, status, false, false, c->kernel_timing && i == 0 && first); },
            [&](bool first) {
                P.first = first;
                hipLaunchKernelGGL(emba_frames_exposure_step_kernel, dim3(nblocks(ch.nf, 64)), dim3(64), 0, c->stream, P);
            }));
        if (gain_out) SEQ_TRY(d2h_pageable(c, gain_out + ch.f0, X.gain.p, ch.nf * sizeof(double)));
        if (bias_out) SEQ_TRY(d2h_pageable(c, bias_out + ch.f0, X.bias.p, ch.nf * sizeof(double)));
        SEQ_TRY(frame_read_loop(c, B, kExposureSums, ch, q_out, sums_out, counts_out, status_out, iters_out, cost0_out, n0_out));
    }
    return EMBA_OK;
}

extern "C" emba_status emba_mosaic_frames_exposure(emba_ctx* c, const uint8_t* frames, const int64_t* frame_t_ns, size_t F, const double* gain, const double* bias,
                                                   const double* knots_xyzw, int32_t K, int64_t t0_ns, int64_t dt_ns, int32_t skip_zero, int32_t accumulate,
                                                   uint64_t* dropped_out, uint64_t* skipped_out, double* pm_out)
{
    if (!c) return EMBA_ERR_INVALID_ARG;
    const MosaicCall m{frames, frame_t_ns, F, knots_xyzw, K, t0_ns, dt_ns, skip_zero, accumulate, dropped_out, skipped_out, pm_out};
    SEQ_TRY(mosaic_refusals(c, m));
    SEQ_TRY(exposure_refusals(c, gain, bias, F));
    return mosaic_vote_frames(c, m, gain, bias);
}
