// emba_amd/csrc/align_host.h — intensity frames aligned to a panorama plane, as host code over the kernels of align_kernels.h: one evaluation of every frame's
// normal equations (emba_frames_align_eval) and the per-frame Levenberg-Marquardt loop on them (emba_frames_align).  What is plain arithmetic — the argument
// checks, the sample with its gradient, the weight, the step, accept / reject and the ways a frame ends — is decided in align_rule.h; here are the buffers
// (emba_ctx::align), the launches and the C ABI.
// Part of emba_hip.hip's translation unit, included by it below sim_host.h; it uses sequence_host.h (SEQ_TRY), transfer_host.h (d2h_pageable),
// panorama_host.h (kSeqStageTimerSlot) and mosaic_host.h (mosaic_launch_mean).  Nothing of the registered window, of the resident sequence, of the resident
// map or of any other stage's buffers is written, but for the mosaic's mean and covered scratch where the mosaic is the plane.
#pragma once
#include "align_kernels.h"
#include "align_rule.h"
#include "context.h"

using namespace emba;

namespace {
// what both calls take, as the C ABI hands it over
struct AlignCall {
    const uint8_t* frames; size_t F; const double* q_xyzw; const double* plane_host; const uint8_t* valid_host;
    int32_t use_mosaic; uint64_t min_weight; double fill, lo, hi; int32_t skip_zero; double huber_k;
};

// every refusal, before anything is uploaded
emba_status align_refusals(emba_ctx* c, const AlignCall& a)
{
    switch (align_args_ok(a.frames != nullptr, a.q_xyzw != nullptr, a.F, a.lo, a.hi, a.huber_k)) {
    case AlignArgStatus::ok: break;
    case AlignArgStatus::frames_null: return fail(c, EMBA_ERR_INVALID_ARG, "frames NULL");
    case AlignArgStatus::q_null: return fail(c, EMBA_ERR_INVALID_ARG, "q_xyzw NULL");
    case AlignArgStatus::too_many_frames: return fail(c, EMBA_ERR_INVALID_ARG, "F = %zu: frames are counted in 31 bits", a.F);
    case AlignArgStatus::tone_not_finite: return fail(c, EMBA_ERR_INVALID_ARG, "lo = %g, hi = %g: the tone needs finite values", a.lo, a.hi);
    case AlignArgStatus::hi_not_above_lo: return fail(c, EMBA_ERR_INVALID_ARG, "hi = %g is not above lo = %g", a.hi, a.lo);
    case AlignArgStatus::huber_not_finite: return fail(c, EMBA_ERR_INVALID_ARG, "huber_k is not a number");
    }
    if (!a.plane_host) {
        if (!a.use_mosaic) return fail(c, EMBA_ERR_INVALID_ARG, "no plane: plane_host NULL and use_mosaic = 0");
        switch (mosaic_get_args_ok(a.min_weight, a.fill)) {
        case MosaicToneStatus::ok: break;
        case MosaicToneStatus::bad_min_weight: return fail(c, EMBA_ERR_INVALID_ARG, "min_weight = 0: a covered cell has a weight of 1 at the least");
        default: return fail(c, EMBA_ERR_INVALID_ARG, "fill = %g is not finite", a.fill);
        }
    }
    const size_t bad = align_first_bad_q(a.q_xyzw, a.F);
    if (bad < a.F) return fail(c, EMBA_ERR_INVALID_ARG, "q_xyzw[%zu] is not finite or has zero norm", bad);
    if (!a.plane_host && !c->mosaic.votes) return fail(c, EMBA_ERR_STATE, "use_mosaic: nothing accumulated (emba_mosaic_frames first)");
    return EMBA_OK;
}

// the plane and its mask into this stage's own buffers: the caller's, or the mosaic's mean and covered cells device to device.  *valid: the mask, or nullptr
emba_status align_load_plane(emba_ctx* c, const AlignCall& a, const uint8_t** valid)
{
    AlignBuffers& B = c->align;
    hipStream_t s = c->stream;
    const size_t n = c->npix;
    SEQ_TRY(ensure<double>(c, B.plane, n));
    *valid = nullptr;
    if (a.plane_host) {
        HIP_TRY(c, hipMemcpyAsync(B.plane.p, a.plane_host, n * sizeof(double), hipMemcpyHostToDevice, s));
        if (a.valid_host) {
            SEQ_TRY(ensure<uint8_t>(c, B.valid, n));
            HIP_TRY(c, hipMemcpyAsync(B.valid.p, a.valid_host, n, hipMemcpyHostToDevice, s));
            *valid = B.valid.as<uint8_t>();
        }
        return EMBA_OK;
    }
    SEQ_TRY(ensure<uint8_t>(c, B.valid, n));
    SEQ_TRY(mosaic_launch_mean(c, a.min_weight, a.fill));
    HIP_TRY(c, hipMemcpyAsync(B.plane.p, c->mosaic.mean.p, n * sizeof(double), hipMemcpyDeviceToDevice, s));
    HIP_TRY(c, hipMemcpyAsync(B.valid.p, c->mosaic.covered.p, n, hipMemcpyDeviceToDevice, s));
    *valid = B.valid.as<uint8_t>();
    return EMBA_OK;
}

// the buffers of a chunk of at most `nf` frames; `loop`: the frames' state as well
emba_status align_ensure_chunk(emba_ctx* c, size_t nf, bool want_pm, bool want_resid, bool loop)
{
    AlignBuffers& B = c->align;
    const size_t S = c->S, nb = nblocks(S, kAlignThreads);
    SEQ_TRY(ensure<uint8_t>(c, B.frames, nf * S));
    if (want_pm) SEQ_TRY(ensure<double>(c, B.pm, 2 * nf * S));
    if (want_resid) SEQ_TRY(ensure<double>(c, B.resid, nf * S));
    SEQ_TRY(ensure<double>(c, B.partial, nf * nb * (size_t)kAlignPartial));
    SEQ_TRY(ensure<double>(c, B.q_trial, 4 * nf));
    SEQ_TRY(ensure<double>(c, B.esums, (size_t)kAlignSums * nf));
    SEQ_TRY(ensure<unsigned long long>(c, B.ecounts, 4 * nf));
    if (!loop) return EMBA_OK;
    SEQ_TRY(ensure<double>(c, B.q, 4 * nf));
    SEQ_TRY(ensure<double>(c, B.sums, (size_t)kAlignSums * nf));
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

// one evaluation of the chunk's nf frames at B.q_trial into B.esums / B.ecounts: the evaluation kernel and the reduction of its partial sums.  `status`: the
// frames' status words, or nullptr (every frame is evaluated); `timed`: timer slot 7 around the evaluation kernel
emba_status align_launch_eval(emba_ctx* c, const AlignCall& a, const uint8_t* valid, size_t nf, const int32_t* status, bool want_pm, bool want_resid, bool timed)
{
    AlignBuffers& B = c->align;
    hipStream_t s = c->stream;
    const unsigned nb = nblocks(c->S, kAlignThreads);
    AlignEvalParams P{c->d_lut.as<double>(), B.q_trial.as<double>(), status, B.frames.as<uint8_t>(), B.plane.as<double>(), valid, (int)c->S, c->W, c->H,
                      c->fx, c->fy, c->cx, c->cy, a.lo, a.hi, a.huber_k, a.skip_zero != 0, B.partial.as<double>(), want_pm ? B.pm.as<double>() : nullptr,
                      want_resid ? B.resid.as<double>() : nullptr};
    if (timed) HIP_TRY(c, hipEventRecord(c->ev_start[kSeqStageTimerSlot], s));
    hipLaunchKernelGGL(emba_frames_align_eval_kernel, dim3(nb, (unsigned)nf), dim3(kAlignThreads), 0, s, P);
    if (timed) HIP_TRY(c, hipEventRecord(c->ev_stop[kSeqStageTimerSlot], s));
    HIP_TRY(c, hipGetLastError());
    hipLaunchKernelGGL(emba_frames_align_reduce_kernel, dim3(nblocks(nf * (size_t)(kAlignSums + 4), kAlignThreads)), dim3(kAlignThreads), 0, s,
                       (const double*)B.partial.as<double>(), (int)nb, (long)nf, status, B.esums.as<double>(), B.ecounts.as<unsigned long long>());
    HIP_TRY(c, hipGetLastError());
    return EMBA_OK;
}
}  // namespace

extern "C" emba_status emba_frames_align_eval(emba_ctx* c, const uint8_t* frames, size_t F, const double* q_xyzw, const double* plane_host, const uint8_t* valid_host,
                                              int32_t use_mosaic, uint64_t min_weight, double fill, double lo, double hi, int32_t skip_zero, double huber_k,
                                              double* sums_out, uint64_t* counts_out, double* pm_out, double* resid_out)
{
    if (!c) return EMBA_ERR_INVALID_ARG;
    const AlignCall a{frames, F, q_xyzw, plane_host, valid_host, use_mosaic, min_weight, fill, lo, hi, skip_zero, huber_k};
    SEQ_TRY(align_refusals(c, a));
    if (!F) return EMBA_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t s = c->stream;
    AlignBuffers& B = c->align;
    const uint8_t* valid = nullptr;
    SEQ_TRY(align_load_plane(c, a, &valid));
    const size_t S = c->S, per = view_chunk_frames(S, 1), chunks = view_chunk_count(F, per);
    SEQ_TRY(align_ensure_chunk(c, std::min(per, F), pm_out != nullptr, resid_out != nullptr, false));
    for (size_t i = 0; i < chunks; ++i) {
        const ViewChunk ch = view_chunk(F, per, i);
        const size_t cells = ch.nf * S, off = ch.f0 * S;
        HIP_TRY(c, hipMemcpyAsync(B.frames.p, frames + off, cells, hipMemcpyHostToDevice, s));
        HIP_TRY(c, hipMemcpyAsync(B.q_trial.p, q_xyzw + 4 * ch.f0, 4 * ch.nf * sizeof(double), hipMemcpyHostToDevice, s));
        SEQ_TRY(align_launch_eval(c, a, valid, ch.nf, nullptr, pm_out != nullptr, resid_out != nullptr, c->kernel_timing && i == 0));
        HIP_TRY(c, hipStreamSynchronize(s));      // (the chunk's bytes have been read: the next chunk overwrites them)
        if (sums_out) SEQ_TRY(d2h_pageable(c, sums_out + (size_t)kAlignSums * ch.f0, B.esums.p, (size_t)kAlignSums * ch.nf * sizeof(double)));
        if (counts_out) SEQ_TRY(d2h_pageable(c, counts_out + 4 * ch.f0, B.ecounts.p, 4 * ch.nf * sizeof(uint64_t)));
        if (pm_out) SEQ_TRY(d2h_pageable(c, pm_out + 2 * off, B.pm.p, 2 * cells * sizeof(double)));
        if (resid_out) SEQ_TRY(d2h_pageable(c, resid_out + off, B.resid.p, cells * sizeof(double)));
    }
    return EMBA_OK;
}

extern "C" emba_status emba_frames_align(emba_ctx* c, const uint8_t* frames, size_t F, const double* q_xyzw, const double* plane_host, const uint8_t* valid_host,
                                         int32_t use_mosaic, uint64_t min_weight, double fill, double lo, double hi, int32_t skip_zero,
                                         const emba_align_settings* set, double* q_out, double* sums_out, uint64_t* counts_out, int32_t* status_out,
                                         int32_t* iters_out, double* cost0_out, uint64_t* n0_out)
{
    if (!c) return EMBA_ERR_INVALID_ARG;
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
    const AlignCall a{frames, F, q_xyzw, plane_host, valid_host, use_mosaic, min_weight, fill, lo, hi, skip_zero, set->huber_k};
    SEQ_TRY(align_refusals(c, a));
    if (!F) return EMBA_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t s = c->stream;
    AlignBuffers& B = c->align;
    const uint8_t* valid = nullptr;
    SEQ_TRY(align_load_plane(c, a, &valid));
    const size_t S = c->S, per = view_chunk_frames(S, 1), chunks = view_chunk_count(F, per);
    SEQ_TRY(align_ensure_chunk(c, std::min(per, F), false, false, true));
    for (size_t i = 0; i < chunks; ++i) {
        const ViewChunk ch = view_chunk(F, per, i);
        HIP_TRY(c, hipMemcpyAsync(B.frames.p, frames + ch.f0 * S, ch.nf * S, hipMemcpyHostToDevice, s));
        HIP_TRY(c, hipMemcpyAsync(B.q_trial.p, q_xyzw + 4 * ch.f0, 4 * ch.nf * sizeof(double), hipMemcpyHostToDevice, s));
        AlignStepParams P{(long)ch.nf, 1, *set, B.q.as<double>(), B.q_trial.as<double>(), B.sums.as<double>(), B.lambda.as<double>(), B.dnorm.as<double>(),
                          B.counts.as<unsigned long long>(), B.status.as<int32_t>(), B.iters.as<int32_t>(), B.have_trial.as<int32_t>(), B.esums.as<double>(),
                          B.ecounts.as<unsigned long long>(), B.cost0.as<double>(), B.n0.as<unsigned long long>(), B.running.as<unsigned int>()};
        // evaluation 0 at the given rotations, then per iteration: step (decide on the evaluated trial, propose the next), evaluation of the frames still running
        for (int32_t it = 0;; ++it) {
            SEQ_TRY(align_launch_eval(c, a, valid, ch.nf, it ? B.status.as<int32_t>() : nullptr, false, false, c->kernel_timing && i == 0 && it == 0));
            P.first = it == 0;
            HIP_TRY(c, hipMemsetAsync(B.running.p, 0, sizeof(unsigned int), s));
            hipLaunchKernelGGL(emba_frames_align_step_kernel, dim3(nblocks(ch.nf, 64)), dim3(64), 0, s, P);
            HIP_TRY(c, hipGetLastError());
            unsigned int running = 0;
            HIP_TRY(c, hipMemcpyAsync(&running, B.running.p, sizeof running, hipMemcpyDeviceToHost, s));
            HIP_TRY(c, hipStreamSynchronize(s));
            if (!running) break;      // (after max_iters trials no frame is running: align_step)
        }
        const size_t f0 = ch.f0, nf = ch.nf;
        if (q_out) SEQ_TRY(d2h_pageable(c, q_out + 4 * f0, B.q.p, 4 * nf * sizeof(double)));
        if (sums_out) SEQ_TRY(d2h_pageable(c, sums_out + (size_t)kAlignSums * f0, B.sums.p, (size_t)kAlignSums * nf * sizeof(double)));
        if (counts_out) SEQ_TRY(d2h_pageable(c, counts_out + 4 * f0, B.counts.p, 4 * nf * sizeof(uint64_t)));
        if (status_out) SEQ_TRY(d2h_pageable(c, status_out + f0, B.status.p, nf * sizeof(int32_t)));
        if (iters_out) SEQ_TRY(d2h_pageable(c, iters_out + f0, B.iters.p, nf * sizeof(int32_t)));
        if (cost0_out) SEQ_TRY(d2h_pageable(c, cost0_out + f0, B.cost0.p, nf * sizeof(double)));
        if (n0_out) SEQ_TRY(d2h_pageable(c, n0_out + f0, B.n0.p, nf * sizeof(uint64_t)));
    }
    return EMBA_OK;
}
