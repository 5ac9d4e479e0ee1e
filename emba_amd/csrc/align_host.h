// emba_amd/csrc/align_host.h — intensity frames aligned to a panorama plane, as host code over the kernels of align_kernels.h: one evaluation of every frame's
// normal equations (emba_frames_align_eval) and the per-frame Levenberg-Marquardt loop on them (emba_frames_align).  What is plain arithmetic — the argument
// checks, the sample with its gradient, the weight, the step, accept / reject and the ways a frame ends — is decided in align_rule.h; here are the buffers
// (emba_ctx::align), the launches and the C ABI.
// Part of emba_hip.hip's translation unit, included by it below frame_host.h; it uses frame_host.h (the buffers of a chunk, one evaluation, the chunked
// evaluation, the loop and its read-back: DESIGN.md §23), sequence_host.h (SEQ_TRY) and mosaic_host.h (mosaic_launch_mean).  Nothing of the registered window, of the resident sequence, of the resident
// map or of any other stage's buffers is written, but for the mosaic's mean and covered scratch where the mosaic is the plane.
#pragma once
#include "align_kernels.h"
#include "align_rule.h"
#include "context.h"
#include "frame_host.h"

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

// one evaluation of the chunk's nf frames at B.q_trial into B.esums / B.ecounts.  `status`: the frames' status words, or nullptr (every frame is evaluated);
// `timed`: timer slot 7 around the evaluation kernel
emba_status align_launch_eval(emba_ctx* c, const AlignCall& a, const uint8_t* valid, size_t nf, const int32_t* status, bool want_pm, bool want_resid, bool timed)
{
    FrameLoopBuffers& B = c->align.loop;
    const AlignEvalParams P{c->d_lut.as<double>(), B.q_trial.as<double>(), status, B.frames.as<uint8_t>(), c->align.plane.as<double>(), valid, (int)c->S, c->W, c->H,
                            c->fx, c->fy, c->cx, c->cy, a.lo, a.hi, a.huber_k, a.skip_zero != 0, B.partial.as<double>(), want_pm ? B.pm.as<double>() : nullptr,
                            want_resid ? B.resid.as<double>() : nullptr};
    return frame_launch_eval(c, B, emba_frames_align_eval_kernel, P, emba_frames_align_reduce_kernel, kAlignSums, nf, timed);
}

// the refusals of the loop's settings (emba_frames_align, emba_frames_exposure_align)
emba_status align_settings_refusal(emba_ctx* c, const emba_align_settings* set)
{
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
    return EMBA_OK;
}

// the step kernel of emba_frames_align's loop on nf frames of B (the tracker runs the same loop on its own buffers); first: the state is made from q_trial
void align_launch_step(emba_ctx* c, FrameLoopBuffers& B, size_t nf, const emba_align_settings& set, bool first)
{
    const AlignStepParams P{(long)nf, first, set, B.q.as<double>(), B.q_trial.as<double>(), B.sums.as<double>(), B.lambda.as<double>(), B.dnorm.as<double>(),
                            B.counts.as<unsigned long long>(), B.status.as<int32_t>(), B.iters.as<int32_t>(), B.have_trial.as<int32_t>(), B.esums.as<double>(),
                            B.ecounts.as<unsigned long long>(), B.cost0.as<double>(), B.n0.as<unsigned long long>(), B.running.as<unsigned int>()};
    hipLaunchKernelGGL(emba_frames_align_step_kernel, dim3(nblocks(nf, 64)), dim3(64), 0, c->stream, P);
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
    FrameLoopBuffers& B = c->align.loop;
    const uint8_t* valid = nullptr;
    SEQ_TRY(align_load_plane(c, a, &valid));
    SEQ_TRY(frame_ensure(c, B, kAlignSums, std::min(view_chunk_frames(c->S, 1), F), pm_out != nullptr, resid_out != nullptr, false));
    return frame_eval_chunks(
        c, B, kAlignSums, frames, q_xyzw, F, [](const ViewChunk&) { return EMBA_OK; },
        [&](size_t nf, bool timed) { return align_launch_eval(c, a, valid, nf, nullptr, pm_out != nullptr, resid_out != nullptr, timed); }, sums_out, counts_out, pm_out,
        resid_out);
}

extern "C" emba_status emba_frames_align(emba_ctx* c, const uint8_t* frames, size_t F, const double* q_xyzw, const double* plane_host, const uint8_t* valid_host,
                                         int32_t use_mosaic, uint64_t min_weight, double fill, double lo, double hi, int32_t skip_zero,
                                         const emba_align_settings* set, double* q_out, double* sums_out, uint64_t* counts_out, int32_t* status_out,
                                         int32_t* iters_out, double* cost0_out, uint64_t* n0_out)
{
    if (!c) return EMBA_ERR_INVALID_ARG;
    SEQ_TRY(align_settings_refusal(c, set));
    const AlignCall a{frames, F, q_xyzw, plane_host, valid_host, use_mosaic, min_weight, fill, lo, hi, skip_zero, set->huber_k};
    SEQ_TRY(align_refusals(c, a));
    if (!F) return EMBA_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    FrameLoopBuffers& B = c->align.loop;
    const uint8_t* valid = nullptr;
    SEQ_TRY(align_load_plane(c, a, &valid));
    const size_t per = view_chunk_frames(c->S, 1), chunks = view_chunk_count(F, per);
    SEQ_TRY(frame_ensure(c, B, kAlignSums, std::min(per, F), false, false, true));
    for (size_t i = 0; i < chunks; ++i) {
        const ViewChunk ch = view_chunk(F, per, i);
        SEQ_TRY(frame_upload_chunk(c, B, frames, q_xyzw, ch));
        SEQ_TRY(frame_lm_loop(
            c, B, [&](const int32_t* status, bool first) { return align_launch_eval(c, a, valid, ch.nf, status, false, false, c->kernel_timing && i == 0 && first); },
            [&](bool first) { align_launch_step(c, B, ch.nf, *set, first); }));
        SEQ_TRY(frame_read_loop(c, B, kAlignSums, ch, q_out, sums_out, counts_out, status_out, iters_out, cost0_out, n0_out));
    }
    return EMBA_OK;
}
