// emba_amd/csrc/track_exposure_host.h — the frame tracker with a per-frame exposure, as host code over the kernels of track_exposure_kernels.h (and the reduce
// and step kernels of exposure_kernels.h): the tracker (emba_frames_track_exposure) and one evaluation against a level's planes as they stand
// (emba_track_exposure_eval).  What is plain arithmetic is decided in track_exposure_rule.h, track_rule.h and exposure_rule.h; here are the buffers
// (emba_ctx::track: the tracker's own, with the gains and biases beside the rotations), the launches and the C ABI.
// Part of emba_hip.hip's translation unit, included by it below track_host.h and exposure_host.h; it uses frame_host.h (frame_ensure with 21 sums,
// frame_launch_eval, frame_eval_chunks, frame_lm_loop: DESIGN.md §23), track_host.h (track_plane, track_refusals, track_level_refusal), exposure_host.h
// (exposure_refusals), mosaic_host.h (mosaic_zero_sums: level 0's planes are the mosaic's sums), sequence_host.h (SEQ_TRY) and transfer_host.h
// (d2h_pageable).  Every buffer of a call is allocated before anything is zeroed.  Nothing of the registered window, of the resident sequence, of the
// resident map or of any other stage's buffers is written, but for the mosaic's sums and its count of votes.
#pragma once
#include "context.h"
#include "exposure_host.h"
#include "frame_host.h"
#include "track_exposure_kernels.h"
#include "track_exposure_rule.h"
#include "track_host.h"

using namespace emba;

namespace {
// one evaluation of nf frames (bytes at `bytes`) at T.loop.q_trial, T.gain_trial, T.bias_trial against `plane` into T.loop.esums / ecounts
emba_status track_exposure_launch_eval(emba_ctx* c, const TrackPlane& plane, const uint8_t* bytes, size_t nf, const int32_t* status, uint64_t min_weight,
                                       int32_t skip_zero, double huber_k, bool want_pm, bool want_resid, bool timed)
{
    TrackBuffers& T = c->track;
    FrameLoopBuffers& L = T.loop;
    const TrackExposureEvalParams P{c->d_lut.as<double>(), L.q_trial.as<double>(), T.gain_trial.as<double>(), T.bias_trial.as<double>(), status, bytes, plane.sum_w,
                                    plane.sum_v, (int)c->S, plane.W, plane.H, plane.scale, c->fx, c->fy, c->cx, c->cy, (unsigned long long)min_weight, huber_k,
                                    skip_zero != 0, L.partial.as<double>(), want_pm ? L.pm.as<double>() : nullptr, want_resid ? L.resid.as<double>() : nullptr};
    return frame_launch_eval(c, L, emba_frames_track_exposure_eval_kernel, P, emba_frames_exposure_reduce_kernel, kExposureSums, nf, timed);
}

emba_status track_exposure_launch_frames(emba_ctx* c, TrackExposureFrameParams P)
{
    hipLaunchKernelGGL(emba_frames_track_exposure_frame_kernel, dim3(nblocks((size_t)P.nf, 64)), dim3(64), 0, c->stream, P);
    HIP_TRY(c, hipGetLastError());
    return EMBA_OK;
}
}  // namespace

extern "C" emba_status emba_frames_track_exposure(emba_ctx* c, const uint8_t* frames, const int64_t* frame_t_ns, size_t F, const double* q0_xyzw,
                                                  const emba_track_exposure_settings* xset, double* q_out, double* gain_out, double* bias_out, int32_t* status_out,
                                                  int32_t* iters_out, double* cost_out, uint64_t* counts_out, double* overlap_out, uint64_t* stats_out, double* pm_out)
{
    if (!c) return EMBA_ERR_INVALID_ARG;
    const emba_track_settings* set = xset ? &xset->track : nullptr;
    SEQ_TRY(track_refusals(c, frames, frame_t_ns, F, q0_xyzw, set));
    switch (track_exposure_args_ok(*xset)) {
    case TrackExposureArgStatus::ok: break;
    case TrackExposureArgStatus::bad_bounds:
        return fail(c, EMBA_ERR_INVALID_ARG, "gain_min = %g, gain_max = %g: finite, 0 < gain_min <= 1 <= gain_max", xset->gain_min, xset->gain_max);
    case TrackExposureArgStatus::bad_estimate: return fail(c, EMBA_ERR_INVALID_ARG, "estimate = %d: a mask of gain (1) and bias (2)", (int)xset->estimate);
    }
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t s = c->stream;
    TrackBuffers& T = c->track;
    FrameLoopBuffers& L = T.loop;
    const size_t S = c->S, NL = (size_t)set->n_levels;

    int vote_levels[kTrackMaxPlanes];
    const int n_planes = track_vote_levels(*set, vote_levels);
    // every buffer of the call is there before anything is zeroed (emba_frames_track's order)
    const size_t per = view_chunk_frames(S, 1), chunks = view_chunk_count(F, per);
    const size_t maxb = std::max<size_t>(std::min(std::min((size_t)set->batch, per), F), 1);
    bool fresh = false;
    for (int k = 0; k < n_planes; ++k) {
        const int l = vote_levels[k];
        if (!l) continue;
        const size_t cells = c->npix >> (2 * l);
        SEQ_TRY(ensure<unsigned long long>(c, T.lw[l], cells, &fresh));
        if (fresh) T.voted &= ~(1u << l);
        SEQ_TRY(ensure<unsigned long long>(c, T.lv[l], cells, &fresh));
        if (fresh) T.voted &= ~(1u << l);
    }
    if (F) {
        SEQ_TRY(ensure<int64_t>(c, T.t, F));
        SEQ_TRY(ensure<double>(c, T.q_all, 4 * F));
        SEQ_TRY(ensure<double>(c, T.gain_all, F));
        SEQ_TRY(ensure<double>(c, T.bias_all, F));
        SEQ_TRY(ensure<int32_t>(c, T.status_all, F));
        SEQ_TRY(ensure<int32_t>(c, T.iters_all, F * NL));
        SEQ_TRY(ensure<double>(c, T.cost_all, F));
        SEQ_TRY(ensure<double>(c, T.overlap_all, F));
        SEQ_TRY(ensure<unsigned long long>(c, T.counts_all, 4 * F));
        SEQ_TRY(ensure<unsigned long long>(c, T.counters, 2));
        SEQ_TRY(ensure<uint8_t>(c, L.frames, std::min(per, F) * S));      // (a chunk's bytes; the batches below are no longer than a chunk)
        SEQ_TRY(ensure<double>(c, T.pred, 4 * maxb));
        SEQ_TRY(ensure<double>(c, T.gain_pred, maxb));
        SEQ_TRY(ensure<double>(c, T.bias_pred, maxb));
        SEQ_TRY(ensure<double>(c, T.gain_trial, maxb));
        SEQ_TRY(ensure<double>(c, T.bias_trial, maxb));
        SEQ_TRY(ensure<double>(c, T.gain, maxb));
        SEQ_TRY(ensure<double>(c, T.bias, maxb));
        SEQ_TRY(frame_ensure(c, L, kExposureSums, maxb, pm_out != nullptr, false, true));
    }
    SEQ_TRY(mosaic_zero_sums(c));      // (it allocates the mosaic's two sums, where they are missing, before it zeroes either)
    T.voted = 0;
    for (int k = 0; k < n_planes; ++k) {
        const int l = vote_levels[k];
        if (!l) continue;
        const size_t cells = c->npix >> (2 * l);
        HIP_TRY(c, hipMemsetAsync(T.lw[l].p, 0, cells * sizeof(unsigned long long), s));
        HIP_TRY(c, hipMemsetAsync(T.lv[l].p, 0, cells * sizeof(unsigned long long), s));
    }
    uint32_t voted = 0;
    for (int k = 0; k < n_planes; ++k) voted |= 1u << vote_levels[k];
    if (!F) {
        HIP_TRY(c, hipStreamSynchronize(s));
        T.voted = voted;
        if (stats_out) stats_out[0] = stats_out[1] = stats_out[2] = stats_out[3] = 0;
        return EMBA_OK;
    }
    TrackExposureVoteParams V{};
    V.lut = c->d_lut.as<double>(); V.S = (int)S; V.n_planes = n_planes;
    V.fx = c->fx; V.fy = c->fy; V.cx = c->cx; V.cy = c->cy; V.skip_zero = set->skip_zero != 0;
    for (int k = 0; k < n_planes; ++k) V.plane[k] = track_plane(c, vote_levels[k]);
    TrackPlane sched[kTrackMaxSchedule];
    for (size_t k = 0; k < NL; ++k) sched[k] = track_plane(c, set->levels[k]);

    // the call's frames: times up, rotations, exposures and statuses resident until the end
    HIP_TRY(c, hipMemcpyAsync(T.t.p, frame_t_ns, F * sizeof(int64_t), hipMemcpyHostToDevice, s));
    HIP_TRY(c, hipMemsetAsync(T.status_all.p, 0, F * sizeof(int32_t), s));
    HIP_TRY(c, hipMemsetAsync(T.counters.p, 0, 2 * sizeof(unsigned long long), s));
    V.counters = T.counters.as<unsigned long long>();
    V.pm = pm_out ? L.pm.as<double>() : nullptr;

    TrackExposureFrameParams B{};
    B.n_levels = (int)NL; B.predict = set->predict != 0; B.min_overlap = set->min_overlap; B.S = (unsigned long long)S;
    track_normalise(q0_xyzw, B.q0);
    B.t = reinterpret_cast<const long long*>(T.t.as<int64_t>());
    B.q_all = T.q_all.as<double>(); B.gain_all = T.gain_all.as<double>(); B.bias_all = T.bias_all.as<double>();
    B.status_all = T.status_all.as<int32_t>(); B.iters_all = T.iters_all.as<int32_t>();
    B.cost_all = T.cost_all.as<double>(); B.overlap_all = T.overlap_all.as<double>(); B.counts_all = T.counts_all.as<unsigned long long>();
    B.pred = T.pred.as<double>(); B.q = L.q.as<double>(); B.q_trial = L.q_trial.as<double>();
    B.gain_pred = T.gain_pred.as<double>(); B.gain = T.gain.as<double>(); B.gain_trial = T.gain_trial.as<double>();
    B.bias_pred = T.bias_pred.as<double>(); B.bias = T.bias.as<double>(); B.bias_trial = T.bias_trial.as<double>();
    B.sums = L.sums.as<double>(); B.counts = L.counts.as<unsigned long long>(); B.status = L.status.as<int32_t>(); B.iters = L.iters.as<int32_t>();

    const emba_exposure_settings xs{set->align, xset->gain_min, xset->gain_max};
    ExposureStepParams P{0, 1, (int)xset->estimate, xs, L.q.as<double>(), L.q_trial.as<double>(), T.gain.as<double>(), T.bias.as<double>(),
                         T.gain_trial.as<double>(), T.bias_trial.as<double>(), L.sums.as<double>(), L.lambda.as<double>(), L.dnorm.as<double>(),
                         L.counts.as<unsigned long long>(), L.status.as<int32_t>(), L.iters.as<int32_t>(), L.have_trial.as<int32_t>(), L.esums.as<double>(),
                         L.ecounts.as<unsigned long long>(), L.cost0.as<double>(), L.n0.as<unsigned long long>(), L.running.as<unsigned int>()};

    bool timed = c->kernel_timing != 0;
    for (size_t i = 0; i < chunks; ++i) {
        const ViewChunk ch = view_chunk(F, per, i);
        HIP_TRY(c, hipMemcpyAsync(L.frames.p, frames + ch.f0 * S, ch.nf * S, hipMemcpyHostToDevice, s));
        for (size_t f0 = ch.f0; f0 < ch.f0 + ch.nf;) {
            const size_t nf = track_batch_frames(f0, F, per, (size_t)set->batch);
            const uint8_t* bytes = L.frames.as<uint8_t>() + (f0 - ch.f0) * S;
            B.nf = (long)nf; B.f0 = (long)f0;
            if (f0 == 0) {
                B.phase = kTrackAnchor;
                SEQ_TRY(track_exposure_launch_frames(c, B));
            } else {
                B.phase = kTrackPredict;
                SEQ_TRY(track_exposure_launch_frames(c, B));
                P.nf = (long)nf;
                for (size_t k = 0; k < NL; ++k) {
                    // §22's loop against this level: evaluation 0 where the previous level ended
                    SEQ_TRY(frame_lm_loop(
                        c, L,
                        [&](const int32_t* status, bool) {
                            const bool t = timed;
                            timed = false;
                            return track_exposure_launch_eval(c, sched[k], bytes, nf, status, set->min_weight, set->skip_zero, set->align.huber_k, false, false, t);
                        },
                        [&](bool first) {
                            P.first = first;
                            hipLaunchKernelGGL(emba_frames_exposure_step_kernel, dim3(nblocks(nf, 64)), dim3(64), 0, s, P);
                        }));
                    B.phase = kTrackLevelEnd; B.level_index = (int)k;
                    SEQ_TRY(track_exposure_launch_frames(c, B));
                }
                B.phase = kTrackVerdict;
                SEQ_TRY(track_exposure_launch_frames(c, B));
            }
            V.q = T.q_all.as<double>() + 4 * f0; V.gain = T.gain_all.as<double>() + f0; V.bias = T.bias_all.as<double>() + f0;
            V.status = T.status_all.as<int32_t>() + f0; V.frames = bytes;
            hipLaunchKernelGGL(emba_frames_track_exposure_vote_kernel, dim3(nblocks(S, kFrameThreads), (unsigned)nf), dim3(kFrameThreads), 0, s, V);
            HIP_TRY(c, hipGetLastError());
            if (pm_out) {
                HIP_TRY(c, hipStreamSynchronize(s));
                SEQ_TRY(d2h_pageable(c, pm_out + 2 * f0 * S, L.pm.p, 2 * nf * S * sizeof(double)));
            }
            f0 += nf;
        }
        HIP_TRY(c, hipStreamSynchronize(s));      // (the chunk's bytes have been read: the next chunk overwrites them)
    }
    // the statuses decide what the mosaic holds; they are read whether the caller asks for them or not
    std::vector<int32_t> status(F);
    SEQ_TRY(d2h_pageable(c, status.data(), T.status_all.p, F * sizeof(int32_t)));
    uint64_t tracked = 0;
    for (size_t f = 0; f < F; ++f) tracked += track_votes(status[f]);
    c->mosaic.votes = tracked * S;
    T.voted = voted;
    unsigned long long cnt[2] = {0, 0};
    HIP_TRY(c, hipMemcpy(cnt, T.counters.p, sizeof cnt, hipMemcpyDeviceToHost));
    if (q_out) SEQ_TRY(d2h_pageable(c, q_out, T.q_all.p, 4 * F * sizeof(double)));
    if (gain_out) SEQ_TRY(d2h_pageable(c, gain_out, T.gain_all.p, F * sizeof(double)));
    if (bias_out) SEQ_TRY(d2h_pageable(c, bias_out, T.bias_all.p, F * sizeof(double)));
    if (status_out) std::copy(status.begin(), status.end(), status_out);
    if (iters_out) SEQ_TRY(d2h_pageable(c, iters_out, T.iters_all.p, F * NL * sizeof(int32_t)));
    if (cost_out) SEQ_TRY(d2h_pageable(c, cost_out, T.cost_all.p, F * sizeof(double)));
    if (counts_out) SEQ_TRY(d2h_pageable(c, counts_out, T.counts_all.p, 4 * F * sizeof(uint64_t)));
    if (overlap_out) SEQ_TRY(d2h_pageable(c, overlap_out, T.overlap_all.p, F * sizeof(double)));
    if (stats_out) { stats_out[0] = tracked; stats_out[1] = F - tracked; stats_out[2] = cnt[0]; stats_out[3] = cnt[1]; }
    return EMBA_OK;
}

extern "C" emba_status emba_track_exposure_eval(emba_ctx* c, const uint8_t* frames, size_t F, const double* q_xyzw, const double* gain, const double* bias,
                                                int32_t level, uint64_t min_weight, int32_t skip_zero, double huber_k, double* sums_out, uint64_t* counts_out,
                                                double* pm_out, double* resid_out)
{
    if (!c) return EMBA_ERR_INVALID_ARG;
    switch (align_args_ok(frames != nullptr, q_xyzw != nullptr, F, 0.0, 255.0, huber_k)) {
    case AlignArgStatus::ok: break;
    case AlignArgStatus::frames_null: return fail(c, EMBA_ERR_INVALID_ARG, "frames NULL");
    case AlignArgStatus::q_null: return fail(c, EMBA_ERR_INVALID_ARG, "q_xyzw NULL");
    case AlignArgStatus::too_many_frames: return fail(c, EMBA_ERR_INVALID_ARG, "F = %zu: frames are counted in 31 bits", F);
    default: return fail(c, EMBA_ERR_INVALID_ARG, "huber_k is not a number");
    }
    SEQ_TRY(track_level_refusal(c, level));
    if (min_weight < 1) return fail(c, EMBA_ERR_INVALID_ARG, "min_weight = 0: a covered cell has a weight of 1 at the least");
    const size_t bad = align_first_bad_q(q_xyzw, F);
    if (bad < F) return fail(c, EMBA_ERR_INVALID_ARG, "q_xyzw[%zu] is not finite or has zero norm", bad);
    SEQ_TRY(exposure_refusals(c, gain, bias, F));
    if (!(c->track.voted >> level & 1u)) return fail(c, EMBA_ERR_STATE, "level %d was not voted into by the last tracker call", (int)level);
    if (!F) return EMBA_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    TrackBuffers& T = c->track;
    const TrackPlane plane = track_plane(c, level);
    const size_t nmax = std::min(view_chunk_frames(c->S, 1), F);
    SEQ_TRY(frame_ensure(c, T.loop, kExposureSums, nmax, pm_out != nullptr, resid_out != nullptr, false));
    SEQ_TRY(ensure<double>(c, T.gain_trial, nmax));
    SEQ_TRY(ensure<double>(c, T.bias_trial, nmax));
    return frame_eval_chunks(
        c, T.loop, kExposureSums, frames, q_xyzw, F,
        [&](const ViewChunk& ch) -> emba_status {
            HIP_TRY(c, hipMemcpyAsync(T.gain_trial.p, gain + ch.f0, ch.nf * sizeof(double), hipMemcpyHostToDevice, c->stream));
            HIP_TRY(c, hipMemcpyAsync(T.bias_trial.p, bias + ch.f0, ch.nf * sizeof(double), hipMemcpyHostToDevice, c->stream));
            return EMBA_OK;
        },
        [&](size_t nf, bool timed) {
            return track_exposure_launch_eval(c, plane, T.loop.frames.as<uint8_t>(), nf, nullptr, min_weight, skip_zero, huber_k, pm_out != nullptr,
                                              resid_out != nullptr, timed);
        },
        sums_out, counts_out, pm_out, resid_out);
}
