// emba_amd/csrc/track_host.h — intensity frames tracked against their own growing mosaic, as host code over the kernels of track_kernels.h (and the reduce
// and step kernels of align_kernels.h): the tracker (emba_frames_track), one evaluation against a level's planes as they stand (emba_track_eval) and the
// planes themselves (emba_track_level_get).  What is plain arithmetic — the argument checks, the levels, the batches, the prediction, the pixel, the verdict
// — is decided in track_rule.h; here are the buffers (emba_ctx::track), the launches and the C ABI.
// Part of emba_hip.hip's translation unit, included by it below align_host.h; it uses frame_host.h (the buffers of a batch, one evaluation, the chunked
// evaluation, the loop: DESIGN.md §23), align_host.h (align_launch_step), sequence_host.h (SEQ_TRY), transfer_host.h (d2h_pageable) and mosaic_host.h
// (mosaic_zero_sums: level 0's planes are the mosaic's sums).  Nothing of the registered window, of
// the resident sequence, of the resident map or of any other stage's buffers is written, but for the mosaic's sums and its count of votes.
#pragma once
#include "align_host.h"
#include "context.h"
#include "frame_host.h"
#include "track_kernels.h"
#include "track_rule.h"

using namespace emba;

namespace {
// the planes of level l as they stand (level 0: the mosaic's)
TrackPlane track_plane(emba_ctx* c, int l)
{
    TrackLevel g{};
    track_level(c->W, c->H, l, &g);
    TrackBuffers& T = c->track;
    return TrackPlane{l ? T.lw[l].as<unsigned long long>() : c->mosaic.sum_w.as<unsigned long long>(), l ? T.lv[l].as<unsigned long long>() : c->mosaic.sum_v.as<unsigned long long>(),
                      g.W, g.H, g.scale};
}

emba_status track_level_refusal(emba_ctx* c, int l)
{
    switch (track_level(c->W, c->H, l, nullptr)) {
    case TrackLevelStatus::ok: break;
    case TrackLevelStatus::out_of_range: return fail(c, EMBA_ERR_INVALID_ARG, "level = %d: levels are 0 ... %d", l, kTrackMaxLevel);
    case TrackLevelStatus::not_divisible: return fail(c, EMBA_ERR_INVALID_ARG, "level = %d: the panorama %d x %d is not divisible by %d", l, c->W, c->H, 1 << l);
    case TrackLevelStatus::too_few_rows: return fail(c, EMBA_ERR_INVALID_ARG, "level = %d leaves %d rows: a sample needs two", l, c->H >> l);
    }
    return EMBA_OK;
}

emba_status track_refusals(emba_ctx* c, const uint8_t* frames, const int64_t* t_ns, size_t F, const double* q0, const emba_track_settings* set)
{
    size_t where = 0;
    switch (track_args_ok(frames != nullptr, t_ns != nullptr, q0, set, t_ns, F, c->S, c->W, c->H, &where)) {
    case TrackArgStatus::ok: break;
    case TrackArgStatus::frames_null: return fail(c, EMBA_ERR_INVALID_ARG, "frames NULL");
    case TrackArgStatus::times_null: return fail(c, EMBA_ERR_INVALID_ARG, "frame_t_ns NULL");
    case TrackArgStatus::q0_null: return fail(c, EMBA_ERR_INVALID_ARG, "q0_xyzw NULL");
    case TrackArgStatus::settings_null: return fail(c, EMBA_ERR_INVALID_ARG, "settings NULL");
    case TrackArgStatus::too_many_frames: return fail(c, EMBA_ERR_INVALID_ARG, "F = %zu: frames are counted in 31 bits", F);
    case TrackArgStatus::schedule_length: return fail(c, EMBA_ERR_INVALID_ARG, "n_levels = %d: a schedule names 1 ... %d levels", (int)set->n_levels, kTrackMaxSchedule);
    case TrackArgStatus::level_range:
    case TrackArgStatus::level_not_divisible:
    case TrackArgStatus::level_too_few_rows: return track_level_refusal(c, set->levels[where]);
    case TrackArgStatus::bad_batch: return fail(c, EMBA_ERR_INVALID_ARG, "batch = %d: a batch has one frame at the least", (int)set->batch);
    case TrackArgStatus::bad_min_overlap: return fail(c, EMBA_ERR_INVALID_ARG, "min_overlap = %g is not in [0, 1]", set->min_overlap);
    case TrackArgStatus::bad_min_weight: return fail(c, EMBA_ERR_INVALID_ARG, "min_weight = 0: a covered cell has a weight of 1 at the least");
    case TrackArgStatus::times_not_increasing: return fail(c, EMBA_ERR_INVALID_ARG, "frame_t_ns[%zu] is not behind frame_t_ns[%zu]", where, where - 1);
    case TrackArgStatus::bad_q0: return fail(c, EMBA_ERR_INVALID_ARG, "q0_xyzw is not finite or has zero norm");
    case TrackArgStatus::bad_align_settings: return fail(c, EMBA_ERR_INVALID_ARG, "settings.align is out of range (emba_frames_align's refusals)");
    case TrackArgStatus::too_many_votes: return fail(c, EMBA_ERR_INVALID_ARG, "%zu frames of %zu pixels: the sums are exact below 2^36 votes", F, (size_t)c->S);
    }
    return EMBA_OK;
}

// one evaluation of nf frames (bytes at `bytes`) at T.q_trial against `plane` into T.esums / T.ecounts: the evaluation kernel and §20's reduction of its
// partial sums.  `status`: the loop's status words, or nullptr (every frame is evaluated); `timed`: timer slot 7 around the evaluation kernel
emba_status track_launch_eval(emba_ctx* c, const TrackPlane& plane, const uint8_t* bytes, size_t nf, const int32_t* status, uint64_t min_weight, int32_t skip_zero,
                              double huber_k, bool want_pm, bool want_resid, bool timed)
{
    FrameLoopBuffers& T = c->track.loop;
    const TrackEvalParams P{c->d_lut.as<double>(), T.q_trial.as<double>(), status, bytes, plane.sum_w, plane.sum_v, (int)c->S, plane.W, plane.H, plane.scale,
                            c->fx, c->fy, c->cx, c->cy, (unsigned long long)min_weight, huber_k, skip_zero != 0, T.partial.as<double>(),
                            want_pm ? T.pm.as<double>() : nullptr, want_resid ? T.resid.as<double>() : nullptr};
    return frame_launch_eval(c, T, emba_frames_track_eval_kernel, P, emba_frames_align_reduce_kernel, kAlignSums, nf, timed);
}

emba_status track_launch_frames(emba_ctx* c, TrackFrameParams P)
{
    hipLaunchKernelGGL(emba_frames_track_frame_kernel, dim3(nblocks((size_t)P.nf, 64)), dim3(64), 0, c->stream, P);
    HIP_TRY(c, hipGetLastError());
    return EMBA_OK;
}
}  // namespace

extern "C" emba_status emba_frames_track(emba_ctx* c, const uint8_t* frames, const int64_t* frame_t_ns, size_t F, const double* q0_xyzw, const emba_track_settings* set,
                                         double* q_out, int32_t* status_out, int32_t* iters_out, double* cost_out, uint64_t* counts_out, double* overlap_out,
                                         uint64_t* stats_out, double* pm_out)
{
    if (!c) return EMBA_ERR_INVALID_ARG;
    SEQ_TRY(track_refusals(c, frames, frame_t_ns, F, q0_xyzw, set));
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t s = c->stream;
    TrackBuffers& T = c->track;
    FrameLoopBuffers& L = T.loop;
    const size_t S = c->S, NL = (size_t)set->n_levels;

    // the planes: every level a tracked frame votes into, zero
    int vote_levels[kTrackMaxPlanes];
    const int n_planes = track_vote_levels(*set, vote_levels);
    // every buffer of the call is there before anything is zeroed: a failed allocation leaves the mosaic and the level planes as they were (a plane
    // that had to grow is new memory: its level counts as not voted until the call has ended)
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
        SEQ_TRY(ensure<int32_t>(c, T.status_all, F));
        SEQ_TRY(ensure<int32_t>(c, T.iters_all, F * NL));
        SEQ_TRY(ensure<double>(c, T.cost_all, F));
        SEQ_TRY(ensure<double>(c, T.overlap_all, F));
        SEQ_TRY(ensure<unsigned long long>(c, T.counts_all, 4 * F));
        SEQ_TRY(ensure<unsigned long long>(c, T.counters, 2));
        SEQ_TRY(ensure<uint8_t>(c, L.frames, std::min(per, F) * S));      // (a chunk's bytes; the batches below are no longer than a chunk)
        SEQ_TRY(ensure<double>(c, T.pred, 4 * maxb));
        SEQ_TRY(frame_ensure(c, L, kAlignSums, maxb, pm_out != nullptr, false, true));
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
    TrackVoteParams V{};
    V.lut = c->d_lut.as<double>(); V.S = (int)S; V.n_planes = n_planes;
    V.fx = c->fx; V.fy = c->fy; V.cx = c->cx; V.cy = c->cy; V.skip_zero = set->skip_zero != 0;
    for (int k = 0; k < n_planes; ++k) V.plane[k] = track_plane(c, vote_levels[k]);
    TrackPlane sched[kTrackMaxSchedule];
    for (size_t k = 0; k < NL; ++k) sched[k] = track_plane(c, set->levels[k]);

    // the call's frames: times up, rotations and statuses resident until the end
    HIP_TRY(c, hipMemcpyAsync(T.t.p, frame_t_ns, F * sizeof(int64_t), hipMemcpyHostToDevice, s));
    HIP_TRY(c, hipMemsetAsync(T.status_all.p, 0, F * sizeof(int32_t), s));
    HIP_TRY(c, hipMemsetAsync(T.counters.p, 0, 2 * sizeof(unsigned long long), s));
    V.counters = T.counters.as<unsigned long long>();
    V.pm = pm_out ? L.pm.as<double>() : nullptr;

    TrackFrameParams B{};
    B.n_levels = (int)NL; B.predict = set->predict != 0; B.min_overlap = set->min_overlap; B.S = (unsigned long long)S;
    track_normalise(q0_xyzw, B.q0);
    B.t = reinterpret_cast<const long long*>(T.t.as<int64_t>());
    B.q_all = T.q_all.as<double>(); B.status_all = T.status_all.as<int32_t>(); B.iters_all = T.iters_all.as<int32_t>();
    B.cost_all = T.cost_all.as<double>(); B.overlap_all = T.overlap_all.as<double>(); B.counts_all = T.counts_all.as<unsigned long long>();
    B.pred = T.pred.as<double>(); B.q = L.q.as<double>(); B.q_trial = L.q_trial.as<double>(); B.sums = L.sums.as<double>();
    B.counts = L.counts.as<unsigned long long>(); B.status = L.status.as<int32_t>(); B.iters = L.iters.as<int32_t>();

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
                SEQ_TRY(track_launch_frames(c, B));
            } else {
                B.phase = kTrackPredict;
                SEQ_TRY(track_launch_frames(c, B));
                for (size_t k = 0; k < NL; ++k) {
                    // §20's loop against this level: evaluation 0 where the previous level ended
                    SEQ_TRY(frame_lm_loop(
                        c, L,
                        [&](const int32_t* status, bool) {
                            const bool t = timed;
                            timed = false;
                            return track_launch_eval(c, sched[k], bytes, nf, status, set->min_weight, set->skip_zero, set->align.huber_k, false, false, t);
                        },
                        [&](bool first) { align_launch_step(c, L, nf, set->align, first); }));
                    B.phase = kTrackLevelEnd; B.level_index = (int)k;
                    SEQ_TRY(track_launch_frames(c, B));
                }
                B.phase = kTrackVerdict;
                SEQ_TRY(track_launch_frames(c, B));
            }
            V.q = T.q_all.as<double>() + 4 * f0; V.status = T.status_all.as<int32_t>() + f0; V.frames = bytes;
            hipLaunchKernelGGL(emba_frames_track_vote_kernel, dim3(nblocks(S, kFrameThreads), (unsigned)nf), dim3(kFrameThreads), 0, s, V);
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
    if (status_out) std::copy(status.begin(), status.end(), status_out);
    if (iters_out) SEQ_TRY(d2h_pageable(c, iters_out, T.iters_all.p, F * NL * sizeof(int32_t)));
    if (cost_out) SEQ_TRY(d2h_pageable(c, cost_out, T.cost_all.p, F * sizeof(double)));
    if (counts_out) SEQ_TRY(d2h_pageable(c, counts_out, T.counts_all.p, 4 * F * sizeof(uint64_t)));
    if (overlap_out) SEQ_TRY(d2h_pageable(c, overlap_out, T.overlap_all.p, F * sizeof(double)));
    if (stats_out) { stats_out[0] = tracked; stats_out[1] = F - tracked; stats_out[2] = cnt[0]; stats_out[3] = cnt[1]; }
    return EMBA_OK;
}

extern "C" emba_status emba_track_eval(emba_ctx* c, const uint8_t* frames, size_t F, const double* q_xyzw, int32_t level, uint64_t min_weight, int32_t skip_zero,
                                       double huber_k, double* sums_out, uint64_t* counts_out, double* pm_out, double* resid_out)
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
    if (!(c->track.voted >> level & 1u)) return fail(c, EMBA_ERR_STATE, "level %d was not voted into by the last emba_frames_track", (int)level);
    if (!F) return EMBA_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    FrameLoopBuffers& T = c->track.loop;
    const TrackPlane plane = track_plane(c, level);
    SEQ_TRY(frame_ensure(c, T, kAlignSums, std::min(view_chunk_frames(c->S, 1), F), pm_out != nullptr, resid_out != nullptr, false));
    return frame_eval_chunks(
        c, T, kAlignSums, frames, q_xyzw, F, [](const ViewChunk&) { return EMBA_OK; },
        [&](size_t nf, bool timed) {
            return track_launch_eval(c, plane, T.frames.as<uint8_t>(), nf, nullptr, min_weight, skip_zero, huber_k, pm_out != nullptr, resid_out != nullptr, timed);
        },
        sums_out, counts_out, pm_out, resid_out);
}

extern "C" emba_status emba_track_level_get(emba_ctx* c, int32_t level, uint64_t* sum_w_out, uint64_t* sum_v_out)
{
    if (!c) return EMBA_ERR_INVALID_ARG;
    SEQ_TRY(track_level_refusal(c, level));
    if (!(c->track.voted >> level & 1u)) return fail(c, EMBA_ERR_STATE, "level %d was not voted into by the last emba_frames_track", (int)level);
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    const TrackPlane plane = track_plane(c, level);
    const size_t bytes = (size_t)plane.W * (size_t)plane.H * sizeof(uint64_t);
    if (sum_w_out) SEQ_TRY(d2h_pageable(c, sum_w_out, plane.sum_w, bytes));
    if (sum_v_out) SEQ_TRY(d2h_pageable(c, sum_v_out, plane.sum_v, bytes));
    return EMBA_OK;
}
