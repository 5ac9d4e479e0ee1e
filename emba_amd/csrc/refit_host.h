// emba_amd/csrc/refit_host.h — tracked frames refitted against the mosaic of the other frames, as host code over the kernels of refit_kernels.h (and the
// evaluation, reduce and step kernels of the tracker with exposure): emba_frames_refit.  What is plain arithmetic is decided in refit_rule.h and the rule
// headers under it; here are the buffers (emba_ctx::track: the trackers' own, with the codes of a sweep beside them), the launches and the C ABI.
// Part of emba_hip.hip's translation unit, included by it below track_exposure_host.h; it uses that header (track_exposure_launch_eval), track_host.h
// (track_plane, track_refusals), frame_host.h (frame_ensure, frame_lm_loop: DESIGN.md §23), mosaic_host.h (mosaic_zero_sums), sequence_host.h (SEQ_TRY) and
// transfer_host.h (d2h_pageable).  Every buffer of a call is allocated before anything is zeroed.  Nothing of the registered window, of the resident
// sequence, of the resident map or of any other stage's buffers is written, but for the mosaic's sums and its count of votes.
#pragma once
#include <vector>

#include "context.h"
#include "frame_host.h"
#include "refit_kernels.h"
#include "refit_rule.h"
#include "track_exposure_host.h"

using namespace emba;

namespace {
emba_status refit_refusals(emba_ctx* c, const uint8_t* frames, const int64_t* t_ns, size_t F, const double* q, const double* gain, const double* bias,
                           const int32_t* status, const emba_refit_settings* set)
{
    static const double identity[4] = {0.0, 0.0, 0.0, 1.0};      // (the trackers' q0: there is none here)
    SEQ_TRY(track_refusals(c, frames, t_ns, F, identity, set ? &set->track.track : nullptr));
    switch (track_exposure_args_ok(set->track)) {
    case TrackExposureArgStatus::ok: break;
    case TrackExposureArgStatus::bad_bounds:
        return fail(c, EMBA_ERR_INVALID_ARG, "gain_min = %g, gain_max = %g: finite, 0 < gain_min <= 1 <= gain_max", set->track.gain_min, set->track.gain_max);
    case TrackExposureArgStatus::bad_estimate: return fail(c, EMBA_ERR_INVALID_ARG, "estimate = %d: a mask of gain (1) and bias (2)", (int)set->track.estimate);
    }
    size_t f = 0;
    switch (refit_args_ok(q, gain, bias, status, F, *set, &f)) {
    case RefitArgStatus::ok: break;
    case RefitArgStatus::q_null: return fail(c, EMBA_ERR_INVALID_ARG, "q_xyzw NULL");
    case RefitArgStatus::gain_null: return fail(c, EMBA_ERR_INVALID_ARG, "gain NULL");
    case RefitArgStatus::bias_null: return fail(c, EMBA_ERR_INVALID_ARG, "bias NULL");
    case RefitArgStatus::status_null: return fail(c, EMBA_ERR_INVALID_ARG, "status NULL");
    case RefitArgStatus::bad_sweeps: return fail(c, EMBA_ERR_INVALID_ARG, "sweeps = %d is negative", (int)set->sweeps);
    case RefitArgStatus::bad_sweep_tol: return fail(c, EMBA_ERR_INVALID_ARG, "sweep_tol = %g is negative or not a number", set->sweep_tol);
    case RefitArgStatus::bad_status: return fail(c, EMBA_ERR_INVALID_ARG, "status[%zu] = %d is not an EMBA_TRACK_* value", f, (int)status[f]);
    case RefitArgStatus::no_voting_frame: return fail(c, EMBA_ERR_INVALID_ARG, "no frame votes: a refit needs an anchor or a tracked frame");
    case RefitArgStatus::bad_q: return fail(c, EMBA_ERR_INVALID_ARG, "q_xyzw[%zu] is not finite or has zero norm", f);
    case RefitArgStatus::bad_gain: return fail(c, EMBA_ERR_INVALID_ARG, "gain[%zu] = %g is not finite or outside the bounds", f, gain[f]);
    case RefitArgStatus::bad_bias: return fail(c, EMBA_ERR_INVALID_ARG, "bias[%zu] is not finite", f);
    }
    return EMBA_OK;
}

emba_status refit_launch_frames(emba_ctx* c, RefitFrameParams P)
{
    hipLaunchKernelGGL(emba_frames_refit_frame_kernel, dim3(nblocks((size_t)P.nf, 64)), dim3(64), 0, c->stream, P);
    HIP_TRY(c, hipGetLastError());
    return EMBA_OK;
}

// one launch of the vote kernel over the batch [f0, f0 + nf), whose bytes lie at `bytes`
emba_status refit_launch_vote(emba_ctx* c, RefitVoteParams V, size_t f0, size_t nf, const uint8_t* bytes, int select, bool negate, double* pm)
{
    TrackBuffers& T = c->track;
    V.q = T.q_all.as<double>() + 4 * f0; V.gain = T.gain_all.as<double>() + f0; V.bias = T.bias_all.as<double>() + f0;
    V.status = T.status_all.as<int32_t>() + f0; V.frames = bytes; V.select = select; V.negate = negate ? 1 : 0; V.pm = negate ? nullptr : pm;
    hipLaunchKernelGGL(emba_frames_refit_vote_kernel, dim3(nblocks((size_t)V.S, kFrameThreads), (unsigned)nf), dim3(kFrameThreads), 0, c->stream, V);
    HIP_TRY(c, hipGetLastError());
    return EMBA_OK;
}
}  // namespace

extern "C" emba_status emba_frames_refit(emba_ctx* c, const uint8_t* frames, const int64_t* frame_t_ns, size_t F, const double* q_xyzw, const double* gain,
                                         const double* bias, const int32_t* status_in, const emba_refit_settings* rset, double* q_out, double* gain_out,
                                         double* bias_out, int32_t* status_out, int32_t* refit_out, int32_t* iters_out, double* cost_out, uint64_t* counts_out,
                                         double* overlap_out, double* sweep_out, int32_t* sweeps_done_out, uint64_t* stats_out, double* pm_out)
{
    if (!c) return EMBA_ERR_INVALID_ARG;
    SEQ_TRY(refit_refusals(c, frames, frame_t_ns, F, q_xyzw, gain, bias, status_in, rset));      // (behind it F >= 1: a frame votes)
    const emba_track_exposure_settings* xset = &rset->track;
    const emba_track_settings* set = &xset->track;
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t s = c->stream;
    TrackBuffers& T = c->track;
    FrameLoopBuffers& L = T.loop;
    const size_t S = c->S, NL = (size_t)set->n_levels;
    const bool recover = rset->recover != 0, alternate = rset->alternate != 0;

    int vote_levels[kTrackMaxPlanes];
    const int n_planes = track_vote_levels(*set, vote_levels);
    // the batches, as the tracker cuts them
    const size_t per = view_chunk_frames(S, 1);
    const size_t maxb = std::max<size_t>(std::min(std::min((size_t)set->batch, per), F), 1);
    struct Batch { size_t f0, nf; };
    std::vector<Batch> batches;
    for (size_t f0 = 0; f0 < F;) {
        const size_t nf = track_batch_frames(f0, F, per, (size_t)set->batch);
        batches.push_back({f0, nf});
        f0 += nf;
    }
    // every buffer of the call is there before anything is zeroed (emba_frames_track's order)
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
    SEQ_TRY(ensure<int64_t>(c, T.t, F));
    SEQ_TRY(ensure<double>(c, T.q_all, 4 * F));
    SEQ_TRY(ensure<double>(c, T.gain_all, F));
    SEQ_TRY(ensure<double>(c, T.bias_all, F));
    SEQ_TRY(ensure<int32_t>(c, T.status_all, F));
    SEQ_TRY(ensure<int32_t>(c, T.refit_all, F));
    SEQ_TRY(ensure<int32_t>(c, T.iters_all, F * NL));
    SEQ_TRY(ensure<double>(c, T.cost_all, F));
    SEQ_TRY(ensure<double>(c, T.overlap_all, F));
    SEQ_TRY(ensure<unsigned long long>(c, T.counts_all, 4 * F));
    SEQ_TRY(ensure<unsigned long long>(c, T.counters, 2));
    SEQ_TRY(ensure<uint8_t>(c, L.frames, std::min(per, F) * S));      // (a chunk's bytes; the batches are no longer than a chunk)
    SEQ_TRY(ensure<double>(c, T.gain_trial, maxb));
    SEQ_TRY(ensure<double>(c, T.bias_trial, maxb));
    SEQ_TRY(ensure<double>(c, T.gain, maxb));
    SEQ_TRY(ensure<double>(c, T.bias, maxb));
    SEQ_TRY(frame_ensure(c, L, kExposureSums, maxb, pm_out != nullptr, false, true));
    std::vector<double> q_before(q_xyzw, q_xyzw + 4 * F), q_after(4 * F), cost(F);
    std::vector<int32_t> code(F), status(F);

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

    RefitVoteParams V{};
    V.lut = c->d_lut.as<double>(); V.S = (int)S; V.n_planes = n_planes;
    V.fx = c->fx; V.fy = c->fy; V.cx = c->cx; V.cy = c->cy; V.skip_zero = set->skip_zero != 0;
    for (int k = 0; k < n_planes; ++k) V.plane[k] = track_plane(c, vote_levels[k]);
    V.counters = T.counters.as<unsigned long long>();
    TrackPlane sched[kTrackMaxSchedule];
    for (size_t k = 0; k < NL; ++k) sched[k] = track_plane(c, set->levels[k]);
    double* pm = pm_out ? L.pm.as<double>() : nullptr;

    // the call's frames: times, rotations, exposures and statuses up, resident until the end
    HIP_TRY(c, hipMemcpyAsync(T.t.p, frame_t_ns, F * sizeof(int64_t), hipMemcpyHostToDevice, s));
    HIP_TRY(c, hipMemcpyAsync(T.q_all.p, q_xyzw, 4 * F * sizeof(double), hipMemcpyHostToDevice, s));
    HIP_TRY(c, hipMemcpyAsync(T.gain_all.p, gain, F * sizeof(double), hipMemcpyHostToDevice, s));
    HIP_TRY(c, hipMemcpyAsync(T.bias_all.p, bias, F * sizeof(double), hipMemcpyHostToDevice, s));
    HIP_TRY(c, hipMemcpyAsync(T.status_all.p, status_in, F * sizeof(int32_t), hipMemcpyHostToDevice, s));
    HIP_TRY(c, hipMemsetAsync(T.counters.p, 0, 2 * sizeof(unsigned long long), s));

    RefitFrameParams B{};
    B.F = (long)F; B.n_levels = (int)NL; B.recover = recover; B.min_overlap = set->min_overlap; B.S = (unsigned long long)S;
    B.t = reinterpret_cast<const long long*>(T.t.as<int64_t>());
    B.q_all = T.q_all.as<double>(); B.gain_all = T.gain_all.as<double>(); B.bias_all = T.bias_all.as<double>();
    B.status_all = T.status_all.as<int32_t>(); B.refit_all = T.refit_all.as<int32_t>(); B.iters_all = T.iters_all.as<int32_t>();
    B.cost_all = T.cost_all.as<double>(); B.overlap_all = T.overlap_all.as<double>(); B.counts_all = T.counts_all.as<unsigned long long>();
    B.q = L.q.as<double>(); B.q_trial = L.q_trial.as<double>();
    B.gain = T.gain.as<double>(); B.gain_trial = T.gain_trial.as<double>();
    B.bias = T.bias.as<double>(); B.bias_trial = T.bias_trial.as<double>();
    B.sums = L.sums.as<double>(); B.counts = L.counts.as<unsigned long long>(); B.status = L.status.as<int32_t>(); B.iters = L.iters.as<int32_t>();

    const emba_exposure_settings xs{set->align, xset->gain_min, xset->gain_max};
    ExposureStepParams P{0, 1, (int)xset->estimate, xs, L.q.as<double>(), L.q_trial.as<double>(), T.gain.as<double>(), T.bias.as<double>(),
                         T.gain_trial.as<double>(), T.bias_trial.as<double>(), L.sums.as<double>(), L.lambda.as<double>(), L.dnorm.as<double>(),
                         L.counts.as<unsigned long long>(), L.status.as<int32_t>(), L.iters.as<int32_t>(), L.have_trial.as<int32_t>(), L.esums.as<double>(),
                         L.ecounts.as<unsigned long long>(), L.cost0.as<double>(), L.n0.as<unsigned long long>(), L.running.as<unsigned int>()};

    // a batch's chunk on the device: the chunk that is there is kept, another one waits for the stream (its bytes overwrite those being read) and goes up
    size_t resident = (size_t)-1;
    auto chunk_bytes = [&](const Batch& b, const uint8_t** bytes) -> emba_status {
        const size_t i = b.f0 / per;
        if (i != resident) {
            const ViewChunk ch = view_chunk(F, per, i);
            HIP_TRY(c, hipStreamSynchronize(s));
            HIP_TRY(c, hipMemcpyAsync(L.frames.p, frames + ch.f0 * S, ch.nf * S, hipMemcpyHostToDevice, s));
            resident = i;
        }
        *bytes = L.frames.as<uint8_t>() + (b.f0 - resident * per) * S;
        return EMBA_OK;
    };
    auto read_pm = [&](const Batch& b) -> emba_status {
        if (!pm_out) return EMBA_OK;
        HIP_TRY(c, hipStreamSynchronize(s));
        return d2h_pageable(c, pm_out + 2 * b.f0 * S, L.pm.p, 2 * b.nf * S * sizeof(double));
    };
    auto sweep_begin = [&]() {
        B.phase = kRefitSweepBegin; B.f0 = 0; B.nf = (long)F;
        return refit_launch_frames(c, B);
    };

    // the build: every voting frame at its given (q, a, b)
    for (const Batch& b : batches) {
        const uint8_t* bytes = nullptr;
        SEQ_TRY(chunk_bytes(b, &bytes));
        SEQ_TRY(refit_launch_vote(c, V, b.f0, b.nf, bytes, kRefitSelectVoting, false, pm));
        SEQ_TRY(read_pm(b));
    }
    if (rset->sweeps == 0) SEQ_TRY(sweep_begin());

    bool timed = c->kernel_timing != 0;
    int32_t done = 0;
    for (int sweep = 0; sweep < rset->sweeps; ++sweep) {
        SEQ_TRY(sweep_begin());
        for (size_t k = 0; k < batches.size(); ++k) {
            const Batch& b = batches[refit_batch_index(sweep, k, batches.size(), alternate)];
            if (!refit_batch_active(status_in, b.f0, b.nf, recover)) continue;
            const uint8_t* bytes = nullptr;
            SEQ_TRY(chunk_bytes(b, &bytes));
            const size_t nf = b.nf;
            SEQ_TRY(refit_launch_vote(c, V, b.f0, nf, bytes, kRefitSelectMovable, true, nullptr));
            B.nf = (long)nf; B.f0 = (long)b.f0;
            B.phase = kRefitStart;
            SEQ_TRY(refit_launch_frames(c, B));
            P.nf = (long)nf;
            for (size_t l = 0; l < NL; ++l) {
                // §24's loop against this level: evaluation 0 where the previous level ended
                SEQ_TRY(frame_lm_loop(
                    c, L,
                    [&](const int32_t* st, bool) {
                        const bool t = timed;
                        timed = false;
                        return track_exposure_launch_eval(c, sched[l], bytes, nf, st, set->min_weight, set->skip_zero, set->align.huber_k, false, false, t);
                    },
                    [&](bool first) {
                        P.first = first;
                        hipLaunchKernelGGL(emba_frames_exposure_step_kernel, dim3(nblocks(nf, 64)), dim3(64), 0, s, P);
                    }));
                B.phase = kRefitLevelEnd; B.level_index = (int)l;
                SEQ_TRY(refit_launch_frames(c, B));
            }
            B.phase = kRefitVerdict;
            SEQ_TRY(refit_launch_frames(c, B));
            SEQ_TRY(refit_launch_vote(c, V, b.f0, nf, bytes, kRefitSelectMovable, false, pm));
            SEQ_TRY(read_pm(b));
        }
        // the sweep's figures: the rotations, the codes and the last-level costs
        HIP_TRY(c, hipStreamSynchronize(s));
        SEQ_TRY(d2h_pageable(c, q_after.data(), T.q_all.p, 4 * F * sizeof(double)));
        SEQ_TRY(d2h_pageable(c, code.data(), T.refit_all.p, F * sizeof(int32_t)));
        SEQ_TRY(d2h_pageable(c, cost.data(), T.cost_all.p, F * sizeof(double)));
        const double change = refit_rotation_change(q_before.data(), q_after.data(), F);
        if (sweep_out) {
            double moved = 0.0, recovered = 0.0, total = 0.0;
            for (size_t f = 0; f < F; ++f) { moved += code[f] == EMBA_REFIT_MOVED; recovered += code[f] == EMBA_REFIT_RECOVERED; total += cost[f]; }
            double* o = sweep_out + 4 * (size_t)sweep;
            o[0] = moved; o[1] = recovered; o[2] = change; o[3] = total;
        }
        q_before.swap(q_after);
        ++done;
        if (refit_converged(change, rset->sweep_tol)) break;
    }
    HIP_TRY(c, hipStreamSynchronize(s));
    // the statuses decide what the mosaic holds; they are read whether the caller asks for them or not
    SEQ_TRY(d2h_pageable(c, status.data(), T.status_all.p, F * sizeof(int32_t)));
    uint64_t voting = 0;
    for (size_t f = 0; f < F; ++f) voting += track_votes(status[f]);
    c->mosaic.votes = voting * S;
    T.voted = voted;
    unsigned long long cnt[2] = {0, 0};
    HIP_TRY(c, hipMemcpy(cnt, T.counters.p, sizeof cnt, hipMemcpyDeviceToHost));
    if (q_out) SEQ_TRY(d2h_pageable(c, q_out, T.q_all.p, 4 * F * sizeof(double)));
    if (gain_out) SEQ_TRY(d2h_pageable(c, gain_out, T.gain_all.p, F * sizeof(double)));
    if (bias_out) SEQ_TRY(d2h_pageable(c, bias_out, T.bias_all.p, F * sizeof(double)));
    if (status_out) std::copy(status.begin(), status.end(), status_out);
    if (refit_out) SEQ_TRY(d2h_pageable(c, refit_out, T.refit_all.p, F * sizeof(int32_t)));
    if (iters_out) SEQ_TRY(d2h_pageable(c, iters_out, T.iters_all.p, F * NL * sizeof(int32_t)));
    if (cost_out) SEQ_TRY(d2h_pageable(c, cost_out, T.cost_all.p, F * sizeof(double)));
    if (counts_out) SEQ_TRY(d2h_pageable(c, counts_out, T.counts_all.p, 4 * F * sizeof(uint64_t)));
    if (overlap_out) SEQ_TRY(d2h_pageable(c, overlap_out, T.overlap_all.p, F * sizeof(double)));
    if (sweeps_done_out) *sweeps_done_out = done;
    if (stats_out) { stats_out[0] = voting; stats_out[1] = F - voting; stats_out[2] = cnt[0]; stats_out[3] = cnt[1]; }
    return EMBA_OK;
}
