// emba_amd/csrc/panorama_host.h — the panorama of warped events along a trajectory, as host code over the kernels of panorama_kernels.h: every event of a
// range of the resident sequence voted onto the equirectangular panorama at its batch's spline pose, and the contrast of that image
// (emba_seq_event_panorama).  What is plain arithmetic — the argument checks, the batches, the votes of one event — is decided in panorama_rule.h; here are
// the buffers (emba_ctx::pano), the launches and the C ABI.
// Also here, for contrast_host.h as well: the pose stage of a range of the resident sequence (seq_range_poses) with its argument messages and its
// status word.
// Part of emba_hip.hip's translation unit, included by it below sequence_host.h (SEQ_TRY; the sequence itself: emba_ctx::evseq) and transfer_host.h
// (d2h_pageable: the pinned staging path).  Nothing of the registered window is read or written.
#pragma once
#include "context.h"
#include "panorama_kernels.h"
#include "panorama_rule.h"

using namespace emba;

namespace {
constexpr int kSeqStageTimerSlot = 7;      // the last of the context's timer slots (emba_timer_*): with kernel timing on, the events around a stage's vote (and gradient) kernels
}

// What the argument checks of a range call found, as the C ABI reports it (too_long: the integer panorama alone can answer it).
static emba_status seq_range_args(emba_ctx* c, PanoArgStatus st, size_t beg, size_t end, int32_t K, int64_t dt_ns)
{
    switch (st) {
    case PanoArgStatus::not_a_range: return fail(c, EMBA_ERR_INVALID_ARG, "[%zu, %zu) is not a range of the resident sequence of %zu events", beg, end, c->evseq.n);
    case PanoArgStatus::too_few_knots: return fail(c, EMBA_ERR_INVALID_ARG, "K = %d: a linear spline has at least two control poses", (int)K);
    case PanoArgStatus::bad_dt: return fail(c, EMBA_ERR_INVALID_ARG, "dt_ns = %lld: the knot spacing must be positive", (long long)dt_ns);
    case PanoArgStatus::too_long:
        return fail(c, EMBA_ERR_INVALID_ARG, "[%zu, %zu): the 32-bit cells of the image count fewer than %zu events exactly", beg, end, kPanoMaxEvents);
    case PanoArgStatus::ok: break;
    }
    return EMBA_OK;
}

// The pose stage of a call on the events [beg, end) (at least one whole batch) that votes on `cells` cells: the range's own batches,
// [beg + 100 b, beg + 100 b + 100) — the midpoints emba_set_events_seq(beg, end) gives that range — and their rotations, into emba_ctx::seq_pose.  head: the
// call's `head_words` 8-byte result words, zeroed here on the stream; word `status_word` takes the pose stage's status (seq_range_status).  A batch
// outside the knots leaves its pose record unwritten and sets that word: the vote rules keep every add inside the image whatever the record holds.
static emba_status seq_range_poses(emba_ctx* c, size_t beg, size_t end, const double* knots_xyzw, int32_t K, int64_t t0_ns, int64_t dt_ns, size_t cells,
                                   DevBuf& head, size_t head_words, size_t status_word)
{
    if (!knots_xyzw) return fail(c, EMBA_ERR_INVALID_ARG, "knots NULL");
    if (cells > 0x7FFFFFFFull) return fail(c, EMBA_ERR_INVALID_ARG, "a panorama of %zu cells is too large for 32-bit cell indices", cells);
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t s = c->stream;
    const size_t nb = pano_batch_count(beg, end);
    SeqPoseBuffers& B = c->seq_pose;
    SEQ_TRY(ensure<int64_t>(c, B.batch_t, nb));
    SEQ_TRY(ensure<double>(c, B.pose, nb * (size_t)kPoseStride));
    SEQ_TRY(ensure<double>(c, B.knots, 4 * (size_t)K));
    SEQ_TRY(ensure<uint64_t>(c, head, head_words));
    HIP_TRY(c, hipMemcpyAsync(B.knots.p, knots_xyzw, (size_t)K * 32, hipMemcpyHostToDevice, s));
    HIP_TRY(c, hipMemsetAsync(head.p, 0, head_words * 8, s));
    hipLaunchKernelGGL(emba_batch_mid_kernel, dim3(nblocks(nb)), dim3(256), 0, s, (const int64_t*)c->evseq.t.as<int64_t>() + beg, (long)nb, B.batch_t.as<int64_t>());
    hipLaunchKernelGGL(emba_pose_kernel, dim3(nblocks(nb, 64)), dim3(64), 0, s, (const int64_t*)B.batch_t.as<int64_t>(), (int)nb, (const double*)B.knots.as<double>(), (int)K,
                       t0_ns, dt_ns, B.pose.as<double>(), reinterpret_cast<int*>(head.as<uint64_t>() + status_word));
    return EMBA_OK;
}

// The status word back on the host, after the call's synchronisation.
static emba_status seq_range_status(emba_ctx* c, uint64_t word, size_t beg, size_t end)
{
    if ((int)(word & 0xFFFFFFFFull) & 1) return fail(c, EMBA_ERR_TIME_RANGE, "a batch midpoint of [%zu, %zu) lies outside the spline's knots", beg, end);
    return EMBA_OK;
}

// What every stage over the range reads of an event (SeqEventParams), from the context and the pose stage's table.
static SeqEventParams seq_event_params(emba_ctx* c, size_t beg, size_t nn, int32_t signed_polarity, unsigned long long* dropped, double* pm)
{
    return SeqEventParams{c->evseq.x.as<uint16_t>() + beg, c->evseq.y.as<uint16_t>() + beg, c->evseq.pol.as<uint8_t>() + beg, c->d_lut.as<double>(), c->seq_pose.pose.as<double>(),
                          (long)nn, c->sw, c->fx, c->fy, c->cx, c->cy, signed_polarity != 0, dropped, pm};
}

extern "C" emba_status emba_seq_event_panorama(emba_ctx* c, size_t beg, size_t end, const double* knots_xyzw, int32_t K, int64_t t0_ns, int64_t dt_ns,
                                               int32_t signed_polarity, int32_t* image_out, uint64_t* j_out, int64_t* sum_out, uint64_t* nonzero_out,
                                               uint64_t* dropped_out, double* pm_out)
{
    if (!c) return EMBA_ERR_INVALID_ARG;
    if (!c->evseq.have) return fail(c, EMBA_ERR_STATE, "no resident sequence (emba_seq_upload first)");
    SEQ_TRY(seq_range_args(c, pano_args_ok(beg, end, c->evseq.n, K, dt_ns), beg, end, K, dt_ns));
    if (!image_out && !j_out && !sum_out && !nonzero_out && !dropped_out && !pm_out) return EMBA_OK;      // nothing asked for: nothing launched
    const size_t nn = pano_events_used(beg, end), cells = c->npix;
    if (!nn) {      // an empty or sub-batch range: no event votes
        if (image_out) std::memset(image_out, 0, cells * sizeof(int32_t));
        if (j_out) *j_out = 0;
        if (sum_out) *sum_out = 0;
        if (nonzero_out) *nonzero_out = 0;
        if (dropped_out) *dropped_out = 0;
        return EMBA_OK;
    }
    SEQ_TRY(seq_range_poses(c, beg, end, knots_xyzw, K, t0_ns, dt_ns, cells, c->pano.out, 8, 4));      // out: [0..2] J, sum, non-zero cells  [3] dropped votes  [4] the status word
    hipStream_t s = c->stream;
    SEQ_TRY(ensure<int32_t>(c, c->pano.image, cells));
    SEQ_TRY(ensure<unsigned long long>(c, c->pano.slots, (size_t)kPanoSums * kPanoReduceSlots));
    if (pm_out) SEQ_TRY(ensure<double>(c, c->pano.pm, 2 * nn));
    unsigned long long* d_out = c->pano.out.as<unsigned long long>();
    HIP_TRY(c, hipMemsetAsync(c->pano.image.p, 0, cells * sizeof(int32_t), s));
    PanoParams P{seq_event_params(c, beg, nn, signed_polarity, d_out + 3, pm_out ? c->pano.pm.as<double>() : (double*)nullptr), c->W, c->H, c->pano.image.as<int32_t>()};
    if (c->kernel_timing) HIP_TRY(c, hipEventRecord(c->ev_start[kSeqStageTimerSlot], s));      // (emba_enable_kernel_timing: emba_timer_elapsed_ms(7) is the vote kernel's time)
    hipLaunchKernelGGL(emba_pano_vote_kernel, dim3(nblocks(nn, kPanoThreads)), dim3(kPanoThreads), 0, s, P);
    if (c->kernel_timing) HIP_TRY(c, hipEventRecord(c->ev_stop[kSeqStageTimerSlot], s));
    // contrast
    const unsigned rblocks = std::min<unsigned>(nblocks(cells, kPanoThreads * 4), kPanoReduceBlocks);
    hipLaunchKernelGGL(emba_pano_reduce_kernel, dim3(rblocks), dim3(kPanoThreads), 0, s, (const int32_t*)c->pano.image.as<int32_t>(), (long)cells, c->pano.slots.as<unsigned long long>());
    hipLaunchKernelGGL(emba_pano_reduce_final_kernel, dim3(1), dim3(64), 0, s, (const unsigned long long*)c->pano.slots.as<unsigned long long>(), (int)(rblocks * (kPanoThreads / 64)), d_out);
    HIP_TRY(c, hipGetLastError());
    unsigned long long h_out[5] = {0, 0, 0, 0, 0};
    HIP_TRY(c, hipMemcpyAsync(h_out, d_out, sizeof h_out, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipStreamSynchronize(s));
    SEQ_TRY(seq_range_status(c, h_out[4], beg, end));
    if (j_out) *j_out = h_out[0];
    if (sum_out) *sum_out = (int64_t)h_out[1];
    if (nonzero_out) *nonzero_out = h_out[2];
    if (dropped_out) *dropped_out = h_out[3];
    if (image_out) SEQ_TRY(d2h_pageable(c, image_out, c->pano.image.p, cells * sizeof(int32_t)));
    if (pm_out) SEQ_TRY(d2h_pageable(c, pm_out, c->pano.pm.p, 2 * nn * sizeof(double)));
    return EMBA_OK;
}
