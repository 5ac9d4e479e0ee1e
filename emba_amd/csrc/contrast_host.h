// emba_amd/csrc/contrast_host.h — the smooth contrast of the panorama of warped events and its gradient with respect to the control poses, as host code
// over the kernels of contrast_kernels.h (emba_seq_contrast_gradient, emba_seq_contrast_gradient_level).  What is plain arithmetic — the argument checks, the votes of one event and their
// derivatives, the gradient of one event, the span plan, the grid of a level and the vote kernel it takes — is decided in contrast_rule.h; here are the buffers (emba_ctx::contrast), the launches and the
// C ABI.
// Part of emba_hip.hip's translation unit, included by it below panorama_host.h (SEQ_TRY, d2h_pageable, the sequence itself: emba_ctx::evseq).  Nothing of
// the registered window or of the integer panorama is read or written: the batch times, the pose table, the control poses, the image and the status word
// of this call are its own.
#pragma once
#include <vector>

#include "context.h"
#include "contrast_kernels.h"
#include "contrast_rule.h"

using namespace emba;

namespace {
constexpr int kContrastTimerSlot = 7;      // with kernel timing on: the events around the vote kernel and the gradient kernel together
constexpr size_t kContrastHead = 3;        // 8-byte words in front of g in emba_ctx::contrast.out: J (a double), dropped votes, the pose stage's status word
}

// Both entry points.  level < 0: emba_seq_contrast_gradient — the panorama's own grid, the <false> instantiations of the vote and gradient kernels, the
// votes in HBM: what it was before there were levels.  level >= 0: emba_seq_contrast_gradient_level — the level's grid (contrast_level_grid), the <true>
// instantiations, and the vote kernel contrast_vote_plan names.
static emba_status contrast_gradient_run(emba_ctx* c, size_t beg, size_t end, const double* knots_xyzw, int32_t K, int64_t t0_ns, int64_t dt_ns,
                                         int32_t signed_polarity, int level, double* j_out, double* grad_out, double* image_out, uint64_t* dropped_out,
                                         double* pm_out, double* d_out, int32_t* cp_out)
{
    if (!c) return EMBA_ERR_INVALID_ARG;
    if (!c->evseq.have) return fail(c, EMBA_ERR_STATE, "no resident sequence (emba_seq_upload first)");
    const bool leveled = level >= 0;
    if (leveled)
        switch (contrast_level_ok(c->W, c->H, level)) {
        case ContrastLevelStatus::bad_level: return fail(c, EMBA_ERR_INVALID_ARG, "level %d: levels are 0 ... %d", level, kContrastMaxLevel);
        case ContrastLevelStatus::not_divisible: return fail(c, EMBA_ERR_INVALID_ARG, "level %d: a panorama of %d x %d cells is not divisible by %d", level, c->W, c->H, 1 << level);
        case ContrastLevelStatus::too_few_rows: return fail(c, EMBA_ERR_INVALID_ARG, "level %d: %d rows of %d leave fewer than two", level, c->H, 1 << level);
        default: break;
        }
    const ContrastLevel lv = contrast_level_grid(c->W, c->H, leveled ? level : 0);
    switch (contrast_args_ok(beg, end, c->evseq.n, K, dt_ns)) {
    case PanoArgStatus::not_a_range: return fail(c, EMBA_ERR_INVALID_ARG, "[%zu, %zu) is not a range of the resident sequence of %zu events", beg, end, c->evseq.n);
    case PanoArgStatus::too_few_knots: return fail(c, EMBA_ERR_INVALID_ARG, "K = %d: a linear spline has at least two control poses", (int)K);
    case PanoArgStatus::bad_dt: return fail(c, EMBA_ERR_INVALID_ARG, "dt_ns = %lld: the knot spacing must be positive", (long long)dt_ns);
    default: break;
    }
    if (!j_out && !grad_out && !image_out && !dropped_out && !pm_out && !d_out && !cp_out) return EMBA_OK;      // nothing asked for: nothing launched
    const size_t nb = pano_batch_count(beg, end), nn = pano_events_used(beg, end), cells = (size_t)lv.W * (size_t)lv.H, ng = 3 * (size_t)K;
    if (!nn) {      // an empty or sub-batch range: no event votes
        if (j_out) *j_out = 0.0;
        if (grad_out) std::memset(grad_out, 0, ng * sizeof(double));
        if (image_out) std::memset(image_out, 0, cells * sizeof(double));
        if (dropped_out) *dropped_out = 0;
        return EMBA_OK;
    }
    if (!knots_xyzw) return fail(c, EMBA_ERR_INVALID_ARG, "knots NULL");
    if (cells > 0x7FFFFFFFull) return fail(c, EMBA_ERR_INVALID_ARG, "a panorama of %zu cells is too large for 32-bit cell indices", cells);
    const bool grad_pass = grad_out || d_out || cp_out;      // (d_out, cp_out: what the gradient pass forms — the seam the tests pin)
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t s = c->stream;
    ContrastBuffers& B = c->contrast;
    SEQ_TRY(ensure<double>(c, B.image, cells));
    SEQ_TRY(ensure<int64_t>(c, B.batch_t, nb));
    SEQ_TRY(ensure<double>(c, B.pose, nb * (size_t)kPoseStride));
    SEQ_TRY(ensure<double>(c, B.knots, 4 * (size_t)K));
    SEQ_TRY(ensure<double>(c, B.slots, kContrastReduceSlots));
    SEQ_TRY(ensure<double>(c, B.out, kContrastHead + ng));
    if (pm_out) SEQ_TRY(ensure<double>(c, B.pm, 2 * nn));
    if (d_out) SEQ_TRY(ensure<double>(c, B.D, 12 * nn));
    if (cp_out) SEQ_TRY(ensure<int32_t>(c, B.cp, nn));
    double* d_head = B.out.as<double>();
    int* d_err = reinterpret_cast<int*>(d_head + 2);
    HIP_TRY(c, hipMemcpyAsync(B.knots.p, knots_xyzw, (size_t)K * 32, hipMemcpyHostToDevice, s));
    HIP_TRY(c, hipMemsetAsync(d_head, 0, (kContrastHead + ng) * sizeof(double), s));
    HIP_TRY(c, hipMemsetAsync(B.image.p, 0, cells * sizeof(double), s));
    // pose stage: the range's own batches, as emba_seq_event_panorama forms them
    hipLaunchKernelGGL(emba_batch_mid_kernel, dim3(nblocks(nb)), dim3(256), 0, s, (const int64_t*)c->evseq.t.as<int64_t>() + beg, (long)nb, B.batch_t.as<int64_t>());
    hipLaunchKernelGGL(emba_pose_kernel, dim3(nblocks(nb, 64)), dim3(64), 0, s, (const int64_t*)B.batch_t.as<int64_t>(), (int)nb, (const double*)B.knots.as<double>(), (int)K,
                       t0_ns, dt_ns, B.pose.as<double>(), d_err);
    // votes, gradient.  (A batch outside the knots leaves its pose record unwritten and sets the status word: whatever that record holds, contrast_vote
    // keeps every add inside the image, the gradient kernel takes no control-pose index outside [0, K - 2], and the result is discarded below.)
    ContrastParams P{c->evseq.x.as<uint16_t>() + beg, c->evseq.y.as<uint16_t>() + beg, c->evseq.pol.as<uint8_t>() + beg, c->d_lut.as<double>(), B.pose.as<double>(), (long)nn,
                     c->sw, lv.W, lv.H, (int)K, lv.scale, c->fx, c->fy, c->cx, c->cy, signed_polarity != 0, B.image.as<double>(),
                     reinterpret_cast<unsigned long long*>(d_head + 1), d_head + kContrastHead, pm_out ? B.pm.as<double>() : (double*)nullptr,
                     d_out ? B.D.as<double>() : (double*)nullptr, cp_out ? B.cp.as<int32_t>() : (int32_t*)nullptr};
    if (c->kernel_timing) HIP_TRY(c, hipEventRecord(c->ev_start[kContrastTimerSlot], s));
    const ContrastVotePath path = leveled ? contrast_vote_plan(lv.W, lv.H, c->opt_contrast_vote) : ContrastVotePath::hbm;
    c->contrast_vote_path = (int)path;
    if (!leveled) {
        hipLaunchKernelGGL(emba_contrast_vote_kernel<false>, dim3(nblocks(nn, kContrastThreads)), dim3(kContrastThreads), 0, s, P);
        if (grad_pass) hipLaunchKernelGGL(emba_contrast_grad_kernel<false>, dim3(nblocks(nn, kContrastThreads)), dim3(kContrastThreads), 0, s, P);
    } else {
        if (path == ContrastVotePath::lds) hipLaunchKernelGGL(emba_contrast_vote_lds_kernel, dim3(contrast_lds_grid(c->n_cu)), dim3(kContrastLdsThreads), 0, s, P);
        else hipLaunchKernelGGL(emba_contrast_vote_kernel<true>, dim3(nblocks(nn, kContrastThreads)), dim3(kContrastThreads), 0, s, P);
        if (grad_pass) hipLaunchKernelGGL(emba_contrast_grad_kernel<true>, dim3(nblocks(nn, kContrastThreads)), dim3(kContrastThreads), 0, s, P);
    }
    if (c->kernel_timing) HIP_TRY(c, hipEventRecord(c->ev_stop[kContrastTimerSlot], s));
    // contrast
    const unsigned rblocks = std::min<unsigned>(nblocks(cells, kContrastThreads * 4), kContrastReduceBlocks);
    hipLaunchKernelGGL(emba_contrast_reduce_kernel, dim3(rblocks), dim3(kContrastThreads), 0, s, (const double*)B.image.as<double>(), (long)cells, B.slots.as<double>());
    hipLaunchKernelGGL(emba_contrast_reduce_final_kernel, dim3(1), dim3(64), 0, s, (const double*)B.slots.as<double>(), (int)(rblocks * (kContrastThreads / 64)), d_head);
    HIP_TRY(c, hipGetLastError());
    std::vector<double> h((grad_out ? ng : 0) + kContrastHead);      // J, dropped, status and g in one copy; the one synchronisation of the call
    HIP_TRY(c, hipMemcpyAsync(h.data(), d_head, h.size() * sizeof(double), hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipStreamSynchronize(s));
    uint64_t words[kContrastHead];
    std::memcpy(words, h.data(), sizeof words);
    if ((int)(words[2] & 0xFFFFFFFFull) & 1) return fail(c, EMBA_ERR_TIME_RANGE, "a batch midpoint of [%zu, %zu) lies outside the spline's knots", beg, end);
    if (j_out) *j_out = h[0];
    if (dropped_out) *dropped_out = words[1];
    if (grad_out) std::memcpy(grad_out, h.data() + kContrastHead, ng * sizeof(double));
    if (image_out) SEQ_TRY(d2h_pageable(c, image_out, B.image.p, cells * sizeof(double)));
    if (pm_out) SEQ_TRY(d2h_pageable(c, pm_out, B.pm.p, 2 * nn * sizeof(double)));
    if (d_out) SEQ_TRY(d2h_pageable(c, d_out, B.D.p, 12 * nn * sizeof(double)));
    if (cp_out) SEQ_TRY(d2h_pageable(c, cp_out, B.cp.p, nn * sizeof(int32_t)));
    return EMBA_OK;
}

extern "C" emba_status emba_seq_contrast_gradient(emba_ctx* c, size_t beg, size_t end, const double* knots_xyzw, int32_t K, int64_t t0_ns, int64_t dt_ns,
                                                  int32_t signed_polarity, double* j_out, double* grad_out, double* image_out, uint64_t* dropped_out,
                                                  double* pm_out, double* d_out, int32_t* cp_out)
{
    return contrast_gradient_run(c, beg, end, knots_xyzw, K, t0_ns, dt_ns, signed_polarity, -1, j_out, grad_out, image_out, dropped_out, pm_out, d_out, cp_out);
}

extern "C" emba_status emba_seq_contrast_gradient_level(emba_ctx* c, size_t beg, size_t end, const double* knots_xyzw, int32_t K, int64_t t0_ns, int64_t dt_ns,
                                                        int32_t signed_polarity, int32_t level, double* j_out, double* grad_out, double* image_out,
                                                        uint64_t* dropped_out, double* pm_out, double* d_out, int32_t* cp_out)
{
    if (c && level < 0) return fail(c, EMBA_ERR_INVALID_ARG, "level %d: levels are 0 ... %d", (int)level, kContrastMaxLevel);
    return contrast_gradient_run(c, beg, end, knots_xyzw, K, t0_ns, dt_ns, signed_polarity, level, j_out, grad_out, image_out, dropped_out, pm_out, d_out, cp_out);
}
