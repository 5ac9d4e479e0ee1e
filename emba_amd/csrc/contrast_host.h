// emba_amd/csrc/contrast_host.h — the smooth contrast of the panorama of warped events and its gradient with respect to the control poses, as host code
// over the kernels of contrast_kernels.h (emba_seq_contrast_gradient, emba_seq_contrast_gradient_level).  What is plain arithmetic — the argument checks, the votes of one event and their
// derivatives, the gradient of one event, the span plan, the grid of a level and the vote kernel it takes — is decided in contrast_rule.h; here are the buffers (emba_ctx::contrast), the launches and the
// C ABI.
// Part of emba_hip.hip's translation unit, included by it below panorama_host.h (the pose stage of a range: seq_range_args, seq_range_poses,
// seq_range_status; SEQ_TRY, d2h_pageable, the sequence itself: emba_ctx::evseq).  Nothing of the registered window or of the integer panorama is read or
// written.
#pragma once
#include <vector>

#include "context.h"
#include "contrast_kernels.h"
#include "contrast_rule.h"

using namespace emba;

namespace {
constexpr size_t kContrastHead = 3;        // 8-byte words in front of g in emba_ctx::contrast.out: J (a double), dropped votes, the pose stage's status word
}

// Both entry points: the level's grid (contrast_level_grid) and one set of kernels.  level < 0: emba_seq_contrast_gradient — level 0 without the level's
// argument checks and with the votes in HBM whatever the image's size, as before there were levels.  level >= 0: emba_seq_contrast_gradient_level — the
// vote kernel contrast_vote_plan names.
static emba_status contrast_gradient_run(emba_ctx* c, size_t beg, size_t end, const double* knots_xyzw, int32_t K, int64_t t0_ns, int64_t dt_ns,
                                         int32_t signed_polarity, int level, double* j_out, double* grad_out, double* image_out, uint64_t* dropped_out,
                                         double* pm_out, double* d_out, int32_t* cp_out)
{
    if (!c) return EMBA_ERR_INVALID_ARG;
    if (!c->evseq.have) return fail(c, EMBA_ERR_STATE, "no resident sequence (emba_seq_upload first)");
    if (level >= 0)
        switch (contrast_level_ok(c->W, c->H, level)) {
        case ContrastLevelStatus::bad_level: return fail(c, EMBA_ERR_INVALID_ARG, "level %d: levels are 0 ... %d", level, kContrastMaxLevel);
        case ContrastLevelStatus::not_divisible: return fail(c, EMBA_ERR_INVALID_ARG, "level %d: a panorama of %d x %d cells is not divisible by %d", level, c->W, c->H, 1 << level);
        case ContrastLevelStatus::too_few_rows: return fail(c, EMBA_ERR_INVALID_ARG, "level %d: %d rows of %d leave fewer than two", level, c->H, 1 << level);
        default: break;
        }
    const ContrastLevel lv = contrast_level_grid(c->W, c->H, level >= 0 ? level : 0);
    SEQ_TRY(seq_range_args(c, contrast_args_ok(beg, end, c->evseq.n, K, dt_ns), beg, end, K, dt_ns));
    if (!j_out && !grad_out && !image_out && !dropped_out && !pm_out && !d_out && !cp_out) return EMBA_OK;      // nothing asked for: nothing launched
    const size_t nn = pano_events_used(beg, end), cells = (size_t)lv.W * (size_t)lv.H, ng = 3 * (size_t)K;
    if (!nn) {      // an empty or sub-batch range: no event votes
        if (j_out) *j_out = 0.0;
        if (grad_out) std::memset(grad_out, 0, ng * sizeof(double));
        if (image_out) std::memset(image_out, 0, cells * sizeof(double));
        if (dropped_out) *dropped_out = 0;
        return EMBA_OK;
    }
    const bool grad_pass = grad_out || d_out || cp_out;      // (d_out, cp_out: what the gradient pass forms — the seam the tests pin)
    ContrastBuffers& B = c->contrast;
    SEQ_TRY(seq_range_poses(c, beg, end, knots_xyzw, K, t0_ns, dt_ns, cells, B.out, kContrastHead + ng, 2));
    hipStream_t s = c->stream;
    SEQ_TRY(ensure<double>(c, B.image, cells));
    SEQ_TRY(ensure<double>(c, B.slots, kContrastReduceSlots));
    if (pm_out) SEQ_TRY(ensure<double>(c, B.pm, 2 * nn));
    if (d_out) SEQ_TRY(ensure<double>(c, B.D, 12 * nn));
    if (cp_out) SEQ_TRY(ensure<int32_t>(c, B.cp, nn));
    double* d_head = B.out.as<double>();
    HIP_TRY(c, hipMemsetAsync(B.image.p, 0, cells * sizeof(double), s));
    // votes, gradient.  (A batch outside the knots: the gradient kernel takes no control-pose index outside [0, K - 2], and the result is discarded below.)
    ContrastParams P{seq_event_params(c, beg, nn, signed_polarity, reinterpret_cast<unsigned long long*>(d_head + 1), pm_out ? B.pm.as<double>() : (double*)nullptr),
                     lv.W, lv.H, (int)K, lv.scale, B.image.as<double>(), d_head + kContrastHead, d_out ? B.D.as<double>() : (double*)nullptr,
                     cp_out ? B.cp.as<int32_t>() : (int32_t*)nullptr};
    if (c->kernel_timing) HIP_TRY(c, hipEventRecord(c->ev_start[kSeqStageTimerSlot], s));
    const ContrastVotePath path = level >= 0 ? contrast_vote_plan(lv.W, lv.H, c->opt_contrast_vote) : ContrastVotePath::hbm;      // (the level-free entry point: HBM whatever the size)
    c->contrast_vote_path = (int)path;
    if (path == ContrastVotePath::lds) hipLaunchKernelGGL(emba_contrast_vote_lds_kernel, dim3(contrast_lds_grid(c->n_cu)), dim3(kContrastLdsThreads), 0, s, P);
    else hipLaunchKernelGGL(emba_contrast_vote_kernel, dim3(nblocks(nn, kContrastThreads)), dim3(kContrastThreads), 0, s, P);
    if (grad_pass) hipLaunchKernelGGL(emba_contrast_grad_kernel, dim3(nblocks(nn, kContrastThreads)), dim3(kContrastThreads), 0, s, P);
    if (c->kernel_timing) HIP_TRY(c, hipEventRecord(c->ev_stop[kSeqStageTimerSlot], s));
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
    SEQ_TRY(seq_range_status(c, words[2], beg, end));
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
