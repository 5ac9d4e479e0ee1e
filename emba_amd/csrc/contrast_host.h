// emba_amd/csrc/contrast_host.h — the smooth contrast of the panorama of warped events and its gradient with respect to the control poses, as host code
// over the kernels of contrast_kernels.h (emba_seq_contrast_gradient, emba_seq_contrast_gradient_level, and against what earlier events voted — the priors,
// emba_ctx::priors — emba_seq_contrast_gradient_prior with emba_seq_contrast_prior_add / _set / _get / _clear).  What is plain arithmetic — the argument checks, the votes of one event and their
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

// What a call starts its image from: nothing — the image is zeroed — or prior_weight times the prior of the call's level.
struct ContrastPriorUse {
    const double* image = nullptr;      // P_l [H_l, W_l] on the device, or nullptr: no prior
    double weight = 0.0;
};

// The three entry points: the level's grid (contrast_level_grid) and one set of kernels.  level < 0: emba_seq_contrast_gradient — level 0 without the level's
// argument checks and with the votes in HBM whatever the image's size, as before there were levels.  level >= 0: emba_seq_contrast_gradient_level — the
// vote kernel contrast_vote_plan names.  prior.image: emba_seq_contrast_gradient_prior — the image starts as prior.weight P_l (emba_contrast_prior_init_kernel
// in the place of the zeroing; both vote kernels add to what stands in HBM), and an empty or sub-batch range still reduces that image.
static emba_status contrast_gradient_run(emba_ctx* c, size_t beg, size_t end, const double* knots_xyzw, int32_t K, int64_t t0_ns, int64_t dt_ns,
                                         int32_t signed_polarity, int level, ContrastPriorUse prior, double* j_out, double* grad_out, double* image_out,
                                         uint64_t* dropped_out, double* pm_out, double* d_out, int32_t* cp_out)
{
    const ContrastLevel lv = contrast_level_grid(c->W, c->H, level >= 0 ? level : 0);
    SEQ_TRY(seq_range_args(c, contrast_args_ok(beg, end, c->evseq.n, K, dt_ns), beg, end, K, dt_ns));
    if (!j_out && !grad_out && !image_out && !dropped_out && !pm_out && !d_out && !cp_out) return EMBA_OK;      // nothing asked for: nothing launched
    const size_t nn = pano_events_used(beg, end), cells = (size_t)lv.W * (size_t)lv.H, ng = 3 * (size_t)K;
    if (!nn && !prior.image) {      // an empty or sub-batch range: no event votes
        if (j_out) *j_out = 0.0;
        if (grad_out) std::memset(grad_out, 0, ng * sizeof(double));
        if (image_out) std::memset(image_out, 0, cells * sizeof(double));
        if (dropped_out) *dropped_out = 0;
        return EMBA_OK;
    }
    const bool grad_pass = nn && (grad_out || d_out || cp_out);      // (d_out, cp_out: what the gradient pass forms — the seam the tests pin)
    ContrastBuffers& B = c->contrast;
    hipStream_t s = c->stream;
    if (nn) SEQ_TRY(seq_range_poses(c, beg, end, knots_xyzw, K, t0_ns, dt_ns, cells, B.out, kContrastHead + ng, 2));
    else {      // (with a prior) no batch, no pose stage: the head alone, zeroed — J of the prior's image, a zero gradient, nothing dropped, status 0
        HIP_TRY(c, hipSetDevice(c->device));
        SEQ_TRY(ensure<uint64_t>(c, B.out, kContrastHead + ng));
        HIP_TRY(c, hipMemsetAsync(B.out.p, 0, (kContrastHead + ng) * 8, s));
    }
    SEQ_TRY(ensure<double>(c, B.image, cells));
    SEQ_TRY(ensure<double>(c, B.slots, kContrastReduceSlots));
    if (pm_out) SEQ_TRY(ensure<double>(c, B.pm, 2 * nn));
    if (d_out) SEQ_TRY(ensure<double>(c, B.D, 12 * nn));
    if (cp_out) SEQ_TRY(ensure<int32_t>(c, B.cp, nn));
    double* d_head = B.out.as<double>();
    const unsigned rblocks = std::min<unsigned>(nblocks(cells, kContrastThreads * 4), kContrastReduceBlocks);
    if (prior.image) hipLaunchKernelGGL(emba_contrast_prior_init_kernel, dim3(rblocks), dim3(kContrastThreads), 0, s, prior.image, prior.weight, (long)cells, B.image.as<double>());
    else HIP_TRY(c, hipMemsetAsync(B.image.p, 0, cells * sizeof(double), s));
    if (nn) {
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
    }
    // contrast
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

// What every contrast entry point refuses before it looks at the range: no context, no sequence, a level the panorama does not admit (level < 0: none asked for).
static emba_status contrast_call_ok(emba_ctx* c, int level)
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
    return EMBA_OK;
}

extern "C" emba_status emba_seq_contrast_gradient(emba_ctx* c, size_t beg, size_t end, const double* knots_xyzw, int32_t K, int64_t t0_ns, int64_t dt_ns,
                                                  int32_t signed_polarity, double* j_out, double* grad_out, double* image_out, uint64_t* dropped_out,
                                                  double* pm_out, double* d_out, int32_t* cp_out)
{
    SEQ_TRY(contrast_call_ok(c, -1));
    return contrast_gradient_run(c, beg, end, knots_xyzw, K, t0_ns, dt_ns, signed_polarity, -1, ContrastPriorUse{}, j_out, grad_out, image_out, dropped_out, pm_out, d_out, cp_out);
}

extern "C" emba_status emba_seq_contrast_gradient_level(emba_ctx* c, size_t beg, size_t end, const double* knots_xyzw, int32_t K, int64_t t0_ns, int64_t dt_ns,
                                                        int32_t signed_polarity, int32_t level, double* j_out, double* grad_out, double* image_out,
                                                        uint64_t* dropped_out, double* pm_out, double* d_out, int32_t* cp_out)
{
    if (c && level < 0) return fail(c, EMBA_ERR_INVALID_ARG, "level %d: levels are 0 ... %d", (int)level, kContrastMaxLevel);
    SEQ_TRY(contrast_call_ok(c, level));
    return contrast_gradient_run(c, beg, end, knots_xyzw, K, t0_ns, dt_ns, signed_polarity, level, ContrastPriorUse{}, j_out, grad_out, image_out, dropped_out, pm_out, d_out, cp_out);
}

// ---- the prior: what earlier events of the resident sequence voted (the rule: contrast_rule.h, include/emba_hip.h)

extern "C" emba_status emba_seq_contrast_gradient_prior(emba_ctx* c, size_t beg, size_t end, const double* knots_xyzw, int32_t K, int64_t t0_ns, int64_t dt_ns,
                                                        int32_t signed_polarity, int32_t level, double prior_weight, double* j_out, double* grad_out,
                                                        double* image_out, uint64_t* dropped_out, double* pm_out, double* d_out, int32_t* cp_out)
{
    if (c && level < 0) return fail(c, EMBA_ERR_INVALID_ARG, "level %d: levels are 0 ... %d", (int)level, kContrastMaxLevel);
    SEQ_TRY(contrast_call_ok(c, level));
    if (!contrast_prior_weight_ok(prior_weight)) return fail(c, EMBA_ERR_INVALID_ARG, "prior_weight = %g: the weight of the prior is finite and not negative", prior_weight);
    if (!c->priors.present[level]) return fail(c, EMBA_ERR_STATE, "level %d has no prior (emba_seq_contrast_prior_add or emba_seq_contrast_prior_set first)", (int)level);
    return contrast_gradient_run(c, beg, end, knots_xyzw, K, t0_ns, dt_ns, signed_polarity, level, ContrastPriorUse{c->priors.image[level].as<double>(), prior_weight},
                                 j_out, grad_out, image_out, dropped_out, pm_out, d_out, cp_out);
}

extern "C" emba_status emba_seq_contrast_prior_add(emba_ctx* c, size_t beg, size_t end, const double* knots_xyzw, int32_t K, int64_t t0_ns, int64_t dt_ns,
                                                   int32_t signed_polarity, uint32_t level_mask, size_t* n_added, uint64_t* dropped_out)
{
    SEQ_TRY(contrast_call_ok(c, -1));
    int bad = -1;
    switch (contrast_prior_mask_ok(c->W, c->H, level_mask, &bad)) {
    case ContrastMaskStatus::empty: return fail(c, EMBA_ERR_INVALID_ARG, "level_mask 0: no level to add to");
    case ContrastMaskStatus::bad_bit: return fail(c, EMBA_ERR_INVALID_ARG, "level_mask 0x%x: levels are 0 ... %d", (unsigned)level_mask, kContrastMaxLevel);
    case ContrastMaskStatus::bad_level: return contrast_call_ok(c, bad);      // (its message)
    case ContrastMaskStatus::ok: break;
    }
    SEQ_TRY(seq_range_args(c, contrast_args_ok(beg, end, c->evseq.n, K, dt_ns), beg, end, K, dt_ns));
    int levels[kContrastLevels];
    const int nl = contrast_prior_levels(level_mask, levels);
    const size_t nn = pano_events_used(beg, end);
    ContrastPriors& R = c->priors;
    hipStream_t s = c->stream;
    constexpr size_t kStatusWord = kContrastLevels;      // out: the dropped votes of entry j of the call's levels, then the pose stage's status word
    uint64_t h[kContrastLevels + 1] = {};
    if (nn) {
        // the pose stage and its status BEFORE anything is voted: a refusal leaves every prior as it was (one synchronisation more; once per window)
        SEQ_TRY(seq_range_poses(c, beg, end, knots_xyzw, K, t0_ns, dt_ns, c->npix, R.out, kContrastLevels + 1, kStatusWord));
        HIP_TRY(c, hipGetLastError());
        HIP_TRY(c, hipMemcpyAsync(h + kStatusWord, R.out.as<uint64_t>() + kStatusWord, 8, hipMemcpyDeviceToHost, s));
        HIP_TRY(c, hipStreamSynchronize(s));
        SEQ_TRY(seq_range_status(c, h[kStatusWord], beg, end));
    } else HIP_TRY(c, hipSetDevice(c->device));
    ContrastPriorParams P{seq_event_params(c, beg, nn, signed_polarity, nullptr, nullptr), nl, {}, {}, R.out.as<unsigned long long>()};
    for (int j = 0; j < nl; ++j) {      // every buffer first: a failed allocation leaves no prior half made
        const ContrastLevel lv = contrast_level_grid(c->W, c->H, levels[j]);
        SEQ_TRY(ensure<double>(c, R.image[levels[j]], (size_t)lv.W * (size_t)lv.H));
        P.lv[j] = lv;
        P.image[j] = R.image[levels[j]].as<double>();
    }
    for (int j = 0; j < nl; ++j)
        if (!R.present[levels[j]]) {      // a prior that does not exist: zeros
            HIP_TRY(c, hipMemsetAsync(P.image[j], 0, (size_t)P.lv[j].W * (size_t)P.lv[j].H * sizeof(double), s));
            R.present[levels[j]] = true;
        }
    if (nn) {
        if (c->kernel_timing) HIP_TRY(c, hipEventRecord(c->ev_start[kSeqStageTimerSlot], s));
        hipLaunchKernelGGL(emba_contrast_prior_vote_kernel, dim3(nblocks(nn, kContrastThreads)), dim3(kContrastThreads), 0, s, P);
        if (c->kernel_timing) HIP_TRY(c, hipEventRecord(c->ev_stop[kSeqStageTimerSlot], s));
        HIP_TRY(c, hipGetLastError());
        HIP_TRY(c, hipMemcpyAsync(h, R.out.p, kContrastLevels * 8, hipMemcpyDeviceToHost, s));
    }
    HIP_TRY(c, hipStreamSynchronize(s));
    if (n_added) *n_added = nn;
    if (dropped_out) {
        std::memset(dropped_out, 0, kContrastLevels * sizeof(uint64_t));
        for (int j = 0; j < nl; ++j) dropped_out[levels[j]] = h[j];
    }
    return EMBA_OK;
}

extern "C" emba_status emba_seq_contrast_prior_set(emba_ctx* c, int32_t level, const double* image_host)
{
    if (c && level < 0) return fail(c, EMBA_ERR_INVALID_ARG, "level %d: levels are 0 ... %d", (int)level, kContrastMaxLevel);
    SEQ_TRY(contrast_call_ok(c, level));
    if (!image_host) { c->priors.present[level] = false; return EMBA_OK; }
    const ContrastLevel lv = contrast_level_grid(c->W, c->H, level);
    const size_t bytes = (size_t)lv.W * (size_t)lv.H * sizeof(double);
    HIP_TRY(c, hipSetDevice(c->device));
    SEQ_TRY(ensure<double>(c, c->priors.image[level], (size_t)lv.W * (size_t)lv.H));
    c->priors.present[level] = false;      // (a failed copy leaves none)
    HIP_TRY(c, hipMemcpyAsync(c->priors.image[level].p, image_host, bytes, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    c->priors.present[level] = true;
    return EMBA_OK;
}

extern "C" emba_status emba_seq_contrast_prior_get(emba_ctx* c, int32_t level, double* image_host, int32_t* present)
{
    if (c && level < 0) return fail(c, EMBA_ERR_INVALID_ARG, "level %d: levels are 0 ... %d", (int)level, kContrastMaxLevel);
    SEQ_TRY(contrast_call_ok(c, level));
    const bool have = c->priors.present[level];
    if (present) *present = have ? 1 : 0;
    if (!have || !image_host) return EMBA_OK;
    const ContrastLevel lv = contrast_level_grid(c->W, c->H, level);
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return d2h_pageable(c, image_host, c->priors.image[level].p, (size_t)lv.W * (size_t)lv.H * sizeof(double));
}

extern "C" emba_status emba_seq_contrast_prior_clear(emba_ctx* c)
{
    if (!c) return EMBA_ERR_INVALID_ARG;
    c->priors.drop();
    return EMBA_OK;
}
