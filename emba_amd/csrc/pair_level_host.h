// emba_amd/csrc/pair_level_host.h — the pair alignment coarse to fine over a pyramid of the sensor frames, with the pair's exposure estimated, as host code
// over the kernels of pair_level_kernels.h and the exposure stage's reduce and step kernels (emba_frames_pair_level_eval, emba_frames_pair_align_levels).  What
// is plain arithmetic is decided in pair_level_rule.h, pair_rule.h and exposure_rule.h; here are the buffers (emba_ctx::pair_level), the launches, the schedule
// over levels and the C ABI.
// Part of emba_hip.hip's translation unit, included by it below pair_host.h; it uses pair_host.h (PairCall, pair_refusals' messages through pair_args_refusal),
// frame_host.h (frame_ensure, frame_launch_reduce, frame_lm_loop: DESIGN.md §23), align_host.h (align_settings_refusal), sequence_host.h (SEQ_TRY) and
// transfer_host.h (d2h_pageable).  The sequence goes up once per call and its pyramid is made once per call; the pairs go in pair_host.h's chunks, the schedule
// runs inside a chunk, and the state stays on the device between levels.  Nothing of the registered window, of the resident sequence, of the mosaic and the
// level planes, of the resident map or of any other stage's buffers is written.
#pragma once
#include <vector>

#include "align_host.h"
#include "context.h"
#include "exposure_kernels.h"
#include "frame_host.h"
#include "pair_host.h"
#include "pair_level_kernels.h"
#include "pair_level_rule.h"

using namespace emba;

namespace {
constexpr int kPairReduceTimerSlot = 6;      // with kernel timing on: the events around the reduce kernel's launches of a call (slot 7: the first evaluation kernel)

// where a level's bytes and table lie in emba_ctx::pair_level (level 0: the sequence and the context's table themselves)
struct PairPyramid {
    unsigned mask = 0;            // bit l: level l >= 1 is made
    int top = 0;
    size_t byte_off[kPairMaxLevel + 1] = {}, lut_off[kPairMaxLevel + 1] = {}, bytes = 0, luts = 0;
};
PairPyramid pair_pyramid_plan(emba_ctx* c, size_t F, const int32_t* levels, size_t n)
{
    PairPyramid y;
    for (size_t k = 0; k < n; ++k) if (levels[k] > 0) y.mask |= 1u << levels[k];
    for (int l = 1; l <= kPairMaxLevel; ++l) {
        if (!(y.mask >> l & 1u)) continue;
        const size_t Sl = (size_t)(c->sw >> l) * (size_t)(c->sh >> l);
        y.top = l;
        y.byte_off[l] = y.bytes; y.bytes += F * Sl;
        y.lut_off[l] = y.luts; y.luts += 3 * Sl;
    }
    return y;
}
const uint8_t* pair_level_bytes_of(emba_ctx* c, const PairPyramid& y, int l)
{
    return l ? c->pair_level.bytes.as<uint8_t>() + y.byte_off[l] : c->pair_level.loop.frames.as<uint8_t>();
}
const double* pair_level_lut_of(emba_ctx* c, const PairPyramid& y, int l) { return l ? c->pair_level.lut.as<double>() + y.lut_off[l] : c->d_lut.as<double>(); }

// the refusals of the schedule, behind pair_host.h's up to huber_k
emba_status pair_levels_refusal(emba_ctx* c, const int32_t* levels, size_t n)
{
    size_t at = 0;
    switch (pair_levels_ok(levels, n, c->sw, c->sh, &at)) {
    case PairLevelArgStatus::ok: break;
    case PairLevelArgStatus::levels_null: return fail(c, EMBA_ERR_INVALID_ARG, "levels NULL or n_levels = 0: a schedule has one level at the least");
    case PairLevelArgStatus::too_many_levels: return fail(c, EMBA_ERR_INVALID_ARG, "n_levels = %zu: a schedule has %d levels at the most", n, kPairMaxLevels);
    case PairLevelArgStatus::level_out_of_range: return fail(c, EMBA_ERR_INVALID_ARG, "levels[%zu] = %d is outside 0 ... %d", at, (int)levels[at], kPairMaxLevel);
    case PairLevelArgStatus::level_too_small:
        return fail(c, EMBA_ERR_INVALID_ARG, "level %d of a %d x %d sensor is %d x %d: a bilinear cell needs 2 x 2", (int)levels[at], c->sw, c->sh, c->sw >> levels[at],
                    c->sh >> levels[at]);
    }
    return EMBA_OK;
}

// the buffers of a call whose chunks hold at most np pairs over a schedule of n levels, the whole sequence into them, and its pyramid
emba_status pair_level_begin(emba_ctx* c, const PairCall& a, const PairPyramid& y, size_t np, size_t n, bool want_uv, bool want_resid, bool loop)
{
    PairLevelBuffers& B = c->pair_level;
    hipStream_t s = c->stream;
    SEQ_TRY(ensure<uint8_t>(c, B.loop.frames, a.F * c->S));      // (all F frames, where frame_ensure asks for a chunk's)
    SEQ_TRY(frame_ensure(c, B.loop, kExposureSums, np, want_uv, want_resid, loop));
    SEQ_TRY(ensure<int32_t>(c, B.pairs, 2 * np));
    SEQ_TRY(ensure<double>(c, B.gain_trial, np));
    SEQ_TRY(ensure<double>(c, B.bias_trial, np));
    SEQ_TRY(ensure<uint8_t>(c, B.bytes, std::max<size_t>(y.bytes, 1)));
    SEQ_TRY(ensure<double>(c, B.lut, std::max<size_t>(y.luts, 1)));
    if (loop) {
        SEQ_TRY(ensure<double>(c, B.gain, np));
        SEQ_TRY(ensure<double>(c, B.bias, np));
        SEQ_TRY(ensure<int32_t>(c, B.out_of, np));
        SEQ_TRY(ensure<double>(c, B.r_q, 4 * np));
        SEQ_TRY(ensure<double>(c, B.r_gain, np));
        SEQ_TRY(ensure<double>(c, B.r_bias, np));
        SEQ_TRY(ensure<double>(c, B.r_sums, (size_t)kExposureSums * np));
        SEQ_TRY(ensure<double>(c, B.r_cost0, np));
        SEQ_TRY(ensure<unsigned long long>(c, B.r_counts, 4 * np));
        SEQ_TRY(ensure<unsigned long long>(c, B.r_n0, np));
        SEQ_TRY(ensure<int32_t>(c, B.r_status, np));
        SEQ_TRY(ensure<int32_t>(c, B.r_iters, np));
        SEQ_TRY(ensure<int32_t>(c, B.r_level_status, n * np));
        SEQ_TRY(ensure<int32_t>(c, B.r_level_iters, n * np));
    }
    HIP_TRY(c, hipMemcpyAsync(B.loop.frames.p, a.frames, a.F * c->S, hipMemcpyHostToDevice, s));
    if (!y.mask) return EMBA_OK;
    // the bytes of every level of the mask: one pass over the sequence, in launches of at most 2^20 workgroups
    PairReduceParams R{};
    R.frames = B.loop.frames.as<uint8_t>();
    for (int l = 1; l <= y.top; ++l) R.out[l] = y.mask >> l & 1u ? B.bytes.as<uint8_t>() + y.byte_off[l] : nullptr;
    R.sw = c->sw; R.sh = c->sh;
    R.tiles_x = (c->sw + kPairTile - 1) / kPairTile;
    R.tiles = R.tiles_x * ((c->sh + kPairTile - 1) / kPairTile);
    R.top = y.top; R.mask = y.mask; R.skip_zero = a.skip_zero != 0;
    const size_t per = std::max<size_t>(((size_t)1 << 20) / (size_t)R.tiles, 1);
    if (c->kernel_timing) HIP_TRY(c, hipEventRecord(c->ev_start[kPairReduceTimerSlot], s));
    for (size_t f0 = 0; f0 < a.F; f0 += per) {
        R.f0 = (long)f0; R.nf = (long)std::min(per, a.F - f0);
        hipLaunchKernelGGL(emba_frames_pair_reduce_kernel, dim3((unsigned)((size_t)R.nf * (size_t)R.tiles)), dim3(kFrameThreads), 0, s, R);
        HIP_TRY(c, hipGetLastError());
    }
    if (c->kernel_timing) HIP_TRY(c, hipEventRecord(c->ev_stop[kPairReduceTimerSlot], s));
    // ... and their tables
    for (int l = 1; l <= y.top; ++l) {
        if (!(y.mask >> l & 1u)) continue;
        const int wl = c->sw >> l, Sl = wl * (c->sh >> l);
        hipLaunchKernelGGL(emba_pair_level_lut_kernel, dim3(nblocks((size_t)Sl, kFrameThreads)), dim3(kFrameThreads), 0, s, (const double*)c->d_lut.as<double>(), c->sw, l, wl,
                           Sl, B.lut.as<double>() + y.lut_off[l]);
        HIP_TRY(c, hipGetLastError());
    }
    return EMBA_OK;
}

// a chunk's pairs, rotations and exposures (ones and zeros where the caller gives none) to where every pair is evaluated
emba_status pair_level_upload_chunk(emba_ctx* c, const PairCall& a, const ViewChunk& ch, const std::vector<double>& ones, const std::vector<double>& zeros)
{
    PairLevelBuffers& B = c->pair_level;
    hipStream_t s = c->stream;
    HIP_TRY(c, hipMemcpyAsync(B.pairs.p, a.pairs + 2 * ch.f0, 2 * ch.nf * sizeof(int32_t), hipMemcpyHostToDevice, s));
    HIP_TRY(c, hipMemcpyAsync(B.loop.q_trial.p, a.Q + 4 * ch.f0, 4 * ch.nf * sizeof(double), hipMemcpyHostToDevice, s));
    HIP_TRY(c, hipMemcpyAsync(B.gain_trial.p, a.gain ? a.gain + ch.f0 : ones.data(), ch.nf * sizeof(double), hipMemcpyHostToDevice, s));
    HIP_TRY(c, hipMemcpyAsync(B.bias_trial.p, a.bias ? a.bias + ch.f0 : zeros.data(), ch.nf * sizeof(double), hipMemcpyHostToDevice, s));
    return EMBA_OK;
}

// one evaluation of the chunk's np pairs at level l, at the trial arrays, into B.loop.esums / ecounts; `timed`: timer slot 7 around the evaluation kernel
emba_status pair_level_launch_eval(emba_ctx* c, const PairCall& a, const PairPyramid& y, int l, size_t np, const int32_t* status, bool want_uv, bool want_resid, bool timed)
{
    PairLevelBuffers& B = c->pair_level;
    FrameLoopBuffers& L = B.loop;
    hipStream_t s = c->stream;
    const int wl = c->sw >> l, hl = c->sh >> l, Sl = wl * hl;
    const PairLevelEvalParams P{pair_level_lut_of(c, y, l), pair_level_bytes_of(c, y, l), B.pairs.as<int32_t>(), L.q_trial.as<double>(), B.gain_trial.as<double>(),
                                B.bias_trial.as<double>(), status, Sl, wl, hl, pair_level_camera(pair_camera(a.fu, a.fv, a.cu, a.cv, a.D), l), a.huber_k, a.skip_zero != 0,
                                L.partial.as<double>(), want_uv ? L.pm.as<double>() : nullptr, want_resid ? L.resid.as<double>() : nullptr};
    const unsigned nb = nblocks((size_t)Sl, kFrameThreads);      // (at most the nblocks(S) that frame_ensure sized partial for)
    if (timed) HIP_TRY(c, hipEventRecord(c->ev_start[kSeqStageTimerSlot], s));
    hipLaunchKernelGGL(emba_frames_pair_exposure_eval_kernel, dim3(nb, (unsigned)np), dim3(kFrameThreads), 0, s, P);
    if (timed) HIP_TRY(c, hipEventRecord(c->ev_stop[kSeqStageTimerSlot], s));
    HIP_TRY(c, hipGetLastError());
    hipLaunchKernelGGL(emba_frames_exposure_reduce_kernel, dim3(nblocks(np * (size_t)(kExposureSums + 4), kFrameThreads)), dim3(kFrameThreads), 0, s,
                       (const double*)L.partial.as<double>(), (int)nb, (long)np, status, L.esums.as<double>(), L.ecounts.as<unsigned long long>());
    HIP_TRY(c, hipGetLastError());
    return EMBA_OK;
}
}  // namespace

extern "C" emba_status emba_frames_pair_level_eval(emba_ctx* c, const uint8_t* frames, size_t F, const int32_t* pairs, size_t P, const double* Q_xyzw, const double* gain,
                                                   const double* bias, double fu, double fv, double cu, double cv, const double* D, int32_t skip_zero, double huber_k,
                                                   int32_t level, double* sums_out, uint64_t* counts_out, double* uv_out, double* resid_out, uint8_t* level_bytes_out,
                                                   double* level_lut_out)
{
    if (!c) return EMBA_ERR_INVALID_ARG;
    const PairCall a{frames, F, pairs, P, Q_xyzw, gain, bias, fu, fv, cu, cv, D, skip_zero, huber_k};
    SEQ_TRY(pair_args_refusal(c, a));
    SEQ_TRY(pair_levels_refusal(c, &level, 1));
    if (!pair_bytes_ok(a.F, c->S)) return fail(c, EMBA_ERR_INVALID_ARG, "F = %zu frames of %zu bytes: the resident sequence is bounded at %zu bytes", a.F, c->S, kPairMaxBytes);
    if (!P) return EMBA_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    FrameLoopBuffers& L = c->pair_level.loop;
    const size_t S = c->S, Sl = (size_t)(c->sw >> level) * (size_t)(c->sh >> level), per = pair_chunk_pairs(S), chunks = view_chunk_count(P, per);
    const PairPyramid y = pair_pyramid_plan(c, F, &level, 1);
    const std::vector<double> ones(gain ? 0 : std::min(per, P), 1.0), zeros(bias ? 0 : std::min(per, P), 0.0);
    SEQ_TRY(pair_level_begin(c, a, y, std::min(per, P), 1, uv_out != nullptr, resid_out != nullptr, false));
    for (size_t i = 0; i < chunks; ++i) {
        const ViewChunk ch = view_chunk(P, per, i);
        const size_t cells = ch.nf * Sl, off = ch.f0 * Sl;
        SEQ_TRY(pair_level_upload_chunk(c, a, ch, ones, zeros));
        SEQ_TRY(pair_level_launch_eval(c, a, y, level, ch.nf, nullptr, uv_out != nullptr, resid_out != nullptr, c->kernel_timing && i == 0));
        HIP_TRY(c, hipStreamSynchronize(c->stream));      // (the chunk's pairs have been read: the next chunk overwrites them)
        if (sums_out) SEQ_TRY(d2h_pageable(c, sums_out + (size_t)kExposureSums * ch.f0, L.esums.p, (size_t)kExposureSums * ch.nf * sizeof(double)));
        if (counts_out) SEQ_TRY(d2h_pageable(c, counts_out + 4 * ch.f0, L.ecounts.p, 4 * ch.nf * sizeof(uint64_t)));
        if (uv_out) SEQ_TRY(d2h_pageable(c, uv_out + 2 * off, L.pm.p, 2 * cells * sizeof(double)));
        if (resid_out) SEQ_TRY(d2h_pageable(c, resid_out + off, L.resid.p, cells * sizeof(double)));
    }
    if (level_bytes_out) SEQ_TRY(d2h_pageable(c, level_bytes_out, pair_level_bytes_of(c, y, level), F * Sl));
    if (level_lut_out) SEQ_TRY(d2h_pageable(c, level_lut_out, pair_level_lut_of(c, y, level), 3 * Sl * sizeof(double)));
    return EMBA_OK;
}

extern "C" emba_status emba_frames_pair_align_levels(emba_ctx* c, const uint8_t* frames, size_t F, const int32_t* pairs, size_t P, const double* Q_xyzw, const double* gain,
                                                     const double* bias, double fu, double fv, double cu, double cv, const double* D, int32_t skip_zero,
                                                     const int32_t* levels, size_t n_levels, int32_t estimate, const emba_exposure_settings* xs, double* q_out,
                                                     double* gain_out, double* bias_out, double* sums_out, uint64_t* counts_out, int32_t* status_out, int32_t* iters_out,
                                                     int32_t* level_status_out, int32_t* level_iters_out, double* cost0_out, uint64_t* n0_out, double* info_out)
{
    if (!c) return EMBA_ERR_INVALID_ARG;
    const PairCall a{frames, F, pairs, P, Q_xyzw, gain, bias, fu, fv, cu, cv, D, skip_zero, xs ? xs->align.huber_k : 0.0};
    SEQ_TRY(pair_args_refusal(c, a));
    SEQ_TRY(pair_levels_refusal(c, levels, n_levels));
    if (!exposure_estimate_ok(estimate)) return fail(c, EMBA_ERR_INVALID_ARG, "estimate = %d: a mask of gain (1) and bias (2)", (int)estimate);
    if (xs && !exposure_bounds_ok(xs->gain_min, xs->gain_max))
        return fail(c, EMBA_ERR_INVALID_ARG, "gain_min = %g, gain_max = %g: finite, 0 < gain_min <= 1 <= gain_max", xs->gain_min, xs->gain_max);
    SEQ_TRY(align_settings_refusal(c, xs ? &xs->align : nullptr));
    if (!pair_bytes_ok(a.F, c->S)) return fail(c, EMBA_ERR_INVALID_ARG, "F = %zu frames of %zu bytes: the resident sequence is bounded at %zu bytes", a.F, c->S, kPairMaxBytes);
    if (!P) return EMBA_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    PairLevelBuffers& B = c->pair_level;
    FrameLoopBuffers& L = B.loop;
    hipStream_t s = c->stream;
    const size_t n = n_levels, per = pair_chunk_pairs(c->S), chunks = view_chunk_count(P, per);
    const PairPyramid y = pair_pyramid_plan(c, F, levels, n);
    const std::vector<double> ones(gain ? 0 : std::min(per, P), 1.0), zeros(bias ? 0 : std::min(per, P), 0.0);
    SEQ_TRY(pair_level_begin(c, a, y, std::min(per, P), n, false, false, true));
    std::vector<double> hs;
    std::vector<uint64_t> hc;
    for (size_t i = 0; i < chunks; ++i) {
        const ViewChunk ch = view_chunk(P, per, i);
        const size_t np = ch.nf, f0 = ch.f0;
        SEQ_TRY(pair_level_upload_chunk(c, a, ch, ones, zeros));
        HIP_TRY(c, hipMemsetAsync(B.out_of.p, 0, np * sizeof(int32_t), s));
        HIP_TRY(c, hipMemsetAsync(B.r_level_status.p, 0, n * np * sizeof(int32_t), s));
        HIP_TRY(c, hipMemsetAsync(B.r_level_iters.p, 0, n * np * sizeof(int32_t), s));
        for (size_t k = 0; k < n; ++k) {
            const int l = levels[k];
            ExposureStepParams SP{(long)np, 1, (int)estimate, pair_level_settings(*xs, l), L.q.as<double>(), L.q_trial.as<double>(), B.gain.as<double>(), B.bias.as<double>(),
                                  B.gain_trial.as<double>(), B.bias_trial.as<double>(), L.sums.as<double>(), L.lambda.as<double>(), L.dnorm.as<double>(),
                                  L.counts.as<unsigned long long>(), L.status.as<int32_t>(), L.iters.as<int32_t>(), L.have_trial.as<int32_t>(), L.esums.as<double>(),
                                  L.ecounts.as<unsigned long long>(), L.cost0.as<double>(), L.n0.as<unsigned long long>(), L.running.as<unsigned int>()};
            SEQ_TRY(frame_lm_loop(
                c, L,
                [&](const int32_t* status, bool first) {      // (a level's first evaluation leaves out the pairs that have left the schedule; out_of is 0 = RUNNING for the rest)
                    return pair_level_launch_eval(c, a, y, l, np, first ? (const int32_t*)B.out_of.as<int32_t>() : status, false, false,
                                                  c->kernel_timing && i == 0 && k == 0 && first);
                },
                [&](bool first) {
                    SP.first = first;
                    hipLaunchKernelGGL(emba_frames_exposure_step_kernel, dim3(nblocks(np, 64)), dim3(64), 0, s, SP);
                }));
            const PairHandoverParams H{(long)np, (int)k, (int)n, L.q.as<double>(), B.gain.as<double>(), B.bias.as<double>(), L.sums.as<double>(), L.cost0.as<double>(),
                                       L.counts.as<unsigned long long>(), L.n0.as<unsigned long long>(), L.status.as<int32_t>(), L.iters.as<int32_t>(),
                                       L.q_trial.as<double>(), B.gain_trial.as<double>(), B.bias_trial.as<double>(), B.out_of.as<int32_t>(), L.esums.as<double>(), L.ecounts.as<unsigned long long>(), B.r_q.as<double>(),
                                       B.r_gain.as<double>(), B.r_bias.as<double>(), B.r_sums.as<double>(), B.r_cost0.as<double>(), B.r_counts.as<unsigned long long>(),
                                       B.r_n0.as<unsigned long long>(), B.r_status.as<int32_t>(), B.r_iters.as<int32_t>(), B.r_level_status.as<int32_t>(),
                                       B.r_level_iters.as<int32_t>()};
            hipLaunchKernelGGL(emba_pair_level_handover_kernel, dim3(nblocks(np, 64)), dim3(64), 0, s, H);
            HIP_TRY(c, hipGetLastError());
        }
        HIP_TRY(c, hipStreamSynchronize(s));
        if (q_out) SEQ_TRY(d2h_pageable(c, q_out + 4 * f0, B.r_q.p, 4 * np * sizeof(double)));
        if (gain_out) SEQ_TRY(d2h_pageable(c, gain_out + f0, B.r_gain.p, np * sizeof(double)));
        if (bias_out) SEQ_TRY(d2h_pageable(c, bias_out + f0, B.r_bias.p, np * sizeof(double)));
        if (sums_out) SEQ_TRY(d2h_pageable(c, sums_out + (size_t)kExposureSums * f0, B.r_sums.p, (size_t)kExposureSums * np * sizeof(double)));
        if (counts_out) SEQ_TRY(d2h_pageable(c, counts_out + 4 * f0, B.r_counts.p, 4 * np * sizeof(uint64_t)));
        if (status_out) SEQ_TRY(d2h_pageable(c, status_out + f0, B.r_status.p, np * sizeof(int32_t)));
        if (iters_out) SEQ_TRY(d2h_pageable(c, iters_out + f0, B.r_iters.p, np * sizeof(int32_t)));
        if (level_status_out) SEQ_TRY(d2h_pageable(c, level_status_out + n * f0, B.r_level_status.p, n * np * sizeof(int32_t)));
        if (level_iters_out) SEQ_TRY(d2h_pageable(c, level_iters_out + n * f0, B.r_level_iters.p, n * np * sizeof(int32_t)));
        if (cost0_out) SEQ_TRY(d2h_pageable(c, cost0_out + f0, B.r_cost0.p, np * sizeof(double)));
        if (n0_out) SEQ_TRY(d2h_pageable(c, n0_out + f0, B.r_n0.p, np * sizeof(uint64_t)));
        if (info_out) {      // (from the ten shared sums of the last level run and its count, on the host: six divisions per pair)
            hs.resize((size_t)kExposureSums * np);
            hc.resize(4 * np);
            SEQ_TRY(d2h_pageable(c, hs.data(), B.r_sums.p, hs.size() * sizeof(double)));
            SEQ_TRY(d2h_pageable(c, hc.data(), B.r_counts.p, hc.size() * sizeof(uint64_t)));
            for (size_t p = 0; p < np; ++p) {
                double ten[kAlignSums];
                exposure_shared_sums(&hs[(size_t)kExposureSums * p], ten);
                pair_information(ten, hc[4 * p], info_out + 6 * (f0 + p));
            }
        }
    }
    return EMBA_OK;
}
