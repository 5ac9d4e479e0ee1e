// emba_amd/csrc/match_host.h — loop-closure pairs found by appearance, as host code over the kernels of match_kernels.h and the pyramid kernel of
// pair_level_kernels.h (emba_frames_match_eval, emba_frames_match_search, emba_match_start).  What is plain arithmetic is decided in match_rule.h; here are
// the buffers (emba_ctx::match), the launches and the C ABI.
// Part of emba_hip.hip's translation unit, included by it below pair_level_host.h; it uses sequence_host.h (SEQ_TRY), panorama_host.h (kSeqStageTimerSlot)
// and transfer_host.h (d2h_pageable).  The sequence goes up once per call and its thumbnails are made once per call (level 0: the frames themselves); the
// pairs go in match_rule.h's chunks.  Nothing of the registered window, of the resident sequence, of the mosaic and the level planes, of the resident map or
// of any other stage's buffers — the pair stages' among them — is written.
#pragma once
#include <vector>

#include "context.h"
#include "match_kernels.h"
#include "match_rule.h"
#include "pair_level_kernels.h"

using namespace emba;

namespace {
constexpr int kMatchSelectTimerSlot = 6;      // with kernel timing on: the events around the select kernel (slot 7: the evaluation kernel of the first chunk)

emba_status match_refusal(emba_ctx* c, const MatchCall& a)
{
    size_t at = 0;
    const int w = a.level >= 0 && a.level <= kPairMaxLevel ? c->sw >> a.level : 0, h = a.level >= 0 && a.level <= kPairMaxLevel ? c->sh >> a.level : 0;
    switch (match_args_ok(a, c->sw, c->sh, sizeof(MatchBest), &at)) {
    case MatchArgStatus::ok: break;
    case MatchArgStatus::frames_null: return fail(c, EMBA_ERR_INVALID_ARG, "frames NULL");
    case MatchArgStatus::bad_frames: return fail(c, EMBA_ERR_INVALID_ARG, "F = %zu: at least one frame, and frames are counted in 31 bits", a.F);
    case MatchArgStatus::pairs_null: return fail(c, EMBA_ERR_INVALID_ARG, "pairs NULL");
    case MatchArgStatus::too_many_pairs: return fail(c, EMBA_ERR_INVALID_ARG, "P = %zu: pairs are counted in 31 bits", a.P);
    case MatchArgStatus::pair_out_of_range:
        return fail(c, EMBA_ERR_INVALID_ARG, "pairs[%zu] = (%d, %d) names a frame outside [0, %zu)", at, (int)a.pairs[2 * at], (int)a.pairs[2 * at + 1], a.F);
    case MatchArgStatus::level_out_of_range: return fail(c, EMBA_ERR_INVALID_ARG, "level = %d is outside 0 ... %d", (int)a.level, kPairMaxLevel);
    case MatchArgStatus::level_too_small:
        return fail(c, EMBA_ERR_INVALID_ARG, "level %d of a %d x %d sensor is %d x %d: a bilinear cell needs 2 x 2", (int)a.level, c->sw, c->sh, w, h);
    case MatchArgStatus::too_many_pixels: {
        const int l = match_smallest_level(c->sw, c->sh);
        if (l <= kPairMaxLevel && pair_level_size_ok(c->sw, c->sh, l))
            return fail(c, EMBA_ERR_INVALID_ARG, "level %d of a %d x %d sensor has %d x %d pixels: a thumbnail has %zu at the most; the smallest level that fits is %d", (int)a.level,
                        c->sw, c->sh, w, h, kMatchMaxPixels, l);
        return fail(c, EMBA_ERR_INVALID_ARG, "level %d of a %d x %d sensor has %d x %d pixels: a thumbnail has %zu at the most, and no level of this sensor fits", (int)a.level,
                    c->sw, c->sh, w, h, kMatchMaxPixels);
    }
    case MatchArgStatus::bad_range:
        return fail(c, EMBA_ERR_INVALID_ARG, "rx = %d, ry = %d: 0 <= rx < %d and 0 <= ry < %d at level %d", (int)a.rx, (int)a.ry, w, h, (int)a.level);
    case MatchArgStatus::n_min_zero: return fail(c, EMBA_ERR_INVALID_ARG, "n_min = 0: a scored shift has one pixel at the least");
    case MatchArgStatus::bad_k: return fail(c, EMBA_ERR_INVALID_ARG, "k = %d is outside 1 ... %d", (int)a.k, kMatchMaxPerFrame);
    case MatchArgStatus::bad_gap: return fail(c, EMBA_ERR_INVALID_ARG, "min_gap = %d is negative", (int)a.min_gap);
    case MatchArgStatus::bad_score_min: return fail(c, EMBA_ERR_INVALID_ARG, "score_min is not a number");
    case MatchArgStatus::bytes:
        return fail(c, EMBA_ERR_INVALID_ARG, "F = %zu frames of %zu bytes: the resident sequence is bounded at %zu bytes", a.F, c->S, kPairMaxBytes);
    case MatchArgStatus::table:
        return fail(c, EMBA_ERR_INVALID_ARG, "F = %zu frames have %llu pairs of %zu bytes: the table of a search is bounded at %zu bytes", a.F,
                    (unsigned long long)match_table_pairs(a.F), sizeof(MatchBest), kMatchMaxTableBytes);
    }
    return EMBA_OK;
}

// the whole sequence into the stage's buffer and its thumbnails of `level` behind it; *thumbs: where they lie
emba_status match_begin(emba_ctx* c, const uint8_t* frames, size_t F, int level, bool skip_zero, const uint8_t** thumbs)
{
    MatchBuffers& B = c->match;
    hipStream_t s = c->stream;
    SEQ_TRY(ensure<uint8_t>(c, B.frames, F * c->S));
    HIP_TRY(c, hipMemcpyAsync(B.frames.p, frames, F * c->S, hipMemcpyHostToDevice, s));
    *thumbs = B.frames.as<uint8_t>();
    if (!level) return EMBA_OK;
    const size_t Sl = (size_t)(c->sw >> level) * (size_t)(c->sh >> level);
    SEQ_TRY(ensure<uint8_t>(c, B.bytes, F * Sl));
    PairReduceParams R{};
    R.frames = B.frames.as<uint8_t>();
    R.out[level] = B.bytes.as<uint8_t>();
    R.sw = c->sw; R.sh = c->sh;
    R.tiles_x = (c->sw + kPairTile - 1) / kPairTile;
    R.tiles = R.tiles_x * ((c->sh + kPairTile - 1) / kPairTile);
    R.top = level; R.mask = 1u << level; R.skip_zero = skip_zero;
    const size_t per = std::max<size_t>(((size_t)1 << 20) / (size_t)R.tiles, 1);
    for (size_t f0 = 0; f0 < F; f0 += per) {
        R.f0 = (long)f0; R.nf = (long)std::min(per, F - f0);
        hipLaunchKernelGGL(emba_frames_pair_reduce_kernel, dim3((unsigned)((size_t)R.nf * (size_t)R.tiles)), dim3(kFrameThreads), 0, s, R);
        HIP_TRY(c, hipGetLastError());
    }
    *thumbs = B.bytes.as<uint8_t>();
    return EMBA_OK;
}

MatchEvalParams match_eval_params(emba_ctx* c, const MatchCall& a, const uint8_t* thumbs, bool skip_zero)
{
    MatchEvalParams E{};
    E.thumbs = thumbs;
    E.F = a.F;
    E.w = c->sw >> a.level; E.h = c->sh >> a.level; E.S = E.w * E.h;
    E.rx = a.rx; E.ry = a.ry; E.shifts = match_shift_count(a.rx, a.ry);
    for (int g = match_lanes_per_shift(E.shifts, kFrameThreads); g > 1; g >>= 1) ++E.g_log2;
    E.skip_zero = skip_zero; E.n_min = a.n_min;
    return E;
}

emba_status match_launch_eval(emba_ctx* c, const MatchEvalParams& E, size_t np, bool timed)
{
    hipStream_t s = c->stream;
    if (timed) HIP_TRY(c, hipEventRecord(c->ev_start[kSeqStageTimerSlot], s));
    hipLaunchKernelGGL(emba_frames_match_eval_kernel, dim3((unsigned)np), dim3(kFrameThreads), 0, s, E);
    if (timed) HIP_TRY(c, hipEventRecord(c->ev_stop[kSeqStageTimerSlot], s));
    HIP_TRY(c, hipGetLastError());
    return EMBA_OK;
}
}  // namespace

extern "C" emba_status emba_frames_match_eval(emba_ctx* c, const uint8_t* frames, size_t F, const int32_t* pairs, size_t P, int32_t level, int32_t rx, int32_t ry,
                                              int32_t skip_zero, uint32_t n_min, double* score_out, int32_t* shift_out, uint64_t* n_out, uint64_t* sums_out)
{
    if (!c) return EMBA_ERR_INVALID_ARG;
    const MatchCall a{frames != nullptr, F, pairs, P, level, rx, ry, n_min, false, 1, 0, 0.0};
    SEQ_TRY(match_refusal(c, a));
    if (!P) return EMBA_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    MatchBuffers& B = c->match;
    hipStream_t s = c->stream;
    const uint8_t* thumbs = nullptr;
    SEQ_TRY(match_begin(c, frames, F, level, skip_zero != 0, &thumbs));
    MatchEvalParams E = match_eval_params(c, a, thumbs, skip_zero != 0);
    const size_t per = std::min(match_chunk_pairs(E.shifts, sums_out != nullptr), P), chunks = match_chunk_count(P, per), per_sums = (size_t)E.shifts * kMatchSums;
    SEQ_TRY(ensure<int32_t>(c, B.pairs, 2 * per));
    SEQ_TRY(ensure<MatchBest>(c, B.records, per));
    if (sums_out) SEQ_TRY(ensure<unsigned long long>(c, B.sums, per * per_sums));
    std::vector<MatchBest> rec(per);
    for (size_t i = 0; i < chunks; ++i) {
        const size_t p0 = i * per, np = std::min(per, P - p0);
        HIP_TRY(c, hipMemcpyAsync(B.pairs.p, pairs + 2 * p0, 2 * np * sizeof(int32_t), hipMemcpyHostToDevice, s));
        E.pairs = B.pairs.as<int32_t>();
        E.out = B.records.as<MatchBest>();
        E.sums = sums_out ? B.sums.as<unsigned long long>() : nullptr;
        SEQ_TRY(match_launch_eval(c, E, np, c->kernel_timing && i == 0));
        HIP_TRY(c, hipStreamSynchronize(s));      // (the chunk's pairs have been read: the next chunk overwrites them)
        SEQ_TRY(d2h_pageable(c, rec.data(), B.records.p, np * sizeof(MatchBest)));
        for (size_t p = 0; p < np; ++p) {
            if (score_out) score_out[p0 + p] = rec[p].score;
            if (shift_out) { shift_out[2 * (p0 + p)] = rec[p].dx; shift_out[2 * (p0 + p) + 1] = rec[p].dy; }
            if (n_out) n_out[p0 + p] = rec[p].n;
        }
        if (sums_out) SEQ_TRY(d2h_pageable(c, sums_out + p0 * per_sums, B.sums.p, np * per_sums * sizeof(uint64_t)));
    }
    return EMBA_OK;
}

extern "C" emba_status emba_frames_match_search(emba_ctx* c, const uint8_t* frames, size_t F, const int32_t* status, int32_t level, int32_t rx, int32_t ry,
                                                int32_t min_gap, int32_t skip_zero, uint32_t n_min, double score_min, int32_t k, int32_t* partner_out,
                                                double* score_out, int32_t* shift_out, uint64_t* n_out)
{
    if (!c) return EMBA_ERR_INVALID_ARG;
    const MatchCall a{frames != nullptr, F, nullptr, 0, level, rx, ry, n_min, true, k, min_gap, score_min};
    SEQ_TRY(match_refusal(c, a));
    const size_t K = (size_t)k;
    // the frames that vote, and whether any pair of them is a candidate: the first and the last voting frame are the farthest apart
    std::vector<uint8_t> votes(F);
    size_t first = F, last = 0;
    for (size_t f = 0; f < F; ++f) {
        votes[f] = match_votes(status, f) ? 1 : 0;
        if (votes[f]) { if (first == F) first = f; last = f; }
    }
    if (first == F || (int64_t)(last - first) <= (int64_t)min_gap) {      // no candidate pair: nothing is launched
        for (size_t o = 0; o < F * K; ++o) {
            if (partner_out) partner_out[o] = -1;
            if (score_out) score_out[o] = kMatchUnscored;
            if (shift_out) shift_out[2 * o] = shift_out[2 * o + 1] = 0;
            if (n_out) n_out[o] = 0;
        }
        return EMBA_OK;
    }
    HIP_TRY(c, hipSetDevice(c->device));
    MatchBuffers& B = c->match;
    hipStream_t s = c->stream;
    const uint8_t* thumbs = nullptr;
    SEQ_TRY(match_begin(c, frames, F, level, skip_zero != 0, &thumbs));
    const size_t pairs = (size_t)match_table_pairs(F), per = match_chunk_pairs(0, false), chunks = match_chunk_count(pairs, per);
    SEQ_TRY(ensure<uint8_t>(c, B.votes, F));
    SEQ_TRY(ensure<MatchBest>(c, B.table, pairs));
    SEQ_TRY(ensure<int32_t>(c, B.partner, F * K));
    SEQ_TRY(ensure<double>(c, B.score, F * K));
    SEQ_TRY(ensure<int32_t>(c, B.shift, 2 * F * K));
    SEQ_TRY(ensure<unsigned long long>(c, B.n, F * K));
    HIP_TRY(c, hipMemcpyAsync(B.votes.p, votes.data(), F, hipMemcpyHostToDevice, s));
    MatchEvalParams E = match_eval_params(c, a, thumbs, skip_zero != 0);
    E.votes = B.votes.as<uint8_t>();
    E.min_gap = min_gap;
    E.out = B.table.as<MatchBest>();
    for (size_t i = 0; i < chunks; ++i) {
        E.p0 = i * per;
        SEQ_TRY(match_launch_eval(c, E, std::min(per, pairs - i * per), c->kernel_timing && i == 0));
    }
    const MatchSelectParams Q{B.table.as<MatchBest>(), B.votes.as<uint8_t>(), F, min_gap, score_min, (int)k, B.partner.as<int32_t>(), B.score.as<double>(),
                              B.shift.as<int32_t>(), B.n.as<unsigned long long>()};
    if (c->kernel_timing) HIP_TRY(c, hipEventRecord(c->ev_start[kMatchSelectTimerSlot], s));
    hipLaunchKernelGGL(emba_frames_match_select_kernel, dim3((unsigned)F), dim3(64), 0, s, Q);
    if (c->kernel_timing) HIP_TRY(c, hipEventRecord(c->ev_stop[kMatchSelectTimerSlot], s));
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipStreamSynchronize(s));      // (votes lives on this call's stack)
    if (partner_out) SEQ_TRY(d2h_pageable(c, partner_out, B.partner.p, F * K * sizeof(int32_t)));
    if (score_out) SEQ_TRY(d2h_pageable(c, score_out, B.score.p, F * K * sizeof(double)));
    if (shift_out) SEQ_TRY(d2h_pageable(c, shift_out, B.shift.p, 2 * F * K * sizeof(int32_t)));
    if (n_out) SEQ_TRY(d2h_pageable(c, n_out, B.n.p, F * K * sizeof(uint64_t)));
    return EMBA_OK;
}

extern "C" emba_status emba_match_start(int32_t dx, int32_t dy, int32_t level, double fu, double fv, double cu, double cv, int32_t sw, int32_t sh, double* q_out)
{
    if (!q_out) return fail(nullptr, EMBA_ERR_INVALID_ARG, "q_out NULL");
    if (!match_start_ok(level, fu, fv, cu, cv, sw, sh))
        return fail(nullptr, EMBA_ERR_INVALID_ARG, "level = %d (0 ... %d), a %d x %d sensor, fu = %g, fv = %g (finite and positive), cu = %g, cv = %g (finite)", (int)level,
                    kPairMaxLevel, (int)sw, (int)sh, fu, fv, cu, cv);
    match_start(dx, dy, level, fu, fv, cu, cv, sw, sh, q_out);
    return EMBA_OK;
}
