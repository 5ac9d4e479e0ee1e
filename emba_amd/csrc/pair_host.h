// emba_amd/csrc/pair_host.h — loops closed among tracked frames, as host code: one frame aligned to another over the kernel of pair_kernels.h and the
// alignment's reduce and step kernels (emba_frames_pair_eval, emba_frames_pair_align), and the rotation graph, which is host code alone
// (emba_rotation_graph_solve).  What is plain arithmetic is decided in pair_rule.h, align_rule.h and graph_rule.h; here are the buffers (emba_ctx::pair),
// the launches and the C ABI.
// Part of emba_hip.hip's translation unit, included by it below refit_host.h; it uses frame_host.h (frame_ensure, frame_launch_eval, frame_lm_loop,
// frame_read_loop: DESIGN.md §23), align_host.h (align_settings_refusal, align_launch_step), sequence_host.h (SEQ_TRY) and transfer_host.h (d2h_pageable).
// Nothing of the registered window, of the resident sequence, of the mosaic and the level planes, of the resident map or of any other stage's buffers is
// written.
#pragma once
#include <vector>

#include "align_host.h"
#include "context.h"
#include "frame_host.h"
#include "graph_rule.h"
#include "pair_kernels.h"
#include "pair_rule.h"

using namespace emba;

namespace {
// what both calls take, as the C ABI hands it over
struct PairCall {
    const uint8_t* frames; size_t F; const int32_t* pairs; size_t P; const double* Q; const double* gain; const double* bias;
    double fu, fv, cu, cv; const double* D; int32_t skip_zero; double huber_k;
};

// the refusals of the arguments up to huber_k (pair_args_ok), which pair_level_host.h's calls begin with as well
emba_status pair_args_refusal(emba_ctx* c, const PairCall& a)
{
    size_t at = 0;
    switch (pair_args_ok(a.frames != nullptr, a.F, a.pairs, a.P, a.Q, a.gain, a.bias, a.fu, a.fv, a.cu, a.cv, a.D, a.huber_k, &at)) {
    case PairArgStatus::ok: break;
    case PairArgStatus::frames_null: return fail(c, EMBA_ERR_INVALID_ARG, "frames NULL");
    case PairArgStatus::pairs_null: return fail(c, EMBA_ERR_INVALID_ARG, "pairs NULL");
    case PairArgStatus::q_null: return fail(c, EMBA_ERR_INVALID_ARG, "Q_xyzw NULL");
    case PairArgStatus::too_many_pairs: return fail(c, EMBA_ERR_INVALID_ARG, "P = %zu: pairs are counted in 31 bits", a.P);
    case PairArgStatus::pair_out_of_range:
        return fail(c, EMBA_ERR_INVALID_ARG, "pairs[%zu] = (%d, %d) names a frame outside [0, %zu)", at, (int)a.pairs[2 * at], (int)a.pairs[2 * at + 1], a.F);
    case PairArgStatus::bad_q: return fail(c, EMBA_ERR_INVALID_ARG, "Q_xyzw[%zu] is not finite or has zero norm", at);
    case PairArgStatus::bad_exposure: return fail(c, EMBA_ERR_INVALID_ARG, "pair %zu: the gain is finite and positive, the bias finite", at);
    case PairArgStatus::bad_focal: return fail(c, EMBA_ERR_INVALID_ARG, "fu = %g, fv = %g: both are finite and positive", a.fu, a.fv);
    case PairArgStatus::bad_centre: return fail(c, EMBA_ERR_INVALID_ARG, "cu = %g, cv = %g are not finite", a.cu, a.cv);
    case PairArgStatus::bad_distortion: return fail(c, EMBA_ERR_INVALID_ARG, "D is not finite");
    case PairArgStatus::huber_not_finite: return fail(c, EMBA_ERR_INVALID_ARG, "huber_k is not a number");
    }
    return EMBA_OK;
}

// every refusal, before anything is uploaded; `set`: the loop's settings, or nullptr for the evaluation alone
emba_status pair_refusals(emba_ctx* c, const PairCall& a, const emba_align_settings* set, bool loop)
{
    SEQ_TRY(pair_args_refusal(c, a));
    if (loop) SEQ_TRY(align_settings_refusal(c, set));
    if (!pair_bytes_ok(a.F, c->S)) return fail(c, EMBA_ERR_INVALID_ARG, "F = %zu frames of %zu bytes: the resident sequence is bounded at %zu bytes", a.F, c->S, kPairMaxBytes);
    return EMBA_OK;
}

// the buffers of a call whose chunks hold at most np pairs, and the whole sequence into them
emba_status pair_begin(emba_ctx* c, const PairCall& a, size_t np, bool want_uv, bool want_resid, bool loop)
{
    PairBuffers& B = c->pair;
    SEQ_TRY(ensure<uint8_t>(c, B.loop.frames, a.F * c->S));      // (all F frames, where frame_ensure asks for a chunk's)
    SEQ_TRY(frame_ensure(c, B.loop, kAlignSums, np, want_uv, want_resid, loop));
    SEQ_TRY(ensure<int32_t>(c, B.pairs, 2 * np));
    if (a.gain) SEQ_TRY(ensure<double>(c, B.gain, np));
    if (a.bias) SEQ_TRY(ensure<double>(c, B.bias, np));
    HIP_TRY(c, hipMemcpyAsync(B.loop.frames.p, a.frames, a.F * c->S, hipMemcpyHostToDevice, c->stream));
    return EMBA_OK;
}

// a chunk's pairs, rotations and exposures into the buffers every pair is evaluated from
emba_status pair_upload_chunk(emba_ctx* c, const PairCall& a, const ViewChunk& ch)
{
    PairBuffers& B = c->pair;
    hipStream_t s = c->stream;
    HIP_TRY(c, hipMemcpyAsync(B.pairs.p, a.pairs + 2 * ch.f0, 2 * ch.nf * sizeof(int32_t), hipMemcpyHostToDevice, s));
    HIP_TRY(c, hipMemcpyAsync(B.loop.q_trial.p, a.Q + 4 * ch.f0, 4 * ch.nf * sizeof(double), hipMemcpyHostToDevice, s));
    if (a.gain) HIP_TRY(c, hipMemcpyAsync(B.gain.p, a.gain + ch.f0, ch.nf * sizeof(double), hipMemcpyHostToDevice, s));
    if (a.bias) HIP_TRY(c, hipMemcpyAsync(B.bias.p, a.bias + ch.f0, ch.nf * sizeof(double), hipMemcpyHostToDevice, s));
    return EMBA_OK;
}

// one evaluation of the chunk's np pairs at B.loop.q_trial into B.loop.esums / ecounts
emba_status pair_launch_eval(emba_ctx* c, const PairCall& a, size_t np, const int32_t* status, bool want_uv, bool want_resid, bool timed)
{
    PairBuffers& B = c->pair;
    FrameLoopBuffers& L = B.loop;
    const PairEvalParams P{c->d_lut.as<double>(), L.frames.as<uint8_t>(), B.pairs.as<int32_t>(), L.q_trial.as<double>(), a.gain ? B.gain.as<double>() : nullptr,
                           a.bias ? B.bias.as<double>() : nullptr, status, (int)c->S, c->sw, c->sh, pair_camera(a.fu, a.fv, a.cu, a.cv, a.D), a.huber_k,
                           a.skip_zero != 0, L.partial.as<double>(), want_uv ? L.pm.as<double>() : nullptr, want_resid ? L.resid.as<double>() : nullptr};
    return frame_launch_eval(c, L, emba_frames_pair_eval_kernel, P, emba_frames_align_reduce_kernel, kAlignSums, np, timed);
}
}  // namespace

extern "C" emba_status emba_frames_pair_eval(emba_ctx* c, const uint8_t* frames, size_t F, const int32_t* pairs, size_t P, const double* Q_xyzw, const double* gain,
                                             const double* bias, double fu, double fv, double cu, double cv, const double* D, int32_t skip_zero, double huber_k,
                                             double* sums_out, uint64_t* counts_out, double* uv_out, double* resid_out)
{
    if (!c) return EMBA_ERR_INVALID_ARG;
    const PairCall a{frames, F, pairs, P, Q_xyzw, gain, bias, fu, fv, cu, cv, D, skip_zero, huber_k};
    SEQ_TRY(pair_refusals(c, a, nullptr, false));
    if (!P) return EMBA_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    FrameLoopBuffers& L = c->pair.loop;
    const size_t S = c->S, per = pair_chunk_pairs(S), chunks = view_chunk_count(P, per);
    SEQ_TRY(pair_begin(c, a, std::min(per, P), uv_out != nullptr, resid_out != nullptr, false));
    for (size_t i = 0; i < chunks; ++i) {
        const ViewChunk ch = view_chunk(P, per, i);
        const size_t cells = ch.nf * S, off = ch.f0 * S;
        SEQ_TRY(pair_upload_chunk(c, a, ch));
        SEQ_TRY(pair_launch_eval(c, a, ch.nf, nullptr, uv_out != nullptr, resid_out != nullptr, c->kernel_timing && i == 0));
        HIP_TRY(c, hipStreamSynchronize(c->stream));      // (the chunk's pairs have been read: the next chunk overwrites them)
        if (sums_out) SEQ_TRY(d2h_pageable(c, sums_out + (size_t)kAlignSums * ch.f0, L.esums.p, (size_t)kAlignSums * ch.nf * sizeof(double)));
        if (counts_out) SEQ_TRY(d2h_pageable(c, counts_out + 4 * ch.f0, L.ecounts.p, 4 * ch.nf * sizeof(uint64_t)));
        if (uv_out) SEQ_TRY(d2h_pageable(c, uv_out + 2 * off, L.pm.p, 2 * cells * sizeof(double)));
        if (resid_out) SEQ_TRY(d2h_pageable(c, resid_out + off, L.resid.p, cells * sizeof(double)));
    }
    return EMBA_OK;
}

extern "C" emba_status emba_frames_pair_align(emba_ctx* c, const uint8_t* frames, size_t F, const int32_t* pairs, size_t P, const double* Q_xyzw, const double* gain,
                                              const double* bias, double fu, double fv, double cu, double cv, const double* D, int32_t skip_zero,
                                              const emba_align_settings* set, double* q_out, double* sums_out, uint64_t* counts_out, int32_t* status_out,
                                              int32_t* iters_out, double* cost0_out, uint64_t* n0_out, double* info_out)
{
    if (!c) return EMBA_ERR_INVALID_ARG;
    const PairCall a{frames, F, pairs, P, Q_xyzw, gain, bias, fu, fv, cu, cv, D, skip_zero, set ? set->huber_k : 0.0};
    SEQ_TRY(pair_refusals(c, a, set, true));
    if (!P) return EMBA_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    FrameLoopBuffers& L = c->pair.loop;
    const size_t per = pair_chunk_pairs(c->S), chunks = view_chunk_count(P, per);
    SEQ_TRY(pair_begin(c, a, std::min(per, P), false, false, true));
    std::vector<double> hs;
    std::vector<uint64_t> hc;
    for (size_t i = 0; i < chunks; ++i) {
        const ViewChunk ch = view_chunk(P, per, i);
        SEQ_TRY(pair_upload_chunk(c, a, ch));
        SEQ_TRY(frame_lm_loop(
            c, L, [&](const int32_t* status, bool first) { return pair_launch_eval(c, a, ch.nf, status, false, false, c->kernel_timing && i == 0 && first); },
            [&](bool first) { align_launch_step(c, L, ch.nf, *set, first); }));
        SEQ_TRY(frame_read_loop(c, L, kAlignSums, ch, q_out, sums_out, counts_out, status_out, iters_out, cost0_out, n0_out));
        if (info_out) {      // (from the accepted state's sums and counts, on the host: six divisions per pair)
            hs.resize((size_t)kAlignSums * ch.nf);
            hc.resize(4 * ch.nf);
            SEQ_TRY(d2h_pageable(c, hs.data(), L.sums.p, hs.size() * sizeof(double)));
            SEQ_TRY(d2h_pageable(c, hc.data(), L.counts.p, hc.size() * sizeof(uint64_t)));
            for (size_t p = 0; p < ch.nf; ++p) pair_information(&hs[(size_t)kAlignSums * p], hc[4 * p], info_out + 6 * (ch.f0 + p));
        }
    }
    return EMBA_OK;
}

extern "C" emba_status emba_rotation_graph_solve(const double* q_xyzw, const int32_t* status, size_t F, const int32_t* edges, const double* Q_xyzw, const double* info,
                                                 size_t E, const emba_graph_settings* set, double* q_out, double* cost_out, int32_t* iters_out, int32_t* end_out,
                                                 size_t* at_out)
{
    size_t at = 0;
    const GraphArgStatus st = graph_args_ok(q_xyzw, status, F, edges, Q_xyzw, info, E, set, &at);
    if (at_out) *at_out = at;
    switch (st) {
    case GraphArgStatus::ok: break;
    case GraphArgStatus::q_null: return fail(nullptr, EMBA_ERR_INVALID_ARG, "q_xyzw NULL");
    case GraphArgStatus::status_null: return fail(nullptr, EMBA_ERR_INVALID_ARG, "status NULL");
    case GraphArgStatus::edges_null: return fail(nullptr, EMBA_ERR_INVALID_ARG, "edges, Q_xyzw or info NULL");
    case GraphArgStatus::settings: return fail(nullptr, EMBA_ERR_INVALID_ARG, "settings NULL or out of range");
    case GraphArgStatus::bad_q: return fail(nullptr, EMBA_ERR_INVALID_ARG, "q_xyzw[%zu] is not finite or has zero norm", at);
    case GraphArgStatus::no_anchor: return fail(nullptr, EMBA_ERR_INVALID_ARG, "no anchor: a rotation graph needs a frame that is held");
    case GraphArgStatus::edge_out_of_range: return fail(nullptr, EMBA_ERR_INVALID_ARG, "edge %zu names a frame outside [0, %zu)", at, F);
    case GraphArgStatus::bad_edge_q: return fail(nullptr, EMBA_ERR_INVALID_ARG, "Q_xyzw[%zu] is not finite or has zero norm", at);
    case GraphArgStatus::info_not_finite: return fail(nullptr, EMBA_ERR_INVALID_ARG, "info[%zu] is not finite", at);
    case GraphArgStatus::unreachable: return fail(nullptr, EMBA_ERR_INVALID_ARG, "frame %zu is named by an edge, but no path of edges leads from an anchor to it", at);
    }
    std::vector<double> q(4 * F);
    const GraphResult r = graph_solve(q_xyzw, status, F, edges, Q_xyzw, info, E, *set, q.data());
    if (q_out) std::copy(q.begin(), q.end(), q_out);
    if (cost_out) { cost_out[0] = r.cost0; cost_out[1] = r.cost; }
    if (iters_out) { iters_out[0] = r.iters; iters_out[1] = r.cg_iters; }
    if (end_out) *end_out = r.end;
    return EMBA_OK;
}
