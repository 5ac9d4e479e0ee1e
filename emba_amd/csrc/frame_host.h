// emba_amd/csrc/frame_host.h — what the host code of the stages over intensity frames shares (align_host.h, track_host.h, exposure_host.h), over
// FrameLoopBuffers (context.h) and the bodies of frame_kernels.h: the buffers of a chunk, a chunk's upload, one evaluation (evaluation kernel, timer slot,
// reduce kernel), the chunked evaluate-and-read-back of the *_eval calls, and the per-frame Levenberg-Marquardt loop with the read-back of its state.  A stage
// brings its evaluation kernel with its parameters, its reduce and step kernels and its number of sums; each stage keeps buffers of its own.  DESIGN.md §23.
// Part of emba_hip.hip's translation unit, included by it below sim_host.h; it uses sequence_host.h (SEQ_TRY), transfer_host.h (d2h_pageable),
// panorama_host.h (kSeqStageTimerSlot) and view_rule.h (the chunks).
#pragma once
#include "context.h"
#include "frame_kernels.h"
#include "view_rule.h"

using namespace emba;

namespace {
using FrameReduceKernel = void (*)(const double*, int, long, const int32_t*, double*, unsigned long long*);

// the buffers of a chunk of at most `nf` frames evaluated into `n_sums` sums; `loop`: the frames' state as well
emba_status frame_ensure(emba_ctx* c, FrameLoopBuffers& B, int n_sums, size_t nf, bool want_pm, bool want_resid, bool loop)
{
    const size_t S = c->S, nb = nblocks(S, kFrameThreads);
    SEQ_TRY(ensure<uint8_t>(c, B.frames, nf * S));
    if (want_pm) SEQ_TRY(ensure<double>(c, B.pm, 2 * nf * S));
    if (want_resid) SEQ_TRY(ensure<double>(c, B.resid, nf * S));
    SEQ_TRY(ensure<double>(c, B.partial, nf * nb * (size_t)frame_partial(n_sums)));
    SEQ_TRY(ensure<double>(c, B.q_trial, 4 * nf));
    SEQ_TRY(ensure<double>(c, B.esums, (size_t)n_sums * nf));
    SEQ_TRY(ensure<unsigned long long>(c, B.ecounts, 4 * nf));
    if (!loop) return EMBA_OK;
    SEQ_TRY(ensure<double>(c, B.q, 4 * nf));
    SEQ_TRY(ensure<double>(c, B.sums, (size_t)n_sums * nf));
    SEQ_TRY(ensure<unsigned long long>(c, B.counts, 4 * nf));
    SEQ_TRY(ensure<double>(c, B.lambda, nf));
    SEQ_TRY(ensure<double>(c, B.dnorm, nf));
    SEQ_TRY(ensure<int32_t>(c, B.status, nf));
    SEQ_TRY(ensure<int32_t>(c, B.iters, nf));
    SEQ_TRY(ensure<int32_t>(c, B.have_trial, nf));
    SEQ_TRY(ensure<double>(c, B.cost0, nf));
    SEQ_TRY(ensure<unsigned long long>(c, B.n0, nf));
    SEQ_TRY(ensure<unsigned int>(c, B.running, 1));
    return EMBA_OK;
}

// a chunk's bytes and rotations into the buffers every frame is evaluated from
emba_status frame_upload_chunk(emba_ctx* c, FrameLoopBuffers& B, const uint8_t* frames, const double* q_xyzw, const ViewChunk& ch)
{
    HIP_TRY(c, hipMemcpyAsync(B.frames.p, frames + ch.f0 * c->S, ch.nf * c->S, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(B.q_trial.p, q_xyzw + 4 * ch.f0, 4 * ch.nf * sizeof(double), hipMemcpyHostToDevice, c->stream));
    return EMBA_OK;
}

// B.esums / B.ecounts of nf frames from B.partial; `status`: the frames' status words, or nullptr (every frame is reduced)
emba_status frame_launch_reduce(emba_ctx* c, FrameLoopBuffers& B, FrameReduceKernel reduce, int n_sums, size_t nf, const int32_t* status)
{
    hipLaunchKernelGGL(reduce, dim3(nblocks(nf * (size_t)(n_sums + 4), kFrameThreads)), dim3(kFrameThreads), 0, c->stream, (const double*)B.partial.as<double>(),
                       (int)nblocks(c->S, kFrameThreads), (long)nf, status, B.esums.as<double>(), B.ecounts.as<unsigned long long>());
    HIP_TRY(c, hipGetLastError());
    return EMBA_OK;
}

// one evaluation of nf frames into B.esums / B.ecounts: the stage's evaluation kernel on its parameters P (P.status: the frames' status words, or nullptr:
// every frame is evaluated) and the reduction of its partial sums; `timed`: timer slot 7 around the evaluation kernel
template <class Params>
emba_status frame_launch_eval(emba_ctx* c, FrameLoopBuffers& B, void (*eval)(Params), const Params& P, FrameReduceKernel reduce, int n_sums, size_t nf, bool timed)
{
    hipStream_t s = c->stream;
    if (timed) HIP_TRY(c, hipEventRecord(c->ev_start[kSeqStageTimerSlot], s));
    hipLaunchKernelGGL(eval, dim3(nblocks(c->S, kFrameThreads), (unsigned)nf), dim3(kFrameThreads), 0, s, P);
    if (timed) HIP_TRY(c, hipEventRecord(c->ev_stop[kSeqStageTimerSlot], s));
    HIP_TRY(c, hipGetLastError());
    return frame_launch_reduce(c, B, reduce, n_sums, nf, P.status);
}

// The *_eval calls: F frames chunk by chunk: the bytes and rotations up, upload_more(chunk) for what else the stage evaluates at, eval(nf, timed), and the sums,
// counts, pm and residuals the caller asks for into its pageable memory.  The buffers are there (frame_ensure).
template <class UploadMore, class Eval>
emba_status frame_eval_chunks(emba_ctx* c, FrameLoopBuffers& B, int n_sums, const uint8_t* frames, const double* q_xyzw, size_t F, UploadMore upload_more, Eval eval,
                              double* sums_out, uint64_t* counts_out, double* pm_out, double* resid_out)
{
    const size_t S = c->S, per = view_chunk_frames(S, 1), chunks = view_chunk_count(F, per);
    for (size_t i = 0; i < chunks; ++i) {
        const ViewChunk ch = view_chunk(F, per, i);
        const size_t cells = ch.nf * S, off = ch.f0 * S;
        SEQ_TRY(frame_upload_chunk(c, B, frames, q_xyzw, ch));
        SEQ_TRY(upload_more(ch));
        SEQ_TRY(eval(ch.nf, c->kernel_timing && i == 0));
        HIP_TRY(c, hipStreamSynchronize(c->stream));      // (the chunk's bytes have been read: the next chunk overwrites them)
        if (sums_out) SEQ_TRY(d2h_pageable(c, sums_out + (size_t)n_sums * ch.f0, B.esums.p, (size_t)n_sums * ch.nf * sizeof(double)));
        if (counts_out) SEQ_TRY(d2h_pageable(c, counts_out + 4 * ch.f0, B.ecounts.p, 4 * ch.nf * sizeof(uint64_t)));
        if (pm_out) SEQ_TRY(d2h_pageable(c, pm_out + 2 * off, B.pm.p, 2 * cells * sizeof(double)));
        if (resid_out) SEQ_TRY(d2h_pageable(c, resid_out + off, B.resid.p, cells * sizeof(double)));
    }
    return EMBA_OK;
}

// The per-frame Levenberg-Marquardt loop on the frames uploaded to B: evaluation 0 where they start, then per iteration a step (decide on the evaluated trial,
// propose the next) and the evaluation of the frames still running.  eval(status or nullptr, first) launches an evaluation, step(first) the stage's step
// kernel, which counts the frames it leaves running into B.running; the stream is waited on once per iteration, for that count.  After max_iters trials no
// frame is running (align_step, exposure_step).
template <class Eval, class Step>
emba_status frame_lm_loop(emba_ctx* c, FrameLoopBuffers& B, Eval eval, Step step)
{
    hipStream_t s = c->stream;
    for (bool first = true;; first = false) {
        SEQ_TRY(eval(first ? nullptr : (const int32_t*)B.status.as<int32_t>(), first));
        HIP_TRY(c, hipMemsetAsync(B.running.p, 0, sizeof(unsigned int), s));
        step(first);
        HIP_TRY(c, hipGetLastError());
        unsigned int running = 0;
        HIP_TRY(c, hipMemcpyAsync(&running, B.running.p, sizeof running, hipMemcpyDeviceToHost, s));
        HIP_TRY(c, hipStreamSynchronize(s));
        if (!running) return EMBA_OK;
    }
}

// the loop's state of a chunk's frames into the caller's pageable memory, what it asks for
emba_status frame_read_loop(emba_ctx* c, FrameLoopBuffers& B, int n_sums, const ViewChunk& ch, double* q_out, double* sums_out, uint64_t* counts_out, int32_t* status_out,
                            int32_t* iters_out, double* cost0_out, uint64_t* n0_out)
{
    const size_t f0 = ch.f0, nf = ch.nf;
    if (q_out) SEQ_TRY(d2h_pageable(c, q_out + 4 * f0, B.q.p, 4 * nf * sizeof(double)));
    if (sums_out) SEQ_TRY(d2h_pageable(c, sums_out + (size_t)n_sums * f0, B.sums.p, (size_t)n_sums * nf * sizeof(double)));
    if (counts_out) SEQ_TRY(d2h_pageable(c, counts_out + 4 * f0, B.counts.p, 4 * nf * sizeof(uint64_t)));
    if (status_out) SEQ_TRY(d2h_pageable(c, status_out + f0, B.status.p, nf * sizeof(int32_t)));
    if (iters_out) SEQ_TRY(d2h_pageable(c, iters_out + f0, B.iters.p, nf * sizeof(int32_t)));
    if (cost0_out) SEQ_TRY(d2h_pageable(c, cost0_out + f0, B.cost0.p, nf * sizeof(double)));
    if (n0_out) SEQ_TRY(d2h_pageable(c, n0_out + f0, B.n0.p, nf * sizeof(uint64_t)));
    return EMBA_OK;
}
}  // namespace
