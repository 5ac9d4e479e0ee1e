// emba_amd/csrc/view_host.h — sensor views along the trajectory, as host code over the kernels of view_kernels.h: the frames a camera would have seen at
// given times, sampled from a panorama plane (emba_render_views), and the per-pixel event counts of the resident sequence between given times
// (emba_seq_event_frames).  What is plain arithmetic — the sample, the tone, the frame of a timestamp, the chunks — is decided in view_rule.h; here are the
// buffers (emba_ctx::view), the launches and the C ABI.
// Part of emba_hip.hip's translation unit, included by it below poisson_host.h (poisson_boundary_check, poisson_solve), sequence_host.h
// (SEQ_TRY; the sequence itself: emba_ctx::evseq) and transfer_host.h (d2h_pageable).  Nothing of the registered window, of the pose stage of the panorama
// calls (emba_ctx::seq_pose) or of their buffers is read or written.
#pragma once
#include "context.h"
#include "view_kernels.h"
#include "view_rule.h"

using namespace emba;

extern "C" emba_status emba_render_views(emba_ctx* c, const double* plane_host, int boundary, const int64_t* frame_t_ns, size_t F, const double* knots_xyzw,
                                         int32_t K, int64_t t0_ns, int64_t dt_ns, double fill, double lo, double hi, double* views_out, uint8_t* views_u8,
                                         uint64_t* outside_out, double* pm_out)
{
    if (!c) return EMBA_ERR_INVALID_ARG;
    if (!knots_xyzw) return fail(c, EMBA_ERR_INVALID_ARG, "knots NULL");
    if (K < 2) return fail(c, EMBA_ERR_INVALID_ARG, "K = %d: a linear spline has at least two control poses", (int)K);
    if (dt_ns <= 0) return fail(c, EMBA_ERR_INVALID_ARG, "dt_ns = %lld: the knot spacing must be positive", (long long)dt_ns);
    if (F && !frame_t_ns) return fail(c, EMBA_ERR_INVALID_ARG, "frame_t_ns NULL");
    if (F > 0x7FFFFFFFull) return fail(c, EMBA_ERR_INVALID_ARG, "F = %zu: the pose stage counts its frames in 31 bits", F);
    if (views_u8 && !(std::isfinite(lo) && std::isfinite(hi))) return fail(c, EMBA_ERR_INVALID_ARG, "lo = %g, hi = %g: the tone of views_u8 needs finite limits", lo, hi);
    if (!plane_host) {
        SEQ_TRY(poisson_boundary_check(c, boundary));
        if (!c->map.state().resident()) return fail(c, EMBA_ERR_STATE, "no map resident and no plane given");
    }
    if (!F || (!views_out && !views_u8 && !outside_out && !pm_out)) return EMBA_OK;      // nothing asked for: nothing launched
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t s = c->stream;
    ViewBuffers& B = c->view;
    const size_t S = c->S;
    // pose stage: every frame time at once, into this stage's own table; the status word as seq_range_poses keeps it
    SEQ_TRY(ensure<int64_t>(c, B.t, F));
    SEQ_TRY(ensure<double>(c, B.pose, F * (size_t)kPoseStride));
    SEQ_TRY(ensure<double>(c, B.knots, 4 * (size_t)K));
    SEQ_TRY(ensure<uint64_t>(c, B.head, 1));
    SEQ_TRY(ensure<unsigned long long>(c, B.outside, F));
    HIP_TRY(c, hipMemcpyAsync(B.knots.p, knots_xyzw, (size_t)K * 32, hipMemcpyHostToDevice, s));
    HIP_TRY(c, hipMemcpyAsync(B.t.p, frame_t_ns, F * sizeof(int64_t), hipMemcpyHostToDevice, s));
    HIP_TRY(c, hipMemsetAsync(B.head.p, 0, 8, s));
    HIP_TRY(c, hipMemsetAsync(B.outside.p, 0, F * sizeof(unsigned long long), s));
    hipLaunchKernelGGL(emba_pose_kernel, dim3(nblocks(F, 64)), dim3(64), 0, s, (const int64_t*)B.t.as<int64_t>(), (int)F, (const double*)B.knots.as<double>(), (int)K, t0_ns, dt_ns,
                       B.pose.as<double>(), reinterpret_cast<int*>(B.head.as<uint64_t>()));
    HIP_TRY(c, hipGetLastError());
    uint64_t word = 0;
    HIP_TRY(c, hipMemcpyAsync(&word, B.head.p, 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipStreamSynchronize(s));      // (the caller's knots and frame times have been read; a frame outside the knots is refused before anything is rendered)
    if ((int)(word & 0xFFFFFFFFull) & 1) return fail(c, EMBA_ERR_TIME_RANGE, "a frame time lies outside the spline's knots");
    // source plane
    const double* plane = nullptr;
    if (plane_host) {
        SEQ_TRY(ensure<double>(c, B.plane, c->npix));
        HIP_TRY(c, hipMemcpyAsync(B.plane.p, plane_host, c->npix * sizeof(double), hipMemcpyHostToDevice, s));
        plane = B.plane.as<double>();
    } else SEQ_TRY(poisson_solve(c, nullptr, nullptr, nullptr, boundary, &plane));      // the panorama of the resident map, on the device

    // frames, chunk by chunk
    const size_t per = view_chunk_frames(S, sizeof(double)), chunks = view_chunk_count(F, per), cap = std::min(per, F) * S;
    if (views_out) SEQ_TRY(ensure<double>(c, B.frames, cap));
    if (views_u8) SEQ_TRY(ensure<uint8_t>(c, B.u8, cap));
    if (pm_out) SEQ_TRY(ensure<double>(c, B.pm, 2 * cap));
    for (size_t i = 0; i < chunks; ++i) {
        const ViewChunk ch = view_chunk(F, per, i);
        ViewParams P{c->d_lut.as<double>(), B.pose.as<double>() + (size_t)kPoseStride * ch.f0, plane, (int)S, c->W, c->H, c->fx, c->fy, c->cx, c->cy, fill, lo, view_scale(lo, hi),
                     views_out ? B.frames.as<double>() : nullptr, views_u8 ? B.u8.as<uint8_t>() : nullptr, pm_out ? B.pm.as<double>() : nullptr,
                     B.outside.as<unsigned long long>() + ch.f0};
        if (c->kernel_timing && i == 0) HIP_TRY(c, hipEventRecord(c->ev_start[kSeqStageTimerSlot], s));      // (emba_enable_kernel_timing: slot 7 is the first chunk's view kernel)
        hipLaunchKernelGGL(emba_view_kernel, dim3(nblocks(S, kViewThreads), (unsigned)ch.nf), dim3(kViewThreads), 0, s, P);
        if (c->kernel_timing && i == 0) HIP_TRY(c, hipEventRecord(c->ev_stop[kSeqStageTimerSlot], s));
        HIP_TRY(c, hipGetLastError());
        HIP_TRY(c, hipStreamSynchronize(s));
        const size_t cells = ch.nf * S, off = ch.f0 * S;
        if (views_out) SEQ_TRY(d2h_pageable(c, views_out + off, B.frames.p, cells * sizeof(double)));
        if (views_u8) SEQ_TRY(d2h_pageable(c, views_u8 + off, B.u8.p, cells));
        if (pm_out) SEQ_TRY(d2h_pageable(c, pm_out + 2 * off, B.pm.p, 2 * cells * sizeof(double)));
    }
    if (outside_out) SEQ_TRY(d2h_pageable(c, outside_out, B.outside.p, F * sizeof(uint64_t)));
    return EMBA_OK;
}

extern "C" emba_status emba_seq_event_frames(emba_ctx* c, size_t beg, size_t end, const int64_t* edge_t_ns, size_t F, int32_t signed_polarity,
                                             int32_t* frames_out, uint64_t* before_out, uint64_t* after_out)
{
    if (!c) return EMBA_ERR_INVALID_ARG;
    if (!c->evseq.have) return fail(c, EMBA_ERR_STATE, "no resident sequence (emba_seq_upload first)");
    if (beg > end || end > c->evseq.n) return fail(c, EMBA_ERR_INVALID_ARG, "[%zu, %zu) is not a range of the resident sequence of %zu events", beg, end, c->evseq.n);
    if (!edge_t_ns) return fail(c, EMBA_ERR_INVALID_ARG, "edge_t_ns NULL");
    if (F >= 0x7FFFFFFFull) return fail(c, EMBA_ERR_INVALID_ARG, "F = %zu: frames are counted in 31 bits", F);
    if (!view_edges_ok(edge_t_ns, F)) return fail(c, EMBA_ERR_INVALID_ARG, "the %zu edges are not strictly increasing", F + 1);
    if (!frames_out && !before_out && !after_out) return EMBA_OK;      // nothing asked for: nothing launched
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t s = c->stream;
    ViewBuffers& B = c->view;
    const size_t S = c->S, n = end - beg;
    SEQ_TRY(ensure<int64_t>(c, B.edge, F + 1));
    SEQ_TRY(ensure<unsigned long long>(c, B.ends, 2));
    HIP_TRY(c, hipMemcpyAsync(B.edge.p, edge_t_ns, (F + 1) * sizeof(int64_t), hipMemcpyHostToDevice, s));
    HIP_TRY(c, hipMemsetAsync(B.ends.p, 0, 2 * sizeof(unsigned long long), s));
    // frames, chunk by chunk: every launch sweeps the range's events and adds those of its own frames; the first one also counts the two ends.  Without
    // frames_out that one launch has no frames of its own.
    const size_t Ff = frames_out ? F : 0;
    const size_t per = view_chunk_frames(S, sizeof(int32_t)), chunks = std::max<size_t>(view_chunk_count(Ff, per), 1);
    if (Ff) SEQ_TRY(ensure<int32_t>(c, B.counts, std::min(per, Ff) * S));
    for (size_t i = 0; i < chunks; ++i) {
        const ViewChunk ch = Ff ? view_chunk(Ff, per, i) : ViewChunk{0, 0};
        if (ch.nf) HIP_TRY(c, hipMemsetAsync(B.counts.p, 0, ch.nf * S * sizeof(int32_t), s));
        if (n) {
            EventFramesParams P{c->evseq.x.as<uint16_t>() + beg, c->evseq.y.as<uint16_t>() + beg, c->evseq.pol.as<uint8_t>() + beg, c->evseq.t.as<int64_t>() + beg, (long)n,
                                B.edge.as<int64_t>(), (long)F, (long)ch.f0, (long)ch.nf, c->sw, S, signed_polarity != 0, i == 0, B.counts.as<int32_t>(),
                                B.ends.as<unsigned long long>()};
            if (c->kernel_timing && i == 0) HIP_TRY(c, hipEventRecord(c->ev_start[kSeqStageTimerSlot], s));      // (slot 7: the first chunk's kernel)
            hipLaunchKernelGGL(emba_event_frames_kernel, dim3(nblocks(n, kViewThreads)), dim3(kViewThreads), 0, s, P);
            if (c->kernel_timing && i == 0) HIP_TRY(c, hipEventRecord(c->ev_stop[kSeqStageTimerSlot], s));
            HIP_TRY(c, hipGetLastError());
        }
        HIP_TRY(c, hipStreamSynchronize(s));
        if (ch.nf) SEQ_TRY(d2h_pageable(c, frames_out + ch.f0 * S, B.counts.p, ch.nf * S * sizeof(int32_t)));
    }
    unsigned long long ends[2] = {0, 0};
    HIP_TRY(c, hipMemcpy(ends, B.ends.p, sizeof ends, hipMemcpyDeviceToHost));
    if (before_out) *before_out = ends[0];
    if (after_out) *after_out = ends[1];
    return EMBA_OK;
}
