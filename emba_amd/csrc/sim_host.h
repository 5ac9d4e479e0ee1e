// emba_amd/csrc/sim_host.h — the event simulator, as host code over the kernels of sim_kernels.h and the view kernel of view_kernels.h: a recording from a
// panorama plane and a trajectory (emba_simulate_events), its downloads (emba_sim_size, emba_sim_get) and its way into the resident sequence, device to device
// (emba_seq_from_sim).  What is plain arithmetic — what a pixel does with one more sample, the chunks, the sort's passes — is decided in sim_rule.h; here are
// the buffers and the recording (emba_ctx::sim), the launches and the C ABI.
// Part of emba_hip.hip's translation unit, included by it below view_host.h (the view kernel and its parameters), poisson_host.h (poisson_boundary_check,
// poisson_solve), sequence_host.h (SEQ_TRY, seq_ingest_begin / seq_ingest_finish, the ingest kernel), order_host.h (dev_scan, dev_sort and the sort pairs)
// and transfer_host.h (d2h_pageable).  The registered window, the pose stage of the panorama calls and the buffers of the views are neither read nor written.
#pragma once
#include "context.h"
#include "sim_kernels.h"
#include "sim_rule.h"
#include "view_kernels.h"

using namespace emba;

namespace {

constexpr int kSimTimerSlot0 = 3;      // with kernel timing on, timer slots 3 ... 7 bracket the first chunk's phases: views, count, scan, emit, sort

// at least need_bytes in b, the first keep_bytes of it kept (DevBuf::ensure keeps nothing): the recording grows chunk by chunk
emba_status sim_grow(emba_ctx* c, DevBuf& b, size_t keep_bytes, size_t need_bytes, size_t limit_bytes)
{
    if (b.p && b.bytes >= need_bytes) return EMBA_OK;
    DevBuf nb;
    const size_t want = std::max(need_bytes, std::min(2 * b.bytes, limit_bytes));
    const hipError_t e = nb.ensure(want, nullptr, c->opt_poison != 0, c->stream);
    if (e != hipSuccess) return fail(c, EMBA_ERR_HIP, "hipMalloc of %zu bytes failed: %s", want, hipGetErrorString(e));
    if (keep_bytes) HIP_TRY(c, hipMemcpyAsync(nb.p, b.p, keep_bytes, hipMemcpyDeviceToDevice, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));      // (the old memory is freed below)
    b = std::move(nb);
    return EMBA_OK;
}

struct SimPhaseTimer {      // the events around the phases of the first chunk
    emba_ctx* c; bool on;
    hipError_t start(int phase) const { return on ? hipEventRecord(c->ev_start[kSimTimerSlot0 + phase], c->stream) : hipSuccess; }
    hipError_t stop(int phase) const { return on ? hipEventRecord(c->ev_stop[kSimTimerSlot0 + phase], c->stream) : hipSuccess; }
};

// the chunk's n events, as emitted, into time order and behind the `base` events the recording's next arrays already hold
emba_status sim_sort_and_gather(emba_ctx* c, size_t n, uint64_t span, int64_t t_base, size_t base)
{
    hipStream_t s = c->stream;
    SimState& B = c->sim;
    uint32_t *k0 = c->ord.keys[0].as<uint32_t>(), *v0 = c->ord.vals[0].as<uint32_t>(), *k1 = c->ord.keys[1].as<uint32_t>(), *v1 = c->ord.vals[1].as<uint32_t>();
    const SimSortPlan plan = sim_sort_plan(span);
    SEQ_TRY(dev_sort(c, &k0, &v0, &k1, &v1, n, plan.lo_bits));
    if (plan.hi_bits) {
        hipLaunchKernelGGL(emba_sim_hikey_kernel, dim3(nblocks(n)), dim3(256), 0, s, (const uint32_t*)v0, (const int64_t*)B.ev_t.as<int64_t>(), t_base, (long)n, k0);
        SEQ_TRY(dev_sort(c, &k0, &v0, &k1, &v1, n, plan.hi_bits));
    }
    hipLaunchKernelGGL(emba_sim_gather_kernel, dim3(nblocks(n)), dim3(256), 0, s, (const uint32_t*)v0, (const int64_t*)B.ev_t.as<int64_t>(), (const uint32_t*)B.ev_sp.as<uint32_t>(),
                       (long)n, c->sw, B.x2.as<uint16_t>() + base, B.y2.as<uint16_t>() + base, B.pol2.as<uint8_t>() + base, B.t2.as<int64_t>() + base);
    HIP_TRY(c, hipGetLastError());
    return EMBA_OK;
}

}  // namespace

extern "C" emba_status emba_simulate_events(emba_ctx* c, const double* plane_host, int boundary, const int64_t* step_t_ns, size_t F, const double* knots_xyzw, int32_t K,
                                            int64_t t0_ns, int64_t dt_ns, double c_on, double c_off, int32_t max_per_step, uint64_t max_events, uint64_t* stats)
{
    if (!c) return EMBA_ERR_INVALID_ARG;
    if (!knots_xyzw) return fail(c, EMBA_ERR_INVALID_ARG, "knots NULL");
    if (!step_t_ns) return fail(c, EMBA_ERR_INVALID_ARG, "step_t_ns NULL");
    if (K < 2) return fail(c, EMBA_ERR_INVALID_ARG, "K = %d: a linear spline has at least two control poses", (int)K);
    if (dt_ns <= 0) return fail(c, EMBA_ERR_INVALID_ARG, "dt_ns = %lld: the knot spacing must be positive", (long long)dt_ns);
    if (F < 1 || F >= 0x7FFFFFFFull) return fail(c, EMBA_ERR_INVALID_ARG, "F = %zu: at least one step, and the pose stage counts its F + 1 frames in 31 bits", F);
    if (!sim_steps_ok(step_t_ns, F)) return fail(c, EMBA_ERR_INVALID_ARG, "the %zu step times are not strictly increasing over less than 2^52 ns", F + 1);
    if (!sim_threshold_ok(c_on) || !sim_threshold_ok(c_off)) return fail(c, EMBA_ERR_INVALID_ARG, "c_on = %g, c_off = %g: the thresholds are positive and finite", c_on, c_off);
    if (max_per_step < 1 || max_per_step > kSimMaxPerStep) return fail(c, EMBA_ERR_INVALID_ARG, "max_per_step = %d: 1 to %d", (int)max_per_step, kSimMaxPerStep);
    const size_t S = c->S;
    if (!sim_sensor_fits(S)) return fail(c, EMBA_ERR_INVALID_ARG, "a sensor of %zu pixels: one step's events do not fit the 32-bit scan", S);
    if (!plane_host) {
        SEQ_TRY(poisson_boundary_check(c, boundary));
        if (!c->map.state().resident()) return fail(c, EMBA_ERR_STATE, "no map resident and no plane given");
    }
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t s = c->stream;
    SimState& B = c->sim;
    const size_t nF = F + 1;
    // pose stage: every step time at once, into this stage's own table; the status word before anything else runs
    SEQ_TRY(ensure<int64_t>(c, B.step_t, nF));
    SEQ_TRY(ensure<double>(c, B.pose, nF * (size_t)kPoseStride));
    SEQ_TRY(ensure<double>(c, B.knots, 4 * (size_t)K));
    SEQ_TRY(ensure<uint64_t>(c, B.head, 1));
    HIP_TRY(c, hipMemcpyAsync(B.knots.p, knots_xyzw, (size_t)K * 32, hipMemcpyHostToDevice, s));
    HIP_TRY(c, hipMemcpyAsync(B.step_t.p, step_t_ns, nF * sizeof(int64_t), hipMemcpyHostToDevice, s));
    HIP_TRY(c, hipMemsetAsync(B.head.p, 0, 8, s));
    hipLaunchKernelGGL(emba_pose_kernel, dim3(nblocks(nF, 64)), dim3(64), 0, s, (const int64_t*)B.step_t.as<int64_t>(), (int)nF, (const double*)B.knots.as<double>(), (int)K, t0_ns, dt_ns,
                       B.pose.as<double>(), reinterpret_cast<int*>(B.head.as<uint64_t>()));
    HIP_TRY(c, hipGetLastError());
    uint64_t word = 0;
    HIP_TRY(c, hipMemcpyAsync(&word, B.head.p, 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipStreamSynchronize(s));
    if ((int)(word & 0xFFFFFFFFull) & 1) return fail(c, EMBA_ERR_TIME_RANGE, "a step time lies outside the spline's knots");
    // source plane
    const double* plane = nullptr;
    if (plane_host) {
        SEQ_TRY(ensure<double>(c, B.plane, c->npix));
        HIP_TRY(c, hipMemcpyAsync(B.plane.p, plane_host, c->npix * sizeof(double), hipMemcpyHostToDevice, s));
        plane = B.plane.as<double>();
    } else SEQ_TRY(poisson_solve(c, nullptr, nullptr, nullptr, boundary, &plane));      // the panorama of the resident map, on the device

    const size_t per = std::min(sim_chunk_steps(S), F), chunks = view_chunk_count(F, per);
    SEQ_TRY(ensure<double>(c, B.frames, (per + 1) * S));
    SEQ_TRY(ensure<unsigned long long>(c, B.outside, per + 1));
    SEQ_TRY(ensure<uint32_t>(c, B.cells, per * S));
    for (int k = 0; k < 2; ++k) { SEQ_TRY(ensure<double>(c, B.ref[k], S)); SEQ_TRY(ensure<uint8_t>(c, B.armed[k], S)); }
    SEQ_TRY(ensure<unsigned long long>(c, B.sums, 4));
    SEQ_TRY(ensure<uint32_t>(c, B.total, 2));
    HIP_TRY(c, hipMemsetAsync(B.sums.p, 0, 4 * sizeof(unsigned long long), s));
    const uint64_t limit = max_events ? std::min<uint64_t>(max_events, kSimMaxEvents) : kSimMaxEvents;
    uint64_t n_needed = 0;      // events of the chunks so far: where the next chunk's begin
    bool over = false;          // more than `limit`: the remaining chunks are only counted
    int cur = 0;                // B.ref[cur], B.armed[cur]: the pixels' state in front of the chunk
    for (size_t i = 0; i < chunks; ++i) {
        const ViewChunk ch = view_chunk(F, per, i);      // steps [f0, f0 + nf): the frames f0 ... f0 + nf in the slots 0 ... nf
        const SimPhaseTimer timer{c, c->kernel_timing && i == 0};
        const size_t ns = ch.nf, cells = ns * S;
        // samples: the first chunk renders its slot 0 too, every other one inherits it from the chunk before
        if (i) HIP_TRY(c, hipMemcpyAsync(B.frames.p, B.frames.as<double>() + per * S, S * sizeof(double), hipMemcpyDeviceToDevice, s));
        const size_t r0 = i ? 1 : 0, nr = ns + 1 - r0;      // rendered: the slots r0 ... ns
        HIP_TRY(c, hipMemsetAsync(B.outside.p, 0, nr * sizeof(unsigned long long), s));
        ViewParams V{c->d_lut.as<double>(), B.pose.as<double>() + (size_t)kPoseStride * (ch.f0 + r0), plane, (int)S, c->W, c->H, c->fx, c->fy, c->cx, c->cy, sim_outside_mark(), 0.0, 1.0,
                     B.frames.as<double>() + r0 * S, nullptr, nullptr, B.outside.as<unsigned long long>()};
        HIP_TRY(c, timer.start(0));
        hipLaunchKernelGGL(emba_view_kernel, dim3(nblocks(S, kViewThreads), (unsigned)nr), dim3(kViewThreads), 0, s, V);
        HIP_TRY(c, timer.stop(0));
        // pass 1: events per (step, pixel), the state behind the chunk, the sums
        SimParams P{};
        P.frames = B.frames.as<double>(); P.step_t = B.step_t.as<int64_t>() + ch.f0; P.S = (int)S; P.ns = (int)ns; P.first = i == 0;
        P.c_on = c_on; P.c_off = c_off; P.max_per_step = max_per_step;
        P.ref_in = B.ref[cur].as<double>(); P.armed_in = B.armed[cur].as<uint8_t>(); P.ref_out = B.ref[cur ^ 1].as<double>(); P.armed_out = B.armed[cur ^ 1].as<uint8_t>();
        P.cells = B.cells.as<uint32_t>(); P.sums = B.sums.as<unsigned long long>();
        HIP_TRY(c, timer.start(1));
        hipLaunchKernelGGL(emba_sim_count_kernel, dim3(nblocks(S, kSimThreads)), dim3(kSimThreads), 0, s, P);
        HIP_TRY(c, timer.stop(1));
        HIP_TRY(c, hipGetLastError());
        // offsets in (step, pixel, k) order; the chunk's total, one word
        HIP_TRY(c, timer.start(2));
        SEQ_TRY(dev_scan(c, P.cells, P.cells, cells, B.total.as<uint32_t>()));
        HIP_TRY(c, timer.stop(2));
        uint32_t h_tot = 0;
        HIP_TRY(c, hipMemcpyAsync(&h_tot, B.total.p, 4, hipMemcpyDeviceToHost, s));
        HIP_TRY(c, hipStreamSynchronize(s));
        const uint64_t base = n_needed;
        n_needed += h_tot;
        if (n_needed > limit) over = true;
        if (!over && h_tot) {
            // pass 2: the same walk from the same state writes the events at their offsets; the stable sort puts them in time order
            const size_t n = h_tot, lim = (size_t)limit;
            SEQ_TRY(sim_grow(c, B.x2, base * 2, (base + n) * 2, lim * 2));
            SEQ_TRY(sim_grow(c, B.y2, base * 2, (base + n) * 2, lim * 2));
            SEQ_TRY(sim_grow(c, B.pol2, base, base + n, lim));
            SEQ_TRY(sim_grow(c, B.t2, base * 8, (base + n) * 8, lim * 8));
            SEQ_TRY(ensure_sort_pairs(c, n));
            SEQ_TRY(ensure<int64_t>(c, B.ev_t, n));
            SEQ_TRY(ensure<uint32_t>(c, B.ev_sp, n));
            P.t_base = step_t_ns[ch.f0]; P.n_total = h_tot;
            P.key = c->ord.keys[0].as<uint32_t>(); P.val = c->ord.vals[0].as<uint32_t>(); P.t = B.ev_t.as<int64_t>(); P.sp = B.ev_sp.as<uint32_t>();
            HIP_TRY(c, timer.start(3));
            hipLaunchKernelGGL(emba_sim_emit_kernel, dim3(nblocks(S, kSimThreads)), dim3(kSimThreads), 0, s, P);
            HIP_TRY(c, timer.stop(3));
            HIP_TRY(c, hipGetLastError());
            HIP_TRY(c, timer.start(4));
            SEQ_TRY(sim_sort_and_gather(c, n, (uint64_t)step_t_ns[ch.f0 + ns] - (uint64_t)step_t_ns[ch.f0], P.t_base, (size_t)base));
            HIP_TRY(c, timer.stop(4));
        } else if (timer.on) {      // (nothing to emit: the two phases are empty intervals)
            for (int ph = 3; ph < 5; ++ph) { HIP_TRY(c, timer.start(ph)); HIP_TRY(c, timer.stop(ph)); }
        }
        cur ^= 1;
    }
    unsigned long long sums[4] = {0, 0, 0, 0};
    HIP_TRY(c, hipMemcpyAsync(sums, B.sums.p, sizeof sums, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipStreamSynchronize(s));
    if (over) {
        if (stats) stats[0] = n_needed;
        return fail(c, EMBA_ERR_CAPACITY, "the recording has %llu events, more than the %llu allowed", (unsigned long long)n_needed, (unsigned long long)limit);
    }
    // the recording is whole: it replaces the one before
    std::swap(B.x, B.x2); std::swap(B.y, B.y2); std::swap(B.pol, B.pol2); std::swap(B.t, B.t2);
    B.n = (size_t)n_needed; B.have = true;
    B.stats[0] = n_needed; B.stats[1] = sums[0]; B.stats[2] = sums[1]; B.stats[3] = sums[2];
    if (stats) for (int k = 0; k < 4; ++k) stats[k] = B.stats[k];
    return EMBA_OK;
}

extern "C" emba_status emba_sim_size(const emba_ctx* c, size_t* n)
{
    if (!c || !n) return EMBA_ERR_INVALID_ARG;
    if (!c->sim.have) return fail(const_cast<emba_ctx*>(c), EMBA_ERR_STATE, "no simulated recording (emba_simulate_events first)");
    *n = c->sim.n;
    return EMBA_OK;
}

extern "C" emba_status emba_sim_get(emba_ctx* c, size_t beg, size_t end, uint16_t* x, uint16_t* y, uint8_t* pol, int64_t* t_ns)
{
    if (!c) return EMBA_ERR_INVALID_ARG;
    if (!c->sim.have) return fail(c, EMBA_ERR_STATE, "no simulated recording (emba_simulate_events first)");
    if (beg > end || end > c->sim.n) return fail(c, EMBA_ERR_INVALID_ARG, "[%zu, %zu) is not a range of the simulated recording of %zu events", beg, end, c->sim.n);
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    const size_t m = end - beg;
    if (x) SEQ_TRY(d2h_pageable(c, x, c->sim.x.as<uint16_t>() + beg, m * 2));
    if (y) SEQ_TRY(d2h_pageable(c, y, c->sim.y.as<uint16_t>() + beg, m * 2));
    if (pol) SEQ_TRY(d2h_pageable(c, pol, c->sim.pol.as<uint8_t>() + beg, m));
    if (t_ns) SEQ_TRY(d2h_pageable(c, t_ns, c->sim.t.as<int64_t>() + beg, m * 8));
    return EMBA_OK;
}

// emba_seq_upload with the simulator's arrays as the source: the same checks, the same ingest kernel (one launch over the whole recording: every event has
// its predecessor in device memory), the same ends.
extern "C" emba_status emba_seq_from_sim(emba_ctx* c, int32_t sampling_rate, size_t* n_kept_out)
{
    if (!c) return EMBA_ERR_INVALID_ARG;
    if (!c->sim.have) return fail(c, EMBA_ERR_STATE, "no simulated recording (emba_simulate_events first)");
    const size_t n = c->sim.n;
    if (n >= 0xFFFFFFFFull) return fail(c, EMBA_ERR_INVALID_ARG, "too many events for 32-bit indices");
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t rate = sampling_stride(sampling_rate), n_kept = sampled_count(n, sampling_rate);
    SEQ_TRY(seq_ingest_begin(c, n_kept));
    if (n) {
        hipLaunchKernelGGL(emba_seq_ingest_kernel, dim3(nblocks(n)), dim3(256), 0, c->stream, (const int64_t*)c->sim.t.as<int64_t>(), (const uint16_t*)c->sim.x.as<uint16_t>(),
                           (const uint16_t*)c->sim.y.as<uint16_t>(), (const uint8_t*)c->sim.pol.as<uint8_t>(), (long)n, 0L, (int64_t)0, c->sw, c->sh, (long)rate, (long)n_kept,
                           c->evseq.x.as<uint16_t>(), c->evseq.y.as<uint16_t>(), c->evseq.pol.as<uint8_t>(), c->evseq.t.as<int64_t>(), c->evseq.status.as<uint32_t>());
        HIP_TRY(c, hipGetLastError());
    }
    return seq_ingest_finish(c, n_kept, n_kept_out);
}
