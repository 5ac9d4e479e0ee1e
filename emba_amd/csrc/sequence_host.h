// emba_amd/csrc/sequence_host.h — the resident event sequence of a sliding-window run, as host code over the kernels of sequence_kernels.h: the upload
// (emba_seq_upload), the event window (emba_seq_window), the registration of a window or of a time shard of one with its halo built on the device
// (emba_set_events_seq[_shard], emba_seq_halo), the sensor-noise filters (emba_seq_filter, emba_seq_hot_pixels) and the downloads.  What is plain arithmetic —
// the layouts of a chunk and of a halo, the window behind the probes, the hot-pixel threshold, what a filter call has to do — is decided in sequence_rule.h;
// here are the buffers, the launches, the state (emba_ctx::evseq) and the C ABI.
// Part of emba_hip.hip's translation unit, included by it below the helpers this file needs (order_host.h: dev_scan, dev_sort and their scratch,
// emba_set_events_dev; transfer_host.h: ensure_stage, d2h_pageable) and above the group host, which calls it on every rank.
#pragma once
#include "context.h"
#include "sequence_kernels.h"
#include "sequence_rule.h"

using namespace emba;

#define SEQ_TRY(call) do { if (const emba_status st_ = (call)) return st_; } while (0)

// Raw events per upload chunk, laid out [t | x | y | pol] in a pinned staging buffer (6.5 of its 8 MB).
namespace {
constexpr size_t kSeqChunk = (size_t)1 << 19;
constexpr SeqChunkLayout kSeqRaw(kSeqChunk);
static_assert(kSeqRaw.bytes <= kStageBytes, "an upload chunk must fit a staging buffer");
}  // namespace

extern "C" emba_status emba_seq_free(emba_ctx* c)
{
    if (!c) return EMBA_ERR_INVALID_ARG;
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    c->evseq.reset();
    c->priors.reset();      // (votes of that sequence's events)
    return EMBA_OK;
}

extern "C" emba_status emba_seq_size(const emba_ctx* c, size_t* n)
{
    if (!c || !n) return EMBA_ERR_INVALID_ARG;
    *n = c->evseq.n;
    return EMBA_OK;
}

namespace {
// The two ends of an ingest of n raw events into the resident sequence, whatever memory they come from (emba_seq_upload: the caller's; emba_seq_from_sim:
// the simulator's).  Begin: the stream drained, the sequence that goes and its contrast priors dropped, the arrays of the n_kept events and the status
// words ready (0xFF: clean).  Finish: the ingest kernel's two words read; the sequence is resident when both are clean.
emba_status seq_ingest_begin(emba_ctx* c, size_t n_kept)
{
    hipStream_t s = c->stream;
    HIP_TRY(c, hipStreamSynchronize(s));
    c->evseq.n = 0; c->evseq.have = false;      // (a second upload replaces the first; a failed one leaves none)
    c->priors.drop();                           // (the contrast priors are votes of the sequence that goes)
    emba_status st;
    if ((st = ensure<uint32_t>(c, c->evseq.status, kStatusWords)) ||
        (st = ensure<uint16_t>(c, c->evseq.x, std::max<size_t>(n_kept, 1))) || (st = ensure<uint16_t>(c, c->evseq.y, std::max<size_t>(n_kept, 1))) ||
        (st = ensure<uint8_t>(c, c->evseq.pol, std::max<size_t>(n_kept, 1))) || (st = ensure<int64_t>(c, c->evseq.t, std::max<size_t>(n_kept, 1))))
        return st;
    HIP_TRY(c, hipMemsetAsync(c->evseq.status.p, 0xFF, kStatusWords * 4, s));      // (the ingest kernel writes kStFirstBad, kStUnsorted)
    return EMBA_OK;
}

emba_status seq_ingest_finish(emba_ctx* c, size_t n_kept, size_t* n_kept_out)
{
    hipStream_t s = c->stream;
    uint32_t h_err[2];
    HIP_TRY(c, hipMemcpyAsync(h_err, c->evseq.status.p, sizeof h_err, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipStreamSynchronize(s));
    if (h_err[kStFirstBad] != 0xFFFFFFFFu) return fail(c, EMBA_ERR_INVALID_ARG, "event %u lies outside the %dx%d sensor", h_err[kStFirstBad], c->sw, c->sh);
    if (h_err[kStUnsorted] != 0xFFFFFFFFu) return fail(c, EMBA_ERR_INVALID_ARG, "timestamps not sorted at event %u", h_err[kStUnsorted]);
    c->evseq.n = n_kept; c->evseq.have = true;
    if (n_kept_out) *n_kept_out = n_kept;
    return EMBA_OK;
}
}  // namespace

extern "C" emba_status emba_seq_upload(emba_ctx* c, const uint16_t* x, const uint16_t* y, const uint8_t* pol, const int64_t* t_ns, size_t n, int32_t sampling_rate,
                                       size_t* n_kept_out)
{
    if (!c) return EMBA_ERR_INVALID_ARG;
    if (n && (!x || !y || !pol || !t_ns)) return fail(c, EMBA_ERR_INVALID_ARG, "event arrays are NULL");
    if (n >= 0xFFFFFFFFull) return fail(c, EMBA_ERR_INVALID_ARG, "too many events for 32-bit indices");
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t s = c->stream;
    const size_t rate = sampling_stride(sampling_rate), n_kept = sampled_count(n, sampling_rate);
    SEQ_TRY(seq_ingest_begin(c, n_kept));
    SEQ_TRY(ensure_stage(c));
    SEQ_TRY(ensure<uint8_t>(c, c->evseq.raw, kSeqRaw.bytes));
    uint32_t* d_err = c->evseq.status.as<uint32_t>();
    uint8_t* raw = c->evseq.raw.as<uint8_t>();
    for (size_t k0 = 0, i = 0; k0 < n; k0 += kSeqChunk, ++i) {
        const size_t m = std::min(kSeqChunk, n - k0);
        uint8_t* h = static_cast<uint8_t*>(c->h_stage[i & 1]);
        HIP_TRY(c, hipEventSynchronize(c->stage_ev[i & 1]));      // the transfer that last used this staging buffer has completed
        std::memcpy(h, t_ns + k0, m * 8); std::memcpy(h + kSeqRaw.x, x + k0, m * 2); std::memcpy(h + kSeqRaw.y, y + k0, m * 2); std::memcpy(h + kSeqRaw.pol, pol + k0, m);
        // (one stream: the copy of chunk i + 1 into `raw` is ordered behind the kernel that reads chunk i)
        HIP_TRY(c, hipMemcpyAsync(raw, h, m * 8, hipMemcpyHostToDevice, s));
        HIP_TRY(c, hipMemcpyAsync(raw + kSeqRaw.x, h + kSeqRaw.x, m * 2, hipMemcpyHostToDevice, s));
        HIP_TRY(c, hipMemcpyAsync(raw + kSeqRaw.y, h + kSeqRaw.y, m * 2, hipMemcpyHostToDevice, s));
        HIP_TRY(c, hipMemcpyAsync(raw + kSeqRaw.pol, h + kSeqRaw.pol, m, hipMemcpyHostToDevice, s));
        HIP_TRY(c, hipEventRecord(c->stage_ev[i & 1], s));
        hipLaunchKernelGGL(emba_seq_ingest_kernel, dim3(nblocks(m)), dim3(256), 0, s, reinterpret_cast<const int64_t*>(raw), reinterpret_cast<const uint16_t*>(raw + kSeqRaw.x),
                           reinterpret_cast<const uint16_t*>(raw + kSeqRaw.y), (const uint8_t*)(raw + kSeqRaw.pol), (long)m, (long)k0, k0 ? t_ns[k0 - 1] : (int64_t)0, c->sw, c->sh,
                           (long)rate, (long)n_kept, c->evseq.x.as<uint16_t>(), c->evseq.y.as<uint16_t>(), c->evseq.pol.as<uint8_t>(), c->evseq.t.as<int64_t>(), d_err);
        HIP_TRY(c, hipGetLastError());
    }
    return seq_ingest_finish(c, n_kept, n_kept_out);
}

// getEventSubset: the kernel finds the first probe past either cursor, sequence_rule.h (seq_window) makes the window of them
extern "C" emba_status emba_seq_window(emba_ctx* c, int64_t t_beg_ns, int64_t t_end_ns, size_t* beg_out, size_t* end_out)
{
    if (!c || !beg_out || !end_out) return c ? fail(c, EMBA_ERR_INVALID_ARG, "beg/end NULL") : EMBA_ERR_INVALID_ARG;
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t s = c->stream;
    const size_t n = c->evseq.n, m = (n + kSeqProbe - 1) / kSeqProbe;
    const SeqCursors cur = seq_window_cursors(t_beg_ns, t_end_ns);
    uint32_t h_res[2] = {kNoProbe, kNoProbe};
    if (m) {
        SEQ_TRY(ensure<uint32_t>(c, c->evseq.status, kStatusWords));
        uint32_t* d_res = c->evseq.status.as<uint32_t>();
        HIP_TRY(c, hipMemsetAsync(d_res, 0xFF, sizeof h_res, s));      // kStProbeA, kStProbeB
        hipLaunchKernelGGL(emba_seq_window_kernel, dim3((unsigned)std::min<size_t>(nblocks(m), 1024)), dim3(256), 0, s, (const int64_t*)c->evseq.t.as<int64_t>(), (long)n, cur.a, cur.b, d_res);
        HIP_TRY(c, hipGetLastError());
        HIP_TRY(c, hipMemcpyAsync(h_res, d_res, sizeof h_res, hipMemcpyDeviceToHost, s));
        HIP_TRY(c, hipStreamSynchronize(s));
    }
    const SeqWindow w = seq_window(n, h_res[kStProbeA], h_res[kStProbeB], kSeqProbe);
    if (w.status == SeqWindowStatus::stops_at_first_probe)
        return fail(c, EMBA_ERR_INVALID_ARG, "window holds no events (the tail search stops at its first probe, event %zu)", w.beg);
    if (w.status == SeqWindowStatus::begins_behind_last) return fail(c, EMBA_ERR_INVALID_ARG, "window holds no events (it begins behind the last event)");
    *beg_out = w.beg; *end_out = w.end;
    return EMBA_OK;
}

extern "C" emba_status emba_set_events_seq(emba_ctx* c, size_t beg, size_t end)
{
    if (!c) return EMBA_ERR_INVALID_ARG;
    if (beg > end || end > c->evseq.n) return fail(c, EMBA_ERR_INVALID_ARG, "[%zu, %zu) is not a range of the resident sequence of %zu events", beg, end, c->evseq.n);
    return emba_set_events_dev(c, c->evseq.x.as<uint16_t>() + beg, c->evseq.y.as<uint16_t>() + beg, c->evseq.pol.as<uint8_t>() + beg, c->evseq.t.as<int64_t>() + beg, end - beg,
                               nullptr, nullptr, nullptr, 0);
}

namespace {
// The halo of the time shard that begins at `lo` of the window that begins at win_beg (sequence_kernels.h: emba_halo_*), into ord.halo in the layout
// emba_set_events stages (HaloLayout of *n_halo entries).  The sequence was checked at its upload: every pixel lies inside the sensor, so
// inside the table.  One small read: the count, which places hx / hy behind the times.  Scratch of its own (evseq) + dev_scan's.
emba_status build_seq_halo(emba_ctx* c, size_t win_beg, size_t lo, size_t* n_halo)
{
    hipStream_t s = c->stream;
    const size_t m = lo - win_beg;
    *n_halo = 0;
    if (!m) return EMBA_OK;
    if (m > 0x7FFFFFFFull) return fail(c, EMBA_ERR_INVALID_ARG, "too many events in front of the shard for 32-bit indices");
    emba_status st;
    if ((st = ensure<int32_t>(c, c->evseq.halo_last, c->S)) || (st = ensure<uint32_t>(c, c->evseq.halo_flag, m)) || (st = ensure<uint32_t>(c, c->evseq.halo_pos, m)) ||
        (st = ensure<uint32_t>(c, c->evseq.status, kStatusWords)))
        return st;
    const uint16_t *x = c->evseq.x.as<uint16_t>() + win_beg, *y = c->evseq.y.as<uint16_t>() + win_beg;
    const int64_t* t = c->evseq.t.as<int64_t>() + win_beg;
    int32_t* last = c->evseq.halo_last.as<int32_t>();
    uint32_t *flag = c->evseq.halo_flag.as<uint32_t>(), *pos = c->evseq.halo_pos.as<uint32_t>(), *d_tot = c->evseq.status.as<uint32_t>() + kStTotal;
    HIP_TRY(c, hipMemsetAsync(last, 0xFF, c->S * sizeof(int32_t), s));      // -1: no event of this pixel
    hipLaunchKernelGGL(emba_halo_last_kernel, dim3(nblocks(m)), dim3(256), 0, s, x, y, (long)m, c->sw, last);
    hipLaunchKernelGGL(emba_halo_flag_kernel, dim3(nblocks(m)), dim3(256), 0, s, x, y, (long)m, c->sw, (const int32_t*)last, flag);
    if ((st = dev_scan(c, flag, pos, m, d_tot))) return st;
    uint32_t h_tot = 0;
    HIP_TRY(c, hipMemcpyAsync(&h_tot, d_tot, sizeof h_tot, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipStreamSynchronize(s));
    if (h_tot > c->S) return fail(c, EMBA_ERR_STATE, "halo of %u entries on a sensor of %zu pixels", h_tot, c->S);
    const size_t n = h_tot;
    const HaloLayout halo(n);
    if ((st = ensure<uint8_t>(c, c->ord.halo, halo.bytes))) return st;
    hipLaunchKernelGGL(emba_halo_gather_kernel, dim3(nblocks(m)), dim3(256), 0, s, x, y, t, (long)m, (const uint32_t*)flag, (const uint32_t*)pos, halo.hx_in(c->ord.halo.p),
                       halo.hy_in(c->ord.halo.p), halo.hbt_in(c->ord.halo.p));
    HIP_TRY(c, hipGetLastError());
    *n_halo = n;
    return EMBA_OK;
}

emba_status check_seq_shard(emba_ctx* c, size_t win_beg, size_t lo, size_t hi)
{
    switch (seq_shard_ok(win_beg, lo, hi, c->evseq.n)) {
    case SeqShardStatus::not_a_range:
        return fail(c, EMBA_ERR_INVALID_ARG, "[%zu, %zu) of the window at %zu is not a range of the resident sequence of %zu events", lo, hi, win_beg, c->evseq.n);
    case SeqShardStatus::off_grid:
        return fail(c, EMBA_ERR_INVALID_ARG, "the shard begins %zu events behind its window: not on the window's batch grid", lo - win_beg);
    case SeqShardStatus::ok: break;
    }
    return EMBA_OK;
}
}  // namespace

extern "C" emba_status emba_set_events_seq_shard(emba_ctx* c, size_t win_beg, size_t lo, size_t hi)
{
    if (!c) return EMBA_ERR_INVALID_ARG;
    emba_status st;
    if ((st = check_seq_shard(c, win_beg, lo, hi))) return st;      // (before anything of the registered window is touched)
    HIP_TRY(c, hipSetDevice(c->device));
    const auto t_begin = std::chrono::steady_clock::now();
    size_t n_halo = 0;
    if ((st = build_seq_halo(c, win_beg, lo, &n_halo))) return st;
    const HaloLayout halo(n_halo);
    void* base = c->ord.halo.p;
    st = emba_set_events_dev(c, c->evseq.x.as<uint16_t>() + lo, c->evseq.y.as<uint16_t>() + lo, c->evseq.pol.as<uint8_t>() + lo, c->evseq.t.as<int64_t>() + lo, hi - lo,
                             n_halo ? halo.hx_in(base) : nullptr, n_halo ? halo.hy_in(base) : nullptr, n_halo ? halo.hbt_in(base) : nullptr, n_halo);
    c->set_events_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_begin).count();      // the halo passes included
    return st;
}

extern "C" emba_status emba_seq_halo(emba_ctx* c, size_t win_beg, size_t lo, uint16_t* hx, uint16_t* hy, int64_t* hbt, size_t cap, size_t* n_halo)
{
    if (!c || !n_halo) return c ? fail(c, EMBA_ERR_INVALID_ARG, "n_halo NULL") : EMBA_ERR_INVALID_ARG;
    emba_status st;
    if ((st = check_seq_shard(c, win_beg, lo, lo))) return st;
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    size_t n = 0;
    if ((st = build_seq_halo(c, win_beg, lo, &n))) return st;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    *n_halo = n;
    if (!hx && !hy && !hbt) return EMBA_OK;
    if (cap < n) return fail(c, EMBA_ERR_CAPACITY, "the halo has %zu entries, the arrays hold %zu", n, cap);
    const HaloLayout halo(n);
    void* base = c->ord.halo.p;
    if (n && hbt && (st = d2h_pageable(c, hbt, halo.hbt_in(base), n * 8))) return st;
    if (n && hx && (st = d2h_pageable(c, hx, halo.hx_in(base), n * 2))) return st;
    if (n && hy && (st = d2h_pageable(c, hy, halo.hy_in(base), n * 2))) return st;
    return EMBA_OK;
}

extern "C" emba_status emba_seq_get(emba_ctx* c, size_t beg, size_t end, uint16_t* x, uint16_t* y, uint8_t* pol, int64_t* t_ns)
{
    if (!c) return EMBA_ERR_INVALID_ARG;
    if (beg > end || end > c->evseq.n) return fail(c, EMBA_ERR_INVALID_ARG, "[%zu, %zu) is not a range of the resident sequence of %zu events", beg, end, c->evseq.n);
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    const size_t m = end - beg;
    emba_status st;
    if (x && (st = d2h_pageable(c, x, c->evseq.x.as<uint16_t>() + beg, m * 2))) return st;
    if (y && (st = d2h_pageable(c, y, c->evseq.y.as<uint16_t>() + beg, m * 2))) return st;
    if (pol && (st = d2h_pageable(c, pol, c->evseq.pol.as<uint8_t>() + beg, m))) return st;
    if (t_ns && (st = d2h_pageable(c, t_ns, c->evseq.t.as<int64_t>() + beg, m * 8))) return st;
    return EMBA_OK;
}

// ---- sensor-noise filters on the resident sequence (sequence_kernels.h: emba_filter_*; the rule: include/emba_hip.h) ------------------------------
// Scratch: the sort pairs, flags and positions of the order preparation (ord.keys / vals / flags / pos, + dev_scan's and dev_sort's) — a registered window
// keeps nothing in them: set_events_core copies what it sorted into the pm-order arrays, prepare_order into the device order and the record slots, and a
// re-binning rebuilds all of it from the pm-order.  What has to outlive the call (starts, hot mask, counters, the fresh arrays) is evseq's own.
namespace {

// What one phase of a filter call leaves for the next: where the pixel-sorted sequence and the keep-flags lie, and what the host has read so far
struct FilterPass {
    const uint32_t *keys = nullptr, *vals = nullptr;      // the sequence sorted by (pixel, index): pixel keys and event indices
    const uint32_t *keep = nullptr, *pos = nullptr;       // keep-flag per event and its exclusive scan (nullptr: every event survives)
    unsigned long long sums[8] = {0, 0, 0, 0, 0, 0, 0, 0};   // f_sums as last read: [0] pixels with events [1] sum c^2 [2] hot pixels [3] their events [4] refractory [5] support
    size_t n_surv = 0;
};

// Everything that can fail for want of memory comes first — the scratch of the sort and of the scans included, and the fresh arrays at their upper bound
// n / rate — so that a failure leaves the sequence AND the previous filter's hot mask as they were.
emba_status filter_reserve(emba_ctx* c, const FilterPlan& plan)
{
    SEQ_TRY(ensure<uint8_t>(c, c->evseq.f_hot, plan.S));
    SEQ_TRY(ensure<uint64_t>(c, c->evseq.f_sums, 8));
    SEQ_TRY(ensure<uint32_t>(c, c->evseq.status, kStatusWords));
    if (plan.sorts) {
        SEQ_TRY(ensure_sort_pairs(c, plan.n));
        SEQ_TRY(ensure<uint32_t>(c, c->ord.flags, plan.n));
        SEQ_TRY(ensure<uint32_t>(c, c->ord.pos, plan.n));
        SEQ_TRY(ensure<uint32_t>(c, c->evseq.f_start, plan.S + 1));
        SEQ_TRY(ensure_sort_scratch(c, plan.n));
        SEQ_TRY(ensure_scan_scratch(c, plan.n));
    }
    if (plan.rewrites) {
        SEQ_TRY(ensure<uint16_t>(c, c->evseq.x2, plan.n_fresh));
        SEQ_TRY(ensure<uint16_t>(c, c->evseq.y2, plan.n_fresh));
        SEQ_TRY(ensure<uint8_t>(c, c->evseq.pol2, plan.n_fresh));
        SEQ_TRY(ensure<int64_t>(c, c->evseq.t2, plan.n_fresh));
    }
    return EMBA_OK;
}

// one stable sort by sensor pixel, and where every pixel's events begin in it (f_start)
emba_status filter_sort_by_pixel(emba_ctx* c, const FilterPlan& plan, FilterPass* f)
{
    hipStream_t s = c->stream;
    const size_t n = plan.n;
    uint32_t *k0 = c->ord.keys[0].as<uint32_t>(), *v0 = c->ord.vals[0].as<uint32_t>(), *k1 = c->ord.keys[1].as<uint32_t>(), *v1 = c->ord.vals[1].as<uint32_t>();
    hipLaunchKernelGGL(emba_pixel_keys_kernel, dim3(nblocks(n)), dim3(256), 0, s, (const uint16_t*)c->evseq.x.as<uint16_t>(), (const uint16_t*)c->evseq.y.as<uint16_t>(), (long)n, c->sw,
                       (const uint16_t*)nullptr, (const uint16_t*)nullptr, 0L, k0, v0);
    SEQ_TRY(dev_sort(c, &k0, &v0, &k1, &v1, n, bits_for(plan.S)));
    hipLaunchKernelGGL(emba_filter_starts_kernel, dim3(nblocks(n)), dim3(256), 0, s, (const uint32_t*)k0, (long)n, (long)plan.S, c->evseq.f_start.as<uint32_t>());
    f->keys = k0; f->vals = v0;
    return EMBA_OK;
}

// the hot-pixel test: the sums over the pixels with events, one 16-byte read, the threshold on the host, the mask
emba_status filter_hot_pixels(emba_ctx* c, const FilterPlan& plan, double hot_sigma, FilterPass* f)
{
    hipStream_t s = c->stream;
    const uint32_t* start = c->evseq.f_start.as<uint32_t>();
    unsigned long long* d_sums = c->evseq.f_sums.as<unsigned long long>();
    const unsigned grid = (unsigned)std::min<size_t>(nblocks(plan.S), 1024);
    hipLaunchKernelGGL(emba_filter_pixel_sums_kernel, dim3(grid), dim3(256), 0, s, start, (long)plan.S, d_sums);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(f->sums, d_sums, 16, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipStreamSynchronize(s));
    if (!f->sums[0]) return fail(c, EMBA_ERR_STATE, "emba_seq_filter: %zu events on no pixel", plan.n);
    const double thr = hot_threshold(plan.n, f->sums[0], f->sums[1], hot_sigma);
    hipLaunchKernelGGL(emba_filter_hot_kernel, dim3(grid), dim3(256), 0, s, start, (long)plan.S, thr, c->evseq.f_hot.as<uint8_t>(), d_sums);
    return EMBA_OK;
}

// keep-flags per event, their scan, and the one read of the survivors' number and of the counters
emba_status filter_flag_and_count(emba_ctx* c, const FilterPlan& plan, int64_t refractory_ns, int64_t support_ns, FilterPass* f)
{
    hipStream_t s = c->stream;
    const size_t n = plan.n;
    uint32_t *keep = c->ord.flags.as<uint32_t>(), *pos = c->ord.pos.as<uint32_t>(), *d_tot = c->evseq.status.as<uint32_t>() + kStCounter;
    unsigned long long* d_sums = c->evseq.f_sums.as<unsigned long long>();
    hipLaunchKernelGGL(emba_filter_flags_kernel, dim3(nblocks(n)), dim3(256), 0, s, f->keys, f->vals, (const int64_t*)c->evseq.t.as<int64_t>(), (long)n, c->sw, c->sh,
                       (const uint32_t*)c->evseq.f_start.as<uint32_t>(), (const uint8_t*)c->evseq.f_hot.as<uint8_t>(), refractory_ns, support_ns, keep, d_sums);
    HIP_TRY(c, hipGetLastError());
    SEQ_TRY(dev_scan(c, keep, pos, n, d_tot));
    uint32_t h_tot = 0;
    HIP_TRY(c, hipMemcpyAsync(&h_tot, d_tot, 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipMemcpyAsync(f->sums, d_sums, 64, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipStreamSynchronize(s));
    if (h_tot > n) return fail(c, EMBA_ERR_STATE, "emba_seq_filter: %u survivors of %zu events", h_tot, n);
    f->n_surv = h_tot; f->keep = keep; f->pos = pos;
    return EMBA_OK;
}

// every rate-th survivor into the fresh arrays, which then become the sequence
emba_status filter_rewrite(emba_ctx* c, const FilterPlan& plan, const FilterPass& f, size_t n_kept)
{
    hipStream_t s = c->stream;
    if (n_kept) {
        hipLaunchKernelGGL(emba_filter_gather_kernel, dim3(nblocks(plan.n)), dim3(256), 0, s, (const uint16_t*)c->evseq.x.as<uint16_t>(), (const uint16_t*)c->evseq.y.as<uint16_t>(),
                           (const uint8_t*)c->evseq.pol.as<uint8_t>(), (const int64_t*)c->evseq.t.as<int64_t>(), (long)plan.n, f.keep, f.pos, (long)plan.rate, (long)n_kept,
                           c->evseq.x2.as<uint16_t>(), c->evseq.y2.as<uint16_t>(), c->evseq.pol2.as<uint8_t>(), c->evseq.t2.as<int64_t>());
        HIP_TRY(c, hipGetLastError());
        HIP_TRY(c, hipStreamSynchronize(s));
        std::swap(c->evseq.x, c->evseq.x2); std::swap(c->evseq.y, c->evseq.y2); std::swap(c->evseq.pol, c->evseq.pol2); std::swap(c->evseq.t, c->evseq.t2);
    }
    c->evseq.n = n_kept;
    if (!n_kept) c->evseq.have = false;      // every event removed: emba_seq_filter finds no sequence until the next upload (the other calls see n = 0)
    return EMBA_OK;
}

}  // namespace

extern "C" emba_status emba_seq_filter(emba_ctx* c, double hot_sigma, int64_t refractory_ns, int64_t support_ns, int32_t sampling_rate, uint64_t* stats)
{
    if (!c) return EMBA_ERR_INVALID_ARG;
    if (!c->evseq.have) return fail(c, EMBA_ERR_STATE, "no resident sequence (emba_seq_upload first)");
    if (std::isnan(hot_sigma)) return fail(c, EMBA_ERR_INVALID_ARG, "hot_sigma is NaN");
    const size_t n = c->evseq.n;
    if (n >= 0x100000000ull) return fail(c, EMBA_ERR_INVALID_ARG, "emba_seq_filter: %zu events are too many for the 32-bit event indices of its sort (limit 2^32 - 1)", n);
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t s = c->stream;
    HIP_TRY(c, hipStreamSynchronize(s));
    const FilterPlan plan(n, c->S, hot_sigma, refractory_ns, support_ns, sampling_rate);
    SEQ_TRY(filter_reserve(c, plan));
    c->priors.drop();              // (the events are re-indexed: the contrast priors are votes of the sequence as it was)
    c->evseq.have_hot = false;     // (from here on the mask is this filter's: all zero unless the hot test below runs)
    HIP_TRY(c, hipMemsetAsync(c->evseq.f_hot.p, 0, plan.S, s));
    HIP_TRY(c, hipMemsetAsync(c->evseq.f_sums.p, 0, 64, s));
    FilterPass f;
    f.n_surv = n;
    if (plan.sorts) {
        SEQ_TRY(filter_sort_by_pixel(c, plan, &f));
        if (plan.hot_on) SEQ_TRY(filter_hot_pixels(c, plan, hot_sigma, &f));
        SEQ_TRY(filter_flag_and_count(c, plan, refractory_ns, support_ns, &f));
    }
    const size_t n_kept = f.n_surv / plan.rate;
    if (plan.rewrites) SEQ_TRY(filter_rewrite(c, plan, f, n_kept));
    c->evseq.have_hot = true;
    if (stats) {
        stats[0] = n; stats[1] = f.sums[2]; stats[2] = f.sums[3]; stats[3] = f.sums[4]; stats[4] = f.sums[5]; stats[5] = n_kept;
    }
    return EMBA_OK;
}

extern "C" emba_status emba_seq_hot_pixels(emba_ctx* c, uint8_t* mask_host)
{
    if (!c) return EMBA_ERR_INVALID_ARG;
    if (!mask_host) return fail(c, EMBA_ERR_INVALID_ARG, "mask NULL");
    if (!c->evseq.have_hot) return fail(c, EMBA_ERR_STATE, "no filter has run on this context (emba_seq_filter first)");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return d2h_pageable(c, mask_host, c->evseq.f_hot.as<uint8_t>(), c->S);
}
