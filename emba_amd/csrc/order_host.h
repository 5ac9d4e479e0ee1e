// emba_amd/csrc/order_host.h — the once-per-window path, as host code over the kernels of order_kernels.h: the registration of a window
// (emba_set_events[_dev], set_events_core), the device scan and sort with their scratch, the order preparation at the window's first evaluation
// (prepare_order, phase by phase) and the accessors that report what the last registration and order decision saw.  The host arithmetic that decides the
// order is order_rule.h (tested on the CPU); here are the buffers, the launches, the state (emba_ctx::win, emba_ctx::order) and the C ABI.
// Part of emba_hip.hip's translation unit, included by it above emba_create / emba_destroy (free_window) and above the step path, the sequence and the
// group, which call prepare_order, size_record_set, dev_scan, dev_sort and emba_set_events_dev.
#pragma once
#include "context.h"
#include "order_kernels.h"
#include "sequence_rule.h"

#include <chrono>

using namespace emba;

namespace {

// A new device order (a new window, or the window is ordered again): nothing of the previous one is kept but the shape and grid of the last tile search,
// which emba_last_tile_geometry reports until another search runs.
OrderState new_order(const OrderState& prev)
{
    OrderState o{};
    o.tile_shape = prev.tile_shape; o.tile_fine = prev.tile_fine;
    return o;
}
void free_window(emba_ctx* c)
{   // (the buffers stay: the next window reuses them, see DevBuf)
    WindowState w{};
    w.last_rebin_stamp = c->rec_stamp - 3;   // a new window may be re-binned at its first drifted evaluation
    w.n_rebin = c->win.n_rebin;              // emba_last_tile_drift counts the re-binnings of the context, not of a window
    // until set_events_core takes the next window (a registration may fail before): emba_event_counts, emba_last_setup_ms and emba_last_tile_drift go on
    // reporting the last one's sizes and drift
    w.n_used = c->win.n_used; w.n_cand = c->win.n_cand; w.n_sorted = c->win.n_sorted; w.n_outside_tile = c->win.n_outside_tile;
    c->win = w;
    OrderState o = new_order(c->order);
    // until the window's first evaluation orders it: emba_last_order_stats and emba_last_order_inlier_estimate go on reporting the last decision
    o.order_per_px = c->order.order_per_px; o.order_lead_frac = c->order.order_lead_frac; o.order_inl_pred = c->order.order_inl_pred;
    c->order = o;
    c->eq.active_done = c->eq.accum_done = false;
    // (counters of the previous window that were never resolved must not be read as this window's)
    begin_evaluation(c);
}

// ros::Time/Duration midpoint of a batch (model.cpp:116-119; rostime semantics per SURVEY Appendix A):
// integer nanoseconds plus one double scale-and-round.  Pose-independent, so it is computed once per window.
int64_t batch_mid_ns(int64_t t_first, int64_t t_last)
{
    const int64_t d = t_last - t_first;
    int64_t dsec = d / 1000000000LL, dnsec = d % 1000000000LL;
    if (dnsec < 0) { dnsec += 1000000000LL; dsec -= 1; }
    const double half = ((double)dsec + 1e-9 * (double)dnsec) * 0.5;   // Duration::toSec() * 0.5
    int64_t hsec = (int64_t)std::floor(half);
    int64_t hnsec = (int64_t)std::round((half - (double)hsec) * 1e9);  // Duration::fromSec
    hsec += hnsec / 1000000000LL;
    hnsec = hnsec % 1000000000LL;
    return t_first + hsec * 1000000000LL + hnsec;
}

// ---- device-side helpers of the once-per-window structure (order_kernels.h) ----------------------------------------------------

// The scratch of a dev_scan over n elements / of a dev_sort of n entries (its histogram, and the scan over it).  dev_scan and dev_sort reserve it themselves;
// a caller that must not fail for want of memory later on (emba_seq_filter) reserves it up front through the same two functions.
size_t scan_tiles(size_t n) { return (n + kScanTile - 1) / kScanTile; }
size_t sort_tiles(size_t n) { return (n + kSortTile - 1) / kSortTile; }
emba_status ensure_scan_scratch(emba_ctx* c, size_t n)
{
    emba_status st;
    if ((st = ensure<uint32_t>(c, c->ord.scan_sums, scan_tiles(n) + 1)) || (st = ensure<uint32_t>(c, c->ord.scan_offs, scan_tiles(n) + 2))) return st;
    return EMBA_OK;
}
emba_status ensure_sort_scratch(emba_ctx* c, size_t n)
{
    emba_status st;
    if ((st = ensure<uint32_t>(c, c->ord.sort_hist, 256 * sort_tiles(n))) || (st = ensure_scan_scratch(c, 256 * sort_tiles(n)))) return st;
    return EMBA_OK;
}

// out[i] = sum_{j<i} in[j]; total_dev[0] = sum of all (may be nullptr).  Scratch: ord.scan_sums, ord.scan_offs.
emba_status dev_scan(emba_ctx* c, const uint32_t* in, uint32_t* out, size_t n, uint32_t* total_dev, int* total_host = nullptr, const int* err_dev = nullptr, int* err_host = nullptr)
{   // (total_host / err_host: pinned, device-visible words the middle launch writes the total and the evaluation's status word to — no copy node)
    hipStream_t s = c->stream;
    const size_t ntiles = scan_tiles(n);
    emba_status st;
    if ((st = ensure_scan_scratch(c, n))) return st;
    uint32_t *sums = c->ord.scan_sums.as<uint32_t>(), *offs = c->ord.scan_offs.as<uint32_t>();
    uint32_t* tot = total_dev ? total_dev : offs + ntiles + 1;
    if (!n) { HIP_TRY(c, hipMemsetAsync(tot, 0, 4, s)); return EMBA_OK; }
    hipLaunchKernelGGL(emba_scan_tile_sums_kernel, dim3((unsigned)ntiles), dim3(256), 0, s, in, (long)n, sums);
    hipLaunchKernelGGL(emba_scan_kernel, dim3(1), dim3(256), 0, s, sums, offs, (long)ntiles, tot, total_host, err_dev, err_host);
    hipLaunchKernelGGL(emba_scan_apply_kernel, dim3((unsigned)ntiles), dim3(256), 0, s, in, (long)n, offs, out);
    HIP_TRY(c, hipGetLastError());
    return EMBA_OK;
}

// Stable LSD radix sort of (keys, vals) on the low `bits` bits of the keys; the sorted arrays end up in (*keys, *vals), the other
// pair of buffers is scratch (pointers are swapped per pass).  Scratch: ord.sort_hist (+ dev_scan's).
emba_status dev_sort(emba_ctx* c, uint32_t** keys, uint32_t** vals, uint32_t** keys_alt, uint32_t** vals_alt, size_t n, int bits)
{
    if (n < 2 || bits <= 0) return EMBA_OK;
    hipStream_t s = c->stream;
    const size_t ntiles = sort_tiles(n);
    emba_status st;
    if ((st = ensure_sort_scratch(c, n))) return st;
    uint32_t* hist = c->ord.sort_hist.as<uint32_t>();
    for (int shift = 0; shift < bits; shift += 8) {
        hipLaunchKernelGGL(emba_sort_hist_kernel, dim3(nblocks(ntiles, 4)), dim3(256), 0, s, *keys, (long)n, shift, (long)ntiles, hist);
        if ((st = dev_scan(c, hist, hist, 256 * ntiles, nullptr))) return st;
        hipLaunchKernelGGL(emba_sort_scatter_kernel, dim3(nblocks(ntiles, 4)), dim3(256), 0, s, *keys, *vals, (long)n, shift, (long)ntiles, hist, *keys_alt, *vals_alt);
        std::swap(*keys, *keys_alt); std::swap(*vals, *vals_alt);
    }
    HIP_TRY(c, hipGetLastError());
    return EMBA_OK;
}

// the two (keys, values) pairs of a sort of n entries
emba_status ensure_sort_pairs(emba_ctx* c, size_t n)
{
    emba_status st;
    for (int i = 0; i < 2; ++i)
        if ((st = ensure<uint32_t>(c, c->ord.keys[i], n)) || (st = ensure<uint32_t>(c, c->ord.vals[i], n))) return st;
    return EMBA_OK;
}

int bits_for(size_t n_values) { int b = 1; while (((size_t)1 << b) < n_values) ++b; return b; }

constexpr size_t kTileRound = (size_t)kWarpNew * kTileWaves;   // entries one round of a tiled workgroup's waves takes

// ---- prepare_order, phase by phase.  The host arithmetic that decides the order is order_rule.h (tested on the CPU); here: the launches that feed it. ----

// control-pose index per batch; a batch outside the knots is an error (BASALT_ASSERT_STREAM at so3_spline.h:221-229)
emba_status order_batch_segments(emba_ctx* c, int64_t t0, int64_t dt, int K)
{
    hipStream_t s = c->stream;
    emba_status st;
    const size_t nbatch = c->win.n_batch;
    if ((st = ensure<uint32_t>(c, c->ord.status, kStatusWords))) return st;
    uint32_t* d_err = c->ord.status.as<uint32_t>();
    HIP_TRY(c, hipMemsetAsync(d_err, 0xFF, kStatusWords * 4, s));
    if ((st = ensure<uint16_t>(c, c->d_cp, nbatch)) || (st = ensure<double>(c, c->d_batch_u, nbatch))) return st;
    if (nbatch) hipLaunchKernelGGL(emba_batch_cp_kernel, dim3(nblocks(nbatch)), dim3(256), 0, s, c->d_batch_t.as<int64_t>(), (long)nbatch, t0, dt, K, c->d_cp.as<uint16_t>(), c->d_batch_u.as<double>(), d_err);
    uint32_t h_err[kStatusWords];
    HIP_TRY(c, hipMemcpyAsync(h_err, d_err, kStatusWords * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipStreamSynchronize(s));
    if (h_err[kStFirstBad] != 0xFFFFFFFFu) {
        int64_t tb = 0;
        (void)hipMemcpy(&tb, c->d_batch_t.as<int64_t>() + h_err[kStFirstBad], 8, hipMemcpyDeviceToHost);
        return fail(c, EMBA_ERR_TIME_RANGE, "batch %u midpoint %lld ns outside spline [%lld, %lld) (K=%d)", h_err[kStFirstBad], (long long)tb, (long long)t0,
                    (long long)(t0 + dt * (K - 1)), K);
    }
    return EMBA_OK;
}

// The order scratch as the tile search and the tile order built from it use it.  status: ord.status (context.h: StatusWord), cleared by order_batch_segments —
// kStTotal the entries of the expanded list, kStHeads the chain heads, kStCounter the predicted inliers, then a candidate's lead-ins.
struct TileSearch {
    uint32_t *bin, *emit, *pos, *pred, *heads, *status; uint8_t* used;
    long n_heads = 0;
    std::vector<uint8_t> h_used;
    unsigned long long* breaks() const { return reinterpret_cast<unsigned long long*>(status + kStCounter); }
};

// the pixels the caller's poses predict for every pm-order entry, the chains of the pm-order, and the inlier fraction f_pred the predicted pixels give
emba_status tile_search_begin(emba_ctx* c, const double* knots_host, int64_t t0, int64_t dt, int K, TileSearch* ts, double* f_pred)
{
    hipStream_t s = c->stream;
    emba_status st;
    const size_t ns = c->win.n_pm, nbatch = c->win.n_batch;
    const size_t max_bins = (size_t)((c->W + 7) / 8) * ((c->H + 1) / 2) + 1;      // (the finest pitch any candidate uses is 8 x 2)
    if ((st = ensure<uint32_t>(c, c->ord.bin, ns)) || (st = ensure<uint32_t>(c, c->ord.flags, ns)) || (st = ensure<uint32_t>(c, c->ord.pos, ns)) ||
        (st = ensure<uint8_t>(c, c->ord.used, max_bins + 8)) || (st = ensure<uint32_t>(c, c->ord.pred_or_y, ns)) || (st = ensure<uint32_t>(c, c->ord.heads_or_pol, ns)))
        return st;
    ts->bin = c->ord.bin.as<uint32_t>(); ts->emit = c->ord.flags.as<uint32_t>(); ts->pos = c->ord.pos.as<uint32_t>(); ts->used = c->ord.used.as<uint8_t>();
    ts->pred = c->ord.pred_or_y.as<uint32_t>(); ts->heads = c->ord.heads_or_pol.as<uint32_t>(); ts->status = c->ord.status.as<uint32_t>();
    ts->h_used.resize(max_bins);
    // the poses the caller starts from (staged through the pinned buffer like every evaluation's)
    HIP_TRY(c, hipMemcpyAsync(c->d_knots.as<double>(), knots_host, (size_t)4 * K * sizeof(double), hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(emba_pose_kernel, dim3(nblocks(nbatch, 64)), dim3(64), 0, s, c->d_batch_t.as<int64_t>(), (int)nbatch, c->d_knots.as<double>(), K, t0, dt, c->d_pose.as<double>(), c->d_err);
    hipLaunchKernelGGL(emba_predict_pixel_kernel, dim3(nblocks(ns)), dim3(256), 0, s, c->d_pm_pix.as<uint32_t>(), c->d_pm_batch.as<uint32_t>(), (long)ns, c->d_pose.as<double>(), kPoseStride, c->d_lut.as<double>(),
                       c->fx, c->fy, c->cx, c->cy, c->W, c->H, ts->pred);
    // the chains of the pm-order: heads -> list (one wave of the assignment kernel per chain)
    uint32_t *d_hflag = ts->emit, *d_hpos = ts->pos, *d_nheads = ts->status + kStHeads;
    hipLaunchKernelGGL(emba_head_flag_kernel, dim3(nblocks(ns)), dim3(256), 0, s, c->d_pm_pix.as<uint32_t>(), (long)ns, d_hflag);
    if ((st = dev_scan(c, d_hflag, d_hpos, ns, d_nheads))) return st;
    hipLaunchKernelGGL(emba_head_list_kernel, dim3(nblocks(ns)), dim3(256), 0, s, d_hflag, d_hpos, (long)ns, ts->heads);
    uint32_t h_nheads = 0;
    HIP_TRY(c, hipMemcpyAsync(&h_nheads, d_nheads, 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipStreamSynchronize(s));
    ts->n_heads = (long)h_nheads;
    HIP_TRY(c, hipMemsetAsync(ts->breaks(), 0, 8, s));
    hipLaunchKernelGGL(emba_count_pred_inliers_kernel, dim3((unsigned)std::min<size_t>(nblocks(ns), 1024)), dim3(256), 0, s, c->d_pm_pix.as<uint32_t>(), ts->pred, (long)ns, c->outlier_px, ts->breaks());
    unsigned long long hi = 0;
    HIP_TRY(c, hipMemcpyAsync(&hi, ts->breaks(), 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipStreamSynchronize(s));
    *f_pred = c->win.n_used ? (double)hi / (double)c->win.n_used : 0.0;
    return EMBA_OK;
}

// lead-ins and occupied tiles of one candidate; leaves its assignment in ts.bin / ts.emit
emba_status tile_search_evaluate(emba_ctx* c, TileSearch& ts, const BinGeom& q, size_t* breaks, size_t* used)
{
    hipStream_t s = c->stream;
    const size_t ns = c->win.n_pm, nb_ = (size_t)q.nbx * q.nby + 1;
    HIP_TRY(c, hipMemsetAsync(ts.used, 0, nb_, s));
    HIP_TRY(c, hipMemsetAsync(ts.breaks(), 0, 8, s));
    hipLaunchKernelGGL(emba_assign_tiles_kernel, dim3((unsigned)((ts.n_heads + 3) / 4)), dim3(256), 0, s, c->d_pm_pix.as<uint32_t>(), ts.pred, ts.heads, ts.n_heads, (long)ns, q, ts.bin, ts.used);
    hipLaunchKernelGGL(emba_expand_count_kernel, dim3(nblocks(ns)), dim3(256), 0, s, c->d_pm_pix.as<uint32_t>(), ts.bin, (long)ns, ts.emit);
    hipLaunchKernelGGL(emba_count_breaks_kernel, dim3((unsigned)std::min<size_t>(nblocks(ns), 1024)), dim3(256), 0, s, ts.emit, (long)ns, ts.breaks());
    unsigned long long hb = 0;
    HIP_TRY(c, hipMemcpyAsync(ts.h_used.data(), ts.used, nb_, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipMemcpyAsync(&hb, ts.breaks(), 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipStreamSynchronize(s));
    *breaks = (size_t)hb; *used = 0;
    for (size_t b = 0; b + 1 < nb_; ++b) *used += ts.h_used[b];
    return EMBA_OK;
}

// ---- which order?  Tile order pays when many events share a panorama pixel (the per-pixel sums are then combined in LDS) and the
// chains of a sensor pixel stay in a tile for a while (every tile entry costs one extra warp of the predecessor).
// Round 6: WHICH tile (order_kernels.h: the window rule).  The 1152-pixel LDS tile comes in four shapes (kernels.h: kTileShapes); every chain is cut into the
// longest segments that fit a tile of the shape on its pitch grid, and the shape with the fewest entries + chunks wins — a fast pan wants wide tiles, a
// trajectory that pitches wants tall ones (scripts/lead_in_sim.py: 5 M events over 4.8 s at 0.5 rad/s: 19.5 % lead-ins at 48 x 24, 11.5 % at 72 x 16).
// tile: the tile order it is, with the winner's assignment left in ord.bin / ord.flags; g, nbins: its pitch grid; breaks, used: its lead-ins and occupied tiles.
struct TileOrderChoice { bool tile = false; BinGeom g{}; size_t nbins = 1, breaks = 0, used = 0; };

emba_status choose_tile_order(emba_ctx* c, const double* knots_host, int64_t t0, int64_t dt, int K, TileOrderChoice* out)
{
    *out = TileOrderChoice{};
    const size_t n_used = c->win.n_used;
    if (!c->win.n_pm || !knots_host || !order_considers_tiles(c->order_mode, n_used, c->opt_tile_min_events)) return EMBA_OK;
    emba_status st;
    TileSearch ts{};
    double f_pred = 1.0;
    if ((st = tile_search_begin(c, knots_host, t0, dt, K, &ts, &f_pred))) return st;
    c->order.order_inl_pred = f_pred;
    if (order_hopeless(c->order_mode, f_pred)) return EMBA_OK;
    const int r = clamp_tile_reserve(c->opt_tile_reserve);
    TileChoice best{kTileRound};
    int last = -1; bool last_fine = false;      // the candidate whose assignment the scratch holds
    size_t br = 0, us = 0;
    // (the tall shape first, the others have to beat it by 2 %: at equal lead-ins 36 x 32 measured 3-5 % faster than 48 x 24 — 3 M events 155 vs 161 us, config 4's
    // shard 245 vs 260, 2 M 111 vs 115, city 463 vs 465; profiles/r06_regime_sweep.txt)
    static const int kShapeOrder[kNumTileShapes] = {3, 0, 1, 2};
    for (int si = 0; si < kNumTileShapes; ++si) {
        const int sh = kShapeOrder[si];
        if (c->opt_tile_shape >= 0 && sh != c->opt_tile_shape) continue;
        if ((st = tile_search_evaluate(c, ts, tile_geometry(c->W, c->H, kTileShapes[sh], false, r), &br, &us))) return st;
        last = sh; last_fine = false;
        best.offer(sh, n_used, br, us);
    }
    if (best.wants_fine(c->opt_tile_fine, n_used)) {
        if ((st = tile_search_evaluate(c, ts, tile_geometry(c->W, c->H, kTileShapes[best.shape], true, r), &br, &us))) return st;
        last = best.shape; last_fine = true;
        best.offer_fine(c->opt_tile_fine, n_used, br, us);
    }
    if (best.shape < 0) return fail(c, EMBA_ERR_INVALID_ARG, "option tile_shape %d: no such shape", c->opt_tile_shape);
    out->g = tile_geometry(c->W, c->H, kTileShapes[best.shape], best.fine, r);
    if (last != best.shape || last_fine != best.fine) { if ((st = tile_search_evaluate(c, ts, out->g, &br, &us))) return st; }   // ord.bin / ord.flags of the winner
    c->order.tile_shape = best.shape; c->order.tile_fine = best.fine;
    out->nbins = (size_t)out->g.nbx * out->g.nby + 1; out->breaks = best.breaks; out->used = best.used;
    c->order.order_per_px = events_per_pano_px(n_used, best.used, out->g); c->order.order_lead_frac = lead_in_fraction(n_used, best.breaks);
    out->tile = tile_order_wins(c->order_mode, n_used, c->opt_tile_min_events, c->order.order_per_px, f_pred, c->order.order_lead_frac);
    return EMBA_OK;
}

// pixel order: the device order is the pm-order
emba_status build_pixel_order(emba_ctx* c)
{
    hipStream_t s = c->stream;
    emba_status st;
    const size_t ns = c->win.n_pm;
    c->order.d_ev_pix = c->d_pm_pix.as<uint32_t>(); c->order.d_ev_batch = c->d_pm_batch.as<uint32_t>();
    c->win.n_sorted = ns;
    // per entry the spline parameter and segment of its batch (the warp kernel's per-event pose: 10 B per entry, streamed with the event words)
    if ((st = ensure<double>(c, c->d_ev_u, std::max<size_t>(ns, 1))) || (st = ensure<uint16_t>(c, c->d_ev_seg, std::max<size_t>(ns, 1)))) return st;
    if (ns) hipLaunchKernelGGL(emba_entry_pose_args_kernel, dim3(nblocks(ns)), dim3(256), 0, s, c->d_pm_batch.as<uint32_t>(), (long)ns, c->d_cp.as<uint16_t>(), c->d_batch_u.as<double>(), c->d_ev_seg.as<uint16_t>(), c->d_ev_u.as<double>());
    // the candidate flags of the device order
    if ((st = ensure<uint32_t>(c, c->ord.flags, std::max<size_t>(ns, 1)))) return st;
    if (ns) hipLaunchKernelGGL(emba_cand_flag_kernel, dim3(nblocks(ns)), dim3(256), 0, s, c->order.d_ev_pix, (long)ns, c->ord.flags.as<uint32_t>());
    return EMBA_OK;
}

// tile order — expanded list: every event, plus a lead-in copy of its predecessor where its chain enters a tile -> stable sort by tile -> chunks.
// Leaves the candidate flags of the device order in ord.flags.
emba_status build_tile_order(emba_ctx* c, const TileOrderChoice& ch)
{
    hipStream_t s = c->stream;
    emba_status st;
    const size_t ns = c->win.n_pm, nbins = ch.nbins;
    uint32_t *d_bin = c->ord.bin.as<uint32_t>(), *d_emit = c->ord.flags.as<uint32_t>(), *d_pos = c->ord.pos.as<uint32_t>(), *d_tot = c->ord.status.as<uint32_t>() + kStTotal;
    if ((st = dev_scan(c, d_emit, d_pos, ns, d_tot))) return st;
    uint32_t nd32 = 0;
    HIP_TRY(c, hipMemcpyAsync(&nd32, d_tot, 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipStreamSynchronize(s));
    const size_t nd = nd32;
    if ((st = ensure_sort_pairs(c, nd)) || (st = ensure<uint32_t>(c, c->ord.bin_start_or_x, nbins + 1))) return st;
    uint32_t *k0 = c->ord.keys[0].as<uint32_t>(), *v0 = c->ord.vals[0].as<uint32_t>(), *k1 = c->ord.keys[1].as<uint32_t>(), *v1 = c->ord.vals[1].as<uint32_t>();
    uint32_t* d_bin_start = c->ord.bin_start_or_x.as<uint32_t>();
    hipLaunchKernelGGL(emba_expand_write_kernel, dim3(nblocks(ns)), dim3(256), 0, s, c->d_pm_pix.as<uint32_t>(), d_bin, d_emit, d_pos, (long)ns, k0, v0);
    if ((st = dev_sort(c, &k0, &v0, &k1, &v1, nd, bits_for(nbins)))) return st;
    if ((st = ensure<uint32_t>(c, c->d_ev_pix_own, nd)) || (st = ensure<uint32_t>(c, c->d_ev_batch_own, nd)) || (st = ensure<uint32_t>(c, c->d_ev_pm, nd)) ||
        (st = ensure<double>(c, c->d_ev_u, nd)) || (st = ensure<uint16_t>(c, c->d_ev_seg, nd)))
        return st;
    c->order.d_ev_pix = c->d_ev_pix_own.as<uint32_t>(); c->order.d_ev_batch = c->d_ev_batch_own.as<uint32_t>(); c->order.have_ev_pm = true;
    HIP_TRY(c, hipMemsetAsync(d_bin_start, 0xFF, (nbins + 1) * 4, s));
    uint32_t* d_cf = d_emit;    // (emit is dead: its buffer now takes the candidate flags of the device order — nd <= 2 ns may exceed it)
    if (nd > ns) { if ((st = ensure<uint32_t>(c, c->ord.flags, nd))) return st; d_cf = c->ord.flags.as<uint32_t>(); }
    hipLaunchKernelGGL(emba_dev_gather_kernel, dim3(nblocks(nd)), dim3(256), 0, s, k0, v0, (long)nd, c->d_pm_pix.as<uint32_t>(), c->d_pm_batch.as<uint32_t>(), c->order.d_ev_pix, c->order.d_ev_batch,
                       c->d_ev_pm.as<uint32_t>(), c->d_cp.as<uint16_t>(), c->d_batch_u.as<double>(), c->d_ev_seg.as<uint16_t>(), c->d_ev_u.as<double>(), d_cf, d_bin_start);
    std::vector<uint32_t> h_start(nbins + 1);
    HIP_TRY(c, hipMemcpyAsync(h_start.data(), d_bin_start, (nbins + 1) * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipStreamSynchronize(s));
    c->order.chunks_lpt = !c->opt_chunk_order_bin;
    const std::vector<ChunkDesc> h_chunks = cut_chunks(kTileRound, h_start.data(), nbins, nd, ch.g, c->n_cu, c->opt_tile_chunk, c->order.chunks_lpt);
    c->order.n_chunks = (long)h_chunks.size();
    if ((st = ensure<ChunkDesc>(c, c->d_chunks, h_chunks.size()))) return st;
    HIP_TRY(c, hipMemcpyAsync(c->d_chunks.as<ChunkDesc>(), h_chunks.data(), h_chunks.size() * sizeof(ChunkDesc), hipMemcpyHostToDevice, s));
    HIP_TRY(c, hipStreamSynchronize(s));
    c->win.n_sorted = nd; c->order.n_lead = nd - c->win.n_used; c->order.tile_order = true;
    return EMBA_OK;
}

// record slots sorted by control-pose pair: candidates of the device order (flags in ord.flags) -> (key, entry) -> stable sort -> slot
emba_status assign_record_slots(emba_ctx* c, int K)
{
    hipStream_t s = c->stream;
    emba_status st;
    const size_t nd = c->win.n_sorted, M = c->win.n_cand;
    if ((st = ensure<uint32_t>(c, c->ord.pos, std::max<size_t>(nd, 1)))) return st;
    uint32_t *d_cf = c->ord.flags.as<uint32_t>(), *d_cpos = c->ord.pos.as<uint32_t>();
    if ((st = dev_scan(c, d_cf, d_cpos, nd, nullptr))) return st;
    if ((st = ensure_sort_pairs(c, std::max<size_t>(M, 1)))) return st;
    uint32_t *k0 = c->ord.keys[0].as<uint32_t>(), *v0 = c->ord.vals[0].as<uint32_t>(), *k1 = c->ord.keys[1].as<uint32_t>(), *v1 = c->ord.vals[1].as<uint32_t>();
    if ((st = ensure<uint32_t>(c, c->d_ev_slot, nd))) return st;
    HIP_TRY(c, hipMemsetAsync(c->d_ev_slot.as<uint32_t>(), 0xFF, std::max<size_t>(nd, 1) * 4, s));
    if (nd) hipLaunchKernelGGL(emba_cand_keys_kernel, dim3(nblocks(nd)), dim3(256), 0, s, c->order.d_ev_pix, c->order.d_ev_batch, c->d_cp.as<uint16_t>(), (long)nd, d_cpos, k0, v0);
    // the key's low half is cp_p, the high half cp_c, both < K: sort on the bits they really use
    const int kb = bits_for((size_t)K);
    if (kb <= 8) {   // fold the two halves into one 16-bit key for the sort (two passes instead of four)
        if (M) hipLaunchKernelGGL(emba_fold_keys_kernel, dim3(nblocks(M)), dim3(256), 0, s, k0, (long)M, 1);
        if ((st = dev_sort(c, &k0, &v0, &k1, &v1, M, 16))) return st;
        if (M) hipLaunchKernelGGL(emba_fold_keys_kernel, dim3(nblocks(M)), dim3(256), 0, s, k0, (long)M, 0);
    } else if ((st = dev_sort(c, &k0, &v0, &k1, &v1, M, 32))) return st;
    if (M) hipLaunchKernelGGL(emba_slot_assign_kernel, dim3(nblocks(M)), dim3(256), 0, s, k0, v0, (long)M, c->d_ev_slot.as<uint32_t>(), c->d_slot_key.as<uint32_t>());
    return EMBA_OK;
}

// where the pair key changes among the sorted slots: the runs the pair-aligned Gram form cuts its wave ranges from (step_rule.h: gram_pair_cuts).  Once per
// order, like the slots themselves; the starts come to the host (a few hundred words; the scan's position buffer is free again and takes them on the device).
emba_status collect_pair_runs(emba_ctx* c)
{
    hipStream_t s = c->stream;
    const size_t M = c->win.n_cand;
    c->order.run_start.clear(); c->order.runs_known = false;
    if (!M) return EMBA_OK;
    emba_status st;
    if ((st = ensure<uint32_t>(c, c->ord.pos, 1 + (size_t)kGramMaxRuns))) return st;
    uint32_t* d_runs = c->ord.pos.as<uint32_t>();
    HIP_TRY(c, hipMemsetAsync(d_runs, 0, 4, s));
    hipLaunchKernelGGL(emba_pair_runs_kernel, dim3(nblocks(M)), dim3(256), 0, s, c->d_slot_key.as<uint32_t>(), (long)M, d_runs, kGramMaxRuns);
    uint32_t n = 0;
    HIP_TRY(c, hipMemcpyAsync(&n, d_runs, 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipStreamSynchronize(s));
    if (!n || n > kGramMaxRuns) return EMBA_OK;
    c->order.run_start.resize(n);
    HIP_TRY(c, hipMemcpy(c->order.run_start.data(), d_runs + 1, (size_t)n * 4, hipMemcpyDeviceToHost));
    std::sort(c->order.run_start.begin(), c->order.run_start.end());
    c->order.runs_known = true;
    return EMBA_OK;
}

// At the first evaluation of a window (and again whenever the spline timing changes): the control-pose pair of every measurement,
// the device order (pixel order, or tile order from the panorama positions the given control poses predict) and the record slots
// sorted by pair.  Pose-independent except for the tile binning, which only affects speed.
emba_status prepare_order(emba_ctx* c, const double* knots_host, int64_t t0, int64_t dt, int K)
{
    if (c->order.keys_ready && c->order.key_t0 == t0 && c->order.key_dt == dt && c->order.key_K == K) return EMBA_OK;
    if (dt <= 0 || K < 2 || K > 65535) return fail(c, EMBA_ERR_INVALID_ARG, "bad spline: dt_ns=%lld K=%d", (long long)dt, K);
    const auto t_begin = std::chrono::steady_clock::now();
    hipStream_t s = c->stream;
    emba_status st;
    const size_t ns = c->win.n_pm;
    c->order = new_order(c->order);      // (a previous order of this window goes away; its buffers are reused)
    TileOrderChoice choice;
    if ((st = order_batch_segments(c, t0, dt, K)) || (st = choose_tile_order(c, knots_host, t0, dt, K, &choice))) return st;
    if ((st = choice.tile ? build_tile_order(c, choice) : build_pixel_order(c))) return st;
    c->win.nblk = (long)((c->win.n_sorted + kWarpNew - 1) / kWarpNew);
    if ((st = assign_record_slots(c, K)) || (st = collect_pair_runs(c))) return st;
    // per-event outputs of the evaluations, indexed in pm-order in both orders
    if ((st = ensure<double>(c, c->d_e_sorted, ns)) || (st = ensure<uint8_t>(c, c->d_flag, ns)) || (st = ensure<int32_t>(c, c->d_inl_idx, ns))) return st;
    HIP_TRY(c, hipMemsetAsync(c->d_flag.as<uint8_t>(), 0, std::max<size_t>(ns, 1), s));
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipStreamSynchronize(s));
    c->order.keys_ready = true; c->order.key_t0 = t0; c->order.key_dt = dt; c->order.key_K = K;
    c->prepare_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_begin).count();
    return EMBA_OK;
}

// ---- the registration of a window (emba_set_events[_dev]) ----------------------------------------------------------------------

// A record set for n_cand candidates.  A record is valid iff it carries the current evaluation's stamp (record_valid): a reused buffer holds older
// stamps only, new memory is cleared.
emba_status size_record_set(emba_ctx* c, RecordSet& rs, size_t n_cand)
{
    bool rec_fresh = false, tag_fresh = false;
    emba_status st;
    if ((st = ensure<double>(c, rs.rec, (std::max<size_t>(n_cand, 1) + kGramPad) * kRecStride, &rec_fresh)) || (st = ensure<double>(c, rs.tag, n_cand + kGramPad, &tag_fresh)))
        return st;
    if (rec_fresh) HIP_TRY(c, hipMemsetAsync(rs.rec.p, 0, rs.rec.bytes, c->stream));
    if (tag_fresh) HIP_TRY(c, hipMemsetAsync(rs.tag.p, 0, rs.tag.bytes, c->stream));
    return EMBA_OK;
}

// Shared by emba_set_events (host arrays: uploaded first) and emba_set_events_dev (arrays already in HBM).  x, y, pol, hx, hy, hbt are
// DEVICE pointers; t_dev (device) or batch_t_host (the nb midpoints, computed by the caller) supplies the times.
emba_status set_events_core(emba_ctx* c, const uint16_t* x, const uint16_t* y, const uint8_t* pol, const int64_t* t_dev, const int64_t* batch_t_host,
                            size_t n, const uint16_t* hx, const uint16_t* hy, const int64_t* hbt, size_t n_halo)
{
    hipStream_t s = c->stream;
    c->win.n_outside_tile = 0;
    const size_t n_used = (n / kBatch) * kBatch;   // quirk Q1: std::ceil of an integer division (model.cpp:79)
    const size_t nb = n_used / kBatch;
    if (n_used + n_halo >= 0x3FFFFFFFull) return fail(c, EMBA_ERR_INVALID_ARG, "too many events for 32-bit indices");
    c->win.n_in = n; c->win.n_used = n_used; c->win.n_halo = n_halo; c->win.n_batch = nb + n_halo;
    const size_t ns = n_used + n_halo;
    c->win.n_pm = ns; c->win.n_sorted = ns;
    emba_status st;
    if ((st = ensure<uint32_t>(c, c->ord.status, kStatusWords))) return st;
    uint32_t* d_err = c->ord.status.as<uint32_t>();      // (the kernel writes kStFirstBad, kStUnsorted, kStBadHalo)
    HIP_TRY(c, hipMemsetAsync(d_err, 0xFF, kStatusWords * 4, s));
    hipLaunchKernelGGL(emba_validate_events_kernel, dim3(nblocks(std::max(n_used, n_halo))), dim3(256), 0, s, x, y, t_dev, (long)n_used, c->sw, c->sh, hx, hy,
                       (long)n_halo, d_err);
    if ((st = ensure<int64_t>(c, c->d_batch_t, c->win.n_batch))) return st;
    if (t_dev) { if (nb) hipLaunchKernelGGL(emba_batch_mid_kernel, dim3(nblocks(nb)), dim3(256), 0, s, t_dev, (long)nb, c->d_batch_t.as<int64_t>()); }
    else if (nb) HIP_TRY(c, hipMemcpyAsync(c->d_batch_t.as<int64_t>(), batch_t_host, nb * 8, hipMemcpyHostToDevice, s));
    if (n_halo) HIP_TRY(c, hipMemcpyAsync(c->d_batch_t.as<int64_t>() + nb, hbt, n_halo * 8, hipMemcpyDeviceToDevice, s));

    // pm-order: stable sort by sensor pixel == the per-pixel vectors of EventMap::addEvent (event_map.h:34-37), halo entries in front
    if ((st = ensure_sort_pairs(c, std::max<size_t>(ns, 1))) || (st = ensure<uint32_t>(c, c->ord.flags, std::max<size_t>(ns, 1))) ||
        (st = ensure<uint32_t>(c, c->ord.pos, std::max<size_t>(ns, 1))))
        return st;
    uint32_t *k0 = c->ord.keys[0].as<uint32_t>(), *v0 = c->ord.vals[0].as<uint32_t>(), *k1 = c->ord.keys[1].as<uint32_t>(), *v1 = c->ord.vals[1].as<uint32_t>();
    uint32_t *d_cf = c->ord.flags.as<uint32_t>(), *d_cpos = c->ord.pos.as<uint32_t>();
    if (ns) hipLaunchKernelGGL(emba_pixel_keys_kernel, dim3(nblocks(ns)), dim3(256), 0, s, x, y, (long)n_used, c->sw, hx, hy, (long)n_halo, k0, v0);
    if ((st = dev_sort(c, &k0, &v0, &k1, &v1, ns, bits_for(c->S)))) return st;
    if ((st = ensure<uint32_t>(c, c->d_pm_pix, ns)) || (st = ensure<uint32_t>(c, c->d_pm_batch, ns)) || (st = ensure<uint32_t>(c, c->d_pm_orig, ns))) return st;
    if (ns) hipLaunchKernelGGL(emba_pm_gather_kernel, dim3(nblocks(ns)), dim3(256), 0, s, k0, v0, (long)ns, pol, (long)nb, c->d_pm_pix.as<uint32_t>(), c->d_pm_batch.as<uint32_t>(), c->d_pm_orig.as<uint32_t>(), d_cf);
    uint32_t* d_tot = d_err + kStTotal;
    if ((st = dev_scan(c, d_cf, d_cpos, ns, d_tot))) return st;    // (only the total is used: the number of measurement candidates)
    uint32_t h_err[kStatusWords];
    HIP_TRY(c, hipMemcpyAsync(h_err, d_err, kStatusWords * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipStreamSynchronize(s));
    if (h_err[kStFirstBad] != 0xFFFFFFFFu) return fail(c, EMBA_ERR_INVALID_ARG, "event %u lies outside the %dx%d sensor", h_err[kStFirstBad], c->sw, c->sh);
    if (h_err[kStUnsorted] != 0xFFFFFFFFu) return fail(c, EMBA_ERR_INVALID_ARG, "timestamps not sorted at event %u", h_err[kStUnsorted]);
    if (h_err[kStBadHalo] != 0xFFFFFFFFu) return fail(c, EMBA_ERR_INVALID_ARG, "halo event %u outside the sensor", h_err[kStBadHalo]);
    c->win.n_cand = ns ? h_err[kStTotal] : 0;
    const size_t n_cand = c->win.n_cand;

    if ((st = ensure<double>(c, c->d_pose, c->win.n_batch * kPoseStride))) return st;
    if ((st = size_record_set(c, c->work, n_cand))) return st;
    if ((st = ensure<uint32_t>(c, c->d_slot_key, n_cand))) return st;
    c->win.n_fblk = (long)std::max<size_t>((ns + kFlagBlk - 1) / kFlagBlk, 1);
    if ((st = ensure<uint32_t>(c, c->d_fblk_cnt, (size_t)c->win.n_fblk)) || (st = ensure<uint32_t>(c, c->d_fblk_off, (size_t)c->win.n_fblk))) return st;
    c->win.n_fsup = (c->win.n_fblk + kFlagSup - 1) / kFlagSup;
    if ((st = ensure<uint32_t>(c, c->d_fsup, (size_t)2 * c->win.n_fsup * kFlagSupStride))) return st;
    HIP_TRY(c, hipMemsetAsync(c->d_fsup.as<uint32_t>(), 0, (size_t)2 * c->win.n_fsup * kFlagSupStride * sizeof(uint32_t), c->stream));      // (both halves: launch A adds into one and zeroes the other for the next step)
    if ((st = ensure<double>(c, c->d_ep, ns))) return st;
    c->eq_in_alt = false;
    if (c->alt.rec.p && (st = size_record_set(c, c->alt, n_cand))) return st;   // the second record set (if an LM loop has made one) follows the window's size
    HIP_TRY(c, hipStreamSynchronize(s));
    c->win.nblk = (long)((ns + kWarpNew - 1) / kWarpNew);
    c->win.have_events = true;
    return EMBA_OK;
}

}  // namespace

extern "C" {

emba_status emba_set_events(emba_ctx* c, const uint16_t* x, const uint16_t* y, const uint8_t* pol, const int64_t* t_ns,
                            size_t n, const uint16_t* hx, const uint16_t* hy, const int64_t* hbt, size_t n_halo)
{
    if (!c) return EMBA_ERR_INVALID_ARG;
    if (n && (!x || !y || !pol || !t_ns)) return fail(c, EMBA_ERR_INVALID_ARG, "event arrays are NULL");
    if (n_halo && (!hx || !hy || !hbt)) return fail(c, EMBA_ERR_INVALID_ARG, "halo arrays are NULL");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    const auto t_begin = std::chrono::steady_clock::now();
    free_window(c);
    const size_t n_used = (n / kBatch) * kBatch, nb = n_used / kBatch;
    // The host only touches the timestamps: sortedness and the batch midpoints (model.cpp:116-119) need two reads per batch plus one
    // pass of comparisons; shipping 8 B per event over PCIe for that would cost more than the pass.
    for (size_t k = 1; k < n_used; ++k)
        if (t_ns[k] < t_ns[k - 1]) return fail(c, EMBA_ERR_INVALID_ARG, "timestamps not sorted at event %zu", k);
    std::vector<int64_t> bt(nb ? nb : 1);
    for (size_t b = 0; b < nb; ++b) bt[b] = batch_mid_ns(t_ns[kBatch * b], t_ns[kBatch * b + kBatch - 1]);
    // x, y, polarity (5 B per event) and the halo go to the device as they are
    hipStream_t s = c->stream;
    const HaloLayout halo(n_halo);
    emba_status st;
    if ((st = ensure<uint16_t>(c, c->ord.bin_start_or_x, std::max<size_t>(n_used, 1))) || (st = ensure<uint16_t>(c, c->ord.pred_or_y, std::max<size_t>(n_used, 1))) ||
        (st = ensure<uint8_t>(c, c->ord.heads_or_pol, std::max<size_t>(n_used, 1))) || (st = ensure<uint8_t>(c, c->ord.halo, halo.bytes)))
        return st;
    uint16_t *dx = c->ord.bin_start_or_x.as<uint16_t>(), *dy = c->ord.pred_or_y.as<uint16_t>();
    uint8_t* dp = c->ord.heads_or_pol.as<uint8_t>();
    int64_t* dhb = halo.hbt_in(c->ord.halo.p);
    uint16_t *dhx = halo.hx_in(c->ord.halo.p), *dhy = halo.hy_in(c->ord.halo.p);
    if (n_used) {
        HIP_TRY(c, hipMemcpyAsync(dx, x, n_used * 2, hipMemcpyHostToDevice, s));
        HIP_TRY(c, hipMemcpyAsync(dy, y, n_used * 2, hipMemcpyHostToDevice, s));
        HIP_TRY(c, hipMemcpyAsync(dp, pol, n_used, hipMemcpyHostToDevice, s));
    }
    if (n_halo) {
        HIP_TRY(c, hipMemcpyAsync(dhb, hbt, n_halo * 8, hipMemcpyHostToDevice, s));
        HIP_TRY(c, hipMemcpyAsync(dhx, hx, n_halo * 2, hipMemcpyHostToDevice, s));
        HIP_TRY(c, hipMemcpyAsync(dhy, hy, n_halo * 2, hipMemcpyHostToDevice, s));
    }
    st = set_events_core(c, dx, dy, dp, nullptr, bt.data(), n, dhx, dhy, dhb, n_halo);
    c->set_events_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_begin).count();
    return st;
}

emba_status emba_set_events_dev(emba_ctx* c, const uint16_t* x_dev, const uint16_t* y_dev, const uint8_t* pol_dev, const int64_t* t_ns_dev, size_t n,
                                const uint16_t* hx_dev, const uint16_t* hy_dev, const int64_t* hbt_dev, size_t n_halo)
{
    if (!c) return EMBA_ERR_INVALID_ARG;
    if (n && (!x_dev || !y_dev || !pol_dev || !t_ns_dev)) return fail(c, EMBA_ERR_INVALID_ARG, "event arrays are NULL");
    if (n_halo && (!hx_dev || !hy_dev || !hbt_dev)) return fail(c, EMBA_ERR_INVALID_ARG, "halo arrays are NULL");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    const auto t_begin = std::chrono::steady_clock::now();
    free_window(c);
    emba_status st = set_events_core(c, x_dev, y_dev, pol_dev, t_ns_dev, nullptr, n, hx_dev, hy_dev, hbt_dev, n_halo);
    c->set_events_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_begin).count();
    return st;
}

emba_status emba_last_tile_drift(const emba_ctx* c, size_t* n_outside, int32_t* n_rebin)
{
    if (!c) return EMBA_ERR_INVALID_ARG;
    if (n_outside) *n_outside = c->win.n_outside_tile;
    if (n_rebin) *n_rebin = c->win.n_rebin;
    return EMBA_OK;
}

emba_status emba_last_setup_ms(const emba_ctx* c, double* set_events_ms, double* prepare_ms, int32_t* tile_order, size_t* n_entries, size_t* n_chunks)
{
    if (!c) return EMBA_ERR_INVALID_ARG;
    if (set_events_ms) *set_events_ms = c->set_events_ms;
    if (prepare_ms) *prepare_ms = c->prepare_ms;
    if (tile_order) *tile_order = c->order.tile_order ? 1 : 0;
    if (n_entries) *n_entries = c->win.n_sorted;
    if (n_chunks) *n_chunks = (size_t)c->order.n_chunks;
    return EMBA_OK;
}

emba_status emba_last_order_stats(const emba_ctx* c, double* events_per_pano_px, double* lead_in_frac)
{
    if (!c) return EMBA_ERR_INVALID_ARG;
    if (events_per_pano_px) *events_per_pano_px = c->order.order_per_px;
    if (lead_in_frac) *lead_in_frac = c->order.order_lead_frac;
    return EMBA_OK;
}

emba_status emba_last_order_inlier_estimate(const emba_ctx* c, double* inlier_frac)
{
    if (!c || !inlier_frac) return EMBA_ERR_INVALID_ARG;
    *inlier_frac = c->order.order_inl_pred;
    return EMBA_OK;
}

emba_status emba_last_tile_geometry(const emba_ctx* c, int32_t* tile_w, int32_t* tile_h, int32_t* pitch_x, int32_t* pitch_y, int32_t* reserve)
{
    if (!c) return EMBA_ERR_INVALID_ARG;
    const BinGeom g = tile_geometry(c->W, c->H, kTileShapes[c->order.tile_shape], c->order.tile_fine, clamp_tile_reserve(c->opt_tile_reserve));
    if (tile_w) *tile_w = g.tw;
    if (tile_h) *tile_h = g.th;
    if (pitch_x) *pitch_x = g.bw;
    if (pitch_y) *pitch_y = g.bh;
    if (reserve) *reserve = g.r;
    return EMBA_OK;
}

emba_status emba_event_counts(const emba_ctx* c, size_t* n_used, size_t* n_cand)
{
    if (!c) return EMBA_ERR_INVALID_ARG;
    if (n_used) *n_used = c->win.n_used;
    if (n_cand) *n_cand = c->win.n_cand;
    return EMBA_OK;
}

}  // extern "C"
