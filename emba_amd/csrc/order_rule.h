// emba_amd/csrc/order_rule.h — the host arithmetic that decides the device order of a window (emba_hip.hip: prepare_order), as functions of plain values.
//
// No HIP in here: plain C++17, so that tests/cpp/order_rule_test.cpp checks it on a CPU in milliseconds.  The kernels' sizes come in as values — `round`: the
// entries one round of a tiled workgroup's waves takes (kWarpNew x kTileWaves of kernels.h), `ts`: one of its kTileShapes.  ChunkDesc, TileShape and BinGeom
// are defined here; kernels.h and order_kernels.h include this file for them.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <utility>
#include <vector>

namespace emba {

struct ChunkDesc { uint32_t begin, end; int32_t x0, y0; };   // entries [begin, end) of the device order; LDS tile origin (panorama px)

// one shape of the tiled kernel's LDS accumulator tile (kernels.h: kTileShapes): {tile w, h, pitch of the tile-origin grid, its finer variant for very dense windows}
struct TileShape { int tw, th, pw, ph, fine_pw, fine_ph; };

struct BinGeom { int W, H, bw, bh, nbx, nby, tw, th, r; };   // pitch grid of tile origins: bw x bh panorama pixels, nbx x nby of them; LDS tile tw x th; reserve r

inline int clamp_tile_reserve(int opt_tile_reserve) { return std::max(0, std::min(opt_tile_reserve, 5)); }

// the pitch grid of one candidate: shape ts, its coarse or fine grid of tile origins, reserve r, on a W x H panorama
inline BinGeom tile_geometry(int W, int H, const TileShape& ts, bool fine, int r)
{
    BinGeom q{};
    q.W = W; q.H = H; q.tw = ts.tw; q.th = ts.th; q.r = r;
    q.bw = fine ? ts.fine_pw : ts.pw; q.bh = fine ? ts.fine_ph : ts.ph;
    q.bw = std::min(q.bw, ts.tw - 2 * r); q.bh = std::min(q.bh, ts.th - 2 * r);     // (a single pixel must fit wherever it lies in its pitch cell)
    q.nbx = (W + q.bw - 1) / q.bw; q.nby = (H + q.bh - 1) / q.bh;
    return q;
}

// what a candidate costs the warp kernel, in entries: every lead-in is a full warp, every chunk zeroes and flushes an LDS tile (~ 256 entries' worth:
// 3 M events, round 3: 902 -> 2520 entries per chunk took the kernel from 191 to 174 us)
inline double candidate_cost(size_t round, size_t n_used, size_t breaks, size_t used)
{
    const double entries = (double)n_used + (double)breaks;
    const double chunks = std::max((double)used, entries / (double)(round * 8));
    return entries + 256.0 * chunks;
}

// The search for a window's tile: the caller measures (lead-ins, occupied tiles) of every coarse candidate and offers them here in the order it prefers them (a later one has to beat the first by 2 %), then of the
// winner's fine grid if wants_fine() asks for it.  shape < 0: nothing offered yet.
struct TileChoice {
    size_t round;      // kWarpNew x kTileWaves
    int shape = -1; bool fine = false;
    double cost = 0; size_t breaks = 0, used = 0;
    void offer(int sh, size_t n_used, size_t br, size_t us)
    {
        const double cc = candidate_cost(round, n_used, br, us);
        if (shape < 0 || cc < 0.98 * cost) { shape = sh; fine = false; cost = cc; breaks = br; used = us; }
    }
    // dense tiles can afford a finer grid of tile origins (segments end closer to the tile's far edge, and a tile's entries spread over more chunks): config 4's
    // shard (11.7 k entries per tile) 258 -> 229 us; at 3-5 k entries per tile it loses (3 M: 162 -> 173, 5 M: 236 -> 271)
    // (... and only below 16 M events: the finer grid doubles the chunks — 40 M events 1749 -> 1879 us, config 5's shard 566 -> 655, 100 M + 2 % per step;
    // profiles/r06_large_window_ab.txt)
    bool wants_fine(int opt_tile_fine, size_t n_used) const
    {
        return shape >= 0 && opt_tile_fine != 0 &&
               (opt_tile_fine == 1 || (n_used < (size_t)16000000 && (double)n_used / std::max<size_t>(used, 1) >= 2.0 * round * 8));
    }
    void offer_fine(int opt_tile_fine, size_t n_used, size_t br, size_t us)
    {
        const double cc = candidate_cost(round, n_used, br, us);
        if (cc < cost || opt_tile_fine == 1) { fine = true; cost = cc; breaks = br; used = us; }
    }
};

// order_mode: option order — 0 auto, 1 pixel, 2 tile.  f_pred: the inlier fraction the predicted pixels give.
// (auto on a window below tile_min_events never takes the tile order: nothing to analyse — 1.2 -> 0.3 ms of a 1 M-event window's first evaluation)
inline bool order_considers_tiles(int order_mode, size_t n_used, int tile_min_events) { return order_mode != 1 && (order_mode == 2 || n_used >= (size_t)tile_min_events); }
// the rule below cannot hold even without a single lead-in: skip the search for a tile
inline bool order_hopeless(int order_mode, double f_pred) { return order_mode == 0 && 83.0 * f_pred <= 41.0; }

inline double events_per_pano_px(size_t n_used, size_t used_bins, const BinGeom& g)     // events per panorama pixel of the occupied pitch cells
{
    return used_bins ? (double)n_used / ((double)used_bins * g.bw * g.bh) : 0.0;
}
inline double lead_in_fraction(size_t n_used, size_t breaks) { return n_used ? (double)breaks / (double)n_used : 1.0; }

// Measured (profiles/r02c_order_sweep.txt): the tile order wins once the working set has left the Infinity Cache (3 M events, 1024x2048:
// 374 vs 394 us per step; 5 M / K=97: 558 vs 618; 100 M: 4.8 vs 8.7 ms warp) and loses below it (1 M events, 24 per pixel: 82 vs 52 us
// — every entry of the tile order is a warp, lead-ins included, and a workgroup's LDS tile is zeroed and flushed for a handful of groups).
// (round 3, with at least 5 groups per wave and chunk: 2 M events 220 vs 246 us per step, 1.5 M 188 vs 155 — the pixel order falls off a cliff
// between 1.5 M and 2 M events: twice the events on the same footprint are twice as close along a chain, nearly all of them inliers — 3 x the atomic requests)
// (round 5: a slow pan over a big sensor — the city shape at 0.1 rad/s: 10 M events on 640x480, 50 events per panorama pixel — is
// atomic-request bound in pixel order (7.3 M requests on 155 k lines); the tile order's LDS sums win there in spite of the extra entries: step 867 vs
// 946-995 us.  Hence the second clause: very dense tiles tolerate more lead-ins.)
// Round 6: the rule prices both orders.  Per million events, fitted to profiles/r06_regime_sweep.txt and r06_sparse_order_ab.txt (warp + Gram kernels, us):
// pixel order 20 + 93 f (it pays per INLIER: an atomic request, a record, a live slot of the Gram kernel's tag stream; f = inlier fraction), tile order
// 31 (1 + lead) + 10 f + 30 (it pays per ENTRY, lead-in copies included, and its Gram kernel reads every candidate's slot).  The tile order wins where
// 83 f > 41 + 31 lead.  f is estimated from the predicted pixels (emba_count_pred_inliers_kernel).  (Rounds 2-5 asked for lead <= 0.35 only: with the window
// rule's fewer lead-ins that sent a 34 %-inlier stream — 10 M events on 640x480 at 0.5 rad/s — to the tile order: 850 us per step against 636 in pixel order.)
inline bool tile_order_wins(int order_mode, size_t n_used, int tile_min_events, double per_px, double f_pred, double lead_frac)
{
    return (order_mode == 2) || (n_used >= (size_t)tile_min_events && per_px >= 8.0 && 83.0 * f_pred > 41.0 + 31.0 * lead_frac);
}

// entries a workgroup of the tiled kernel should get, for a device order of nd entries on a chip of n_cu compute units (option tile_chunk > 0 overrides)
inline size_t chunk_target(size_t round, size_t nd, int n_cu, int opt_tile_chunk)
{
    const size_t slots = (size_t)n_cu * 2;      // workgroups of the tiled kernel the chip holds at a time
    // chunk size: enough workgroups for ~8 rounds of the chip, at most 16 groups of 63 entries per wave
    size_t chunk = (nd + slots * 8 - 1) / (slots * 8);
    // (at least 5 groups per wave: a workgroup zeroes and flushes its 55-KB LDS tile whatever it has to do — 3 M events: 902 -> 2520 entries per
    // chunk, warp kernel 191 -> 174 us; 5 M: 280 -> 271; from 10 M on the first rule gives more than that anyway)
    // round 4, with the chunks dispatched longest first: 8 groups per wave up to ~8 M entries (3 M events: 1339 chunks, warp kernel 160 -> 153 us;
    // 5 M: 257 -> 242), 5 beyond (10 M: 8 groups 493 us, 5 groups 464 — there the first rule decides most chunks anyway)
    const size_t min_groups = nd < (size_t)8000000 ? 8 : 5;
    chunk = std::min<size_t>(std::max<size_t>(chunk, round * min_groups), round * 16);
    if (opt_tile_chunk > 0) chunk = (size_t)opt_tile_chunk;
    return chunk;
}

// chunks: every occupied tile is cut into workgroup-sized pieces (host: <= 32 k tiles).  bin_start[b]: first entry of tile b in the device order of nd entries,
// 0xFFFFFFFF for an empty tile (nbins of them; an occupied tile ends where the next occupied one starts).
inline std::vector<ChunkDesc> cut_chunks(size_t round, const uint32_t* bin_start, size_t nbins, size_t nd, const BinGeom& g, int n_cu, int opt_tile_chunk, bool lpt)
{
    std::vector<std::pair<uint32_t, uint32_t>> occ;   // (bin, start)
    for (size_t b = 0; b < nbins; ++b) if (bin_start[b] != 0xFFFFFFFFu) occ.emplace_back((uint32_t)b, bin_start[b]);
    std::vector<ChunkDesc> chunks;
    const size_t chunk = chunk_target(round, nd, n_cu, opt_tile_chunk);
    for (size_t k = 0; k < occ.size(); ++k) {
        const uint32_t b = occ[k].first, b0 = occ[k].second, b1 = (k + 1 < occ.size()) ? occ[k + 1].second : (uint32_t)nd;
        // (pieces in whole ROUNDS of the workgroup's waves: a piece of G groups takes ceil(G / 8) rounds whatever it holds, so only a tile's last piece may be ragged)
        const size_t cnt = b1 - b0, nch = (cnt + chunk - 1) / chunk, per = ((cnt + nch - 1) / nch + round - 1) / round * round;
        const int bx = (int)(b % (uint32_t)g.nbx), by = (int)(b / (uint32_t)g.nbx);
        for (size_t q = 0; q < nch; ++q) {
            ChunkDesc d;
            d.begin = b0 + (uint32_t)(q * per); d.end = (uint32_t)std::min<size_t>(b0 + (q + 1) * per, b1);
            d.x0 = bx * g.bw - g.r; d.y0 = by * g.bh - g.r;
            if (d.begin < d.end) chunks.push_back(d);
        }
    }
    // Chunk sizes differ (every bin is cut on its own) and the grid is a few rounds of the chip's workgroup slots: with the longest chunks FIRST the
    // last round is made of the short ones (longest-processing-time order; workgroups are dispatched in grid order as slots free up).
    // Option chunk_order_bin keeps the bins' order (neighbouring chunks on one XCD).
    if (lpt) std::stable_sort(chunks.begin(), chunks.end(), [](const ChunkDesc& a, const ChunkDesc& b) { return a.end - a.begin > b.end - b.begin; });
    return chunks;
}

}  // namespace emba
