// emba_amd/csrc/step_rule.h — the host arithmetic of the step path (step_host.h: evaluateDataError + formNormalEq + applyL2Reg), as functions of plain values:
// the layout of the pack, where an evaluation takes its Hessians and poses from, how many blocks clear in front of it, which form the gather and the Gram
// launch take, the Gram launch's plan, and when a drifted tile order is binned again.
//
// No HIP in here: plain C++17, so that tests/cpp/step_rule_test.cpp checks it on a CPU in milliseconds.  The kernels' sizes come in as values (GramSizes,
// `rec_stride`: kRecStride, `gather_max_units`: kGatherMaxUnits of kernels.h).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

// (the containment rule below is also what the active-set write evaluates on the device)
#if defined(__HIPCC__)
#define EMBA_RULE_HD __host__ __device__
#else
#define EMBA_RULE_HD
#endif

namespace emba {

// The pack of K control poses: [A11 (3K)^2 | b1 (3K) | 5 doubles per active pixel (A22 | b2)] — what formNormalEq leaves, the solvers read and exchange 2 carries.
struct PackLayout {
    size_t b1, A22b2, head;   // offsets of b1 and of the per-pixel rows; head = A22b2: the doubles in front of the rows
    explicit PackLayout(int K) : b1((size_t)9 * K * K), A22b2(b1 + (size_t)3 * K), head(A22b2) {}
    size_t len(size_t P) const { return head + 5 * P; }              // the pack of P active pixels
    size_t need(size_t npix) const { return len(npix); }             // a pack no active set of this panorama outgrows
    size_t max_P(size_t cap) const { return (cap - head) / 5; }      // active pixels a pack of `cap` doubles (>= head) has room for
};

// Hessian source of an evaluation — 0: the on-the-fly stencil, 1: every texel packed, 3: texels packed inside the rectangle an earlier evaluation touched.
// With several events per panorama pixel (measured break-even: ~4) the full texel pack (one 48-B gather per measurement instead of an 18-load stencil) pays
// for itself; otherwise texels are packed only inside the bounding box of the pixels an earlier evaluation touched, and the warp kernel falls back to the
// stencil outside it.  texel_mode: option texel — 0 auto, 1 / 2 / 3 force pack / stencil / rectangle.
inline int hessian_source(int texel_mode, size_t n_sorted, size_t npix)
{
    return texel_mode == 1 ? 1 : texel_mode == 2 ? 0 : texel_mode == 3 ? 3 : (n_sorted > 4 * npix ? 1 : 3);
}

// Pixel order: per-event pose from the segment records too (warp_lane SEGPOSE; round 4, late) instead of one 112-B pose record per batch gathered by
// every event — 7 x 16-B gathers over 64 different lines per wave, and past ~7 M events a table that no longer fits the L2s.  Measured, same box,
// step time: 1 M events 101.2 -> 98.2 us, 1.5 M 150.8 -> 143.5, 10 M on 640x480 (city shape) 779 -> 714 (warp 0.60 -> 0.68 of the roofline),
// 10 M on 2048x4096 / K = 256 940 -> 861.  (Round 1 had measured the opposite at 1 M events, + 6 us, on a kernel that was then VALU-heavier in
// other places; option segpose = 1 keeps the per-batch table for comparison.)  segpose_mode: option segpose — 0 auto = yes, 1 no, 2 yes.
inline bool segpose_in_pixel_order(bool tile_order, int segpose_mode) { return !tile_order && (segpose_mode ? segpose_mode == 2 : true); }

// The packed texels (source 3) describe ONE map and ONE rectangle.  They are packed again when either no longer holds, not in every evaluation: on the same map and
// inside the same rectangle the pack writes the same bytes (a poses-only refinement, every re-evaluation on one map, the benchmark).
//   the map: the host counts every call that changes or rebinds the planes (map_rule.h: MapState) and remembers which count the last pack read.  A map the caller bound is the
//   caller's memory and may change without a call: it is never taken for unchanged.
//   the rectangle: the pack covers the last formed evaluation's box grown by kRectMargin, and the warp kernel trusts the PACKED rectangle only (outside it: the
//   stencil, slow, never wrong).  The active-set write's last block, which reduces the new box, compares it on the device with the packed one and publishes the
//   verdict beside the counts the host waits for anyway (no round trip; the host never reads a rectangle): fresh while the new box stays inside the packed box grown
//   by kRectFreshSlack — half the margin, so that the next evaluation's pixels may move as far again before one of them meets the stencil.
constexpr int kRectMargin = 24;
constexpr int kRectFreshSlack = 12;
static_assert(kRectFreshSlack <= kRectMargin, "texels exist only inside the packed box grown by kRectMargin");
// boxes {xmin, ymin, xmax, ymax}, inclusive, empty if max < min.  An empty new box needs no texels; nothing lies inside an empty packed box.
EMBA_RULE_HD inline bool rect_contained(int nx0, int ny0, int nx1, int ny1, int px0, int py0, int px1, int py1, int slack)
{
    if (nx1 < nx0 || ny1 < ny0) return true;
    if (px1 < px0 || py1 < py0) return false;
    return nx0 >= px0 - slack && ny0 >= py0 - slack && nx1 <= px1 + slack && ny1 <= py1 + slack;
}
// verdict_seq: the word the last block publishes — the step's sequence number where the new box is contained, 0 where it is not; step_seq: the host's number of the
// last step that reduced a box.  They differ while that step's verdict has not arrived (or no step has run): not known to be fresh.
inline bool texels_stale(bool map_owned, uint32_t map_version, uint32_t packed_version, int verdict_seq, int step_seq)
{
    return !map_owned || map_version != packed_version || step_seq == 0 || verdict_seq != step_seq;
}
// The texel blocks of the launch in front of the warp kernel: 1024 for source 3 with stale texels, none otherwise
inline int texel_blocks(int hessian_src, bool stale) { return (hessian_src == 3 && stale) ? 1024 : 0; }

// No launch in front of the warp kernel at all (option step_prep: 0 the launch always; 1 where this rule allows — measured at 1 M events: the hand-off
// costs the warp kernel what the launch cost): what is left of it once the lines are clean and the texels fresh is
// one block that writes K - 1 segment records; workgroup 0 of the warp kernel writes them instead and hands them to the others (kernels.h: inline_seg_*).  Pixel order
// with segment records, the control poses in the kernel arguments, a window with entries, and nothing else for the launch to do.
inline bool prep_inside_warp(int step_prep, bool tile_order, bool segpose, int K, int inline_knots, size_t n_sorted, int n_prep_blk, int n_tex_blk, int hessian_src)
{
    return step_prep == 1 && !tile_order && segpose && K <= inline_knots && n_sorted > 0 && n_prep_blk == 0 && n_tex_blk == 0 && hessian_src != 1;
}

// ... or the K - 1 records formed by the HOST (option step_prep = 2, the default; seg_record_rule.h: segment_records) and carried to the warp kernel by value in its
// arguments (kernels.h: SegRecordsByValue, `seg_by_value` = kSegByValue records): the same steady step — pixel order with segment poses, no texel blocks, no
// clearing blocks, a window with entries — as long as the K - 1 records fit the carrier.  Everything else keeps the launch: stale texels, a first evaluation,
// the tile order, the per-batch pose table, a larger K, an empty window.
inline bool prep_on_host(int step_prep, bool tile_order, bool segpose, int K, int seg_by_value, size_t n_sorted, int n_prep_blk, int n_tex_blk, int hessian_src)
{
    return step_prep == 2 && !tile_order && segpose && K >= 2 && K - 1 <= seg_by_value && n_sorted > 0 && n_prep_blk == 0 && n_tex_blk == 0 && hessian_src != 1;
}

// Blocks of the clearing pass over count map + accumulator lines in front of an evaluation.  It is only needed when the previous evaluation's sums are still
// in their lines (it was never formed by the resident step, whose gather clears them behind itself); the count map's entries are stamped and need no clearing
// (... and only when a warp kernel follows to re-mark it — an EMPTY window launches none, so its count map and active set would be the
// previous window's; the reference clears, model.cpp:85, and finds P = 0)
inline int prep_blocks(bool lines_clean, size_t n_sorted, size_t npix) { return (lines_clean && n_sorted) ? 0 : (int)((npix + 1023) / 1024); }

// The warp kernel writes its records with non-temporal stores where the Gram kernel cannot find them in the Infinity Cache anyway: the tile order (dense
// regime), or more record bytes than kRecCachedBytes (1 M slots = 128 MB: kept in the Infinity Cache for the Gram kernel).
constexpr size_t kRecCachedBytes = (size_t)144 << 20;
inline bool records_non_temporal(bool tile_order, size_t n_cand, int rec_stride) { return tile_order || n_cand * (size_t)(rec_stride * 8) > kRecCachedBytes; }

// The list-driven gather of the resident step (launch A writes per-unit active lists, four waves of every Gram block gather from them) — may it be used?
// step_gather: option — 0 the sweeping kernel, 1 the list-driven gather as a kernel of its own, 2 (default) in the Gram launch, 3 the lists everywhere (comparison).
// (round 4, late: the gather is the work of 4 of a Gram block's 16 waves BESIDE the record stream, not a head in front of it: step time
// with it / with the sweeping launch — 1 M 92.6 / 96.4 us, 1.5 M 134.7 / 143.8, 2 M (tile order) 193.4 / 208.5, 3 M 274.4 / 280.9, 10 M on
// 640x480 (pixel order) 612.5 / 626.1, on 2048x4096 766.7 / 776.3; but 5 M (tile) 436.0 / 432.2, 40 M 3137 / 3014: a bandwidth-bound stream
// misses the four waves more than it gains from the launch — pixel order everywhere, tile order up to kGatherTileMaxCand candidates)
constexpr size_t kGatherTileMaxCand = 3500000;
inline bool gather_lists_ok(bool consume, int step_gather, bool a22_from_records, long n_ablk, long gather_max_units, size_t n_cand, bool tile_order)
{
    return consume && step_gather && !a22_from_records && n_ablk <= gather_max_units && n_cand && (step_gather == 3 || !tile_order || n_cand <= kGatherTileMaxCand);
}
// ... and is it: launch A builds the lists only beside a dense pass of its own — markers to materialise, or exchanged byte counts to read
inline bool gather_uses_lists(bool lists_ok, bool counts_raw, bool global_bytes) { return lists_ok && (counts_raw || global_bytes); }
// A sharded rank's exchanged byte counts: launch A reads them beside this rank's own counts where it builds the lists; everywhere else they are expanded into
// the count map first and the sweeping forms see global counts
inline bool global_counts_need_expanding(bool lists_ok, bool ep_deferred, size_t n_sorted, bool counts_raw) { return !(lists_ok && ep_deferred && n_sorted && !counts_raw); }
// the deferred gather rides in the Gram launch (else: a kernel of its own)
inline bool gather_rides_in_gram(bool lists, int step_gather) { return lists && step_gather >= 2; }

// The tag stream pays where slots are dead (pixel order: about half of them at the BASELINE workload); in the tile order (dense regime: nearly every
// slot is live) the warp kernel's scattered 8-B tag stores cost more than the Gram kernel saves (40 M events: +370 vs -180 us).  use_tags: option gram_tags.
inline bool gram_tags(int use_tags, bool tile_order, bool ep_host) { return use_tags && !tile_order && !ep_host; }

// Sparse slot streams (pixel order on a large panorama: most inliers fall on pixels that stay inactive): stages of 128 tags, only the live records fetched
// (180 -> 78 us at 10 M events on 2048 x 4096, K = 256).  Which form: option gram_sparse (0 / 1), else by the LAST formed equations of this context — at least
// thres records per active pixel are live, and where 4 thres P is still below a quarter of the slots the stream is sparse (BASELINE: 5 x 68.6 k of 1 M
// slots = 0.34 -> dense; 10 M events on 2048 x 4096: 0.055)
inline bool gram_sparse(bool tags, int opt_gram_sparse, size_t P_prev, size_t n_cand, int thres)
{
    return tags && (opt_gram_sparse == 1 || (opt_gram_sparse < 0 && P_prev > 0 && n_cand >= (2u << 20) && 16ull * (size_t)thres * P_prev < n_cand));
}

// Gather waves per Gram block (option gather_waves = 1|2|4 overrides).  Measured: with ONE gather wave the gather outlasts the stream at every size — Gram
// kernel 57 vs 36 us at 1 M events, 1288 vs 1047 at 40 M —, two are within noise of four or of the sweeping launch from 5 M events up: four wherever the
// lists are used
inline int gather_waves(int opt_gather_waves) { return (opt_gather_waves == 1 || opt_gather_waves == 2 || opt_gather_waves == 4) ? opt_gather_waves : 4; }

// kernels.h: kGramBlock, kGramChunk, kGramChunkMin, kEpTailBlk
struct GramSizes { int block, chunk, chunk_min, ep_tail_blk; };

// The Gram launch over n_cand record slots.  Slots per wave: whole rounds of one 16-wave block per CU with equal shares (1 M events: one round of 236 slots
// per wave), between chunk_min and chunk slots.  (sparse form: up to four times the slots per wave — a wave's pipeline takes three stages to fill; option
// gram_sparse_chunk: 1 ... 8, no difference from 2 up.)  ep_tail: the residual vector is compacted by tail blocks of this launch, one per ep_tail_blk
// pm-order entries.
struct GramPlan { int chunk; long waves; int n_gram_blocks; unsigned ep_tail_blocks, grid; int gather_waves; };
inline GramPlan gram_plan(size_t n_cand, bool sparse, int opt_gram_sparse_chunk, int n_cu, bool ep_tail, size_t n_pm, int opt_gather_waves, const GramSizes& k)
{
    GramPlan g{};
    const long chunk_cap = sparse ? (long)opt_gram_sparse_chunk * k.chunk : k.chunk;
    const long per_round = (long)n_cu * (k.block / 64);
    const long rounds = std::max<long>(1, ((long)n_cand + per_round * chunk_cap - 1) / (per_round * chunk_cap));
    long chunk = ((long)n_cand + per_round * rounds - 1) / (per_round * rounds);
    chunk = (chunk + 7) & ~7L;
    chunk = std::min<long>(std::max<long>(chunk, k.chunk_min), chunk_cap);
    g.chunk = (int)chunk;
    g.waves = ((long)n_cand + chunk - 1) / chunk;
    const long wpb = k.block / 64;
    g.grid = (unsigned)((g.waves + wpb - 1) / wpb);
    g.n_gram_blocks = (int)g.grid;
    if (ep_tail) {
        g.ep_tail_blocks = (unsigned)((n_pm + k.ep_tail_blk - 1) / k.ep_tail_blk);
        g.grid += g.ep_tail_blocks;
    }
    g.gather_waves = gather_waves(opt_gather_waves);
    return g;
}

// The pair-aligned form of the dense pixel-order Gram launch.  Slots are sorted by control-pose pair key; gram_plan's equal shares ignore where a pair's
// run of slots starts, so a wave that meets such a start leaves the fast path (per-record keys, a flush through the block's CAS-keyed LDS table in mid-stream)
// and a block may meet more pairs than that table holds.  Here every streaming wave is given a range inside ONE run: each wave's whole stream is the fast
// path, its only flush is the plain-store tile at its end, and the block sums its waves' tiles per pair in wave order (a fixed order) — no LDS atomics, no
// key table.  A window has more runs than knots (the pair of a measurement is the segment of the event AND of its predecessor on the pixel: at 1 M
// uniform events on K = 21 158 runs, 68 of them shorter than a wave's share), which is why the unit of the cut is the wave and not the block: a tiny run costs one wave.
// Every wave then streams a range of its own, not a share of the block's window — taken only while the records stay in the Infinity Cache
// (records_non_temporal), and only for the dense tag-stream form in pixel order; everything else keeps the multi-key form.  opt_multikey: option gram_multikey.
constexpr uint32_t kGramMaxRuns = 4096;   // run starts the order preparation keeps; a window with more keeps the multi-key form
inline bool gram_paired(int opt_multikey, bool tags, bool sparse, bool tile_order, bool runs_known, bool records_nt)
{
    return !opt_multikey && tags && !sparse && !tile_order && runs_known && !records_nt;
}
// run_start: the n_runs sorted first slots of the runs (run_start[0] = 0); n_sw: streaming waves per block; base: gram_plan's plan of the same launch.
// cuts: [start, end) per wave slot, block/64 slots per block of which the first n_sw are used.  The share is the smallest multiple of 8 with which the
// waves fit base's blocks; past share_max (what a streaming wave of a full multi-key block walks) the grid grows instead.  A run's waves get equal shares.
struct GramPairPlan { int share; long waves; int n_gram_blocks; };
inline GramPairPlan gram_pair_cuts(const uint32_t* run_start, size_t n_runs, size_t n_cand, int n_sw, const GramPlan& base, const GramSizes& k, std::vector<uint32_t>& cuts)
{
    const long wpb = k.block / 64;
    const long slots = (long)base.n_gram_blocks * n_sw;
    const long share_max = ((wpb * k.chunk + n_sw - 1) / n_sw + 7) & ~7L;
    auto run_len = [&](size_t r) { return (long)((r + 1 < n_runs ? run_start[r + 1] : (uint32_t)n_cand) - run_start[r]); };
    auto waves_at = [&](long share) { long n = 0; for (size_t r = 0; r < n_runs; ++r) n += (run_len(r) + share - 1) / share; return n; };
    long share = (((long)n_cand + slots - 1) / std::max<long>(slots, 1) + 7) & ~7L;
    share = std::min(std::max<long>(share, k.chunk_min), share_max);
    while (share < share_max && waves_at(share) > slots) share += 8;
    GramPairPlan g{};
    g.share = (int)share;
    g.waves = waves_at(share);
    g.n_gram_blocks = (int)std::max<long>(1, (g.waves + n_sw - 1) / n_sw);
    cuts.assign((size_t)g.n_gram_blocks * wpb * 2, 0u);
    long w = 0;
    for (size_t r = 0; r < n_runs; ++r) {
        const long len = run_len(r), n = (len + share - 1) / share;
        const long each = n ? (((len + n - 1) / n + 7) & ~7L) : 0;      // (<= share: share is a multiple of 8)
        for (long i = 0; i < n; ++i, ++w) {
            const size_t at = (size_t)((w / n_sw) * wpb + w % n_sw) * 2;
            cuts[at] = run_start[r] + (uint32_t)std::min(i * each, len);
            cuts[at + 1] = run_start[r] + (uint32_t)std::min((i + 1) * each, len);
        }
    }
    return g;
}

// Tile order: the bins were predicted with the trajectory of the window's first evaluation.  Events that have since left their tile (+ margin) are still
// handled correctly, but one by one through HBM atomics; once that is a fifth of the inliers the order is rebuilt from the CURRENT trajectory at the next
// evaluation (an LM loop that starts far from its solution).
// (not again within three evaluations: a loop whose every trial moves the events further than the margin would re-bin each time)
inline bool tile_rebin_due(bool tile_order, size_t n_inliers, size_t n_outside_tile, uint32_t rec_stamp, uint32_t last_rebin_stamp)
{
    return tile_order && n_inliers && n_outside_tile * 5 > n_inliers && rec_stamp - last_rebin_stamp >= 3;
}

}  // namespace emba
