// emba_amd/csrc/context.h — the context behind the C ABI of include/emba_hip.h: what it owns in HBM, what the host knows about the window, the order,
// the evaluation, the equations and the last solve, and the helpers every host function uses (fail, HIP_TRY, ensure, nblocks).
// Included by emba_hip.hip and the host headers of its translation unit (transfer_host.h, order_host.h, step_host.h, map_host.h, readback_host.h,
// cost_host.h, options_host.h, timing_host.h, solve_host.h, poisson_host.h, render_host.h, sequence_host.h, cmax_host.h, panorama_host.h, contrast_host.h, view_host.h, mosaic_host.h, sim_host.h, frame_host.h, align_host.h, track_host.h, exposure_host.h, group.h); host code only.
#pragma once
#include "../../include/emba_hip.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <string>
#include <vector>

#include "kernels.h"
#include "solve_kernels.h"
#include "map_rule.h"
#include "cmax_rule.h"
#include "contrast_rule.h"

// Owned device memory, grow-only: ensure() re-allocates only when the buffer has to grow, so that registering the next window of a sliding-window run
// (same sizes) costs kernels, not hipMalloc / hipFree of gigabytes (measured at 100 M events: 270 ms of allocator time around 10 ms of kernels).
// The memory goes with the buffer (move-only); the context frees its buffers after draining its stream, the group each rank's with the rank's device current.
struct DevBuf {
    void* p = nullptr;
    size_t bytes = 0;     // capacity
    DevBuf() = default;
    DevBuf(DevBuf&& o) noexcept : p(o.p), bytes(o.bytes) { o.p = nullptr; o.bytes = 0; }
    DevBuf& operator=(DevBuf&& o) noexcept { if (this != &o) { reset(); std::swap(p, o.p); std::swap(bytes, o.bytes); } return *this; }
    ~DevBuf() { reset(); }
    template <typename T> T* as() const { return static_cast<T*>(p); }
    void reset() { if (p) (void)hipFree(p); p = nullptr; bytes = 0; }
    // at least n bytes (8 at the least); *fresh: the memory is new — uninitialised, or 0xFF bytes (written on `s`) with poison
    hipError_t ensure(size_t n, bool* fresh = nullptr, bool poison = false, hipStream_t s = nullptr)
    {
        n = std::max<size_t>(n, 8);
        if (fresh) *fresh = false;
        if (p && bytes >= n) return hipSuccess;
        reset();
        hipError_t e = hipMalloc(&p, n);
        if (e != hipSuccess) { p = nullptr; return e; }
        bytes = n;
        if (fresh) *fresh = true;
        return poison ? hipMemsetAsync(p, 0xFF, n, s) : hipSuccess;
    }
};

// a record set: what one evaluation wrote, per candidate slot (records_valid: stamped with the evaluation number `stamp`)
struct RecordSet { DevBuf rec, tag; uint32_t stamp = 0; };

struct SolveLists { uint32_t* off = nullptr; emba::RecView sorted{}; };   // per-pixel record lists of a solve — sorted: the participating records in pixel order; off[i]: first record of pixel i

// The normal equations currently in the pack, as the host knows them.  One value: an evaluation that sets the equations aside copies it (eq_saved), a
// rejection copies it back — whatever describes "the equations in the pack" belongs here, so that it cannot be forgotten in one of the two directions.
struct EqState {
    bool active_done = false, accum_done = false;   // emba_form_active (and its count P resolved) / emba_form_accumulate ran
    bool finish_done = false;         // emba_form_finish ran (L2 applied): the state the solvers work on
    bool compact_valid = false;       // d_compact matches the active set (built on demand)
    bool l2_fused = false;            // applyL2Reg has been applied to these blocks (by the gather of emba_step, or by emba_form_finish)
    bool force_generic_a22 = false;   // decided by form_active, read by emba_form_accumulate: the per-pixel sums were consumed, A22 | b2 come from the records
    size_t P = 0, pack_len = 0;
    int K = 0, thres = 0, irls = 0; double eta = 0;
};

// The evaluation in flight: what is known on the host about the last emba_eval_launch and the products derived from it.  begin_evaluation() is the one reset.
struct EvalState {
    bool launched = false, done = false;   // emba_eval_launch ran / its inlier count and status word have reached the host
    bool ep_deferred = false;     // residual compaction not launched yet (it rides along with the active-set kernels)
    bool inl_pending = false, P_pending = false;   // counters enqueued for readback but not yet resolved (no host sync yet)
    bool seq_armed = false;       // the pending counts come from kernels that publish the sequence number
    bool inl_idx_valid = false;   // the per-event inlier numbers are produced on demand (dumps, caller-supplied ep): 4 B/event the step does not write
    bool ep_valid = false;        // d_ep holds this evaluation's residuals in the reference's order (the resident step's Gram launch compacts them in its tail blocks)
    bool ep_in_gram = false;      // ... the Gram launch of the equations being formed will do that (set by form_active's fused branch)
    bool ep_after_gram = false;   // ... or, for windows too long for the tail form, the scan + compaction launches behind it
    bool pix_starts_valid = false;   // h_pix_starts is emba_get_inlier_pixel_starts of this evaluation (for emba_get_ep_by_pixel)
    uint32_t count_stamp = 0;     // record stamp (set_stamp) of the evaluation whose materialised, LOCAL counts d_count_own holds; 0: none (build_lists)
    int acc_irls = 0; double acc_eta = 0.0;   // the robust cost the per-pixel sums of this evaluation were weighted with
    int use_texel = 0;            // the Hessian source this evaluation uses: 0 fly, 1 full pack, 3 rectangle (step_rule.h: hessian_source)
    bool prep_on_host = false;    // no launch in front of the warp kernel: the host formed the segment records, they travel in the warp kernel's arguments (step_rule.h: prep_on_host)
    bool prep_in_warp = false;    // no launch in front of the warp kernel: its workgroup 0 formed the segment records (step_rule.h: prep_inside_warp)
    bool texels_packed = false;   // the launch in front of the warp kernel carried texel blocks (source 3: only when the texels were stale)
    int n_seg = 0;                // segment records this evaluation left in d_seg (K - 1 in the tile order and with segpose, else none): emba_dump_segments
    bool segpose = false;         // pixel order: this evaluation takes the pose per event from segment records (option segpose); emba_dump_state re-warps the same way
    bool readable() const { return launched && (done || inl_pending || ep_deferred); }   // there is an evaluation whose residuals / counts can be asked for
};

// What the host knows about the count map (d_count) and the per-pixel accumulator lines (d_pixacc): whether they have been cleared at all, whether the lines
// are zero, and whether the count map holds counts or the last warp kernel's markers.  The members change through the transitions only.
struct PixAccState {
    bool first_use() const { return dirty_all_; }     // num_ev_map.setTo(0), model.cpp:85 (+ every accumulator line) is still to be done
    bool lines_clean() const { return clean_; }       // every accumulator line is zero: the last evaluation's sums were gathered AND cleared by the resident step (no prep blocks needed)
    bool lines_consumed() const { return consumed_; } // ... so a second formNormalEq on the same evaluation rebuilds A22 | b2 from the records instead
    bool counts_raw() const { return raw_; }          // the count map holds the warp kernel's markers, not yet the counts (see ensure_counts)
    int32_t marker() const { return mark_; }          // count_marker(stamp) of the last evaluation: what its touched pixels hold in a raw count map
    void bound() { dirty_all_ = true; clean_ = false; }              // another count buffer: it says nothing about which lines are dirty
    void first_use_cleared() { dirty_all_ = false; clean_ = true; }  // both have just been zeroed
    void marked(int32_t marker) { mark_ = marker; clean_ = false; consumed_ = false; raw_ = true; }   // a warp launch marks the touched pixels and adds into their lines
    void not_marked() { raw_ = false; }                // an evaluation of an empty window: no warp launch
    void materialised() { raw_ = false; }              // a dense pass turned the markers into counts
    void consumed_by_gather() { clean_ = true; consumed_ = true; }   // the resident step's gather is the lines' only reader and zeroes them behind itself
private:
    bool dirty_all_ = true, clean_ = false, consumed_ = false, raw_ = false;
    int32_t mark_ = 0;
};

// The map planes in HBM and what the host knows about them (map_rule.h: MapState).  own, trial: the context's buffers, grown by the calls that fill them
// (map_host.h).  The current (accepted) planes are own's, or the caller's memory (emba_bind_map_dev); the planes the next evaluation reads are the current
// ones, or the trial's (emba_update_map).  The pointers and the state move together, through the functions below only.  The buffers are public so that
// ensure() can grow them: map_host.h alone writes them, and only immediately before the transition that announces what it wrote (uploaded, trial_built,
// blurred) — a filled buffer without its transition is never read.
struct MapPlanes {
    DevBuf own_x, own_y, trial_x, trial_y;
    const double* Gx() const { return x_; }           // the planes the next evaluation reads (current or trial)
    const double* Gy() const { return y_; }
    const double* cur_Gx() const { return cur_x_; }   // current (accepted) map: own upload, bound, or accepted trial
    const double* cur_Gy() const { return cur_y_; }
    const emba::MapState& state() const { return st_; }
    void uploaded() { to_own(); st_.uploaded(); }     // own_x / own_y have been filled
    void bound(const double* gx, const double* gy) { x_ = cur_x_ = gx; y_ = cur_y_ = gy; st_.bound(); }
    void trial_built() { x_ = trial_x.as<double>(); y_ = trial_y.as<double>(); st_.trial_built(); }   // trial_x / trial_y have been filled from the current planes
    // the trial buffers become the current map; our previous buffers become the next trial buffers (nothing reads them: the current map was either
    // they or a bound one)
    void accepted() { std::swap(own_x, trial_x); std::swap(own_y, trial_y); to_own(); st_.accepted(); }
    void rejected() { x_ = cur_x_; y_ = cur_y_; st_.rejected(); }
    void blurred() { to_own(); st_.blurred(); }       // own_x / own_y have been filled with the blurred current planes
    void texels_packed() { st_.texels_packed(); }
private:
    void to_own() { x_ = cur_x_ = own_x.as<double>(); y_ = cur_y_ = own_y.as<double>(); }
    const double *x_ = nullptr, *y_ = nullptr, *cur_x_ = nullptr, *cur_y_ = nullptr;
    emba::MapState st_;
};

// What the fused branch of form_active leaves for the Gram launch of the same equations (emba_form_accumulate).  Neither an evaluation nor a trial resets it:
// the halves of d_fsup alternate from step to step.
struct PostWarpState {
    bool gather_deferred = false; emba::ActiveWriteParams gather{};   // the gather of the running step, to be issued with its Gram launch
    int fsup_half = 0;                                                // the half of d_fsup the last launch A filled
    void defer(const emba::ActiveWriteParams& aw) { gather = aw; gather_deferred = true; }
};

// Call options of the internal eval_launch / form_active (the extern "C" entry points pass the defaults).  irls, eta: the robust cost the per-pixel sums are
// weighted with; keep_alt_set: the caller re-forms the equations itself, nothing of the previous ones can be gone back to — no second record set (ADVICE r3:
// +12.8 GB at 100 M events for callers that can never reject)
struct EvalOpts { int irls = 0; double eta = 0.0; bool keep_alt_set = false; };
struct FormOpts {
    bool consume = false, wants_ep = false;   // the resident step: this gather is the per-pixel sums' only reader; ... and ep is compacted with its Gram launch
    const uint8_t* global_u8 = nullptr;       // emba_step_form_active: the all-reduced saturated byte counts activity is decided from
    double fused_alpha = 0.0;                 // A22 | b2 come from the accumulator lines: applyL2Reg rides along with the gather
};

// What the host knows about the registered window (emba_set_events*).  free_window() is the one reset: a fresh value, less what it names as carried over.
struct WindowState {
    bool have_events = false;
    size_t n_in = 0, n_used = 0, n_halo = 0, n_pm = 0, n_sorted = 0, n_batch = 0, n_cand = 0;   // n_pm: pm-order entries (events + halo); n_sorted: entries of the device order
    long nblk = 0;                    // waves of the pixel-order warp kernel over the device order
    long n_fblk = 0, n_fsup = 0;      // inlier-flag blocks of kFlagBlk pm-order entries; ... summed per kFlagSup of those
    size_t P_prev = 0;                // active pixels of the last equations whose count the host has seen (this window): the Gram kernel's form is chosen by it
    // tile order: inliers found outside their tile in the last evaluation; how often a window of this context was re-binned; the evaluation that did it last
    size_t n_outside_tile = 0; int n_rebin = 0; uint32_t last_rebin_stamp = 0;
};

// The device order of the window and the decision that led to it (prepare_order).  new_order() is the one reset, at a new window and at every re-ordering.
struct OrderState {
    bool keys_ready = false; int64_t key_t0 = 0, key_dt = 0; int key_K = 0;   // the order is built, for this spline timing
    uint32_t* d_ev_pix = nullptr; uint32_t* d_ev_batch = nullptr;   // borrowed — pixel order: the pm-order arrays; tile order: d_ev_pix_own / d_ev_batch_own
    bool tile_order = false, have_ev_pm = false;
    long n_chunks = 0;                // tile order: workgroups of the tiled warp kernel
    size_t n_lead = 0;                // lead-in copies the tile order added
    bool chunks_lpt = false;          // the chunk list is sorted longest first and walked in grid order (no XCD-contiguous remapping)
    int tile_shape = 0; bool tile_fine = false;   // what the last tile search chose: index into kTileShapes, its finer pitch grid
    double order_per_px = 0.0, order_lead_frac = 0.0;   // what the last order decision saw (diagnostics: emba_last_order_stats)
    double order_inl_pred = 0.0;      // ... and the inlier fraction the predicted pixels give (the rule's estimate of what the pixel order pays per event)
    // the runs of equal pair key among the record slots (sorted first slots; known unless the window has more than kGramMaxRuns), and what the pair-aligned
    // Gram form has cut from them into d_gram_cuts: for how many streaming waves per block and which plan of gram_plan, into how many blocks (step_host.h: ensure_gram_cuts)
    std::vector<uint32_t> run_start; bool runs_known = false;
    int cuts_sw = 0, cuts_base_blocks = 0, cuts_blocks = 0;
};

// The words of a 64-byte status block (ord.status of the window registration and the order preparation; evseq.status of the resident sequence uses the
// same words, and two of its own in emba_seq_window).  The validation words hold the smallest offending index, 0xFFFFFFFF when clean.
enum StatusWord : int {
    kStFirstBad = 0,      // the first event outside the sensor (emba_validate_events_kernel, emba_seq_ingest_kernel); order_batch_segments: the first batch outside the knots
    kStUnsorted = 1,      // the first event earlier than its predecessor
    kStProbeA = 0, kStProbeB = 1,   // emba_seq_window only: the first probe past either cursor (kNoProbe = 0xFFFFFFFF: none)
    kStBadHalo = 2,       // a halo event outside the sensor
    kStTotal = 4,         // the total of a scan: measurement candidates, entries of the expanded list, halo entries
    kStHeads = 6,         // the tile search: chain heads of the pm-order
    kStCounter = 8,       // [8..9] a 64-bit counter (the tile search: predicted inliers, then a candidate's lead-ins); emba_seq_filter: the survivors' number
    kStatusWords = 16
};

// The key of the lists cache: whose records (packed: the ones this rank RECEIVED as the owner of the pixels [lo, lo + P), keyed by its own working set's stamp —
// the ranks evaluate and form in lockstep; else the local ones, lo = 0), of which evaluation, over how many pixels and records.
struct ListsKey {
    bool packed = false; uint32_t stamp = 0; size_t P = 0, nrec = 0; long lo = 0;
    bool operator==(const ListsKey& o) const { return packed == o.packed && stamp == o.stamp && P == o.P && nrec == o.nrec && lo == o.lo; }
};

// What the last solve left behind for the next one.
struct SolveCache {
    // the per-pixel record lists + pixel-ordered records of the last solve (lists.off, lists.sorted): a re-solve of the same equations with another
    // lambda (a rejected LM trial, solver.cpp:340-352) reuses them; round 6: so does the SHARDED solve — a re-solve skips count, pack and the all-to-all
    bool lists_valid = false; ListsKey key;
    bool perm_valid = false;   // sv.perm holds the column order of U for the local Schur solve (solve_perm), valid with the lists
    size_t perm_lo = 0, perm_n = 0;   // ... of the pixels [perm_lo, perm_lo + perm_n) of the active set (a rank's owned range in the sharded solve)
    size_t x2_resident_P = (size_t)-1;   // d_x2 holds the x2 of the last solve on this context (for that many pixels)
    int info = 0;              // last Schur solve: bit 0 a 2x2 block not positive definite (error), bit 1 a pivot of S vanished (zero update, like Eigen's ldlt)
    // emba_cg_shard_*: the session's sizes; its vectors are the solve scratch (sv), its lists the lists cache.  active: begin succeeded, and since then neither
    // another solve nor a failed emba_cg_shard_* call has taken the scratch
    struct CgShard { bool active = false; int rank = 0, n_ranks = 1, n = 0, skip = 0; size_t lo = 0, npix = 0, Nl = 0; double lambda = 0; } cg;
    void invalidate() { lists_valid = false; perm_valid = false; }   // the records or the active set changed: neither the lists nor the column order hold
};

// Grow-only buffers of contrast maximisation (cmax_host.h): the per-slice results of emba_seq_cmax (t_ref: one entry more than slices), and the
// candidates of emba_seq_cmax_objective with their J and their images.
struct CmaxBuffers { DevBuf omega, t_ref, j0, j, evals, cand, cand_j, cand_iwe; };

// Grow-only buffers of the pose stage of a range of the resident sequence (seq_range_poses, panorama_host.h): the midpoints and the pose table of the
// range's batches and the control poses they were evaluated from (the registered window's are left alone).  One set for the panorama and the contrast
// calls alike: each call rebuilds all three from its own arguments and synchronises the stream before it returns, so nothing in them outlives a call.
struct SeqPoseBuffers { DevBuf batch_t, pose, knots; };

// Grow-only buffers of the panorama of warped events (panorama_host.h): the int32 image [H, W]; one slot per wave of the reduction; out: J, sum, non-zero
// cells, dropped votes and the pose stage's status word; pm: the projected events, where asked for.
struct PanoBuffers { DevBuf image, slots, out, pm; };

// Grow-only buffers of the smooth contrast and its gradient (contrast_host.h): the fp64 image [H, W]; one slot per wave of the reduction; out: J, dropped
// votes, the pose stage's status word and, behind them, the gradient [3 K]; pm, D, cp: the projected events, their 2x6 Jacobians and their control-pose
// indices, where asked for.
struct ContrastBuffers { DevBuf image, slots, out, pm, D, cp; };

// The priors of the smooth contrast (contrast_host.h): per level at most one image P_l [H_l, W_l] of what earlier events of the resident
// sequence voted — present[l]: there is one; its buffer stays allocated when it is dropped (the sizes are the context's own).  out: the dropped votes per
// level of one emba_seq_contrast_prior_add and, behind them, the pose stage's status word.  All levels together are at most 4/3 of one H x W fp64 image.
struct ContrastPriors {
    DevBuf image[emba::kContrastLevels], out;
    bool present[emba::kContrastLevels] = {};
    void drop() { for (bool& b : present) b = false; }      // the sequence was replaced or re-indexed, or emba_seq_contrast_prior_clear
    void reset() { drop(); for (DevBuf& b : image) b.reset(); }      // emba_seq_free
};

// Grow-only buffers of the sensor views (view_host.h).  emba_render_views: a caller's source plane [H, W]; the frame times, their pose table and the control
// poses they were evaluated from (this stage's own: emba_ctx::seq_pose is left alone); head: the pose stage's status word; one chunk of frames as fp64,
// as bytes and as pm; outside: the count per frame.  emba_seq_event_frames: the edges, one chunk of int32 frames, ends: the events before and after.
struct ViewBuffers { DevBuf plane, t, pose, knots, head, frames, u8, pm, outside, edge, counts, ends; };

// The mosaic of intensity frames (mosaic_host.h).  sum_w, sum_v: the two uint64 sums per cell [H, W], resident between calls; votes: the frame pixels
// accumulated into them since they were last zeroed (0: nothing accumulated; below 2^36: mosaic_rule.h).  Scratch of one call: the frame times, their pose
// table and the control poses they were evaluated from (this stage's own); head: the pose stage's status word; one chunk of frames as bytes and as pm;
// counters: [0] dropped votes, [1] skipped pixels, [2] covered cells; the mean and its covered bytes; the log-intensity plane, the bytes of the cells that
// stay covered under it, and the two gradient planes.
struct MosaicBuffers {
    DevBuf sum_w, sum_v; uint64_t votes = 0;
    DevBuf t, pose, knots, head, frames, pm, counters, mean, covered, L, covered_log, gx, gy;
};

// What a stage that evaluates intensity frames and runs the per-frame Levenberg-Marquardt loop on them keeps (frame_host.h); all of it scratch of one call,
// and each stage has its own.  One chunk of frames as bytes, as pm and as residuals; partial: the evaluation kernel's sums per (frame, workgroup); q_trial,
// esums, ecounts: the rotation every frame of the chunk is evaluated at and what the evaluation gave there; q ... have_trial: the members of the rule header's
// frame state (AlignFrame, ExposureFrame), one array each; cost0, n0: the first evaluation's cost and n; running: the frames a step left running.
struct FrameLoopBuffers {
    DevBuf frames, pm, resid, partial, q_trial, esums, ecounts;
    DevBuf q, sums, counts, lambda, dnorm, status, iters, have_trial, cost0, n0, running;
};

// Intensity frames aligned to a panorama plane (align_host.h); all of it scratch of one call.  plane, valid: the plane the frames are aligned to and its mask
// (a caller's, or the mosaic's mean and covered cells).
struct AlignBuffers { DevBuf plane, valid; FrameLoopBuffers loop; };

// Intensity frames tracked against their own growing mosaic (track_host.h).  lw, lv: the two uint64 sums per cell of the levels 1 ... 7 [H_l, W_l], resident
// between calls (level 0's are the mosaic's sum_w, sum_v); voted: bit l is set when the last successful emba_frames_track voted into level l.  Scratch of one
// call, over its F frames: the frame times, every frame's rotation, status, iterations per level, cost, counts and overlap; counters: [0] dropped votes,
// [1] skipped pixels.  Over one batch (or one chunk of emba_track_eval): pred, the predicted starts, and the loop's state; loop.frames: one chunk of bytes.
// The tracker with exposure (track_exposure_host.h) keeps beside them every frame's gain and bias (gain_all, bias_all) and, over one batch, the start, the
// trial and the accepted gain and bias (gain_pred / gain_trial / gain, and the same three of the bias).  The refit (refit_host.h) keeps beside them every
// frame's code of the sweep (refit_all).
struct TrackBuffers {
    DevBuf lw[8], lv[8]; uint32_t voted = 0;
    DevBuf t, q_all, status_all, iters_all, cost_all, overlap_all, counts_all, counters, pred;
    DevBuf gain_all, bias_all, gain_pred, bias_pred, gain_trial, bias_trial, gain, bias;
    DevBuf refit_all;
    FrameLoopBuffers loop;
};

// Per-frame exposure (exposure_host.h); all of it scratch of one call.  gain_trial, bias_trial: where, with loop.q_trial, every frame of the chunk is
// evaluated; gain, bias: the rest of exposure_rule.h's ExposureFrame.  vote_gain, vote_bias: all F gains and biases of emba_mosaic_frames_exposure.  (The plane
// and its mask are AlignBuffers'; the pose table, the bytes and the counters of the vote are MosaicBuffers'.)
struct ExposureBuffers {
    FrameLoopBuffers loop;
    DevBuf gain_trial, bias_trial, gain, bias;
    DevBuf vote_gain, vote_bias;
};

// One frame aligned to another (pair_host.h); all of it scratch of one call.  loop.frames: the whole sequence [F, S], uploaded once per call (where the other
// stages keep a chunk); loop.pm: uv; the rest of loop over one chunk of pairs; pairs, gain, bias: the chunk's (i, j) and relative exposures.
struct PairBuffers { DevBuf pairs, gain, bias; FrameLoopBuffers loop; };

// The pair alignment coarse to fine (pair_level_host.h); all of it scratch of one call.  loop.frames: the whole sequence [F, S], uploaded once per call;
// bytes: the bytes [F, S_l] of every distinct level above 0 of the schedule, one behind the other; lut: their tables [S_l, 3] likewise; pairs, gain_trial,
// bias_trial, gain, bias and the rest of loop: one chunk of pairs at one level (exposure_rule.h's ExposureFrame); out_of and r_*: the chunk's result over
// the schedule (pair_level_kernels.h: PairHandoverParams).
struct PairLevelBuffers {
    DevBuf pairs, gain_trial, bias_trial, gain, bias, bytes, lut, out_of;
    DevBuf r_q, r_gain, r_bias, r_sums, r_cost0, r_counts, r_n0, r_status, r_iters, r_level_status, r_level_iters;
    FrameLoopBuffers loop;
};

// Loop-closure pairs found by appearance (match_host.h); all of it scratch of one call.  frames: the whole sequence [F, S], uploaded once per call; bytes: its
// thumbnails [F, S_l] of the level asked for (level 0: frames itself); pairs, records, sums: one chunk of a pair list, its results (match_rule.h: MatchBest)
// and the six sums of every shift; votes [F], table (the triangular table of MatchBest) and partner, score, shift, n [F, k]: a search.
struct MatchBuffers { DevBuf frames, bytes, pairs, records, sums, votes, table, partner, score, shift, n; };

// The event simulator (sim_host.h).  The simulated recording, resident: x, y, pol, t of n events (have: a simulation has succeeded, also one of no events) and
// the stats of the call that made it; x2 ... t2 take the next one and are swapped in when it has succeeded.  Scratch of one call: a caller's source plane
// [H, W]; the step times, their pose table and the control poses they were evaluated from (this stage's own); head: the pose stage's status word; frames: one
// chunk of samples and the frame in front of it; outside: the view kernel's count per frame (the simulator counts for itself); cells: events per (step,
// pixel) of a chunk, then their offsets; ref / armed: the pixels' state in front of and behind a chunk; sums: positive events, capped and outside cells;
// total: the chunk's number of events; ev_t, ev_sp: a chunk's events as emitted (the sort pairs are the order preparation's, as emba_seq_filter's are).
struct SimState {
    DevBuf x, y, pol, t, x2, y2, pol2, t2; size_t n = 0; bool have = false; uint64_t stats[4] = {0, 0, 0, 0};
    DevBuf plane, step_t, pose, knots, head, frames, outside, cells, ref[2], armed[2], sums, total, ev_t, ev_sp;
};

// Grow-only buffers of the intensity panorama (poisson_host.h).  The tables are made once per context, each when its buffer is new; the planes are scratch
// of one solve.  Forms: dense (option poisson = 1) and Fourier (every other), the latter folded (poisson_folds) or not, under either boundary.
struct PoissonBuffers {
    DevBuf SH;        // table: the sine matrix S_H (H x H); every form makes it with lamH, the dense and the unfolded Fourier form multiply by it
    DevBuf lamH;      // table: the eigenvalues lambda_H (H); every form
    DevBuf SW;        // table: the sine matrix S_W (W x W); dense
    DevBuf lamW;      // table: the eigenvalues lambda_W (W); dense
    DevBuf thomas;    // table: the Thomas factors of T_W + lambda1[i] I (W x H); Fourier
    DevBuf wrapq;     // table: q = T_{W-1}^-1 (e_0 + e_{W-2}) per H-frequency (W x H, row W-1 zero; poisson_rule.h); Fourier under EMBA_POISSON_WRAP_X
    DevBuf Sfold;     // table: S_H folded by its symmetry, two (H/2 x H/2) blocks; folded Fourier
    DevBuf Gx, Gy;    // planes: the caller's gradient maps, where the solve is given host planes and not the resident map; every form
    DevBuf F;         // plane: the divergence and every second intermediate, and at the end of a solve the panorama M (H x W); every form
    DevBuf T;         // plane: the other intermediate (Fourier: the transposed plane, W x H); every form
    DevBuf EO;        // plane: [E | O] of a folded transform (W x H/2 each); folded Fourier
};

struct emba_ctx {
    emba_cfg cfg{};
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    std::string err;

    int sw = 0, sh = 0, W = 0, H = 0;
    size_t S = 0, npix = 0;
    double fx = 0, fy = 0, cx = 0, cy = 0, C_th = 0, outlier_px = 10.0;
    double fov_x = M_PI, fov_y = M_PI;    // the sensor's field of view (rad), from the bearing LUT

    // persistent device buffers
    DevBuf d_lut;
    DevBuf d_texel;
    MapPlanes map;            // the map planes and what the host knows about them
    SolveCache solve;         // what the last solve left behind
    int solve_perm_mode = -1;                               // option solve_perm (A/B): -1 auto, 0 off, 1 on
    double* h_cost = nullptr;           // pinned: {data cost sum, reg cost sum, error word, sequence number} of the cost launch (cost_host.h), written by the kernel itself
    double* h_cost_dev = nullptr; DevBuf d_cost_acc; int cost_seq = 0;      // its device pointer; device: {data, reg} partial sums + the blocks' ticket counter (zero between calls)
    DevBuf d_x2;              // the x2 of the last solve on this context (solve.x2_resident_P)
    DevBuf d_count_own; int32_t* d_count = nullptr;
    DevBuf d_pixacc;          // per-pixel A22/b2 accumulator lines (64 B each)
    PixAccState pix;          // what the host knows about the count map and the lines
    int texel_mode = 0;   // 0 auto, 1 pack every texel, 2 always on-the-fly stencil, 3 texel rectangle (option texel)
    DevBuf d_rect;       // [0..3] {xmin,ymin,xmax,ymax} of the pixels the last formed evaluation touched; [4..7] the box the texels are PACKED for (what the warp kernel trusts)
    uint32_t seg_seq = 0;     // the flag value of the last in-warp hand-off of segment records (never 0: the flag word starts at 0)
    int step_prep = 2, step_prep_polls = 1024;   // option step_prep (A/B): 0 the launch in front of the warp kernel always, 1 none where its work fits the warp launch, 2 (default) none where the host can form the records; option step_prep_polls: the consumers' poll budget (0: none)
    emba::SegHostDuties seg_duties{}; emba::SegRecordsByValue seg_host{};   // ... and where the host formed the records (ev.prep_on_host)
    emba::InlineSegParams seg_inline{}; emba::InlineKnots seg_knots{};   // what launch_prep_pose_texel leaves for the warp launch of the same evaluation (ev.prep_in_warp)
    DevBuf d_seg_flag;   // [0] the segment records' flag (a line of its own), [32] waves that formed their records themselves (diagnostics)
    DevBuf d_blk_rect;   // per prep-block boxes
    DevBuf d_compact, d_active_bits;   // 1 bit per pixel: count >= thres of the current active set
    DevBuf d_active;
    DevBuf d_ablk_cnt, d_ablk_off; size_t n_ablk = 0;
    DevBuf d_pack_own;
    double* d_pack = nullptr; size_t pack_cap = 0; bool pack_bound = false;   // d_pack_own, or the caller's buffer (emba_bind_exchange_buffers)
    DevBuf d_knots;
    int* d_err = nullptr;           // status word of the CURRENT evaluation: one of the two words of d_err2 (they alternate: an evaluation's first launch
    DevBuf d_err2;                  // clears the NEXT evaluation's word while its own pose threads may already be setting bits of the current one)
    uint32_t eval_seq = 0;
    DevBuf d_total;                 // [0] inliers, [1] active pixels
    std::vector<uint32_t> h_pix_starts;   // emba_get_inlier_pixel_starts of the current evaluation (ev.pix_starts_valid), for emba_get_ep_by_pixel
    void* h_stage[2] = {nullptr, nullptr}; hipEvent_t stage_ev[2]{};   // two pinned 8-MB buffers: device -> PAGEABLE host memory in pipelined chunks (d2h_chunks)
    int* h_pinned = nullptr;        // pinned, device-visible status words the kernels write: [0] inliers [1] err [2] P [3], [4] step sequence number [5] the packed texels still cover the step's box (the step's number, else 0)
    int seq = 0;                    // sequence number of the last step whose post-warp kernels publish [3]
    bool spun = false;              // counts were taken by polling: later kernels of the stream may still be running
    int* h_pinned_dev = nullptr;    // the same memory through its device pointer
    double* h_knots_dev = nullptr;  // device pointer of the pinned control-pose staging buffer

    // per-window (set_events) state — all of it lives on the device (order_kernels.h); the buffers outlive the window, what the host knows of it is win / order
    WindowState win;
    OrderState order;
    DevBuf d_pm_pix, d_pm_batch, d_pm_orig;                                                         // pm-order = (sensor pixel, time): the reference's per-pixel vectors laid end to end
    DevBuf d_ev_slot;                                                                               // device order: record slot per entry
    DevBuf d_ev_pix_own, d_ev_batch_own;                                                            // tile order: the arrays order.d_ev_pix / d_ev_batch point to
    DevBuf d_ev_pm;                                                                                 // tile order only: entry -> pm index (order.have_ev_pm)
    DevBuf d_cp, d_batch_u;                                                                         // control-pose index (= spline segment) and spline parameter per batch
    DevBuf d_ev_u, d_ev_seg;                                                                        // tile order: the same per entry of the device order
    DevBuf d_chunks;                                                                                // tile order: one per workgroup of the tiled warp kernel (order.n_chunks)
    int segpose_mode = 0;      // option segpose (A/B; 0 auto = yes, 1 no, 2 yes): pixel order evaluates the pose per event from segment records (default: yes; ev.segpose)
    int order_mode = 0;        // option order: 0 auto, 1 pixel, 2 tile
    DevBuf d_batch_t, d_pose;   // pose table: 112 B per batch (pixel order; the tile order only uses it to predict the bins)
    DevBuf d_seg;                                             // tile order: per-segment constants the tiled kernel evaluates each event's pose from (12 doubles per segment)
    int step_gather = 2;    // option step_gather: how emba_step writes its active set + A22 | b2 rows — 0 the sweeping kernel (emba_active_write_kernel), 1 the list-driven
                            // gather as a kernel of its own, 2 (default) the list-driven gather as the head of the compact Gram kernel
    DevBuf d_seg_act;   // launch A's per-unit active lists (offsets inside the unit), n_ablk * kActivePix entries
    PostWarpState post;   // the deferred gather and the flag sums a fused form_active leaves for its Gram launch
    int step_one_set = 1;      // option step_one_set = 0: emba_step alternates between two record sets like an LM loop's evaluations (A/B)
    int step_fast = 1;   // option step_fast = 0: emba_step keeps the clearing pass in front of every evaluation (A/B)
    int use_tags = 1;   // the records' tags (per slot {pano pixel, stamp}) let the Gram kernel skip dead slots without fetching them (option gram_tags = 0 disables)
    DevBuf d_gram_cuts; std::vector<uint32_t> h_gram_cuts; bool last_gram_paired = false;   // the pair-aligned Gram form's wave ranges (OrderState); did the last Gram launch take that form
    DevBuf d_slot_key; uint32_t rec_stamp = 0;   // evaluation number stamped into the records (record_valid)
    // Two record sets (a rejected LM trial must not cost a re-evaluation).  `work` is the WORKING set: what
    // the last evaluation wrote and what formNormalEq and the solvers read.  An evaluation that would overwrite records the current normal
    // equations were formed from (eq.accum_done) first sets them aside — eq_saved = eq, and the other record set is swapped in; emba_map_reject /
    // emba_trial_reject swaps back and takes eq = eq_saved, so the solver can be called again with a larger lambda on untouched equations
    // (solver.cpp:340-352 reuses A, b).  Nothing else needs a second copy: the pack, the active set and the compact index are written by
    // formNormalEq only, which never runs on a rejected trial.
    RecordSet work, alt;
    bool eq_in_alt = false;   // the equations in the pack (eq_saved) belong to the OTHER set: a trial evaluation has been written since
    EqState eq, eq_saved;     // the equations in the pack; ... as they were when a trial evaluation set them aside (eq_in_alt)
    EvalState ev;             // the evaluation in flight
    DevBuf d_e_sorted, d_flag, d_inl_idx;
    int opt_poison = 0;          // option poison = 1 (tests): every NEW device allocation of the context is filled with 0xFF bytes
    int opt_tile_reserve = 2, opt_tile_shape = -1, opt_tile_fine = -1, opt_tile_min_events = 1650000, opt_tile_chunk = 0;   // emba_set_option: the tile order's window rule (prepare_order)
    int opt_gather_waves = 0, opt_chunk_order_bin = 0, opt_solve_counts = -1, opt_syrk_dense = 0, opt_syrk_lists = 0, opt_gram_sparse = -1, opt_gram_sparse_chunk = 4, opt_gram_multikey = 0, opt_syrk_min_cols = 512, opt_syrk_item_cap = 4096, opt_solve_debug = 0, opt_poisson = 0, opt_gemm64 = 0;   // emba_set_option
    int step_ep = 1;              // emba_step produces ep (what evaluateDataError returns, model.cpp:256) in every step; 0: on demand only (A/B, bench.py's no_ep block)
    DevBuf d_fblk_cnt, d_fblk_off;   // inlier-flag counts per kFlagBlk pm-order entries (win.n_fblk)
    DevBuf d_fsup;                   // ... summed per kFlagSup of those by launch A (win.n_fsup; two arrays used alternately: post.fsup_half)
    DevBuf d_ep;
    double set_events_ms = 0, prepare_ms = 0;   // wall time of the last emba_set_events[_dev] / order preparation (diagnostics)

    // per-iteration state
    size_t n_inliers = 0;
    int cost_irls = 0; double cost_eta = 0.0;   // robust cost declared with emba_set_cost: what the NEXT evaluation weights its per-pixel sums with
    double* h_knots = nullptr; int h_knots_cap = 0; hipEvent_t knots_copied = nullptr; bool knots_in_flight = false;   // pinned staging for the control poses

    // timing
    hipEvent_t ev_start[8]{}, ev_stop[8]{};
    bool kernel_timing = false;
    hipEvent_t kt_sets[16][5]{}; hipEvent_t* kt = kt_sets[0]; int kt_slot = 0;  // per slot: warp start/stop, accum start/stop (emba_enable_kernel_timing), [4]: in front of the step's first launch
    bool kt_valid[16][3]{};
    bool kt_all = false;        // emba_kernel_timing_all: also record [4], so that the four intervals [4]->[0]->[1]->[2]->[3] tile the whole step (prep | warp | post-warp | Gram)
    hipEvent_t cal_ev[2]{};     // emba_bracket_overhead_us / emba_clock_probe
    DevBuf d_probe;
    bool kt_warp_valid = false, kt_accum_valid = false;
    int n_cu = 256;  // compute units of the device (hipDeviceProp_t::multiProcessorCount)
    int ablate = 0;  // diagnostics builds only (-DEMBA_DIAG): EMBA_ABLATE bit mask; always 0 in the shipped library
    // ---- grow-only scratch, by phase.  A buffer named for two roles serves both (no phase holds it while the other runs): sharing keeps the peak down.
    struct {   // once-per-window order preparation (set_events_core, prepare_order) and the device scan / sort
        DevBuf scan_sums, scan_offs;   // dev_scan
        DevBuf sort_hist;              // dev_sort
        DevBuf status;                 // 64 B of status words (StatusWord): set_events_core, prepare_order
        DevBuf keys[2], vals[2];       // radix-sort pairs: set_events_core (pm-order), prepare_order (tile order, record slots)
        DevBuf flags;                  // set_events_core: candidate flags; prepare_order: chain-head flags, the tile binning's emit flags, candidate flags
        DevBuf pos;                    // set_events_core: candidate positions; prepare_order: head / emit positions, candidate positions
        DevBuf bin, used;              // prepare_order: tile of every entry, occupied bins
        DevBuf bin_start_or_x;         // prepare_order: first entry of every tile; emba_set_events: upload of x
        DevBuf pred_or_y;              // prepare_order: predicted pixels; emba_set_events: upload of y
        DevBuf heads_or_pol;           // prepare_order: chain heads; emba_set_events: upload of the polarities
        DevBuf halo;                   // emba_set_events: upload of the halo (times, x, y)
    } ord;
    struct Solve {   // the solvers (an LM loop solves every iteration).  Schur: emba_solve_normal_eq, emba_solve_shard_*; CG: emba_solve_normal_eq_cg, emba_cg_shard_*
        DevBuf S_or_x, rhs_or_r, U_or_p, y_or_z, cf_or_t, x2_or_invd;   // Schur: S_aug, x1, U block, y, 2x2 factors, x2; CG: x, r, p, z, t, inverse diagonal
        DevBuf info_or_sc;             // Schur: status word; CG: device scalars
        DevBuf slab, mask, list, cnt, range, pair_items, items;         // schur_accumulate: the block-sparse SYRK
        DevBuf perm_cnt, perm_tick, perm;   // solve_perm (perm: the column order, valid with solve.perm_valid)
        DevBuf shard_cnt;              // emba_solve_shard_count -> emba_solve_shard_pack: counts, offsets, cursors per rank
    } sv;
    struct {   // build_lists.  off / sorted are the lists cache (solve.lists_valid) that a re-solve, emba_solve_shard_cached / _finish and a CG session read
        DevBuf off, cursor, sorted, tmp;
    } lists;
    struct {   // downloads
        DevBuf out;          // emba_get_map_active, emba_get_inlier_pixels, the pixel list of emba_get_inlier_pixel_starts
        DevBuf pix_starts;   // emba_get_inlier_pixel_starts
        DevBuf A22b2;        // emba_form_finish: unpacked A22 | b2
    } dl;
    PoissonBuffers poisson;       // f3, the intensity panorama from the gradient map (poisson_host.h)
    // record_data images (render_kernels.h): radix-select state, its histograms (zero between uses) and candidates, the 8-bit images, a host plane's upload
    DevBuf d_rstate, d_rhist, d_rcand;
    DevBuf d_img, d_nsrc;
    // the whole (down-sampled) event sequence of a sliding-window run (sequence_kernels.h): uploaded once by emba_seq_upload, registered window by window by
    // emba_set_events_seq, which builds the window's structure from [beg, end) of these arrays and keeps no pointer into them.  raw: one chunk of the upload;
    // halo_*: emba_set_events_seq_shard's passes — last event per sensor pixel, halo flags and positions per event in front of the shard.
    // emba_seq_filter: x2 ... t2 take the survivors and are swapped with x ... t (never compacted in place); f_start: per-pixel starts of the pixel-sorted
    // sequence (S + 1), f_hot: the last filter's hot-pixel mask (S bytes, have_hot), f_sums: its eight 64-bit counters.  have: a sequence is resident (an
    // upload succeeded, also one of no events, and no filter has removed every event since).  The host code: sequence_host.h.
    struct {
        DevBuf x, y, pol, t, raw, status, halo_last, halo_flag, halo_pos; size_t n = 0;
        DevBuf x2, y2, pol2, t2, f_start, f_hot, f_sums; bool have = false, have_hot = false;
        void reset()      // emba_seq_free: every buffer above, and what the host knows about them
        {
            for (DevBuf* b : {&x, &y, &pol, &t, &raw, &status, &halo_last, &halo_flag, &halo_pos, &x2, &y2, &pol2, &t2, &f_start, &f_hot, &f_sums}) b->reset();
            n = 0; have = have_hot = false;
        }
    } evseq;
    // contrast maximisation on that sequence (cmax_host.h): the pinhole of the image plane, fitted to the bearing LUT by emba_create (ok: there is one);
    // the per-slice results of emba_seq_cmax (t_ref: one entry more, the last estimated event's time); the candidates of emba_seq_cmax_objective, their J
    // and their images.
    emba::CmaxPinhole cmax_pin;
    CmaxBuffers cmax;
    SeqPoseBuffers seq_pose;      // the pose stage of the two below (seq_range_poses)
    PanoBuffers pano;             // the panorama of warped events on that sequence (panorama_host.h)
    ContrastBuffers contrast;     // its smooth contrast and the gradient with respect to the control poses (contrast_host.h)
    ContrastPriors priors;        // what earlier events voted, per level: the image a call of emba_seq_contrast_gradient_prior starts from
    int opt_contrast_vote = -1;   // option contrast_vote: the vote kernel of a level call — -1 by the image's size (contrast_rule.h: contrast_vote_plan), 0 HBM, 1 LDS where it fits
    int contrast_vote_path = -1;  // the vote kernel the last contrast call launched: 0 HBM, 1 LDS; -1 none yet (emba_get_option "contrast_vote_path")
    ViewBuffers view;             // sensor views along the trajectory: predicted frames and event frames (view_host.h)
    SimState sim;                 // the event simulator: the simulated recording and the scratch of a call (sim_host.h)
    MosaicBuffers mosaic;         // the mosaic of intensity frames: the resident sums and the scratch of a call (mosaic_host.h)
    AlignBuffers align;           // intensity frames aligned to a panorama plane: the scratch of a call (align_host.h)
    TrackBuffers track;           // intensity frames tracked against their own growing mosaic: the level planes and the scratch of a call (track_host.h)
    ExposureBuffers exposure;     // per-frame exposure: the scratch of a call (exposure_host.h)
    PairBuffers pair;             // one frame aligned to another: the resident sequence of a call and the scratch of a chunk of pairs (pair_host.h)
    PairLevelBuffers pair_level;  // the pair alignment coarse to fine: the sequence, its pyramid and the scratch of a chunk of pairs (pair_level_host.h)
    MatchBuffers match;           // loop-closure pairs found by appearance: the sequence, its thumbnails, a chunk of pairs or the table of a search (match_host.h)
    DevBuf d_blur;                // emba_median_blur3[_map]: the plane the stencil writes (it must not read its own output)
};

namespace {

thread_local std::string g_create_error;   // the message of a failure that has no context to keep it (emba_create)

emba_status fail(emba_ctx* c, emba_status st, const char* fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (c) c->err = buf; else g_create_error = buf;
    return st;
}

#define HIP_TRY(c, call)                                                                         \
    do {                                                                                         \
        hipError_t e_ = (call);                                                                  \
        if (e_ != hipSuccess)                                                                    \
            return fail((c), EMBA_ERR_HIP, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), \
                        __FILE__, __LINE__);                                                     \
    } while (0)

// a grow-only buffer of the context (DevBuf) holds at least `count` elements of T.  Option poison (tests): new memory reads as NaN / 0xFFFFFFFF, so that a
// read of never-written memory shows.
template <typename T>
emba_status ensure(emba_ctx* c, DevBuf& b, size_t count, bool* fresh = nullptr)
{
    const hipError_t e = b.ensure(count * sizeof(T), fresh, c->opt_poison != 0, c->stream);
    if (e != hipSuccess) return fail(c, EMBA_ERR_HIP, "hipMalloc of %zu bytes failed: %s", count * sizeof(T), hipGetErrorString(e));
    return EMBA_OK;
}

// A new evaluation begins, or the last one can no longer be asked about (its window is gone, its trial was rejected): nothing that was derived from it —
// pending counters, the residual vector, inlier numbers, the pixel-starts table, the count map's stamp — outlives this (EvalState).
void begin_evaluation(emba_ctx* c) { c->ev = EvalState{}; }

inline unsigned nblocks(size_t n, unsigned per = 256) { return (unsigned)std::max<size_t>((n + per - 1) / per, 1); }
long grid8(long n) { return (n + 7) / 8 * 8; }   // a grid of whole rounds over the chip's eight XCDs

}  // namespace
