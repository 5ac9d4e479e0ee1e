/* include/emba_hip.h — C ABI of the MI355X (gfx950) implementation of EMBA's hot path.
 *
 * This is the drop-in boundary.  The reference has no FFI layer; its seam is the
 * C++ object EMBA::LEGM (reference include/emba/model.h:72-133), owned by EMBA::EMBA
 * (include/emba/emba.h:109) and called only from EMBA::solveTimeWindow (src/emba/solver.cpp:63-353).
 * The functions below are what a thin `EMBA::LEGM` adapter binds (INTEGRATION.md shows it):
 *
 *   emba_create / emba_destroy      <- LEGM::LEGM / ~LEGM                 model.cpp:56-70, model.h:80
 *   emba_set_events                 <- the EventPacket argument of evaluateDataError + the
 *                                      pose-independent part of event_map_ (event_map.h:34-47)
 *   emba_eval_data_error            <- LEGM::evaluateDataError            model.cpp:72-258
 *   emba_form_normal_eq             <- LEGM::formNormalEq / formNormalEqIRLS + applyL2Reg
 *                                                                          model.cpp:316-491, 493-687, 689-719
 *   emba_data_cost / emba_reg_cost  <- 0.5*ep.ep, evaluateRobustDataCost, evaluateRegError
 *                                                                          solver.cpp:88-91, model.cpp:260-314
 *   emba_get_A12_sparse             <- the rank-1 factors of the dense A12 of model.cpp:358,483-487
 *
 * plus the phase-level entry points (emba_*_launch / *_finish) that keep every operand resident in
 * HBM, used by bench.py and by the multi-GPU host (one process per GPU; the two exchanges per
 * Gauss-Newton iteration — the int32 pixel-count map and the fp64 normal-equation pack — are
 * all-reduced by the caller between phases on buffers it binds with emba_bind_exchange_buffers).
 *
 * Conventions: plain C, no C++ types, no exceptions across the boundary.  Every function returns an
 * emba_status; the adapter turns non-zero into LOG(FATAL) to keep the reference's fail-fast
 * contract (glog CHECKs at model.cpp:247,350,378).  All floating point is IEEE double, indices are
 * int32/uint32, exactly as in the reference.  Single caller thread per context (non-reentrant), like
 * the reference.  "host" pointers are ordinary host memory; "dev" pointers are HIP device memory of
 * the context's device.  There is NO CPU fallback: without a GPU emba_create fails with
 * EMBA_ERR_NO_DEVICE.
 */
#ifndef EMBA_HIP_H
#define EMBA_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define EMBA_ABI_VERSION 2

typedef enum {
    EMBA_OK = 0,
    EMBA_ERR_INVALID_ARG = 1,   /* null pointer, bad size, unsorted timestamps, pixel out of sensor */
    EMBA_ERR_NO_DEVICE = 2,     /* no HIP device / requested ordinal absent */
    EMBA_ERR_HIP = 3,           /* a HIP runtime call failed; see emba_last_error */
    EMBA_ERR_TIME_RANGE = 4,    /* a batch midpoint lies outside the spline's knots
                                   (BASALT_ASSERT at so3_spline.h:221-229 in the reference) */
    EMBA_ERR_STATE = 5,         /* call order violated (e.g. form before eval) */
    EMBA_ERR_CAPACITY = 6,      /* a caller-provided buffer is too small */
    EMBA_ERR_NUMERIC = 7        /* a 2x2 block A22_i + lambda*diag(A22_i) is not positive definite: the reference's A22m_i.inverse()
                                   (model.cpp:750) yields inf/nan there and the LM step is lost.  (A vanishing pivot of the Schur
                                   complement is NOT an error: like Eigen's ldlt, model.cpp:789, it gives a zero update.) */
} emba_status;

typedef struct emba_ctx emba_ctx;

typedef struct {
    int32_t sensor_w, sensor_h;   /* camera_info.width/height        (model.cpp:67-68) */
    int32_t pano_w, pano_h;       /* panorama size, W = 2H           (emba.cpp:552-553) */
    const double* bearing_lut;    /* host, sensor_w*sensor_h*3 f64, row-major by y*w+x: the
                                     precomputed_bearing_vectors_ of event_pano_warper.cpp:27-41 */
    double C_th;                  /* contrast threshold               (model.cpp:60) */
    int32_t event_batch;          /* 0 or 100: the reference hard-codes 100 (model.cpp:78) */
    double outlier_px;            /* 0 -> 10.0                        (model.cpp:200) */
    int32_t device;               /* HIP device ordinal */
    void* stream;                 /* hipStream_t to enqueue on, or NULL for the context's own stream */
} emba_cfg;

/* Library/ABI identification (no GPU needed). */
int emba_abi_version(void);
const char* emba_build_info(void);

emba_status emba_create(const emba_cfg* cfg, emba_ctx** out);
void emba_destroy(emba_ctx* ctx);
/* Human-readable description of the last non-OK status on this context (or of a failed
 * emba_create when ctx == NULL). */
const char* emba_last_error(const emba_ctx* ctx);

/* Once per time window.  Events sorted by time (rosbag_loading.cpp:61-65 order is taken as
 * ground truth, quirk Q10); the last n % 100 events are ignored (quirk Q1, model.cpp:77-79).
 * Builds the pose-independent structure the reference rebuilds on every evaluateDataError call:
 * per-batch midpoint times (model.cpp:116-119), the per-sensor-pixel event lists
 * (event_map.h:34-47) laid out pixel-major in HBM, and uploads them.
 *
 * Sharding: a rank holds a contiguous range of whole global batches and, in
 * halo_*, for each sensor pixel the LAST event before its range (if any) together with the
 * midpoint time of the batch that event belongs to; halo events are warped but are not
 * measurements of this rank.  Pass n_halo = 0 on a single GPU. */
emba_status emba_set_events(emba_ctx* ctx, const uint16_t* x, const uint16_t* y, const uint8_t* pol,
                            const int64_t* t_ns, size_t n,
                            const uint16_t* halo_x, const uint16_t* halo_y,
                            const int64_t* halo_batch_t_ns, size_t n_halo);

/* The same with every array already in HBM (device pointers; t_ns is needed here: validation and the batch midpoints run on the
 * device too).  Nothing of the once-per-window structure is built on the host: the (sensor pixel, time) order is a stable LSD
 * radix sort, the record slots a second one by control-pose pair (emba_amd/csrc/order_kernels.h).  The arrays may be freed
 * when the call returns. */
emba_status emba_set_events_dev(emba_ctx* ctx, const uint16_t* x_dev, const uint16_t* y_dev, const uint8_t* pol_dev,
                                const int64_t* t_ns_dev, size_t n,
                                const uint16_t* halo_x_dev, const uint16_t* halo_y_dev,
                                const int64_t* halo_batch_t_ns_dev, size_t n_halo);

/* Diagnostics of the once-per-window work: wall time of the last emba_set_events[_dev] and of the order preparation done by
 * the first evaluation (control-pose pairs, record slots, optional tile order), whether the tile order is in use (events grouped
 * by the panorama tile the first trajectory sends their chain segment to: option "order"), entries of the device order (events +
 * halo / lead-in copies) and workgroup chunks of the tiled kernel.  Any pointer may be NULL. */
emba_status emba_last_setup_ms(const emba_ctx* ctx, double* set_events_ms, double* prepare_ms, int32_t* tile_order,
                               size_t* n_entries, size_t* n_chunks);

/* What the last pixel / tile order decision of a window saw (at its first evaluation): events per panorama pixel of the occupied cells of the tile-origin grid
 * under the first trajectory, and the fraction of lead-in copies the tile order would add.  Diagnostics; either pointer may be NULL. */
emba_status emba_last_order_stats(const emba_ctx* ctx, double* events_per_pano_px, double* lead_in_frac);
/* ... and the inlier fraction it estimated from the predicted pixels (round 6: the rule prices the pixel order per inlier and the tile order per entry). */
emba_status emba_last_order_inlier_estimate(const emba_ctx* ctx, double* inlier_frac);
/* The LDS tile that decision chose for the window (round 6: one of four shapes of 1152 panorama pixels), the pitch of its origin grid and the reserve kept free
 * on every side of a tile for the drift of trial poses (options tile_shape, tile_fine, tile_reserve).  Diagnostics; any pointer may be NULL. */
emba_status emba_last_tile_geometry(const emba_ctx* ctx, int32_t* tile_w, int32_t* tile_h, int32_t* pitch_x, int32_t* pitch_y, int32_t* reserve);

/* Tile order only: inliers of the last resolved evaluation that the tiled kernel found outside their LDS tile — the
 * trajectory has moved them since the order was built; they are handled correctly, one HBM atomic each — and how many times this
 * context has rebuilt the order of a window for that reason (done at the next evaluation once a fifth of the inliers are outside).
 * No reference counterpart (the reference has no device order).  Either pointer may be NULL. */
emba_status emba_last_tile_drift(const emba_ctx* ctx, size_t* n_outside, int32_t* n_rebin);

/* Number of events actually used (floor(n/100)*100) and of measurement candidates
 * (events that have a predecessor at their sensor pixel). */
emba_status emba_event_counts(const emba_ctx* ctx, size_t* n_used, size_t* n_candidates);

/* ---- one-shot, host-buffer entry points (what the LEGM adapter calls) ------------------------ */

/* LEGM::evaluateDataError(traj, Gx, Gy, events, eval_deriv=true, num_ev_map)   model.cpp:72-258.
 * knots_xyzw: K unit quaternions (x,y,z,w) = traj->getControlPose(i).unit_quaternion();
 * t0_ns/dt_ns: the spline's start_t_ns_/dt_ns_ (trajectory.cpp:59-64).
 * Gx, Gy: host, pano_h*pano_w f64 row-major (CV_64FC1 continuous); both NULL = use the map already resident on the
 * device (emba_upload_map / emba_bind_map_dev / emba_update_map).
 * ep_out: host, capacity >= n_used, receives the residuals in the reference's order (sensor pixel
 * major, then time; model.cpp:179-186,221); *n_inliers = ep.size().  num_ev_map_out: host int32
 * pano_h*pano_w (model.cpp:227) or NULL.  eval_deriv must be non-zero (the reference never passes
 * false, solver.cpp:75,251; quirk Q4). */
emba_status emba_eval_data_error(emba_ctx* ctx, const double* knots_xyzw, int32_t K, int64_t t0_ns,
                                 int64_t dt_ns, const double* Gx, const double* Gy, int32_t eval_deriv,
                                 double* ep_out, size_t* n_inliers, int32_t* num_ev_map_out);

/* LEGM::formNormalEq[IRLS] + LEGM::applyL2Reg   model.cpp:316-491, 493-687, 689-719.
 * Uses the device-resident state of the last emba_eval_data_error (the reference's hidden
 * event_map_ coupling, solver.cpp:99-102).  ep: host residuals to use (same layout as ep_out) or
 * NULL for the device-resident ones.  irls: 0 quadratic, 1 huber, 2 cauchy (model.cpp:599-618);
 * eta its parameter.  alpha: L2 weight; pass 0 to skip applyL2Reg.
 * Outputs (host; any may be NULL): A11 3K*3K col-major, b1 3K, *P active pixels,
 * active_idx (cap pano_h*pano_w, ascending pano index = std::set order, model.cpp:371-377),
 * A22 P*4 (each block [xx xy; xy yy]), b2 2P, A12_dense 3K x 2P col-major (model.cpp:358; only
 * sensible at small sizes — 3K*2P*8 bytes).  cap_P bounds A22/b2/A12 capacity in pixels. */
emba_status emba_form_normal_eq(emba_ctx* ctx, const double* ep, int32_t thres_valid_pixel,
                                int32_t irls, double eta, double alpha, double* A11, double* b1,
                                size_t* P, uint32_t* active_idx, size_t cap_P, double* A22, double* b2,
                                double* A12_dense);

/* Sparse form of A12: one rank-1 factor per measurement candidate, in the device's
 * (control-pose-pair)-sorted order.  A12[3*cp_c+i, 2*pix+d] += w*jc[i]*dp[d];
 * A12[3*cp_p+i, 2*pix+d] += w*jp[i]*dp[d].  pix = -1 marks outliers / inactive pixels.
 * All pointers host, capacity n_candidates (see emba_event_counts); any may be NULL. */
emba_status emba_get_A12_sparse(emba_ctx* ctx, int32_t* cp_c, int32_t* cp_p, int32_t* pix, double* w,
                                double* jc /*n*6*/, double* jp /*n*6*/, double* dp /*n*2*/);

/* Enqueue the compaction of the last evaluation's residuals into the reference-order vector `ep` (model.cpp:221,256) and the per-event inlier
 * numbers, on the device.  Nothing on the device reads `ep`.  The resident step (emba_step, option step_ep) produces it in the tail blocks of its
 * Gram launch (round 5) — this call is then a no-op; the phase-level calls of an LM loop leave it to whoever asks; the one-shot
 * emba_eval_data_error always pays for it. */
emba_status emba_compact_ep(emba_ctx* ctx);
/* The last evaluation's `ep` (what LEGM::evaluateDataError returns, model.cpp:256) to the host: as the resident step left it, or compacted now.
 * ep_host: capacity `cap` doubles (EMBA_ERR_CAPACITY below the inlier count); *n_inliers (may be NULL) its length.  Synchronizes. */
emba_status emba_get_ep(emba_ctx* ctx, double* ep_host, size_t cap, size_t* n_inliers);

/* Sensor pixel (y * sensor_w + x) of every inlier measurement of the last evaluation, in the order of ep (sensor pixel major, then time;
 * model.cpp:179-186): pix_host has capacity n_inliers.  What a multi-GPU host merges the ranks' residual vectors by (emba_group_eval). */
emba_status emba_get_inlier_pixels(emba_ctx* ctx, uint32_t* pix_host);
/* The same in S + 1 words (S = sensor_w * sensor_h): starts_host[p] = number of inlier measurements at sensor pixels < p, i.e. where pixel p's residuals begin in this
 * context's ep; starts_host[S] = the inlier count.  Kept by the context for emba_get_ep_by_pixel.  Synchronizes. */
emba_status emba_get_inlier_pixel_starts(emba_ctx* ctx, uint32_t* starts_host);
/* The last evaluation's ep placed pixel block by pixel block: the residuals of sensor pixel p go to ep_out[dst[p] ...] (dst: S element offsets).  What a multi-GPU host
 * merges time-sharded ranks' residual vectors with (model.cpp:179-186 orders them by sensor pixel, then time: inside a pixel, earlier ranks first): every rank writes
 * its own pieces of ONE output vector, streamed through pinned buffers, and ranks may do so concurrently from their own threads.  Synchronizes. */
emba_status emba_get_ep_by_pixel(emba_ctx* ctx, double* ep_out, const uint64_t* dst);

/* Cost terms of the caller (solver.cpp:88-91,257-268), reduced on the device from the resident
 * residuals / map: data = 0.5*ep.ep (irls 0) or evaluateRobustDataCost (model.cpp:279-314);
 * reg = 0.5*alpha*sum(Gx^2+Gy^2) over all pixels (model.cpp:260-277). */
emba_status emba_data_cost(emba_ctx* ctx, int32_t irls, double eta, double* cost);
emba_status emba_reg_cost(emba_ctx* ctx, double alpha, double* cost);
/* Both terms with one host synchronisation (the LM loop asks for them together at every trial point, solver.cpp:88-91, 265-268).
 * reg_cost may be NULL (a rank of a sharded host whose map is a replica).  emba_costs_launch / emba_costs_finish: the same in two halves, so
 * that a multi-GPU host can enqueue every rank's reductions before it waits for any. */
emba_status emba_costs(emba_ctx* ctx, int32_t irls, double eta, double alpha, double* data_cost, double* reg_cost);
emba_status emba_costs_launch(emba_ctx* ctx, int32_t irls, double eta, int32_t with_reg);
emba_status emba_costs_finish(emba_ctx* ctx, int32_t irls, double eta, double alpha, double* data_cost, double* reg_cost);

/* Per-event state dump in ORIGINAL (time) order for parity tests: what State_LEGM holds after
 * evaluateDataError (state.h:56-83).  All host, capacity n; any may be NULL.
 * pm n*2, D n*12 (dpm_ddrot_cp row-major 2x6), cp_idx n, inlier_idx n (-1 outlier, -2 not a
 * measurement), pm_int n*2 (-1 if not an inlier), dp/Gpm/temp n*2. */
emba_status emba_dump_state(emba_ctx* ctx, double* pm, double* D, int32_t* cp_idx, int32_t* inlier_idx,
                            int32_t* pm_int, double* dp, double* Gpm, double* temp);
/* The segment records the last evaluation left on the device, for parity tests: 12 doubles {p0 xyzw, delta xyz, r1, k xyz, r2} per pair of
 * neighbouring control poses, K - 1 of them in the tile order and in pixel order with the pose per event, none with the per-batch pose table.
 * *n_seg (may be NULL) their number; seg (host, capacity `cap` records; NULL to ask for the number only).  Synchronizes. */
emba_status emba_dump_segments(emba_ctx* ctx, double* seg, size_t cap, size_t* n_seg);

/* ---- phase-level, HBM-resident entry points (bench.py, multi-GPU host) ----------------------- */

/* Copy the map to the device (host -> HBM), or adopt caller-owned device planes without a copy. */
emba_status emba_upload_map(emba_ctx* ctx, const double* Gx_host, const double* Gy_host);
emba_status emba_bind_map_dev(emba_ctx* ctx, const double* Gx_dev, const double* Gy_dev);

/* LM-loop residency: LEGM::updateMap(Gx_new, Gy_new, x2, damping, active, inactive), model.cpp:863-903, on
 * the device-resident map with the active set of the last emba_form_active: trial = current; trial[active_i] += damping*x2[2i],
 * x2[2i+1]; trial[every other pixel] = 0.  From then on evaluations use the TRIAL map (pass Gx = Gy = NULL to
 * emba_eval_data_error, or call emba_eval_launch) until the caller reports the LM decision: emba_map_accept makes the trial map
 * current (solver.cpp:299-339), emba_map_reject drops it (:340-352; with no trial map pending it is emba_trial_reject).  x2_host: 2P doubles, or NULL: the x2 the last
 * emba_solve_normal_eq[_cg] on this context left on the device (the reference hands x2 from the solver straight to updateMap,
 * solver.cpp:193-239 — 2P doubles that need not cross to the host and back).  emba_update_map_dev: x2 in device memory (a sharded
 * host's all-reduced x2), NULL as above.  emba_download_map copies the map the next evaluation would use. */
emba_status emba_update_map(emba_ctx* ctx, const double* x2_host, double damping);
emba_status emba_update_map_dev(emba_ctx* ctx, const double* x2_dev, double damping);
emba_status emba_map_accept(emba_ctx* ctx);
emba_status emba_map_reject(emba_ctx* ctx);
/* A rejected LM trial without a re-evaluation (solver.cpp:340-352 simply reuses A and b).  An evaluation that follows emba_form_* writes its
 * factor records into a SECOND record set, so the records, pack and active set the current normal equations consist of stay intact while
 * the trial point is evaluated.  emba_trial_reject (called by emba_map_reject; callable on its own when no map update was involved) makes
 * them current again: emba_solve_normal_eq[_cg], emba_update_map, emba_form_finish downloads work as if the trial evaluation had not
 * happened.  An ACCEPTED trial needs no call: the following emba_form_* forms new equations from the trial's records.  After a rejection
 * formNormalEq needs a new evaluation first (count map and per-pixel sums are the trial's). */
emba_status emba_trial_reject(emba_ctx* ctx);
emba_status emba_download_map(emba_ctx* ctx, double* Gx_host, double* Gy_host);
/* The map the next evaluation would use (the trial map after emba_update_map), at the P pixels of the current active set only:
 * gxy_host[2i] = Gx[active_i], gxy_host[2i+1] = Gy[active_i].  By model.cpp:892-901 the trial map is ZERO at every other pixel, so this is the
 * whole result of LEGM::updateMap in 16 B x P instead of 16 B x H x W (the drop-in adapter zero-fills the caller's Mats around it). */
emba_status emba_get_map_active(emba_ctx* ctx, double* gxy_host, size_t cap_P);

/* Intensity panorama from the gradient map: poisson_reconstruction::reconstructFromGradient,
 * src/image_rec/poisson_reconstruction.cpp:9-50 + pde::poisolve (Dirichlet, zero boundary), src/image_rec/laplace.cpp:587-797,
 * as the reference calls it for its map images (solver.cpp:417,471).  Gx_host/Gy_host: pano_h x pano_w row-major doubles, or
 * both NULL to use the map resident on the device (the one the next evaluation would use).  M_host: pano_h x pano_w doubles,
 * or NULL to leave the result in the context's device buffer (timing).  The 2-D DST-I is applied as products with the sine
 * matrix on the fp64 matrix cores (the transform lengths 2(n+1) have large prime factors); the matrices are built on first
 * use and kept (8 (H^2 + W^2) bytes). */
emba_status emba_reconstruct_intensity(emba_ctx* ctx, const double* Gx_host, const double* Gy_host, double* M_host);
/* The same reconstruction under a boundary rule.  The panorama is equirectangular: column W-1 is the neighbour of column 0.
 *   EMBA_POISSON_DIRICHLET  the reference's rule, above: the image is a flat rectangle with intensity 0 all round; the last row and the last column of the
 *                           divergence are 0.  emba_reconstruct_intensity and emba_render_map_images are the _bc forms at this boundary, bit for bit.
 *   EMBA_POISSON_WRAP_X     wrap in x, and the reference's zero Dirichlet rows beyond the poles.  Divergence, for every row i < H-1 and EVERY column j:
 *                               F[i][j] = Gx[i][(j+1) mod W] - Gx[i][j] + Gy[i+1][j] - Gy[i][j]            (row H-1 of F is 0, as in the reference)
 *                           M solves  M[i-1][j] + M[i+1][j] + M[i][(j-1) mod W] + M[i][(j+1) mod W] - 4 M[i][j] = F[i][j]  with M[-1][:] = M[H][:] = 0, i.e.
 *                               M = DST-I_H( FFT_W^-1( FFT_W(DST-I_H(F)) / (lambda1[i] + mu[k]) ) ) / (2 (H+1)),
 *                               lambda1[i] = -4 sin^2(pi (i+1) / (2 (H+1))),  mu[k] = -4 sin^2(pi k / W).
 *                           lambda1[i] + mu[k] <= lambda1[0] < 0: never singular, no null space, no mean to fix.  Rolling Gx, Gy by k columns rolls M.
 *                           On the device: the DST-I along H as above, and per H-frequency the cyclic system along W, condensed on its last unknown.
 * Refused, with the outputs and the context as they were: a boundary that is neither (EMBA_ERR_INVALID_ARG); EMBA_POISSON_WRAP_X on a panorama of fewer than 3
 * columns (EMBA_ERR_INVALID_ARG) or with option poisson = 1, whose dense sine transforms along W have no wrapped meaning (EMBA_ERR_STATE).  Options poisson = 2
 * and gemm64 keep their meaning.  emba_render_map_images_bc checks the boundary whether or not poisson_u8 is given. */
#define EMBA_POISSON_DIRICHLET 0
#define EMBA_POISSON_WRAP_X 1
emba_status emba_reconstruct_intensity_bc(emba_ctx* ctx, const double* Gx_host, const double* Gy_host, double* M_host, int boundary);

/* The map images of the reference's record_data output (EMBA::saveEvoData / saveOptData, solver.cpp:370-479), rendered on the device from the map the
 * next evaluation would use (the one emba_download_map copies).  Host pointers, H x W bytes each (rgb_u8: H x W x 3, interleaved R, G, B); a NULL pointer
 * skips that image, a NULL poisson_u8 also skips the Poisson solve.
 *   gx_u8 / gy_u8   image_util::normalizeRobust(G, pct_discard) (image_utils.cpp:14-38): rmin / rmax are the exact order statistics of ranks
 *                   int(f32(0.5 pct / 100) * n) and int(f32(1 - 0.5 pct / 100) * n) (clamped to n - 1), u8 = sat(rint(scale (v - rmin))),
 *                   scale = 255 / (rmax - rmin) or 1 when rmax == rmin — bit for bit emba_amd/io.normalize_robust
 *   rgb_u8          hue = 0.5 * orientation of (Gx, Gy) in degrees, min-max normalised to [0, 179]; S = 255; value = magnitude, min-max normalised to
 *                   [0, 255]; OpenCV's 8-bit HSV -> RGB (render_kernels.h states the arithmetic; not pinned against OpenCV's approximate cartToPolar)
 *   poisson_u8      emba_reconstruct_intensity of the resident map, robust-normalised as above
 * The images come back through the context's pinned staging buffers; the call returns when they are in host memory. */
emba_status emba_render_map_images(emba_ctx* ctx, double pct_discard, uint8_t* gx_u8, uint8_t* gy_u8, uint8_t* rgb_u8, uint8_t* poisson_u8);
/* poisson_u8 from emba_reconstruct_intensity_bc at `boundary`; everything else as above. */
emba_status emba_render_map_images_bc(emba_ctx* ctx, double pct_discard, uint8_t* gx_u8, uint8_t* gy_u8, uint8_t* rgb_u8, uint8_t* poisson_u8, int boundary);
/* The same robust normalisation of any plane of n doubles (host memory): dst_host (n bytes, or NULL) and the order statistics rmin / rmax (or NULL).
 * Needs a context only (no map, no events). */
emba_status emba_normalize_robust(emba_ctx* ctx, const double* src_host, size_t n, double pct_discard, uint8_t* dst_host, double* rmin, double* rmax);

/* ---- A whole recording refined in sliding windows: what EMBA::EMBA + EMBA::Run do around solveTimeWindow (emba.cpp:281-304, 357-364, 400-532) ----
 * The event sequence crosses to the device ONCE and stays there; every time window is then registered from a range of it (overlapping windows
 * re-read HBM, not host memory).  The library keeps no host copy of the sequence.  emba_amd/driver.py: run_sequence is the caller.
 *
 * emba_seq_upload: the event down-sampling of emba.cpp:281-304 and the checks of emba_set_events, on the device.  Host arrays of the WHOLE sequence (sorted
 * by time) go through the context's pinned staging buffers in chunks; every raw event is checked (a pixel outside the sensor or a timestamp earlier than its
 * predecessor anywhere in the sequence: EMBA_ERR_INVALID_ARG, and no sequence is resident afterwards).  sampling_rate <= 1 keeps every event; otherwise
 * exactly the events with original index rate-1, 2 rate-1, ... survive (sampling_count reaches the rate at every rate-th event), *n_kept = n / rate
 * (may be NULL).  A second upload replaces the first.  emba_seq_size: events resident (0: none).  emba_seq_free releases the memory (emba_destroy does too). */
emba_status emba_seq_upload(emba_ctx* ctx, const uint16_t* x, const uint16_t* y, const uint8_t* pol, const int64_t* t_ns, size_t n,
                            int32_t sampling_rate, size_t* n_kept);
emba_status emba_seq_size(const emba_ctx* ctx, size_t* n);
emba_status emba_seq_free(emba_ctx* ctx);
/* EMBA::getEventSubset (emba.cpp:473-510) on the resident sequence of length n, one launch: with a = t_beg_ns + 1 000 000 and b = t_end_ns - 1 000 000
 * (t_epsilon = ros::Duration(1e-3); ros::Time comparison is integer comparison), *beg = the smallest multiple of 100 below n with t[beg] > a, or the first
 * multiple of 100 >= n if there is none; end0 = the smallest multiple of 100 in [beg, n) with t[end0] > b; *end = end0 - 100 if it exists, else n.
 * Where the reference's tail search stops at its first probe (end0 == beg) its `idx_ev_subset_end -= 100` underflows size_t (beg == 0: the subset silently
 * becomes the whole sequence) or leaves end < beg, and where no event lies behind a and n is no multiple of 100 it also ends with end < beg: a vector
 * built from a reversed iterator range, undefined behaviour.  Both are EMBA_ERR_INVALID_ARG ("window holds no events") here. */
emba_status emba_seq_window(emba_ctx* ctx, int64_t t_beg_ns, int64_t t_end_ns, size_t* beg, size_t* end);
/* event_subset_ = events_[beg, end) (emba.cpp:508-509) handed to solveTimeWindow: registers that range of the resident sequence as the context's window,
 * exactly as emba_set_events_dev does with pointers into it — no copy, no halo (a rank of a time-sharded window: emba_set_events_seq_shard below);
 * emba_last_setup_ms reports it like any other registration.  The sequence stays valid across windows and across emba_set_events* calls. */
emba_status emba_set_events_seq(emba_ctx* ctx, size_t beg, size_t end);
/* A time shard of a window (the window is the event_subset_ of emba.cpp:473-510): this rank's part [lo, hi) of the window that begins at win_beg of
 * the resident sequence.  The halo — for every sensor pixel with an event in [win_beg, lo) its last such event k, in ascending k, as (x[k], y[k], midpoint of
 * the WINDOW's batch (k - win_beg) / 100, model.cpp:116-119) — is built on the device from the resident arrays (three passes: last event per pixel, flags +
 * scan, gather; one small read for the count), then the range is registered exactly as emba_set_events_dev(x + lo, ..., hi - lo, halo ...) would: what
 * emba_group_set_events / emba_amd.sharded.shard_events compute on the host from a slice, bit for bit.  lo == win_beg: identical to
 * emba_set_events_seq(lo, hi).  emba_last_setup_ms includes the halo passes.  EMBA_ERR_INVALID_ARG: not win_beg <= lo <= hi <= n, or
 * (lo - win_beg) % 100 != 0 — the registered window is then left as it was. */
emba_status emba_set_events_seq_shard(emba_ctx* ctx, size_t win_beg, size_t lo, size_t hi);
/* The halo that call builds, to the host (tests, diagnostics): capacity cap entries each (EMBA_ERR_CAPACITY below *n_halo, which is set);
 * array pointers may be NULL to ask for the count only.  Leaves the registered window as it is. */
emba_status emba_seq_halo(emba_ctx* ctx, size_t win_beg, size_t lo, uint16_t* hx, uint16_t* hy, int64_t* hbt, size_t cap, size_t* n_halo);
/* [beg, end) of the resident sequence back to the host (tests, diagnostics): capacity end - beg each; any pointer may be NULL. */
emba_status emba_seq_get(emba_ctx* ctx, size_t beg, size_t end, uint16_t* x, uint16_t* y, uint8_t* pol, int64_t* t_ns);

/* ---- Sensor noise (no counterpart in the reference, whose only defence is outlier_px): hot pixels, bursts at one pixel and isolated background-activity
 * events of a DVS / DAVIS recording are removed from the resident sequence on the device, once per recording, before any window is cut from it.
 * Every event is judged from the RAW resident sequence (sorted by time; "earlier" = smaller index, which also orders equal timestamps), with
 * p(k) = y[k] * sensor_w + x[k], so the three tests are independent:
 *   hot pixels   (hot_sigma > 0)       c[p] = events of pixel p, m = pixels with c > 0, s1 = sum c = n, s2 = sum c^2 (exact, uint64); in double, one rounding per
 *                                      operation (no fused multiply-add): mean = s1 / m, var = s2 / m - mean * mean (0 if negative), thr = mean + hot_sigma * sqrt(var).
 *                                      Pixel p is hot iff double(c[p]) > thr; every event of a hot pixel fails.
 *   refractory   (refractory_ns > 0)   prev(k) = the latest earlier event of the same pixel, surviving or not; k fails iff it exists and t[k] - t[prev(k)] < refractory_ns.
 *   support      (support_ns > 0)      k passes iff an earlier event j at one of the up to eight neighbouring pixels inside the sensor (not the pixel itself),
 *                                      that pixel not hot, has t[k] - t[j] <= support_ns (only the latest earlier event of each neighbour matters).
 * The survivors — the events that fail no enabled test — keep their order; the down-sampling of emba.cpp:281-304 then runs over the SURVIVORS: with
 * sampling_rate >= 2 the survivor of rank r (from 0) is kept iff (r + 1) % sampling_rate == 0.  stats (6 values, may be NULL): events in, hot pixels, events
 * failing hot, failing refractory, failing support (each counted over all events on its own: overlaps count in each), events kept.
 * With every test off and sampling_rate <= 1 the sequence is left exactly as it is.  The survivors are gathered into fresh arrays that replace the resident
 * ones; a registered window is not disturbed (emba_set_events_seq keeps no pointer into the sequence), ranges taken from emba_seq_window before the call no
 * longer apply.  EMBA_ERR_STATE: no sequence resident.  EMBA_ERR_INVALID_ARG: hot_sigma is NaN, or 2^32 events or more (the sort carries 32-bit event
 * indices) — the sequence is then left as it was.  Every event removed: EMBA_OK with stats[5] = 0, and no sequence is resident afterwards (emba_seq_size: 0).
 * "Resident" is asked by emba_seq_filter and emba_group_seq_filter alone: a successful emba_seq_upload makes a sequence resident, also one of no events (the
 * filter of it is EMBA_OK with all-zero statistics); emba_seq_free, a failed upload and a filter that removes every event end that, and a further filter
 * is then EMBA_ERR_STATE until the next upload.  Every other emba_seq_* call and emba_set_events_seq* go by the event count, as before: they see a
 * sequence of 0 events (emba_seq_window: the empty range; emba_seq_get and emba_set_events_seq: the range [0, 0) only).  Lack of memory: EMBA_ERR_HIP, with
 * the sequence and the previous filter's hot mask left as they were (every allocation precedes the first write).
 * emba_amd.io.filter_events is the same rule in numpy.  Launches and timings: DESIGN.md §10. */
emba_status emba_seq_filter(emba_ctx* ctx, double hot_sigma, int64_t refractory_ns, int64_t support_ns, int32_t sampling_rate, uint64_t* stats);
/* The hot pixels of the last emba_seq_filter on this context: sensor_w * sensor_h bytes, 1 = hot (all 0 where hot_sigma was off).  EMBA_ERR_STATE before any. */
emba_status emba_seq_hot_pixels(emba_ctx* ctx, uint8_t* mask_host);

/* ---- Angular velocity from the events alone: contrast maximisation (Gallego & Scaramuzza, RA-L 2017; no counterpart in the reference, which takes its raw
 * poses from a front end) on the resident sequence as it stands (after any filter and down-sampling), n events.  For every slice of m = slice_events events,
 * slice s = [s m, (s + 1) m), s < n_slices = n / m (the tail behind the last whole slice is not estimated), t_ref(s) = t[s m], the angular velocity w whose
 * image of warped events is sharpest.  The objective is exact integer arithmetic, so emba_amd.io.cmax_objective / estimate_angular_velocity (numpy) give the
 * same numbers bit for bit and the search takes the same decisions.  All floating point below: IEEE double, one rounding per operation (no fused
 * multiply-add), in the order written.
 *   warp of event k   dt = double(t[k] - t_ref) * 1e-9, a = w * (dt * 0.5), b = bearing_lut[y[k] * sensor_w + x[k]],
 *                     aa = (ax ax + ay ay) + az az, c = a x b, d = a x c (cx = ay bz - az by, ...), b' = (1 + aa) * b + 2 * (c + d): the unnormalised Cayley
 *                     rotation of b about w, by 2 atan(|w| dt / 2) rather than |w| dt (relative difference (|w| dt)^2 / 12: DESIGN.md §11).
 *   image plane       an ideal pinhole fitted to the LUT alone: u = f * (b'x / b'z) + cu, v = f * (b'y / b'z) + cv; f, cu, cv by least squares over the
 *                     LUT's centre row and centre column (the formula: emba_amd/csrc/cmax_rule.h, cmax_pinhole_fit).  b'z <= 0 votes nowhere.
 *   votes             cells of 2^shift sensor pixels, shift the smallest for which ceil(w / 2^shift) x ceil(h / 2^shift) uint32 cells fit 64 KiB (240x180:
 *                     shift 1, 120x90; 64x48: shift 0).  g = u / 2^shift (v likewise), i = floor(g), wx = floor((gx - ix) * 16), wy likewise; the cells
 *                     (ix, iy), (ix + 1, iy), (ix, iy + 1), (ix + 1, iy + 1) get (16 - wx)(16 - wy), wx (16 - wy), (16 - wx) wy, wx wy — 256 in all; a vote
 *                     whose cell lies outside the grid is dropped.
 *   objective         J(w) = sum over the cells of I^2, uint64, exact for fewer than 2^24 events.
 *   search            per slice, from w = 0, step = omega_max / 2: an iteration evaluates w +- step e_i in the order +x -x +y -y +z -z and moves to the best of
 *                     the six (ties: the earlier) iff its J is strictly greater than the centre's, else halves the step; it ends when step < omega_max 2^-12
 *                     or after 64 iterations.  A slice whose first and last timestamps are equal gets w = 0 after the one evaluation of J(0).
 * emba_seq_cmax: one workgroup per slice, the whole search inside one launch (emba_amd/csrc/cmax_kernels.h).  Per slice: omega_out [3] (rad/s, body frame: the
 * pose of event k is R(t_ref) exp(w (t[k] - t_ref)), the convention of warpEventToMap's R * bearing), j0_out = J(0), j_out = J(w), evals_out = evaluations of J
 * (1 + 6 per iteration); t_ref_ns_out: t_ref of every slice and, behind them, the timestamp of the last estimated event — cap_slices + 1 entries, the other
 * arrays cap_slices (3 cap_slices doubles for omega_out).  Any of the arrays may be NULL; *n_slices (may be NULL) is always set, and with every array NULL
 * nothing is launched.  EMBA_ERR_STATE: no sequence resident, or the LUT admits no pinhole fit.  EMBA_ERR_INVALID_ARG: slice_events < 1 or >= 2^24, omega_max
 * not finite and positive.  EMBA_ERR_CAPACITY: cap_slices < n_slices.  n_slices = 0 (fewer events than one slice) is EMBA_OK.  Timings: DESIGN.md §11. */
emba_status emba_seq_cmax(emba_ctx* ctx, int64_t slice_events, double omega_max, double* omega_out, int64_t* t_ref_ns_out, uint64_t* j0_out, uint64_t* j_out,
                          int32_t* evals_out, size_t cap_slices, size_t* n_slices);
/* The objective alone, for M given candidates omega [M, 3] over the events [beg, end) of the resident sequence, t_ref = t[beg] (tests, diagnostics; one
 * workgroup per candidate): j_out [M] and, where iwe_out is not NULL, the images of warped events [M, grid_h, grid_w] (uint32, row-major).  *grid_w, *grid_h,
 * *shift (each may be NULL) are always set, and with M = 0 or both outputs NULL nothing else happens — the grid of a context needs no sequence.  An empty range:
 * J = 0, an empty image.  EMBA_ERR_STATE: no sequence resident.  EMBA_ERR_INVALID_ARG: not beg <= end <= n, 2^24 events or more, omega NULL or not finite. */
emba_status emba_seq_cmax_objective(emba_ctx* ctx, size_t beg, size_t end, const double* omega, size_t M, uint64_t* j_out, uint32_t* iwe_out, int32_t* grid_w,
                                    int32_t* grid_h, int32_t* shift);

/* ---- The panorama of warped events along a trajectory, and its contrast (no map, no ground truth: "is this trajectory better than that one, on these
 * events?") on [beg, end) of the resident sequence as it stands.  The trajectory is a linear SO(3) spline as emba_eval_launch takes it: K
 * control poses knots_xyzw [K, 4], t0_ns, dt_ns.
 *   batches           nn = ((end - beg) / 100) * 100 events are used, the tail is ignored (quirk Q1).  Batch b of the range is [beg + 100 b, beg + 100 b + 100);
 *                     its pose is the spline at the batch's midpoint by the rule of model.cpp:116-119 — the integer midpoint emba_set_events_seq(beg, end)
 *                     gives that range — so the image is what the bundle adjustment sees.
 *   warp              pm = project(R(midpoint) * bearing_lut[y[k] * sensor_w + x[k]]): the spline evaluation and the equirectangular projection of the
 *                     evaluation path (emba_amd/csrc/device_math.h), no second formulation.  A pm that is not finite votes nowhere.
 *   votes             ix = floor(pm_x), wx = floor((pm_x - ix) * 16), iy, wy likewise; the cells (ix, iy), (ix + 1, iy), (ix, iy + 1), (ix + 1, iy + 1) get
 *                     (16 - wx)(16 - wy), wx (16 - wy), (16 - wx) wy, wx wy — 256 per event in all, the convention of the cmax grid.  Columns wrap modulo
 *                     pano_w (azimuth is periodic).  A vote — a non-zero weight — whose row lies outside [0, pano_h) is dropped and counted in *dropped_out
 *                     (votes, not events).  signed_polarity != 0: events with pol == 0 vote negative; == 0: every event votes positive.
 *   image, contrast   cells are int32, pano_h x pano_w, row-major; J = sum I^2 (uint64), sum = sum I (int64), nonzero = cells != 0.  Exact for fewer than
 *                     2^23 events in the range (the formula: emba_amd/csrc/panorama_rule.h, pano_vote).
 * Any output may be NULL, and with every output NULL nothing is launched.  image_out: host memory of pano_h * pano_w int32; pm_out: host memory of nn * 2
 * doubles, pm of every used event in event order (the seam the tests pin, like iwe_out above).  The registered window, its order and the last evaluation
 * are left as they are.  EMBA_ERR_STATE: no sequence resident.  EMBA_ERR_INVALID_ARG: not beg <= end <= n, K < 2, dt_ns <= 0, nn >= 2^23, knots NULL.
 * EMBA_ERR_TIME_RANGE: a batch midpoint outside the knots (the outputs are then untouched).  An empty or sub-batch range is EMBA_OK with J = 0 and a zero image.
 * emba_amd.io.event_panorama is the same rule in numpy (given pm: the same integers).  Launches and timings: DESIGN.md §12.  While emba_enable_kernel_timing
 * is on, the call records timer slot 7 around its vote kernel: emba_timer_elapsed_ms(ctx, 7, &ms) afterwards is that kernel's time. */
emba_status emba_seq_event_panorama(emba_ctx* ctx, size_t beg, size_t end, const double* knots_xyzw, int32_t K, int64_t t0_ns, int64_t dt_ns,
                                    int32_t signed_polarity, int32_t* image_out, uint64_t* j_out, int64_t* sum_out, uint64_t* nonzero_out,
                                    uint64_t* dropped_out, double* pm_out);

/* ---- The smooth contrast of that panorama and its gradient with respect to the control poses (what moves a trajectory uphill on the events alone;
 * DESIGN.md §13).  The integer image above is piecewise constant in the poses; this one is fp64 with real bilinear weights.  Range, batches, midpoints, pm,
 * column wrap and pole rows are exactly those of emba_seq_event_panorama.
 *   votes             ix = floor(pm_x), ax = pm_x - ix, iy, ay likewise; the cells (ix, iy), (ix + 1, iy), (ix, iy + 1), (ix + 1, iy + 1) get the weights
 *                     (1 - ax)(1 - ay), ax (1 - ay), (1 - ax) ay, ax ay.  Their derivatives in pm_x are -(1 - ay), +(1 - ay), -ay, +ay, in pm_y
 *                     -(1 - ax), -ax, +(1 - ax), +ax.  A cell whose row lies outside [0, pano_h) is dropped, and counted in *dropped_out where its weight
 *                     is not zero.  A pm that is not finite votes nowhere.
 *   image, contrast   I(c) = sum_k s_k w_kc with s_k = 1, or +-1 by polarity where signed_polarity != 0 (pol == 0: -1); J = sum_c I(c)^2, fp64.
 *   gradient          with respect to the increments x of knot_i <- exp(x_i) knot_i (emba_amd.io.incremental_update): grad_out has 3 K entries.  For
 *                     event k of a batch whose spline segment begins at control pose cp: gp = sum_i I(c_i) (dwx_i, dwy_i) over the kept cells,
 *                     ge = 2 s_k gp^T D_k with D_k the 2x6 dpm_ddrot_cp of the evaluation path (J23 [I - J1 | J1]); ge[0:3] is added to g[3 cp ..],
 *                     ge[3:6] to g[3 (cp + 1) ..].  A component of ge that is not finite adds nothing.
 * The formula: emba_amd/csrc/contrast_rule.h; emba_amd.io.contrast_votes / contrast_gradient are the same rule in numpy given pm, D and cp.  The adds into
 * the image and into g are fp64 atomics whose order is not fixed: both depend on it in their last bits, so results are compared by tolerance, not by bits
 * (given the image, J is deterministic).  Any output may be NULL, and with every output NULL nothing is launched.  With grad_out, d_out and cp_out NULL
 * the gradient pass is not launched (a line search asks for J alone).  image_out: pano_h * pano_w doubles; pm_out [nn, 2], d_out [nn, 2, 6], cp_out [nn]
 * (-1: no pose): per used event in event order, the seam the tests pin.  Statuses and the empty range as emba_seq_event_panorama (J = 0, grad = 0, a zero
 * image), without its limit of 2^23 events: fp64 cells do not overflow.  EMBA_ERR_TIME_RANGE leaves the outputs untouched.  The registered window, its
 * order, the last evaluation and the integer panorama's buffers are left as they are.  While emba_enable_kernel_timing is on, timer slot 7 brackets the
 * vote kernel and the gradient kernel together. */
emba_status emba_seq_contrast_gradient(emba_ctx* ctx, size_t beg, size_t end, const double* knots_xyzw, int32_t K, int64_t t0_ns, int64_t dt_ns,
                                       int32_t signed_polarity, double* j_out, double* grad_out /* 3K or NULL */, double* image_out /* H*W or NULL */,
                                       uint64_t* dropped_out, double* pm_out /* [nn,2] or NULL */, double* d_out /* [nn,2,6] or NULL */,
                                       int32_t* cp_out /* [nn] or NULL */);

/* ---- The same contrast and gradient on a coarser grid (coarse to fine: the ascent of the control poses climbs first where the objective's features are
 * 2^level pixels wide).  Level l in [0, 8] is the rule of emba_seq_contrast_gradient on a grid of W_l = pano_w >> l by H_l = pano_h >> l
 * cells with the vote coordinate pm_l = pm 2^-l and D_l = D 2^-l, both exact scalings: floor, the four weights and their derivatives, the column wrap
 * (modulo W_l), the rows dropped and counted (outside [0, H_l)), a pm that is not finite, the polarity signs, ge and where it is added are those of that
 * rule with W_l, H_l for pano_w, pano_h.  Level 0 is that rule.  A J of one level is not comparable with a J of another.
 *   image_out         H_l * W_l doubles
 *   pm_out, d_out     the UNSCALED pm and D of the evaluation path, as emba_seq_contrast_gradient gives them (the seam the tests pin): the numpy form is
 *                     emba_amd.io.contrast_gradient on emba_amd.io.contrast_level(pm, D, pano_w, pano_h, level)
 * EMBA_ERR_INVALID_ARG, outputs untouched: level outside [0, 8]; pano_w or pano_h not divisible by 2^level; H_l < 2.  Everything else — the other
 * arguments, statuses, NULL outputs, the empty range, what is left alone, timer slot 7 — as emba_seq_contrast_gradient.  An image of at most 8 192 cells is
 * summed in LDS by a fixed grid of persistent workgroups and only their non-zero cells are added in HBM; a larger one takes every add in HBM (option
 * contrast_vote; emba_get_option "contrast_vote_path": what the last call took).  The formula and the plan: emba_amd/csrc/contrast_rule.h. */
emba_status emba_seq_contrast_gradient_level(emba_ctx* ctx, size_t beg, size_t end, const double* knots_xyzw, int32_t K, int64_t t0_ns, int64_t dt_ns,
                                             int32_t signed_polarity, int32_t level, double* j_out, double* grad_out /* 3K or NULL */,
                                             double* image_out /* H_l*W_l or NULL */, uint64_t* dropped_out, double* pm_out /* [nn,2] or NULL */,
                                             double* d_out /* [nn,2,6] or NULL */, int32_t* cp_out /* [nn] or NULL */);

/* ---- The same contrast and gradient against what earlier events already voted: the prior (what ties a window of a sliding-window run to the panorama the
 * windows before it placed).  A context holds, per level l in [0, 8], at most one prior image P_l of H_l x W_l doubles (H_l = pano_h >> l,
 * W_l = pano_w >> l), absent until written.  The rule, once:
 *   image             with a prior, the image of a call is I(c) = prior_weight * P_l(c) + sum_k s_k w_kc
 *   contrast          J = sum_c I(c)^2: the window's own contrast, twice its correlation with prior_weight P_l, and a constant
 *   gradient          the rule of emba_seq_contrast_gradient on that I (gp gathers I, so ge = 2 s (lambda P + I_w) . dw D)
 * Votes, weights, derivatives, column wrap, rows dropped and counted, a pm that is not finite, polarity signs, batches of 100 and their midpoints are exactly
 * those of emba_seq_contrast_gradient_level.  The priors are votes of the resident sequence's events: every call that replaces or re-indexes the sequence
 * (emba_seq_upload, emba_seq_free, emba_seq_filter) drops all of them.  All levels together are at most 4/3 of one pano_h x pano_w fp64 image.
 *
 * emba_seq_contrast_prior_add: for every level whose bit is set in level_mask (bit l: level l), P_l += the level-l votes of the used events of [beg, end)
 * along the trajectory — one launch, every event warped once and voted at every level; a prior that does not exist is created as zeros first (also by an
 * empty or sub-batch range, which adds nothing).  *n_added = the events used, ((end - beg) / 100) * 100; dropped_out: NULL or 9 entries, entry l the votes of
 * level l whose row lies outside [0, H_l) (0 for a level not in the mask).  EMBA_ERR_INVALID_ARG: level_mask 0, a bit at 9 or above, a set level the
 * panorama does not admit (not divisible by 2^l, H_l < 2); the range, K and dt_ns checks and EMBA_ERR_STATE / EMBA_ERR_TIME_RANGE as the gradient entry
 * points.  EMBA_ERR_TIME_RANGE, and every other refusal, leaves every prior bit for bit as it was: the pose stage's status is read before anything is voted,
 * one synchronisation more than an evaluation takes.
 * emba_seq_contrast_prior_set: P_level <- image_host (H_l * W_l doubles), or, with image_host NULL, no prior at that level.
 * emba_seq_contrast_prior_get: *present = 1 / 0; where there is a prior and image_host is not NULL, its H_l * W_l doubles (else image_host is untouched).
 * emba_seq_contrast_prior_clear: no prior at any level.  set and get: EMBA_ERR_STATE without a resident sequence, EMBA_ERR_INVALID_ARG for a level the
 * panorama does not admit.
 *
 * emba_seq_contrast_gradient_prior: emba_seq_contrast_gradient_level with the rule above — every argument, output, status and the choice of the vote kernel
 * (option contrast_vote, "contrast_vote_path") as there, timer slot 7 likewise.  EMBA_ERR_STATE, outputs untouched: no prior at that level.
 * EMBA_ERR_INVALID_ARG: prior_weight not finite or negative.  An empty or sub-batch range is EMBA_OK with J = prior_weight^2 sum P^2, a zero gradient and
 * image_out = prior_weight P (the image is still formed and reduced on the device).  prior_weight = 0 is the rule without a prior.  A call never changes a
 * prior.  The numpy form: emba_amd.io.contrast_gradient(..., prior = prior_weight * P). */
emba_status emba_seq_contrast_prior_add(emba_ctx* ctx, size_t beg, size_t end, const double* knots_xyzw, int32_t K, int64_t t0_ns, int64_t dt_ns,
                                        int32_t signed_polarity, uint32_t level_mask, size_t* n_added, uint64_t* dropped_out /* [9] or NULL */);
emba_status emba_seq_contrast_prior_set(emba_ctx* ctx, int32_t level, const double* image_host /* NULL: drop this level's prior */);
emba_status emba_seq_contrast_prior_get(emba_ctx* ctx, int32_t level, double* image_host /* or NULL */, int32_t* present);
emba_status emba_seq_contrast_prior_clear(emba_ctx* ctx);
emba_status emba_seq_contrast_gradient_prior(emba_ctx* ctx, size_t beg, size_t end, const double* knots_xyzw, int32_t K, int64_t t0_ns, int64_t dt_ns,
                                             int32_t signed_polarity, int32_t level, double prior_weight, double* j_out, double* grad_out /* 3K or NULL */,
                                             double* image_out /* H_l*W_l or NULL */, uint64_t* dropped_out, double* pm_out /* [nn,2] or NULL */,
                                             double* d_out /* [nn,2,6] or NULL */, int32_t* cp_out /* [nn] or NULL */);

/* ---- Sensor views along the trajectory: what the camera would have seen at a time t, a frame at sensor resolution sampled from a panorama
 * plane, and what it reported between two times, the per-pixel event count of the resident sequence.  The brightness change between two predicted frames,
 * over C_th, is the event count the generative model expects at that sensor pixel.
 *
 * emba_render_views: F frames at the times frame_t_ns [F] along the linear SO(3) spline (knots_xyzw [K, 4], t0_ns, dt_ns, as emba_eval_launch takes it).
 *   source plane      plane_host: pano_h * pano_w doubles, any plane (an intensity panorama, a 0/1 coverage mask), uploaded into a buffer of the call's own.
 *                     plane_host NULL: the intensity panorama of the resident map under `boundary` (EMBA_POISSON_DIRICHLET / EMBA_POISSON_WRAP_X), which the
 *                     call reconstructs itself, as emba_render_map_images_bc does; `boundary` is read in that case only.
 *   poses             the spline at every frame time (the pose kernel of the evaluation path, all F at once, into a table of this call's own).
 *   warp              per frame and sensor pixel s = y * sensor_w + x: pm = project(R(frame) * bearing_lut[s]), the functions of emba_seq_event_panorama.
 *   sample            ix = floor(pm_x), ax = pm_x - ix, iy, ay likewise.  The columns ix, ix + 1 wrap modulo pano_w, always (whatever `boundary` was).
 *                     iy < 0 or iy + 1 > pano_h - 1 (and a pm that is not finite): the pixel is outside — views_out = fill, views_u8 = 0, counted in
 *                     outside_out[f].  Otherwise v = (1 - ay) ((1 - ax) P[iy][ix] + ax P[iy][ix + 1]) + ay ((1 - ax) P[iy + 1][ix] + ax P[iy + 1][ix + 1]),
 *                     in this order, without contraction (emba_amd/csrc/view_rule.h: view_sample).  No occlusion, no exposure model.
 *   tone              views_u8 = sat(rint(scale (v - lo))), scale = 255 / (hi - lo), or 1 where hi == lo: the arithmetic of emba_normalize_robust.  A caller
 *                     takes lo / hi from that call on the panorama, so the tone is constant across frames.  lo, hi are read with views_u8 only.
 * Outputs, each may be NULL (with all of them NULL, or F = 0, nothing is launched): views_out [F, sensor_h, sensor_w] doubles, views_u8 the same in bytes,
 * outside_out [F], pm_out [F, sensor_h * sensor_w, 2] (the seam the tests pin: emba_amd.io.render_views(plane, pm, fill) gives views_out bit for bit).
 * Frames are rendered in chunks of at most 65 535 frames and 32 MiB of doubles (one frame at the least); F < 2^31.  The registered window, its order, the
 * last evaluation and the buffers of the panorama and contrast calls are left as they are; with plane_host NULL the Poisson workspace is rewritten.
 * EMBA_ERR_INVALID_ARG: knots or frame_t_ns NULL, K < 2, dt_ns <= 0, F >= 2^31, lo / hi not finite with views_u8; with plane_host NULL also the refusals of
 * emba_reconstruct_intensity_bc's boundary.  EMBA_ERR_STATE: plane_host NULL and no map resident.  EMBA_ERR_TIME_RANGE: a frame time outside the knots
 * (t < t0_ns or t >= t0_ns + (K - 1) dt_ns).  A refused call leaves every output untouched.  While emba_enable_kernel_timing is on, timer slot 7 brackets the
 * view kernel of the first chunk.
 *
 * emba_seq_event_frames: F frames of signed event counts with the edges edge_t_ns [F + 1], strictly increasing.  EVERY event k of [beg, end) of the resident
 * sequence counts — not whole batches of 100: no pose is involved.  Event k belongs to frame f when edge[f] <= t[k] < edge[f + 1]; its pixel of frame f
 * gets +1, or -1 for polarity 0 where signed_polarity != 0.  Events before edge[0] are counted in *before_out, events at or after edge[F] in *after_out.
 * frames_out: [F, sensor_h, sensor_w] int32; each output may be NULL.  Exact integers: emba_amd.io.event_frames gives the same bits.  Chunks of frames as
 * above (32 MiB of int32); every chunk's launch sweeps the events of the range.  EMBA_ERR_STATE: no sequence resident.  EMBA_ERR_INVALID_ARG: not
 * beg <= end <= n, edge_t_ns NULL or not strictly increasing, F >= 2^31 - 1.  A refused call leaves every output untouched.  Nothing else of the context
 * is read or written.  Timer slot 7 as above. */
emba_status emba_render_views(emba_ctx* ctx, const double* plane_host /* H*W or NULL */, int boundary, const int64_t* frame_t_ns, size_t F,
                              const double* knots_xyzw, int32_t K, int64_t t0_ns, int64_t dt_ns, double fill, double lo, double hi,
                              double* views_out /* [F, sh, sw] or NULL */, uint8_t* views_u8 /* [F, sh, sw] or NULL */, uint64_t* outside_out /* [F] or NULL */,
                              double* pm_out /* [F, sh*sw, 2] or NULL */);
emba_status emba_seq_event_frames(emba_ctx* ctx, size_t beg, size_t end, const int64_t* edge_t_ns /* F+1, strictly increasing */, size_t F,
                                  int32_t signed_polarity, int32_t* frames_out /* [F, sh, sw] */, uint64_t* before_out, uint64_t* after_out);

/* ---- The mosaic of intensity frames: frames -> panorama, the way back from emba_render_views.  Frames of bytes at sensor resolution
 * (a DAVIS sensor's intensity frames, or what emba_render_views wrote) are stitched into the panorama along a trajectory; the mosaic's log-intensity
 * plane and its backward differences are a gradient map that does not depend on the events at all.
 *
 * emba_mosaic_frames: F frames [F, sensor_h, sensor_w] of bytes at the times frame_t_ns [F] along the linear SO(3) spline (knots_xyzw [K, 4], t0_ns, dt_ns).
 *   vote              pixel s = y * sensor_w + x of frame f has the byte v.  pm = project(R(frame_t[f]) * bearing_lut[s]), the pose stage and the warp of
 *                     emba_render_views, unchanged.  The pixel votes as an event of emba_seq_event_panorama does (emba_amd/csrc/panorama_rule.h:
 *                     pano_vote): the four cells around pm, weights in 256ths, 256 in all, columns wrapped modulo pano_w.  A row outside [0, pano_h) has no
 *                     cell: its non-zero weight is a dropped vote.  Cell c receives w into sum_w[c] and w * v into sum_v[c], both uint64.  Integer sums do
 *                     not depend on the order of the adds: emba_amd.io.mosaic_votes gives the same integers from the same pm.
 *   skip_zero         non-zero: a pixel whose byte is 0 casts no vote and is counted in *skipped_out.  emba_render_views writes 0 for the pixels outside
 *                     the panorama, so its frames need this flag; a real frame does not.
 *   accumulate        0: both sums are zeroed first.  Otherwise the call adds to what is there: frames can be streamed in pieces.  The sums stay on the
 *                     device; the frames go up in chunks of at most 65 535 frames and 32 MiB of bytes (one frame at the least).
 *   exactness         the votes accumulated since the sums were last zeroed number F * sensor_h * sensor_w (skipped pixels count); they stay below 2^36, so
 *                     that 65 280 * votes < 2^53 and both sums convert to double exactly.  A call that would reach 2^36 is refused.
 * *dropped_out, *skipped_out: this call's dropped votes and skipped pixels; pm_out [F, sensor_h * sensor_w, 2] or NULL, the seam the tests pin.  F = 0 votes
 * nothing (and without `accumulate` leaves zero sums with nothing accumulated).  EMBA_ERR_INVALID_ARG: frames, frame_t_ns or knots NULL with F > 0, K < 2,
 * dt_ns <= 0, F >= 2^31, the 2^36 bound.  EMBA_ERR_TIME_RANGE: a frame time outside the knots, decided before anything is voted or zeroed.  A refused call
 * leaves every output and the sums untouched.  A call that FAILS (EMBA_ERR_HIP: an allocation, a copy or a launch, possibly in a later chunk) is not a
 * refusal: some chunks may have been voted, dropped_out / skipped_out are unwritten, and the mosaic is undefined until emba_mosaic_clear (or a call
 * without `accumulate`).  While emba_enable_kernel_timing is on, timer slot 7 brackets the vote kernel of the first chunk.
 *
 * emba_mosaic_get: the sums and their mean.  covered[c] = sum_w[c] >= min_weight (min_weight >= 1; 256 is one whole pixel's worth);
 * mean[c] = double(sum_v[c]) / double(sum_w[c]) where covered, else `fill` — one IEEE division of two exactly converted integers
 * (emba_amd.io.mosaic_mean: the same bits); *n_covered_out the number of covered cells.  Each output may be NULL.
 *
 * emba_mosaic_map: the log-intensity plane and the gradient map (emba_amd/csrc/mosaic_rule.h: mosaic_log, mosaic_gradient).
 *   plane             I = lo + mean * (hi - lo) / 255, in this order and without contraction: the inverse of emba_render_views' tone.  take_log == 0: L = I (the
 *                     frames of run_ba.py --views-hz are log intensity already).  Otherwise L = log(I + eps), and a cell with I + eps <= 0 becomes
 *                     uncovered.  L_out holds 0 in uncovered cells.
 *   map               Gx[i][j] = L[i][j] - L[i][(j - 1) mod pano_w] where both cells are covered, else 0; Gy[i][j] = L[i][j] - L[i - 1][j] where both
 *                     are covered and i >= 1, else 0: backward differences, the field whose divergence in emba_reconstruct_intensity is the 5-point operator.
 *                     Given the device's L and the covered cells, emba_amd.io.gradient_from_plane gives the same bits.
 *   make_resident     non-zero: Gx, Gy become the context's resident map, device to device, exactly as emba_upload_map of the same planes would leave it
 *                     (a pending trial map is dropped).
 * L_out, Gx_out, Gy_out: pano_h * pano_w doubles each, or NULL.
 *
 * emba_mosaic_clear: zero sums, nothing accumulated.
 * EMBA_ERR_INVALID_ARG (get, map): min_weight < 1; fill, lo, hi or eps not finite; hi <= lo.  EMBA_ERR_STATE (get, map): nothing accumulated.  A refused call
 * leaves every output, the sums and the resident map untouched.  The registered window, its order, the last evaluation, the resident sequence and the
 * buffers of every other stage are left as they are by all four calls; without make_resident so is the resident map. */
emba_status emba_mosaic_frames(emba_ctx* ctx, const uint8_t* frames /* [F, sh, sw] */, const int64_t* frame_t_ns, size_t F,
                               const double* knots_xyzw, int32_t K, int64_t t0_ns, int64_t dt_ns, int32_t skip_zero, int32_t accumulate,
                               uint64_t* dropped_out, uint64_t* skipped_out, double* pm_out /* [F, sh*sw, 2] or NULL */);
emba_status emba_mosaic_get(emba_ctx* ctx, uint64_t min_weight, double fill, uint64_t* sum_w_out, uint64_t* sum_v_out, double* mean_out,
                            uint8_t* covered_out, uint64_t* n_covered_out);
emba_status emba_mosaic_map(emba_ctx* ctx, uint64_t min_weight, double lo, double hi, double eps, int32_t take_log,
                            double* L_out, double* Gx_out, double* Gy_out /* each H*W or NULL */, int32_t make_resident);
emba_status emba_mosaic_clear(emba_ctx* ctx);

/* ---- The event simulator: a recording from a log-intensity panorama plane and a trajectory — the events a sensor would report whose pixels see
 * the samples of emba_render_views change.  No noise, no refractory period, no exposure model; inside a step the brightness of a pixel is linear in time.
 *
 * emba_simulate_events: F >= 1 steps between the F + 1 step times step_t_ns, strictly increasing, step_t_ns[F] - step_t_ns[0] < 2^52.
 *   samples      V_f[s], f = 0 ... F, s = y * sensor_w + x: exactly what emba_render_views gives for the frame time step_t_ns[f] — the same source plane
 *                (plane_host, or with NULL the intensity panorama of the resident map under `boundary`), poses, warp and sample, and the same pixels outside.
 *   per pixel    a state machine over f = 0 ... F, independent of the other pixels, every operation in fp64, in this order, without contraction
 *                (emba_amd/csrc/sim_rule.h: sim_frame, sim_step):
 *                  V_f outside: the pixel is disarmed.
 *                  V_f inside, the pixel not armed: ref = V_f, the pixel is armed; no event in the step that ends at f.
 *                  V_f inside, the pixel armed (so V_{f-1} was inside): prev = V_{f-1}, cur = V_f, d = step_t_ns[f] - step_t_ns[f-1].  While
 *                  fabs(cur - ref) >= C — C = c_on and sgn = +1 where cur - ref > 0, otherwise C = c_off and sgn = -1 — and at most max_per_step times:
 *                    ref = ref + sgn * C;  frac = (ref - prev) / (cur - prev), 0 where it is not >= 0 (a NaN too), 1 where it is > 1;
 *                    off = (int64)(frac * (double)d) truncated, at most d - 1;  the event (x, y, polarity = sgn > 0, t = step_t_ns[f-1] + off).
 *                  What the cap leaves over is carried: ref stays behind and the next step goes on from it.
 *                Every event of the step that ends at f has step_t_ns[f-1] <= t <= step_t_ns[f] - 1: the steps are disjoint in time.
 *   order        ascending t; among equal t ascending pixel index s; among those the order of emission.
 *   stats        uint64 [4] or NULL: [0] events, [1] positive events, [2] (pixel, step) pairs where the condition still held after max_per_step events,
 *                [3] (pixel, f) pairs with V_f outside, f = 0 ... F.
 *   thresholds   c_on, c_off > 0 and finite; max_per_step 1 ... 255; max_events: 0 stands for 2^32 - 2, the limit of the 32-bit scan and sort (and the most any
 *                value allows).
 * The recording stays on the device, in buffers of the simulator's own, and replaces the one before only when the call succeeds.  The steps go in chunks of at
 * most 32 MiB of samples and 65 534 steps (one step at the least): per chunk the view kernel of emba_render_views, a count pass, a scan, an emit pass and the
 * stable 32-bit sort.  (The simulator knows an outside sample by the bits of one quiet NaN, 0x7FF8000053494D31, which it passes to the view kernel as its
 * fill: a plane that holds these very bits reads as outside there.)  EMBA_ERR_INVALID_ARG: knots or step_t_ns NULL, K < 2, dt_ns <= 0, F = 0 or F >= 2^31 - 1,
 * step times not strictly increasing or spanning 2^52 ns or more, a threshold not positive or not finite, max_per_step outside 1 ... 255, a sensor of more
 * than (2^32 - 2) / 255 pixels; with plane_host NULL also the refusals of emba_reconstruct_intensity_bc's boundary.  EMBA_ERR_STATE: plane_host NULL and no map
 * resident.  EMBA_ERR_TIME_RANGE: a step time outside the knots; the pose stage's status word is read before anything else runs.  These refusals leave the
 * previous simulated recording, stats, the resident sequence, the registered window and the last evaluation untouched.  EMBA_ERR_CAPACITY: more than
 * max_events events — stats[0] is the number that would have been needed, the rest of stats is untouched, nothing is emitted and the previous recording is
 * kept.  No events at all is a success with stats[0] = 0.  The sort pairs of the order preparation are scratch here as in emba_seq_filter; with plane_host
 * NULL the Poisson workspace is rewritten.  While emba_enable_kernel_timing is on, the timer slots 3 ... 7 bracket the first chunk's views, count, scan, emit
 * and sort.  The numpy form, given the samples: emba_amd.io.simulate_events.
 *
 * emba_sim_size, emba_sim_get: the number of events of the simulated recording, and [beg, end) of it; any of the four pointers may be NULL, as in
 * emba_seq_get.  EMBA_ERR_STATE before the first successful simulation; EMBA_ERR_INVALID_ARG: not beg <= end <= n.
 *
 * emba_seq_from_sim: the simulated recording becomes the resident sequence, device to device: what emba_seq_upload of the same four arrays with the same
 * sampling_rate leaves, bit for bit — the same checks, the same down-sampling, the same effect on the contrast priors, the filter's hot mask and the
 * registered window.  The simulated recording itself stays.  EMBA_ERR_STATE before the first successful simulation. */
emba_status emba_simulate_events(emba_ctx* ctx, const double* plane_host /* H*W or NULL */, int boundary, const int64_t* step_t_ns /* F+1 */, size_t F,
                                 const double* knots_xyzw, int32_t K, int64_t t0_ns, int64_t dt_ns, double c_on, double c_off, int32_t max_per_step,
                                 uint64_t max_events, uint64_t* stats /* [4] or NULL */);
emba_status emba_sim_size(const emba_ctx* ctx, size_t* n);
emba_status emba_sim_get(emba_ctx* ctx, size_t beg, size_t end, uint16_t* x, uint16_t* y, uint8_t* pol, int64_t* t_ns);
emba_status emba_seq_from_sim(emba_ctx* ctx, int32_t sampling_rate, size_t* n_kept);

/* ---- Intensity frames aligned to the panorama: poses from frames.  The mosaic stitches frames along a GIVEN trajectory; here each frame's
 * own rotation is refined by direct photometric alignment against a panorama plane — a 3-DoF Levenberg-Marquardt per frame, the frames independent.  The
 * rule lives in emba_amd/csrc/align_rule.h; emba_amd.io.align_sample / align_terms / align_sums / align_step / align_frames are the same rule in numpy.
 *
 * Frame f has the rotation q_xyzw[f] (xyzw, unit; a per-frame input, not a spline); pixel s = y * sensor_w + x of it has the byte v.
 *   warp              rb = R(q_f) * bearing_lut[s]; pm and J23 = d pm / d delta for the left perturbation R <- exp(delta) R, by the projection of the step
 *                     path with its Jacobian.  pm is computed without contraction, as in emba_render_views: it feeds floor().
 *   sample            ix, iy, ax, ay, the wrapped columns c0, c1 and the outside test are emba_render_views' (view_sample).  val is its value;
 *                     gx = (1 - ay) (P[iy][c1] - P[iy][c0]) + ay (P[iy+1][c1] - P[iy+1][c0]), gy = (1 - ax) (P[iy+1][c0] - P[iy][c0]) + ax (P[iy+1][c1] - P[iy][c1]),
 *                     in this order, without contraction: numpy gives the same bits from the same pm.
 *   which pixels      outside: as in emba_render_views.  masked: a `valid` plane is there and any of the four cells holds 0.  skipped: skip_zero != 0 and
 *                     v == 0.  Counted per frame in this precedence; every other pixel is used (n).
 *   residual          I = lo + v * (hi - lo) / 255, in this order, without contraction (the inverse tone of emba_mosaic_map); r = val - I.  The plane and
 *                     the frames are in the same units; whether that is intensity or its logarithm is the caller's business.
 *   weight            huber_k <= 0: w = 1, rho = r^2.  Otherwise the same for |r| <= huber_k, and w = huber_k / |r|, rho = 2 huber_k |r| - huber_k^2 beyond.
 *   sums              g = gx J23[0,:] + gy J23[1,:].  Per frame H = sum w g^T g (six entries: 00 01 02 11 12 22), b = sum w g^T r (three), cost = sum rho,
 *                     and n.  The sums of a frame are reduced in a fixed order: the same call on the same inputs returns the same bits.
 *   plane             plane_host: pano_h * pano_w doubles, uploaded into a buffer of this stage's own, with valid_host (pano_h * pano_w bytes, or NULL: no
 *                     mask).  plane_host NULL and use_mosaic != 0: the mean of the mosaic as it stands (emba_mosaic_get's, under min_weight and fill, in byte
 *                     units: lo = 0, hi = 255 make I = v) with its covered cells as the mask, device to device; valid_host is not read.  min_weight and
 *                     fill are read in that case only, use_mosaic only where plane_host is NULL.
 *
 * emba_frames_align_eval: one evaluation.  Outputs, each may be NULL: sums_out [F, 10] (H's six, b's three, cost), counts_out [F, 4] (used, outside, masked,
 * skipped), pm_out [F, sensor_h * sensor_w, 2] (the seam the tests pin) and resid_out [F, sensor_h * sensor_w] (r, 0 where the pixel is not used).
 *
 * emba_frames_align: the loop, per frame, the frames and their rotations resident on the device between iterations.
 *   step              (H + lambda diag H) delta = -b by a 3 x 3 Cholesky.  A frame is degenerate when a pivot is not positive or n < min_pixels: it is frozen.
 *                     The trial is q' = normalise(exp(delta) (x) q); it is accepted when n' >= min_pixels and cost' / n' < cost / n (the means: pixels enter
 *                     and leave the panorama and the mask).  Accepted: q <- q', lambda <- max(lambda / lambda_down, lambda_min).  Rejected:
 *                     lambda <- lambda * lambda_up.  The sums of an accepted trial are the next iteration's: an iteration costs one evaluation.
 *   a frame ends      EMBA_ALIGN_CONVERGED: |delta| < tol_rot on an accepted step; EMBA_ALIGN_STALLED: lambda > lambda_max; EMBA_ALIGN_ITERATIONS: max_iters
 *                     trials were evaluated; EMBA_ALIGN_DEGENERATE.
 * Outputs, each may be NULL: q_out [F, 4]; sums_out, counts_out as above, at q_out (bit for bit what emba_frames_align_eval gives there); status_out [F];
 * iters_out [F] (trials evaluated); cost0_out, n0_out [F]: cost and n at q_xyzw.
 *
 * Both calls cut F into chunks of at most 65 535 frames and 32 MiB of bytes (one frame at the least); a chunk's bytes go up once.  F = 0 launches nothing.
 * Refusals are decided before anything is uploaded and leave every output untouched.  EMBA_ERR_INVALID_ARG: frames or q_xyzw NULL with F > 0; F >= 2^31; lo or
 * hi not finite, hi <= lo; huber_k a NaN; a q that is not finite or has zero norm; neither plane_host nor use_mosaic; with use_mosaic min_weight < 1 or fill
 * not finite; settings NULL, max_iters < 0, lambda_up or lambda_down <= 1, lambda0 <= 0, not 0 <= lambda_min <= lambda_max, tol_rot < 0, min_pixels < 3.
 * EMBA_ERR_STATE: use_mosaic with nothing accumulated.  The registered window, its order, the last evaluation, the resident sequence, the mosaic's sums, the
 * resident map and every other stage's buffers are left as they are (use_mosaic rewrites the mosaic's mean and covered scratch, as emba_mosaic_get does).
 * While emba_enable_kernel_timing is on, timer slot 7 brackets the first evaluation kernel of the first chunk. */
#define EMBA_ALIGN_RUNNING 0      /* (never reported) */
#define EMBA_ALIGN_CONVERGED 1
#define EMBA_ALIGN_STALLED 2
#define EMBA_ALIGN_ITERATIONS 3
#define EMBA_ALIGN_DEGENERATE 4
typedef struct {
    int32_t max_iters, min_pixels;
    double lambda0, lambda_up, lambda_down, lambda_min, lambda_max, tol_rot, huber_k;
} emba_align_settings;
emba_status emba_frames_align_eval(emba_ctx* ctx, const uint8_t* frames /* [F, sh, sw] */, size_t F, const double* q_xyzw /* [F, 4] */,
                                   const double* plane_host /* H*W or NULL */, const uint8_t* valid_host /* H*W or NULL */, int32_t use_mosaic,
                                   uint64_t min_weight, double fill, double lo, double hi, int32_t skip_zero, double huber_k,
                                   double* sums_out /* [F, 10] */, uint64_t* counts_out /* [F, 4] */, double* pm_out /* [F, sh*sw, 2] */,
                                   double* resid_out /* [F, sh*sw] */);
emba_status emba_frames_align(emba_ctx* ctx, const uint8_t* frames /* [F, sh, sw] */, size_t F, const double* q_xyzw /* [F, 4] */,
                              const double* plane_host /* H*W or NULL */, const uint8_t* valid_host /* H*W or NULL */, int32_t use_mosaic,
                              uint64_t min_weight, double fill, double lo, double hi, int32_t skip_zero, const emba_align_settings* settings,
                              double* q_out /* [F, 4] */, double* sums_out /* [F, 10] */, uint64_t* counts_out /* [F, 4] */, int32_t* status_out /* [F] */,
                              int32_t* iters_out /* [F] */, double* cost0_out /* [F] */, uint64_t* n0_out /* [F] */);

/* ---- Intensity frames tracked against their own growing mosaic: poses from the frames alone.  The alignment above needs a finished plane
 * and a start for every frame; here there is no trajectory at all.  Frame 0 is put at q0, every later frame is aligned to the mosaic of the frames tracked
 * before it and then voted into it.  The rule lives in emba_amd/csrc/track_rule.h; emba_amd.io.track_level_pm / track_votes / track_terms / track_predict /
 * track_frames are the same rule in numpy.
 *
 * Frames f = 0 ... F - 1 of bytes, taken at frame_t_ns (strictly increasing).
 *   levels            level l (0 ... 7) is the panorama with cells 2^l pixels wide: W_l = W >> l, H_l = H >> l, pm_l = pm * 2^-l, J23_l = J23 * 2^-l (exact).
 *                     Per level the context holds two uint64 planes sum_w_l, sum_v_l [H_l, W_l]; level 0's are the mosaic's sums themselves, so that
 *                     emba_mosaic_get / emba_mosaic_map work on the tracked mosaic as they stand.  settings.levels[0 ... n_levels) is the schedule, coarse to
 *                     fine as the caller orders it.
 *   vote              a tracked frame (and the anchor) is warped once and votes at every level of the schedule, and at level 0 whether the schedule names
 *                     it or not: emba_mosaic_frames' vote (four cells, 256 units, columns wrapped, rows outside dropped and counted, w into sum_w_l and w * v
 *                     into sum_v_l by integer atomics) on the grid (W_l, H_l) at pm_l.  With skip_zero a byte of 0 casts no vote and is counted.  Integer
 *                     sums: numpy gives the same sums from the same pm.
 *   sample            P_l[c] = sum_v_l[c] / sum_w_l[c], one IEEE division, formed for the four cells of emba_render_views' cell of pm_l on (W_l, H_l); no
 *                     mean plane is written.  A pixel is masked when any of its four cells has sum_w_l < min_weight (the same min_weight at every level).
 *                     Everything else is emba_frames_align's with lo = 0, hi = 255 (I = v): outside / masked / skipped in this precedence, the value and
 *                     the gradient, the weight, g = gx J23_l[0,:] + gy J23_l[1,:], the ten sums, reduced in a fixed order.
 *   prediction        a < b the last two tracked frames (the anchor counts).  predict != 0 and both there: the start of frame f is
 *                     normalise(exp(omega (t_f - t_b) / (t_b - t_a)) (x) q_b), omega = log(q_b (x) q_a^-1).  Otherwise q_b.
 *   batches           frame 0 is the anchor: voted at normalise(q0), never aligned.  Behind it the frames [f0, f0 + batch) are aligned at once against the
 *                     mosaic of the frames tracked before f0, each from its own prediction, and the tracked ones among them are then voted in one launch.
 *                     batch = 1 is pure frame-to-mosaic tracking.  A batch ends at the end of its chunk (below).
 *   per frame         for each level of the schedule in order emba_frames_align's loop under settings.align, started where the previous level ended; a
 *                     level that ends degenerate leaves q as it was.  Behind the last level overlap = used / (S - skipped) at q_out (0 where every pixel
 *                     was skipped).  The frame is EMBA_TRACK_TRACKED when the last level did not end degenerate and overlap >= min_overlap; otherwise
 *                     EMBA_TRACK_LOST: q_out is its prediction, it casts no vote, and later predictions skip it.
 *
 * emba_frames_track zeroes the mosaic and every level plane first (tracking against a mosaic that is there is not built).  Outputs, each may be NULL: q_out
 * [F, 4]; status_out [F]; iters_out [F, n_levels] (trials evaluated per level); cost_out [F] and counts_out [F, 4] (used, outside, masked, skipped) of the
 * last level at the rotation it ended at; overlap_out [F]; stats_out [4]: tracked frames (the anchor among them), lost frames, dropped votes (over every
 * plane), skipped pixels (of the voted frames); pm_out [F, sensor_h * sensor_w, 2]: the level-0 pm each voted frame voted with, NaN for a lost frame (the seam
 * the tests pin; asking for it makes every batch wait for its download).  The anchor reports 0 iterations, cost 0, counts 0 and overlap 0.
 * emba_track_eval: one evaluation of F frames at q_xyzw against the planes of `level` as they stand; outputs as emba_frames_align_eval's, pm_out the level's pm.
 * emba_track_level_get: the two planes of a level [H_l, W_l], each may be NULL.
 *
 * The frames go up in chunks of at most 65 535 frames and 32 MiB; a chunk boundary is a batch boundary.  Rotations and statuses stay on the device between
 * batches.  F = 0 zeroes the planes and launches nothing else.  Refusals are decided before anything is zeroed and leave every output, the mosaic and the
 * level planes untouched.  EMBA_ERR_INVALID_ARG: frames or frame_t_ns NULL with F > 0; q0 or settings NULL; F >= 2^31; n_levels not 1 ... 8; a level not
 * 0 ... 7, W or H not divisible by 2^level, H_l < 2; batch < 1; min_overlap not in [0, 1]; min_weight < 1; frame times not strictly increasing; q0 not finite
 * or of zero norm; settings.align refused as emba_frames_align refuses it (huber_k a NaN among it); F * S >= 2^36 votes.  emba_track_eval: frames or q_xyzw
 * NULL with F > 0, F >= 2^31, the level as above, min_weight < 1, huber_k a NaN, a q not finite or of zero norm.  EMBA_ERR_STATE: emba_track_eval or
 * emba_track_level_get at a level that the last successful emba_frames_track did not vote into.  The registered window, its order, the last evaluation, the
 * resident sequence and the resident map are left as they are.  While emba_enable_kernel_timing is on, timer slot 7 brackets the first evaluation kernel. */
#define EMBA_TRACK_ANCHOR 1
#define EMBA_TRACK_TRACKED 2
#define EMBA_TRACK_LOST 3
typedef struct {
    int32_t n_levels, levels[8], batch, predict, skip_zero;
    uint64_t min_weight;
    double min_overlap;
    emba_align_settings align;
} emba_track_settings;
emba_status emba_frames_track(emba_ctx* ctx, const uint8_t* frames /* [F, sh, sw] */, const int64_t* frame_t_ns /* [F] */, size_t F, const double* q0_xyzw /* [4] */,
                              const emba_track_settings* settings, double* q_out /* [F, 4] */, int32_t* status_out /* [F] */, int32_t* iters_out /* [F, n_levels] */,
                              double* cost_out /* [F] */, uint64_t* counts_out /* [F, 4] */, double* overlap_out /* [F] */, uint64_t* stats_out /* [4] */,
                              double* pm_out /* [F, sh*sw, 2] */);
emba_status emba_track_eval(emba_ctx* ctx, const uint8_t* frames /* [F, sh, sw] */, size_t F, const double* q_xyzw /* [F, 4] */, int32_t level, uint64_t min_weight,
                            int32_t skip_zero, double huber_k, double* sums_out /* [F, 10] */, uint64_t* counts_out /* [F, 4] */, double* pm_out /* [F, sh*sw, 2] */,
                            double* resid_out /* [F, sh*sw] */);
emba_status emba_track_level_get(emba_ctx* ctx, int32_t level, uint64_t* sum_w_out /* [H_l, W_l] */, uint64_t* sum_v_out /* [H_l, W_l] */);

/* ---- Per-frame exposure: the photometric half of the alignment.  A camera with auto-exposure changes its tone from frame to frame; here
 * frame f carries (q_f, a_f, b_f), its compensated intensity is a_f * I0 + b_f, the two are estimated with the rotation and applied when the frames are
 * stitched.  The rule lives in emba_amd/csrc/exposure_rule.h; emba_amd.io.exposure_terms / exposure_sums / exposure_step / align_frames_exposure /
 * exposure_bytes / exposure_gauge are the same rule in numpy.
 *
 *   model             I0 = lo + v * (hi - lo) / 255, emba_frames_align's expression.  I = gain[f] * I0 + bias[f]: multiply, then add, without contraction.
 *                     r = val - I.  The warp, the cell, the sample and its gradient, the Huber weight, g and the precedence outside / masked / skipped are
 *                     emba_frames_align's; skipped tests the raw byte v.  With gain = 1 and bias = 0, I is I0 exactly.
 *   parameters        five per frame: delta (the rotation's left perturbation), a, b.  The Jacobian row of r is J = (g, -I0, -1).
 *   sums              21 per frame: H = sum w J^T J as the 15 entries of its upper triangle in row-major order (00 01 02 03 04 11 12 13 14 22 23 24 33 34 44),
 *                     b = sum w J^T r (five), cost = sum rho.  Entries 0 1 2 5 6 9, 15 16 17 and 20 are emba_frames_align_eval's ten, from the same
 *                     operations in the same order of reduction: with gain = 1, bias = 0 they are its bits.  The four counts are its counts.
 *   estimate          a bitmask: EMBA_EXPOSURE_GAIN, EMBA_EXPOSURE_BIAS.  A parameter that is not estimated keeps its input value and has no row or column
 *                     in the solve.  The rotation is always estimated.
 *   step              (H + lambda diag H) x = -b on the active rows by a Cholesky, the leading 3 x 3 block in emba_frames_align's order of operations
 *                     (estimate = 0 gives its bits).  A frame is degenerate when a pivot is not positive or n < min_pixels — and, with both gain and bias
 *                     estimated, when their columns are collinear: the damping keeps the pivots of such a system positive, so the undamped pivot of the
 *                     bias behind the gain, H44 - H34^2 / H33, is tested against 1e-9 of H44.  A frame of one constant byte is degenerate this way.
 *   trial             q' = normalise(exp(delta) (x) q), a' = a + x_a, b' = b + x_b.  Accepted as emba_frames_align accepts; a trial whose estimated gain
 *                     lies outside [gain_min, gain_max] is rejected like one that raises the mean cost.  lambda and the four ways a frame ends are
 *                     emba_frames_align's; converged tests |delta| < tol_rot, the rotation alone.
 *   compensated byte  clamp(rint(a * v + b), 0, 255), ties to even, in fp64 without contraction: what frame f votes into the mosaic in the place of v.  The
 *                     mosaic is in byte units (lo = 0, hi = 255), and so is a bias that is used here.  The two integer sums keep their units and their
 *                     2^36 bound; emba_mosaic_get, emba_mosaic_map, use_mosaic and emba_frames_track read them as they stand.
 *   gauge             aligning to a fixed plane has no freedom left.  Aligning to the frames' own mosaic leaves the common affine tone free; a caller who
 *                     alternates fixes it on the host after every round: alpha = mean a, beta = mean b over the frames that count, a <- a / alpha,
 *                     b <- (b - beta) / alpha (exposure_rule.h: exposure_gauge; emba_amd.io.exposure_gauge).
 *
 * emba_frames_exposure_eval: emba_frames_align_eval with gain [F] and bias [F]; sums_out [F, 21], the other outputs as there.
 * emba_frames_exposure_align: emba_frames_align with gain_in, bias_in [F], estimate and the two bounds; gain_out, bias_out [F] beside q_out; sums_out [F, 21].
 * emba_mosaic_frames_exposure: emba_mosaic_frames with gain [F] and bias [F]: the same pose stage, warp, vote, skip_zero (on the raw byte), accumulate, chunks,
 * counters and pm_out, the compensated byte in the place of v.  With gain = 1, bias = 0 the sums are emba_mosaic_frames'.
 * Refusals: everything the three originals refuse, and EMBA_ERR_INVALID_ARG for gain or bias NULL with F > 0, a gain or bias that is not finite, a gain <= 0,
 * estimate outside 0 ... 3, gain bounds that are not finite or not 0 < gain_min <= 1 <= gain_max.  They are decided before anything is uploaded, zeroed or
 * voted and leave every output and the mosaic untouched.  What the originals leave alone, these leave alone.  While emba_enable_kernel_timing is on, timer
 * slot 7 brackets the first evaluation kernel (the first chunk's vote kernel) of a call. */
#define EMBA_EXPOSURE_GAIN 1
#define EMBA_EXPOSURE_BIAS 2
typedef struct {
    emba_align_settings align;
    double gain_min, gain_max;
} emba_exposure_settings;
emba_status emba_frames_exposure_eval(emba_ctx* ctx, const uint8_t* frames /* [F, sh, sw] */, size_t F, const double* q_xyzw /* [F, 4] */,
                                      const double* gain /* [F] */, const double* bias /* [F] */, const double* plane_host /* H*W or NULL */,
                                      const uint8_t* valid_host /* H*W or NULL */, int32_t use_mosaic, uint64_t min_weight, double fill, double lo, double hi,
                                      int32_t skip_zero, double huber_k, double* sums_out /* [F, 21] */, uint64_t* counts_out /* [F, 4] */,
                                      double* pm_out /* [F, sh*sw, 2] */, double* resid_out /* [F, sh*sw] */);
emba_status emba_frames_exposure_align(emba_ctx* ctx, const uint8_t* frames /* [F, sh, sw] */, size_t F, const double* q_xyzw /* [F, 4] */,
                                       const double* gain_in /* [F] */, const double* bias_in /* [F] */, int32_t estimate, const double* plane_host /* H*W or NULL */,
                                       const uint8_t* valid_host /* H*W or NULL */, int32_t use_mosaic, uint64_t min_weight, double fill, double lo, double hi,
                                       int32_t skip_zero, const emba_exposure_settings* settings, double* q_out /* [F, 4] */, double* gain_out /* [F] */,
                                       double* bias_out /* [F] */, double* sums_out /* [F, 21] */, uint64_t* counts_out /* [F, 4] */, int32_t* status_out /* [F] */,
                                       int32_t* iters_out /* [F] */, double* cost0_out /* [F] */, uint64_t* n0_out /* [F] */);
emba_status emba_mosaic_frames_exposure(emba_ctx* ctx, const uint8_t* frames /* [F, sh, sw] */, const int64_t* frame_t_ns, size_t F, const double* gain /* [F] */,
                                        const double* bias /* [F] */, const double* knots_xyzw, int32_t K, int64_t t0_ns, int64_t dt_ns, int32_t skip_zero,
                                        int32_t accumulate, uint64_t* dropped_out, uint64_t* skipped_out, double* pm_out /* [F, sh*sw, 2] or NULL */);

/* ---- The frame tracker with a per-frame exposure: emba_frames_track for the frames of a camera with auto-exposure.  Frame f carries
 * (q_f, a_f, b_f); gain and bias are estimated with the rotation at every level of the schedule, and every tracked frame votes its compensated bytes into
 * every level plane.  The rule lives in emba_amd/csrc/track_exposure_rule.h, over track_rule.h and exposure_rule.h; emba_amd.io.track_exposure_terms /
 * track_votes_exposure / track_frames_exposure are the same rule in numpy.  Everything that is not said here is emba_frames_track's.
 *
 *   pixel             emba_track_eval's pixel with the frame's gain and bias: the cell of pm_l, the mask on sum_w_l < min_weight, the four means formed in
 *                     registers, the sample and its gradient, the precedence outside / masked / skipped (skipped tests the raw byte v).  Then I0 = v (the
 *                     level planes are in byte units: lo = 0, hi = 255), r = val - (a * I0 + b): multiply, then add, without contraction; the Huber weight;
 *                     g from the level's J23.  The Jacobian row of r is (g, -I0, -1), the 21 sums are emba_frames_exposure_eval's.  With a = 1, b = 0 every
 *                     member of the term is emba_track_eval's bit for bit, and entries 0 1 2 5 6 9, 15 16 17 and 20 of the sums are its ten.
 *   step              emba_frames_exposure_align's, as it is, on the active rows of settings.estimate: the gain bounds, the collinear test when both are
 *                     estimated, converged on |delta| < tol_rot alone.  estimate = 0 is emba_frames_track: the same bits in every output and every plane.
 *   anchor            frame 0 is voted at normalise(q0) with a = 1, b = 0.  It fixes the common tone: a frame aligned to a mosaic that the anchor started has
 *                     no affine freedom left, so there is no gauge step inside the tracker.
 *   start of a frame  the rotation as emba_frames_track predicts it; gain and bias those of the last tracked frame in front of the frame's batch (the anchor
 *                     counts), whether predict is on or off: exposure is not extrapolated.
 *   levels            (q, a, b) of a level start where the previous level ended; a level that ends degenerate leaves all three as they were.
 *   verdict           emba_frames_track's.  A lost frame reports its predicted rotation and its start gain and bias, casts no vote, and is skipped by later
 *                     frames for the rotation and for the exposure alike.
 *   vote              a tracked frame votes clamp(rint(a_f * v + b_f), 0, 255) (emba_mosaic_frames_exposure's compensated byte) in the place of v into every
 *                     plane emba_frames_track votes into; skip_zero tests the raw byte.  The integer sums keep their units and their 2^36 bound:
 *                     emba_mosaic_get, emba_mosaic_map, use_mosaic, emba_track_level_get and emba_track_eval read them as they stand.
 *
 * emba_frames_track_exposure: emba_frames_track with settings.estimate and the two bounds of the gain; gain_out, bias_out [F] beside q_out (the anchor's are 1
 * and 0); cost_out is entry 20 of the last level's sums.  emba_track_exposure_eval: emba_track_eval with gain [F] and bias [F]; sums_out [F, 21].  Both read
 * and write the level planes emba_frames_track does: either tracker's planes serve either evaluation.
 * Refusals: emba_frames_track_exposure refuses what emba_frames_track refuses, then gain bounds that are not finite or not 0 < gain_min <= 1 <= gain_max, then
 * an estimate outside 0 ... 3; emba_track_exposure_eval refuses what emba_track_eval refuses, and gain or bias NULL with F > 0, a gain or bias that is not
 * finite, a gain <= 0; EMBA_ERR_STATE at a level that the last successful tracker call did not vote into.  Refusals are decided before anything is zeroed
 * and leave every output, the mosaic and the level planes untouched.  Chunks, batches, stats_out, pm_out and timer slot 7 are emba_frames_track's. */
typedef struct {
    emba_track_settings track;
    int32_t estimate;
    double gain_min, gain_max;
} emba_track_exposure_settings;
emba_status emba_frames_track_exposure(emba_ctx* ctx, const uint8_t* frames /* [F, sh, sw] */, const int64_t* frame_t_ns /* [F] */, size_t F,
                                       const double* q0_xyzw /* [4] */, const emba_track_exposure_settings* settings, double* q_out /* [F, 4] */,
                                       double* gain_out /* [F] */, double* bias_out /* [F] */, int32_t* status_out /* [F] */, int32_t* iters_out /* [F, n_levels] */,
                                       double* cost_out /* [F] */, uint64_t* counts_out /* [F, 4] */, double* overlap_out /* [F] */, uint64_t* stats_out /* [4] */,
                                       double* pm_out /* [F, sh*sw, 2] */);
emba_status emba_track_exposure_eval(emba_ctx* ctx, const uint8_t* frames /* [F, sh, sw] */, size_t F, const double* q_xyzw /* [F, 4] */,
                                     const double* gain /* [F] */, const double* bias /* [F] */, int32_t level, uint64_t min_weight, int32_t skip_zero, double huber_k,
                                     double* sums_out /* [F, 21] */, uint64_t* counts_out /* [F, 4] */, double* pm_out /* [F, sh*sw, 2] */,
                                     double* resid_out /* [F, sh*sw] */);

/* ---- Tracked frames refitted against the mosaic of the other frames.  A tracker aligns every frame once, against the frames before it
 * only.  The level planes are exact integer sums, so a frame's votes can be taken out again exactly: the same warp and the same cells, the added values
 * negated modulo 2^64.  What is left is the mosaic of all the other frames, earlier and later; aligning the frame to it and voting it back is one
 * Gauss-Seidel step of a global photometric refit.  The rule lives in emba_amd/csrc/refit_rule.h, over track_rule.h, track_exposure_rule.h and
 * exposure_rule.h; emba_amd.io.refit_frames is the same rule in numpy.  Everything that is not said here is emba_frames_track_exposure's.
 *
 *   input             F frames of bytes at frame_t_ns (strictly increasing) and per frame q [F, 4], gain [F], bias [F], status [F] (EMBA_TRACK_*): what either
 *                     tracker returns (the plain tracker's output takes gain 1 and bias 0).  The rotations are used as they are given: unit quaternions.
 *                     Anchors vote and never move: they are the gauge; any number of them, none among it.  At least one frame votes.
 *   settings          settings.track: the schedule, batch, skip_zero, min_weight, min_overlap, align, estimate and the gain bounds (predict is ignored);
 *                     sweeps >= 0; alternate: the odd sweeps visit the batches from the last to the first; recover: lost frames are tried; sweep_tol: the
 *                     call ends behind a sweep whose largest rotation change (rad) is below it, 0: never.
 *   build             the mosaic and every level plane of the schedule, and level 0, are zeroed, and every voting frame votes at its given (q, a, b):
 *                     emba_frames_track_exposure's vote.  What the context held is not trusted.  sweeps = 0 is this alone: a stitch at given rotations.
 *   a sweep           visits the batches as the tracker cuts them (frame 0 alone, then `batch` frames, a chunk boundary a batch boundary; a batch of
 *                     anchors alone is passed over).  Per batch:
 *                       un-vote   every tracked frame of the batch takes its votes out of every plane and its counts out of the two counters (dropped,
 *                                 skipped): the vote's kernel with every added value negated modulo 2^64
 *                       start     a tracked frame starts at its own (q, a, b).  With recover a lost frame starts from the nearest voting frames a < f < b by
 *                                 index, as the statuses stand at the start of the batch: the prediction's formula at t_f, whose factor (t_f - t_b) /
 *                                 (t_b - t_a) is negative — an interpolation — and gain and bias linear in the same factor; with a voting frame on one side
 *                                 only, that frame's values.  Without recover a lost frame is passed over
 *                       align     emba_frames_track_exposure's loop, level by level, against planes that no longer hold the batch's frames
 *                       verdict   emba_frames_track's.  A tracked frame that passes takes the new (q, a, b): EMBA_REFIT_MOVED; one that fails keeps what it
 *                                 had: EMBA_REFIT_KEPT.  A lost frame that passes becomes tracked: EMBA_REFIT_RECOVERED; one that fails keeps its input
 *                                 (q, a, b): EMBA_REFIT_LOST.  An anchor reports EMBA_REFIT_ANCHOR
 *                       vote      every tracked frame of the batch votes at the values it has now (a kept frame puts back what it took out)
 *   invariant         behind every batch every plane and both counters equal, as integers, the vote of all voting frames at their current (q, a, b).
 *
 * Outputs, each may be NULL: q_out, gain_out, bias_out, status_out (EMBA_TRACK_*) as they stand behind the call; refit_out [F]: the code of the last sweep
 * (behind sweeps = 0: EMBA_REFIT_ANCHOR for an anchor, EMBA_REFIT_LOST for a lost frame, 0 for a tracked one); iters_out [F, n_levels], cost_out, counts_out,
 * overlap_out: the last sweep's, 0 for a frame it did not align; sweep_out [sweeps, 4]: per sweep that ran the frames moved, the frames recovered, the
 * largest rotation change (rad; formed on the host from the rotations before and behind the sweep) and the sum of the last-level costs; sweeps_done_out;
 * stats_out [4] as emba_frames_track's; pm_out [F, sh*sw, 2]: the level-0 pm of each frame's last vote, NaN for a frame that does not vote.
 * Every sweep uploads the frames again chunk by chunk; rotations, exposures and statuses stay on the device for the whole call; behind each sweep the host
 * reads the rotations, the codes and the costs.  Refusals are decided before anything is zeroed and leave every output, the mosaic and the level planes
 * untouched: what emba_frames_track_exposure refuses (but for q0), and EMBA_ERR_INVALID_ARG for q, gain, bias or status NULL with F > 0, sweeps < 0, a
 * sweep_tol that is negative or a NaN, a status outside the three values, no voting frame, a q that is not finite or of zero norm, a gain that is not finite or
 * outside the bounds, a bias that is not finite.  What the trackers leave alone, this leaves alone. */
#define EMBA_REFIT_ANCHOR 1
#define EMBA_REFIT_MOVED 2
#define EMBA_REFIT_KEPT 3
#define EMBA_REFIT_RECOVERED 4
#define EMBA_REFIT_LOST 5
typedef struct {
    emba_track_exposure_settings track;
    int32_t sweeps, alternate, recover;
    double sweep_tol;
} emba_refit_settings;
emba_status emba_frames_refit(emba_ctx* ctx, const uint8_t* frames /* [F, sh, sw] */, const int64_t* frame_t_ns /* [F] */, size_t F, const double* q_xyzw /* [F, 4] */,
                              const double* gain /* [F] */, const double* bias /* [F] */, const int32_t* status /* [F] */, const emba_refit_settings* settings,
                              double* q_out /* [F, 4] */, double* gain_out /* [F] */, double* bias_out /* [F] */, int32_t* status_out /* [F] */,
                              int32_t* refit_out /* [F] */, int32_t* iters_out /* [F, n_levels] */, double* cost_out /* [F] */, uint64_t* counts_out /* [F, 4] */,
                              double* overlap_out /* [F] */, double* sweep_out /* [sweeps, 4] */, int32_t* sweeps_done_out, uint64_t* stats_out /* [4] */,
                              double* pm_out /* [F, sh*sw, 2] */);

/* ---- Loops closed among tracked frames: one frame aligned to another, and a rotation graph over all of them.  Every stage above compares a
 * frame with a panorama plane; here two frames that see the same place are compared with each other, and all rotations are solved for at once with the
 * anchors held exactly.  The rules live in emba_amd/csrc/pair_rule.h (over align_rule.h) and emba_amd/csrc/graph_rule.h; emba_amd.io.pair_* and
 * io.rotation_graph_solve are the same rules in numpy.
 *
 *   a pair            p = (i, j): source frame i, target frame j, both of the context's sensor [sh, sw]; a relative rotation Q_p (xyzw; used as it is given: a unit
 *                     quaternion) and a relative exposure (a_p, b_p), given and not estimated (NULL: 1 and 0).  A bearing
 *                     b of camera i is the bearing R(Q_p) b of camera j: with camera-to-world rotations Q = q_j^-1 (x) q_i, and with per-frame exposures
 *                     a = a_i / a_j, b = (b_i - b_j) / a_j.  i = j is a pair like any other, and a pair may be listed more than once.
 *   project           rb = R(Q) bearing_lut[s] by frame_warp's matrix and three sums; rb_z <= 0 is outside.  x = rb_x / rb_z, y = rb_y / rb_z; the
 *                     plumb_bob forward model with D = (k1, k2, p1, p2, k3) (NULL: zero, the pinhole): r2 = x^2 + y^2, c = 1 + ((k3 r2 + k2) r2 + k1) r2,
 *                     x' = x c + (2 p1 x y + p2 (r2 + 2 x^2)), y' = y c + (p1 (r2 + 2 y^2) + 2 p2 x y); u = fu x' + cu, v = fv y' + cv.  Without
 *                     contraction.  The intrinsics are arguments of the call: the context holds the bearing table alone.
 *   sample            frame j's bytes bilinearly at (u, v): ix = floor(u), iy = floor(v); outside for ix < 0, ix + 1 > sw - 1, iy < 0, iy + 1 > sh - 1, a
 *                     point that is not finite or >= 2^31 in size.  No wrap.  val, gx, gy are emba_frames_align's expressions on the four bytes as doubles.
 *   classes           emba_frames_align's four in its precedence: outside; masked: skip_zero and any of the four target bytes is 0; skipped: skip_zero
 *                     and the source byte is 0; used.
 *   term              r = val - (a v + b) in byte units (multiply, add, subtract: no contraction); the Huber weight of emba_frames_align;
 *                     g = gx Ju[0,:] + gy Ju[1,:] with Ju = d(u, v) / d rb (-[rb]x): the left perturbation Q <- exp(delta) Q.  The ten sums and the four
 *                     counts are emba_frames_align's, summed in a fixed order: the same inputs give the same bits.
 *   loop              emba_frames_align's, per pair, under the same settings, with the same four ways to end.
 *   information       info [6] = H / s^2 (00 01 02 11 12 22), s^2 = cost / max(n - 3, 1), of the accepted state: in camera j's coordinates.
 *
 * emba_frames_pair_eval: one evaluation of every pair at Q.  Outputs, each may be NULL: sums_out [P, 10], counts_out [P, 4] (used, outside, masked,
 * skipped), uv_out [P, sh*sw, 2] (NaN where rb_z <= 0), resid_out [P, sh*sw] (0 where the pixel is not used).
 * emba_frames_pair_align: the loop; q_out, sums_out, counts_out, status_out (EMBA_ALIGN_*), iters_out, cost0_out, n0_out as emba_frames_align's, info_out
 * [P, 6].  The frames are uploaded once, whole, into a buffer of this stage's own; the pairs are cut into chunks of at most 65 535 (and 32 MiB of source
 * pixels); a chunk's state stays on the device between iterations.  P = 0 launches nothing.  Timer slot 7 as in emba_frames_align.
 * Refusals, before anything is uploaded, every output untouched, EMBA_ERR_INVALID_ARG in this order: frames, pairs or Q NULL with P > 0; P >= 2^31; a pair
 * with a frame outside [0, F); a Q that is not finite or of zero norm; a gain that is not finite or not positive, a bias that is not finite; fu or fv not
 * finite or not positive; cu or cv not finite; a D that is not finite; huber_k a NaN; the settings as emba_frames_align refuses them; F * sh * sw above
 * 2^30 bytes (the sequence is resident for the whole call).  Nothing of the registered window, the last evaluation, the resident sequence, the mosaic, the
 * level planes, the resident map or any other stage's buffers is written. */
emba_status emba_frames_pair_eval(emba_ctx* ctx, const uint8_t* frames /* [F, sh, sw] */, size_t F, const int32_t* pairs /* [P, 2] */, size_t P,
                                  const double* Q_xyzw /* [P, 4] */, const double* gain /* [P] or NULL */, const double* bias /* [P] or NULL */, double fu, double fv,
                                  double cu, double cv, const double* D /* [5] or NULL */, int32_t skip_zero, double huber_k, double* sums_out /* [P, 10] */,
                                  uint64_t* counts_out /* [P, 4] */, double* uv_out /* [P, sh*sw, 2] */, double* resid_out /* [P, sh*sw] */);
emba_status emba_frames_pair_align(emba_ctx* ctx, const uint8_t* frames /* [F, sh, sw] */, size_t F, const int32_t* pairs /* [P, 2] */, size_t P,
                                   const double* Q_xyzw /* [P, 4] */, const double* gain /* [P] or NULL */, const double* bias /* [P] or NULL */, double fu, double fv,
                                   double cu, double cv, const double* D /* [5] or NULL */, int32_t skip_zero, const emba_align_settings* settings,
                                   double* q_out /* [P, 4] */, double* sums_out /* [P, 10] */, uint64_t* counts_out /* [P, 4] */, int32_t* status_out /* [P] */,
                                   int32_t* iters_out /* [P] */, double* cost0_out /* [P] */, uint64_t* n0_out /* [P] */, double* info_out /* [P, 6] */);

/* ---- The pair alignment coarse to fine over a pyramid of the sensor frames, with the pair's exposure estimated.  emba_frames_pair_align
 * starts inside the basin of the full-resolution alignment and takes the pair's exposure as given; here the same pair is aligned level by level, from frames
 * box-reduced by 2^l down to the frames themselves, and its relative gain and bias are estimated with its rotation.  The rule lives in
 * emba_amd/csrc/pair_level_rule.h (over pair_rule.h and exposure_rule.h); emba_amd.io.pair_level_* / pair_exposure_* / pair_align_levels are the same rule in
 * numpy.
 *
 *   level sizes       level l of the sensor [sh, sw] is [sh >> l, sw >> l], l = 0 ... 7; level pixel (X, Y) is the box of the pixels x in [X 2^l, (X + 1) 2^l),
 *                     y likewise; the columns and rows left over at the right and at the bottom take no part.  A level below 2 x 2 is refused.
 *   level bytes       (sum of the box + 4^l / 2) >> 2l in integers, formed from level 0 directly.  Under skip_zero a box that holds a zero byte is 0 ("no
 *                     data" stays "no data"), and a box without one gives 1 at the least.  Level 0 is the frame.
 *   level bearings    level 0 is the context's table (x', y', 1).  For l >= 1 the centre of a box is the corner shared by its four central pixels, and the
 *                     level's bearing is 0.25 ((b00 + b01) + (b10 + b11)) of those four, componentwise in this order: z stays 1.  Behind a pinhole that is
 *                     the centre's bearing but for rounding; behind a lens it is the bilinear midpoint.
 *   level camera      fu_l = fu / 2^l, fv_l = fv / 2^l, cu_l = (cu - (2^l - 1) / 2) / 2^l, cv_l likewise, D unchanged.  Level 0 is the camera bit for bit.
 *   term              emba_frames_pair_eval's, on the level's table, bytes, size and camera; with the source byte v the Jacobian row of r = val - (a v + b) in
 *                     (delta, a, b) is (g, -v, -1), and the 21 sums and four counts are emba_frames_exposure_eval's with I0 = v.  The ten sums they share
 *                     with emba_frames_pair_eval are its bits at level 0, and so are uv, the residuals and the counts.
 *   loop of a level   emba_frames_exposure_align's step on those sums: estimate (EMBA_EXPOSURE_GAIN | EMBA_EXPOSURE_BIAS), the gain bounds on the pair's
 *                     relative gain, the four ways to end.  min_pixels at level l is min_pixels >> 2l, but not below min(min_pixels, 8); every other setting
 *                     is the same at every level.
 *   schedule          levels[0 ... n_levels), 1 <= n_levels <= 8, each 0 ... 7, in any order.  A pair starts level k + 1 from its accepted (Q, a, b) of level
 *                     k.  A level that ends converged, on iterations or stalled hands its accepted state on; a level that ends degenerate ends the pair
 *                     there: its final status is degenerate and its outputs are that level's accepted state.  The final status, sums and counts are the
 *                     last level run; info is emba_frames_pair_align's, from that level's ten shared sums.  The schedule (0) with estimate = 0 is
 *                     emba_frames_pair_align bit for bit.
 *
 * emba_frames_pair_level_eval: one evaluation of every pair at Q on level `level`, S_l = (sh >> l) (sw >> l).  Outputs, each may be NULL: sums_out [P, 21],
 * counts_out [P, 4], uv_out [P, S_l, 2], resid_out [P, S_l], level_bytes_out [F, S_l], level_lut_out [S_l, 3].
 * emba_frames_pair_align_levels: the schedule.  Outputs, each may be NULL: q_out [P, 4], gain_out, bias_out [P], sums_out [P, 21], counts_out [P, 4],
 * status_out [P], iters_out [P] (summed over the levels), level_status_out and level_iters_out [P, n_levels] (0 where a level was not run), cost0_out and
 * n0_out [P] (of the first level), info_out [P, 6].  The frames are uploaded once and their pyramid is made once per call; the pairs go in
 * emba_frames_pair_align's chunks, the schedule runs inside a chunk, and the state stays on the device between levels.  P = 0 launches nothing.  Timer slot 7
 * brackets the first evaluation kernel of a call, timer slot 6 the launches of the kernel that makes the level bytes (where a level above 0 is asked for).
 * Refusals, before anything is uploaded, every output untouched, EMBA_ERR_INVALID_ARG in this order: emba_frames_pair_eval's up to huber_k; levels NULL or
 * n_levels = 0; n_levels > 8; a level outside 0 ... 7; a level too small for the sensor, named in the message; estimate outside 0 ... 3; the gain bounds;
 * the loop's settings; F * sh * sw above 2^30 bytes.  (emba_frames_pair_level_eval: the arguments, the level, the bytes.)  Nothing of the registered window,
 * the resident sequence, the mosaic, the level planes of the trackers, the resident map or any other stage's buffers is written. */
emba_status emba_frames_pair_level_eval(emba_ctx* ctx, const uint8_t* frames /* [F, sh, sw] */, size_t F, const int32_t* pairs /* [P, 2] */, size_t P,
                                        const double* Q_xyzw /* [P, 4] */, const double* gain /* [P] or NULL */, const double* bias /* [P] or NULL */, double fu,
                                        double fv, double cu, double cv, const double* D /* [5] or NULL */, int32_t skip_zero, double huber_k, int32_t level,
                                        double* sums_out /* [P, 21] */, uint64_t* counts_out /* [P, 4] */, double* uv_out /* [P, S_l, 2] */,
                                        double* resid_out /* [P, S_l] */, uint8_t* level_bytes_out /* [F, S_l] */, double* level_lut_out /* [S_l, 3] */);
emba_status emba_frames_pair_align_levels(emba_ctx* ctx, const uint8_t* frames /* [F, sh, sw] */, size_t F, const int32_t* pairs /* [P, 2] */, size_t P,
                                          const double* Q_xyzw /* [P, 4] */, const double* gain /* [P] or NULL */, const double* bias /* [P] or NULL */, double fu,
                                          double fv, double cu, double cv, const double* D /* [5] or NULL */, int32_t skip_zero, const int32_t* levels /* [n_levels] */,
                                          size_t n_levels, int32_t estimate, const emba_exposure_settings* settings, double* q_out /* [P, 4] */,
                                          double* gain_out /* [P] */, double* bias_out /* [P] */, double* sums_out /* [P, 21] */, uint64_t* counts_out /* [P, 4] */,
                                          int32_t* status_out /* [P] */, int32_t* iters_out /* [P] */, int32_t* level_status_out /* [P, n_levels] */,
                                          int32_t* level_iters_out /* [P, n_levels] */, double* cost0_out /* [P] */, uint64_t* n0_out /* [P] */,
                                          double* info_out /* [P, 6] */);

/* emba_rotation_graph_solve: the rotation graph, on the host (it needs no context; emba_last_error(NULL) has the message of a refusal).
 *   unknowns          one rotation per frame (camera to world, xyzw).  Frames whose status is EMBA_TRACK_ANCHOR are constants: the gauge is exact.  A frame
 *                     that no edge names keeps its input.  q_out of either is the input bit for bit.
 *   edge              (i, j, Q_ij, Lambda_ij [6]: 00 01 02 11 12 22): e = log(Q_ij (x) q_i^-1 (x) q_j), the rotation vector of the shorter way round, in
 *                     camera j's coordinates, where emba_frames_pair_align's info lives.  The cost is the sum of e^T Lambda e over the edges.
 *   step              with q <- exp(delta) q on both ends e' ~ e + Jr^-1(e) R_j^T (delta_j - delta_i); (A + lambda diag A) delta = -g by conjugate
 *                     gradients with the 3 x 3 block-Jacobi preconditioner, matrix-free over the edges in edge order, ended at |r| <= cg_tol |r0| or
 *                     behind cg_max_iters iterations.  The trial is accepted when its cost is below the cost: lambda <- max(lambda / lambda_down,
 *                     lambda_min); otherwise lambda <- lambda lambda_up.
 *   ends              EMBA_GRAPH_CONVERGED: |delta|_inf < tol (also: nothing is free); EMBA_GRAPH_STALLED: lambda > lambda_max; EMBA_GRAPH_ITERATIONS:
 *                     max_iters trials; EMBA_GRAPH_DEGENERATE: a diagonal block is not positive definite.
 * Outputs, each may be NULL: q_out [F, 4]; cost_out [2]: before and behind; iters_out [2]: the trials and the conjugate-gradient iterations of all of
 * them; end_out; at_out: the frame or edge a refusal names.  Refusals, EMBA_ERR_INVALID_ARG in this order, every output but at_out untouched: q or status
 * NULL with F > 0; edges, Q or info NULL with E > 0; settings NULL or out of range; a q that is not finite or of zero norm; no anchor; an edge with a frame
 * outside [0, F); an edge's Q not finite or of zero norm; an info that is not finite; a frame that is no anchor, that an edge names and that no path of
 * edges connects to an anchor: the first such frame. */
#define EMBA_GRAPH_CONVERGED 1
#define EMBA_GRAPH_STALLED 2
#define EMBA_GRAPH_ITERATIONS 3
#define EMBA_GRAPH_DEGENERATE 4
typedef struct {
    int32_t max_iters, cg_max_iters;
    double lambda0, lambda_up, lambda_down, lambda_min, lambda_max, tol, cg_tol;
} emba_graph_settings;
emba_status emba_rotation_graph_solve(const double* q_xyzw /* [F, 4] */, const int32_t* status /* [F] */, size_t F, const int32_t* edges /* [E, 2] */,
                                      const double* Q_xyzw /* [E, 4] */, const double* info /* [E, 6] */, size_t E, const emba_graph_settings* settings,
                                      double* q_out /* [F, 4] */, double* cost_out /* [2] */, int32_t* iters_out /* [2] */, int32_t* end_out, size_t* at_out);

/* ---- Loop-closure pairs found by appearance: coarse frame matching.  The pairs above are chosen from the tracked rotations, so a loop that
 * the tracker's drift hides is not found.  Here pairs are proposed from the frames' bytes alone: every frame's thumbnail is compared with every other's under
 * every integer shift of a range, and a matched pair brings the coarse start its shift stands for.  The rule lives in emba_amd/csrc/match_rule.h (over
 * pair_level_rule.h); emba_amd.io.match_* is the same rule in numpy.  Everything is integer arithmetic up to one score per shift, whose five floating-point
 * operations are correctly rounded on both sides: numpy gives the same integers and the same score bits.
 *
 *   thumbnails        level l of every frame by emba_frames_pair_level_eval's level bytes, under skip_zero as there (a box that holds a zero is 0: "no data");
 *                     level 0 is the frames themselves.  w = sw >> l, h = sh >> l, S_l = w h <= 16 384.
 *   a shift           d = (dx, dy), |dx| <= rx, |dy| <= ry, claims A_i(x, y) ~ A_j(x + dx, y + dy).  Its overlap is every (x, y) with both points inside
 *                     [0, w) x [0, h); under skip_zero a point where either byte is 0 takes no part.  Over the overlap six integer sums: n, sum a, sum b,
 *                     sum a^2, sum b^2, sum a b (each below 2^32; reported as uint64).  The shift index is row-major: dy from -ry, then dx from -rx.
 *   score             cov = n sab - sa sb, va = n saa - sa^2, vb = n sbb - sb^2, exact in int64; score = (double)cov |(double)cov| / ((double)va (double)vb),
 *                     in this order, without contraction: the signed square of the zero-mean normalised correlation.  A shift is not scored where
 *                     n < n_min, va = 0 or vb = 0.
 *   best of a pair    the scored shift of greatest score, ties to the lowest shift index; a pair with no scored shift reports score = -2, d = (0, 0), n = 0.
 *   search            candidates are the pairs i < j with j - i > min_gap whose frames both vote (status [F]: EMBA_TRACK_ANCHOR or EMBA_TRACK_TRACKED; NULL:
 *                     every frame).  Per frame f the k partners, on either side of f, of greatest best score among those with score >= score_min (a pair
 *                     without a scored shift never is one), ties to the lower partner index.  The shift is oriented from the lower index to the higher, as
 *                     evaluated (the sums are symmetric: only i < j is evaluated).  Where fewer than k qualify: partner -1, score -2, shift (0, 0), n 0.
 *   start             emba_match_start: with c = ((sw - 1) / 2, (sh - 1) / 2) and t = 2^l (dx, dy) / 2, the pixels p_i = c - t of frame i and p_j = c + t of
 *                     frame j show the same place.  Pinhole bearings ((x - cu) / fu, (y - cv) / fv, 1), normalised: b = (bx, by, 1) / sqrt((bx^2 + by^2) + 1).
 *                     Q = (b_i x b_j, 1 + ((b_ix b_jx + b_iy b_jy) + b_iz b_jz)) / its norm sqrt(((x^2 + y^2) + z^2) + w^2): the shortest arc, R(Q) b_i =
 *                     b_j, zero roll — emba_frames_pair_eval's convention.  A lens is ignored: the alignment refines the start.  d = 0 is (0, 0, 0, 1).
 *
 * emba_frames_match_eval: the best shift of every pair of a list (i = j and i > j are pairs like any other, evaluated as given).  Outputs, each may be NULL:
 * score_out [P], shift_out [P, 2] (dx, dy), n_out [P], sums_out [P, (2 rx + 1)(2 ry + 1), 6].
 * emba_frames_match_search: the search.  Outputs, each may be NULL: partner_out [F, k], score_out [F, k], shift_out [F, k, 2], n_out [F, k].
 * The frames are uploaded once and their thumbnails are made once per call (emba_frames_pair_level_eval's pyramid kernel; none at level 0).  One workgroup
 * per pair, in launches of at most 2^20 pairs (with sums_out: at most 64 MiB of sums); the search keeps the best of every pair i < j in a triangular table of
 * 24 bytes per pair on the device, bounded at 2^30 bytes (F = 9 459), and one wave per frame selects from it.  P = 0, or a search without a candidate pair,
 * launches nothing (the search then fills its outputs with "none").  With kernel timing on, timer slot 7 brackets the first evaluation launch of a call and
 * timer slot 6 the select kernel.
 * Refusals, before anything is uploaded, every output untouched, EMBA_ERR_INVALID_ARG in this order: frames NULL; F = 0 or F >= 2^31; (the list) pairs NULL
 * with P > 0, P >= 2^31, a pair with a frame outside [0, F); a level outside 0 ... 7; a level below 2 x 2, named in the message; S_l > 16 384, with the smallest
 * level that fits in the message; rx < 0, ry < 0, rx >= w or ry >= h; n_min = 0; (the search) k outside 1 ... 64, min_gap < 0, score_min a NaN; F * sh * sw
 * above 2^30 bytes; (the search) the table above 2^30 bytes.  emba_match_start needs no context (emba_last_error(NULL) has the message): q_out NULL, a level
 * outside 0 ... 7, sw or sh not positive, fu or fv not finite or not positive, cu or cv not finite.  Nothing of the registered window, the resident sequence,
 * the mosaic, the level planes, the resident map or any other stage's buffers is written. */
emba_status emba_frames_match_eval(emba_ctx* ctx, const uint8_t* frames /* [F, sh, sw] */, size_t F, const int32_t* pairs /* [P, 2] */, size_t P, int32_t level,
                                   int32_t rx, int32_t ry, int32_t skip_zero, uint32_t n_min, double* score_out /* [P] */, int32_t* shift_out /* [P, 2] */,
                                   uint64_t* n_out /* [P] */, uint64_t* sums_out /* [P, shifts, 6] */);
emba_status emba_frames_match_search(emba_ctx* ctx, const uint8_t* frames /* [F, sh, sw] */, size_t F, const int32_t* status /* [F] or NULL */, int32_t level,
                                     int32_t rx, int32_t ry, int32_t min_gap, int32_t skip_zero, uint32_t n_min, double score_min, int32_t k,
                                     int32_t* partner_out /* [F, k] */, double* score_out /* [F, k] */, int32_t* shift_out /* [F, k, 2] */,
                                     uint64_t* n_out /* [F, k] */);
emba_status emba_match_start(int32_t dx, int32_t dy, int32_t level, double fu, double fv, double cu, double cv, int32_t sensor_w, int32_t sensor_h,
                             double* q_out /* [4] */);

/* The median blur of the initial map (emba.cpp:357-364): convertTo(CV_32FC1) (round to nearest even), cv::medianBlur(., ., 3) with replicated borders
 * (SURVEY.md Appendix A), convertTo(CV_64FC1).  The median selects one of its nine inputs, so the result is exact; NaN input is undefined, as in OpenCV.
 * emba_median_blur3_map: both planes of the CURRENT resident map, in place (a map bound with emba_bind_map_dev is left untouched: the blurred map becomes
 * the context's own).  EMBA_ERR_STATE without a resident map or while a trial map is pending.  emba_median_blur3: the same for any h x w host plane
 * (row-major doubles; dst_host may be src_host); needs a context only. */
emba_status emba_median_blur3_map(emba_ctx* ctx);
emba_status emba_median_blur3(emba_ctx* ctx, const double* src_host, int32_t h, int32_t w, double* dst_host);

/* Schur-complement solve: LEGM::solveNormalEq(A11, A12, A22_blocks, b1, b2, lambda, x1, x2), model.cpp:721-792,
 * on the device-resident normal equations of the last emba_form_finish (so after applyL2Reg, as in solver.cpp:130,190-202),
 * consuming the SPARSE A12 factors: S = A11m - A12 A22m^-1 A12^T is formed chunk-wise from per-pixel column pairs built from the
 * records, x1 = S \ (b1 - A12 A22m^-1 b2) by a blocked Cholesky that treats a vanishing pivot the way Eigen's ldlt does (model.cpp:789:
 * the pseudo-inverse of D — a control pose no event constrains gets a ZERO update; emba_last_solve_info bit 1 reports it),
 * x2 = A22m^-1 (b2 - A12^T x1).  LM damping as the reference:
 * A11m = A11 + lambda*diag(A11), A22m = A22 + lambda*diag(A22).  fix_first_pose != 0 reproduces the first-window trim of
 * solver.cpp:156-165 (rows/cols 0..2 dropped; x1[0..2] = 0 on return).  x1_host: 3K doubles, x2_host: 2P doubles (either may
 * be NULL).  Works on this context's own records: with a sharded window use emba_solve_shard_* (a pixel's A12 columns are sums over all
 * ranks' records, so the records are first re-distributed by pixel owner). */
emba_status emba_solve_normal_eq(emba_ctx* ctx, double lambda, int32_t fix_first_pose, double* x1_host, double* x2_host);
/* The two halves of that solve, each with the other unknown held fixed.  Same preconditions (after emba_form_finish, no trial evaluation pending), same damping.
 *   emba_solve_map_only    mapping with known poses, x1 = 0: the residual is linear in the map and an event touches one panorama pixel, so the map block is
 *                          block diagonal — x2_i = (A22_i + lambda diag A22_i)^-1 b2_i per active pixel, by the Schur solve's own 2x2 rule (a block that is not
 *                          positive definite: info bit 0, EMBA_ERR_NUMERIC).  Well posed from an all-zero map, where the joint system is singular (every pose
 *                          Jacobian vanishes with G = 0): the way to start a run without a front-end map.  Reads the A22 | b2 rows of the pack only — no record
 *                          lists, no Schur matrix.  x2_host: 2P doubles or NULL; x2 stays on the device for emba_update_map(ctx, NULL, damping) either way.
 *                          P = 0: EMBA_OK, nothing written.
 *   emba_solve_poses_only  the pose block alone, (A11 + lambda diag A11) x1 = b1, by the same Cholesky: fix_first_pose as above (x1[0..2] = 0), a vanishing pivot
 *                          is a zero update (info bit 1), an indefinite or NaN matrix info bit 2 (EMBA_ERR_NUMERIC).  x1_host: 3K doubles.  Keeps no x2 and
 *                          drops a kept one: emba_update_map(ctx, NULL, ...) is EMBA_ERR_STATE until another solve leaves one.  A rejected trial of such a step
 *                          is reported with emba_map_reject / emba_trial_reject as usual (there is no trial map: only the equations come back).
 * Neither changes what a later emba_solve_normal_eq[_cg] on the same equations returns. */
emba_status emba_solve_map_only(emba_ctx* ctx, double lambda, double* x2_host);
emba_status emba_solve_poses_only(emba_ctx* ctx, double lambda, int32_t fix_first_pose, double* x1_host);
/* Diagnostics of the last Schur solve of this context (emba_solve_map_only / _poses_only included): bit 0 = a 2x2 block was not positive definite (EMBA_ERR_NUMERIC was returned),
 * bit 1 = a pivot of S vanished and its component got a zero update (what ldlt.info() == NumericalIssue is in the reference: never read). */
emba_status emba_last_solve_info(const emba_ctx* ctx, int32_t* info);

/* The same Schur solve for a window sharded over n_ranks GPUs (events sharded by time, A12 factors stay sharded).
 * A pixel's A12 columns are sums over ALL ranks' records of that pixel, and S needs the outer products of the summed columns, so the
 * records are first re-distributed by pixel owner (rank r owns the active pixels [P r / n, P (r+1) / n) in ascending panorama order):
 *   emba_solve_shard_count   counts_host[n_ranks] = this rank's valid records on active pixels, by owner
 *   emba_solve_shard_pack    packs them owner-major into send_dev (16 doubles each; tail word = {compact pixel index, pose-pair key})
 *   -- caller: all-to-all of the records (RCCL send/recv, torch.distributed.all_to_all_single) into recv_dev / n_recv --
 *   emba_solve_shard_partial S_part_dev (emba_solve_shard_size doubles) = - sum over the OWNED pixels of U_aug U_aug^T
 *   -- caller: all-reduce(SUM) of S_part_dev --
 *   emba_solve_shard_finish  adds the replicated [A11m | b1], factors, x1 -> x1_host (identical on every rank); x2 of the owned pixels
 *                            into x2_full_dev (2P doubles, zero elsewhere: the caller all-reduces it to get every rank's full x2)
 * Call after emba_form_finish (A22/b2 all-reduced, L2 applied), all on the context's stream.  Tested as rank threads on one GPU
 * against the single-process oracle (tests/test_gpu_sharded.py).
 * Re-solves (round 6): solver.cpp:340-352 solves the SAME equations again with a larger lambda after every rejected trial.  A rank keeps the records it received
 * for its pixels (in pixel order) until new equations are formed; emba_solve_shard_cached says whether it still holds them for the current equations — when every
 * rank does, skip count / pack / all-to-all and pass recv_dev = NULL, n_recv = the cached count to _partial and _finish. */
emba_status emba_solve_shard_size(emba_ctx* ctx, size_t* s_doubles);
emba_status emba_solve_shard_count(emba_ctx* ctx, int32_t n_ranks, size_t* counts_host);
emba_status emba_solve_shard_pack(emba_ctx* ctx, int32_t n_ranks, double* send_dev);
emba_status emba_solve_shard_cached(emba_ctx* ctx, int32_t rank, int32_t n_ranks, int32_t* cached, size_t* n_recv);
emba_status emba_solve_shard_partial(emba_ctx* ctx, int32_t rank, int32_t n_ranks, const double* recv_dev, size_t n_recv,
                                     double lambda, double* S_part_dev);
emba_status emba_solve_shard_finish(emba_ctx* ctx, int32_t rank, int32_t n_ranks, const double* recv_dev, size_t n_recv,
                                    double lambda, int32_t fix_first_pose, double* S_dev, double* x1_host, double* x2_full_dev);

/* LEGM::solveNormalEqCG for a sharded window (round 6; model.cpp:794-840 with the pixels sharded by owner as in the Schur solve): the per-rank steps around the
 * caller's collectives.  A CG vector is [3K pose entries, replicated | this rank's pixels' map entries]; `red_dev` holds emba_cg_shard_size doubles = 3K + 2:
 *   emba_cg_shard_begin      (after the record exchange, or with recv_dev = NULL where emba_solve_shard_cached allows) x = 0, r = b, p = invd r;
 *                            red[3K] = r.r, red[3K+1] = r.p, partial                           -- caller: all-reduce(SUM) red_dev (3K + 2) --
 *   emba_cg_shard_apply      t = M p on the rank's pixels; red[0..3K) = its share of the pose part of t, red[3K] = its p.t    -- all-reduce red_dev (3K + 2) --
 *   emba_cg_shard_pt         takes the reduced pose part; *pt = p.t (host, identical on every rank)        [alpha = r.z / p.t]
 *   emba_cg_shard_update     x += alpha p, r -= alpha t, z = invd r; red[3K] = r.r, red[3K+1] = r.z, partial         -- all-reduce red_dev + 3K (2) --
 *   emba_cg_shard_direction  p = z + beta p                                                                [beta = r.z / previous r.z]
 *   emba_cg_shard_end        x1 -> x1_host; the rank's x2 into x2_full_dev (2P doubles, zero elsewhere)               -- all-reduce x2_full_dev (2P) --
 * The loop and its stopping rule are Eigen's (ConjugateGradient.h:28-88): emba_group_solve_cg, emba_amd/sharded.py: ShardedLEGM.solveNormalEqCG. */
emba_status emba_cg_shard_size(emba_ctx* ctx, size_t* red_doubles);
emba_status emba_cg_shard_begin(emba_ctx* ctx, int32_t rank, int32_t n_ranks, const double* recv_dev, size_t n_recv, double lambda, int32_t fix_first_pose, double* red_dev);
emba_status emba_cg_shard_apply(emba_ctx* ctx, double* red_dev);
emba_status emba_cg_shard_pt(emba_ctx* ctx, const double* red_dev, double* pt);
emba_status emba_cg_shard_update(emba_ctx* ctx, double alpha, double* red_dev);
emba_status emba_cg_shard_direction(emba_ctx* ctx, double beta);
emba_status emba_cg_shard_end(emba_ctx* ctx, double* x1_host, double* x2_full_dev);

/* LEGM::solveNormalEqCG (model.cpp:794-840; selected by BA_config.use_CG at solver.cpp:190-202): Eigen's ConjugateGradient (default
 * diagonal preconditioner, zero initial guess; max_iter <= 0 -> 100, tol <= 0 -> 1e-6 as in the reference) on the full system
 * [A11m A12; A12^T A22m], applied matrix-free through the sparse A12 factors.  iterations / error = cg.iterations() / cg.error(). */
emba_status emba_solve_normal_eq_cg(emba_ctx* ctx, double lambda, int32_t fix_first_pose, int32_t max_iter, double tol,
                                    double* x1_host, double* x2_host, int32_t* iterations, double* error);

/* Bind caller-owned device buffers that the caller all-reduces between phases:
 *   count_map_dev : int32 pano_h*pano_w                       (exchange 1)
 *   pack_dev      : f64, capacity pack_cap doubles, laid out [A11 9K^2 | b1 3K | A22b2 5P]
 *                   with A22b2 = per active pixel {xx, xy, yy, bx, by}   (exchange 2)
 * Pass NULLs to return to context-owned buffers. */
emba_status emba_bind_exchange_buffers(emba_ctx* ctx, int32_t* count_map_dev, double* pack_dev,
                                       size_t pack_cap);

/* Enqueue whatever is still needed for the device count map (own or bound with emba_bind_exchange_buffers) to hold num_ev_map of the
 * last evaluation (model.cpp:227).  The evaluation itself only marks touched pixels there — the count of a pixel is accumulated
 * next to its A22/b2 sums, one atomic request per measurement — and the markers become counts in the first dense pass that follows
 * (emba_form_active, emba_count_compress, a map download).  A host that reads or all-reduces a BOUND count map directly, before
 * any of those, calls this first. */
emba_status emba_count_map_ready(emba_ctx* ctx);

/* Exchange-1 compression for multi-GPU hosts: the merged count map only decides `count >= thres` (model.cpp:333,409), so each rank
 * may send min(count, cap) as ONE BYTE per pixel (cap * world_size <= 255, thres <= cap) — a quarter of the int32 volume on the
 * xGMI links.  emba_count_compress writes the saturated bytes of the context's count map to u8_dev (pano_h*pano_w bytes);
 * emba_count_expand stores the (all-reduced) bytes back as int32.  After that the map holds saturated, not exact, totals. */
emba_status emba_count_compress(emba_ctx* ctx, uint8_t* u8_dev, int32_t cap);
emba_status emba_count_expand(emba_ctx* ctx, const uint8_t* u8_dev);

/* Phase F1 of a RESIDENT step on a rank of a sharded window (round 5: what emba_step does on one GPU, between the two exchanges): emba_eval_finish +
 * emba_form_active in the step's form — launch A leaves per-unit active lists and zeroes the touched-but-inactive accumulator lines, the active-set write +
 * A22 | b2 gather ride inside the Gram launch of the emba_form_accumulate that follows and zero the lines they read, so the next evaluation needs no clearing
 * pass.  global_counts_u8_dev: the all-reduced saturated byte counts of exchange 1 (emba_count_compress on every rank, then the caller's all-reduce) — activity is
 * decided from THEM (model.cpp:333,409 on the global counts) while the context's own count map keeps this rank's counts; NULL: from the count map.  Asynchronous;
 * P comes from emba_last_counts once the Gram launch is enqueued.  No applyL2Reg here: emba_form_finish(alpha) after exchange 2.  This evaluation's per-pixel
 * sums are consumed: a second formNormalEq on it rebuilds A22 | b2 from the records. */
emba_status emba_step_form_active(emba_ctx* ctx, int32_t thres_valid_pixel, const uint8_t* global_counts_u8_dev);

/* Phase E1: pose table, Hessian/texel pack, warp + residual + count + factor records.  Asynchronous
 * on the context's stream.  After it the count map holds THIS rank's counts. */
emba_status emba_eval_launch(emba_ctx* ctx, const double* knots_xyzw_host, int32_t K, int64_t t0_ns,
                             int64_t dt_ns);
/* Phase E2: residual compaction into reference order.  With any non-NULL output it synchronizes, returns the
 * inlier count and copies ep / the (possibly all-reduced) count map to the host; with all three NULL it only
 * enqueues work (the count is available from emba_last_counts after the next synchronizing call). */
emba_status emba_eval_finish(emba_ctx* ctx, double* ep_out_host, size_t* n_inliers,
                             int32_t* num_ev_map_out_host);
/* Phase F1: active set from the (all-reduced) count map.  With P or pack_len non-NULL it synchronizes to return P
 * and the number of doubles of the pack [A11 | b1 | A22b2] that exchange 2 must all-reduce; with both NULL it only
 * enqueues work (single-GPU steps then need ONE host synchronization, in emba_form_finish). */
emba_status emba_form_active(emba_ctx* ctx, int32_t thres_valid_pixel, size_t* P, size_t* pack_len);
/* Phase F2: zero the pack and accumulate this rank's measurements into it.  Asynchronous.
 * ep_host as in emba_form_normal_eq. */
emba_status emba_form_accumulate(emba_ctx* ctx, const double* ep_host, int32_t irls, double eta);
/* Phase F3: applyL2Reg on the (all-reduced) pack — at most once per emba_form_accumulate, later calls with alpha != 0 only
 * download — then optional download (any pointer may be NULL); synchronizes. */
emba_status emba_form_finish(emba_ctx* ctx, double alpha, double* A11, double* b1, uint32_t* active_idx,
                             size_t cap_P, double* A22, double* b2, double* A12_dense);

/* One whole resident step in one call (what bench.py times on a single GPU): emba_eval_launch + emba_eval_finish +
 * emba_form_active + emba_form_accumulate(device-resident ep) + emba_form_finish(alpha, no downloads), one host
 * synchronisation at the end.  n_inliers / P may be NULL. */
emba_status emba_step(emba_ctx* ctx, const double* knots_xyzw_host, int32_t K, int64_t t0_ns, int64_t dt_ns,
                      int32_t thres_valid_pixel, int32_t irls, double eta, double alpha, size_t* n_inliers, size_t* P);

/* Declare the robust cost of the formNormalEq[IRLS] calls that will follow the next evaluations (irls: 0 quadratic, 1 huber,
 * 2 cauchy; eta as in formNormalEqIRLS, model.cpp:493-687).  The reference applies the IRLS weight w(e) to A22/b2 in
 * formNormalEqIRLS (model.cpp:599-636); the weight only depends on the residual, which the evaluation has in hand, so an
 * evaluation that knows the cost accumulates the WEIGHTED per-pixel sums directly and the following emba_form_accumulate with the
 * same (irls, eta) takes A22/b2 from them instead of a second pass over the records.  Purely a speed hint: results are the same
 * with any declaration (a mismatch falls back to the records).  emba_step declares its own cost for its own evaluation. */
emba_status emba_set_cost(emba_ctx* ctx, int32_t irls, double eta);

/* Tuning and A/B switches: options by name, integer values, part of the ABI (EMBA_ABI_VERSION 2); an unknown name or a value out
 * of range is EMBA_ERR_INVALID_ARG.  Every option changes SPEED or the internal form only — results are the same under all of them (tests/test_gpu_variants.py
 * runs every kernel variant they select against the oracle; tests/option_matrix.py lists which test covers each option and value, or why none has to).
 * Defaults are what the measurements under profiles/ chose.
 *   order          0 auto | 1 pixel order | 2 tile order of the device's event stream (takes effect at the next evaluation: the order is rebuilt)
 *   texel          0 auto | 1 pack every texel | 2 3x3 stencil on the fly | 3 pack inside the previous footprint's rectangle
 *                  (3: packed when the map has changed — upload, bind, update, accept, reject, blur — or the footprint has left the packed rectangle, not in every
 *                  evaluation; a map bound with emba_bind_map_dev is the caller's memory and counts as changed at every evaluation)
 *   segpose        0 auto (= 2) | 1 per-batch pose table in pixel order | 2 per-event pose from the K-1 segment records
 *   gram_tags      1 the pixel order's 8-B tag stream lets the Gram kernel skip dead slots | 0 decide from the records
 *   step_ep        1 emba_step compacts the residuals into ep (what evaluateDataError returns): in the tail of its Gram launch, or for windows of more than
 *                  8.4 M entries by a scan + a compaction launch behind it (2: that form always) | 0 on demand only.  (emba_get_option "ep_valid", read-only: the device holds ep)
 *   step_fast      1 emba_step zeroes the per-pixel sums behind their reader (no clearing pass) | 0 keeps the clearing pass
 *   step_gather    0 sweeping active-set write | 1 list-driven gather as a launch | 2 (default) inside the Gram kernel | 3 inside it at every size
 *   step_one_set   1 emba_step keeps one record set | 0 alternates between two like an LM loop
 *   step_prep      0 the launch in front of the warp kernel always | 2 (default) none on clean accumulator lines and fresh texels (pixel order, segpose, K <= seg_by_value + 1):
 *                  the host forms the K-1 segment records (the launch's own chain compiled for the host; its atan / sin / cos are the host C library's, the launch's
 *                  are the device library's: the records agree to the last bits, not always in them) and the warp kernel takes them by value in its arguments; its
 *                  workgroup 0 leaves them in device memory for later readers | 1 the same step (K <= 104):
 *                  workgroup 0 of the warp kernel forms the K-1 segment records and hands them to the others inside the launch (measured: no faster).  step_prep_polls (1024; 0 ... 65536): polls a wave waits for
 *                  the records before it forms its own (0: every wave does; same bits).
 *                  emba_get_option, read-only, of the last evaluation: "prep_on_host", "prep_in_warp" (no launch in front: value 2, value 1), "texels_packed"
 *                  (its launch packed texels); "step_prep_fallbacks": waves that formed their own records since the context was created (drains the stream);
 *                  "seg_by_value": segment records the warp kernel's arguments have room for
 *   gram_sparse    -1 auto (by the active-pixel count of the window's last equations) | 0 | 1 the Gram kernel's form for slot streams with few live records (pixel
 *                  order on a large panorama): stages of 128 tags, the live slots compacted, only their records fetched;  gram_sparse_chunk 1 ... 8 (4): its slots per wave, x 1024
 *   gather_waves   0 auto (4) | 1 | 2 | 4 waves of a Gram workgroup do its slice of the gather
 *   gram_multikey  0 (default) the dense pixel-order Gram launch is pair-aligned while the records fit the Infinity Cache: every streaming wave's slot range lies
 *                  inside one control-pose pair's run of slots, cut once per window | 1 the multi-key form always (equal shares of the slot range, pair changes
 *                  in mid-stream go through the workgroup's keyed LDS table).  emba_get_option "gram_paired", read-only: the last Gram launch was pair-aligned
 *   chunk_order_bin 0 tile-order chunks longest first | 1 in bin order
 *   tile_shape     -1 auto (fewest entries + chunks) | 0 48x24 | 1 72x16 | 2 96x12 | 3 36x32: the tiled kernel's LDS tile;  tile_fine -1 auto | 0 | 1 the finer grid of tile origins;
 *                  tile_reserve 0 ... 5 (2): pixels kept free on every side of a tile when chains are cut into tile-sized segments;  tile_min_events (1650000): fewest
 *                  events for which order = 0 considers the tile order;  tile_chunk 0 auto | entries per workgroup of the tiled kernel
 *   solve_perm     -1 auto | 0 | 1 U's columns ordered by panorama column in the Schur solve
 *   solve_counts   -1 auto | 0 list lengths counted from the records | 2 both, compared
 *   syrk_dense     1 dense instead of block-sparse SYRK;  syrk_lists 0 auto | 1 the block-sparse SYRK's per-pair slice lists always | 2 its (pair, chunk) items always;
 *                  syrk_min_cols 64 ... 4096 (512): fewest columns of U a workgroup of the dense split-K SYRK takes;  syrk_item_cap 1 ... 65536 (4096): slabs of the item
 *                  form (an item beyond them adds its tile to S by global atomics)
 *   poison         1 (tests) fills every NEW device allocation of the context with 0xFF bytes: a read of never-written workspace then shows as NaN / 0xFFFFFFFF
 *   solve_debug    1 prints the band statistics of a solve
 *   contrast_vote  -1 auto | 0 | 1 the vote kernel of emba_seq_contrast_gradient_level: by the size of the level's image (at most 8 192 cells: in LDS) | every
 *                  add in HBM | in LDS wherever the image fits.  emba_get_option "contrast_vote_path", read-only: the vote kernel of the last contrast call,
 *                  0 HBM | 1 LDS | -1 none yet
 *   poisson        0 folded Fourier form | 1 dense sine transforms | 2 no folding;  gemm64 1 forces the 64-wide GEMM tiles */
emba_status emba_set_option(emba_ctx* ctx, const char* name, int32_t value);
emba_status emba_get_option(emba_ctx* ctx, const char* name, int32_t* value);

/* Inlier count of the last evaluation and active-pixel count of the last emba_form_active, once resolved
 * (after any synchronizing call, e.g. emba_form_finish or emba_sync). */
emba_status emba_last_counts(emba_ctx* ctx, size_t* n_inliers, size_t* P);

/* Stream / event helpers so a host without HIP bindings can time the phases on the stream the
 * kernels run on (bench.py's roofline leg). */
emba_status emba_sync(emba_ctx* ctx);
emba_status emba_timer_start(emba_ctx* ctx, int32_t slot);   /* records a hipEvent on the stream */
emba_status emba_timer_stop(emba_ctx* ctx, int32_t slot);
emba_status emba_timer_elapsed_ms(emba_ctx* ctx, int32_t slot, float* ms); /* synchronizes on stop */
/* Device-measured duration (ms, HIP events around the launch) of the dominant kernel
 * (warp+residual+record kernel, "emba_warp_residual_kernel") in the most recent emba_eval_launch,
 * valid after a sync when kernel timing was enabled with emba_enable_kernel_timing(ctx, 1). */
emba_status emba_enable_kernel_timing(emba_ctx* ctx, int32_t on);      /* on = 0: off; 1 + slot (slot < 16): the events of the next step go to that slot */
emba_status emba_last_kernel_ms(emba_ctx* ctx, float* warp_ms, float* accum_ms);
/* ... read LATER, after the timed loop: sampled steps then cost their event records only, not a host wait each (bench.py) */
emba_status emba_kernel_ms_slot(emba_ctx* ctx, int32_t slot, float* warp_ms, float* accum_ms);
/* All launches of a sampled step (VERDICT r4 #1a).  emba_kernel_timing_all(ctx, 1): sampled steps also record an event in front of their first
 * launch, so that four consecutive intervals tile the step's device time; emba_kernel_ms_all returns them for a slot:
 * ms4[0] prep || pose || texel, [1] the warp kernel, [2] post-warp launch A (+ the sweeping active write where it is a launch of its own),
 * [3] the Gram kernel (with the active-set gather where it rides inside); -1 where a sampled step did not record them. */
emba_status emba_kernel_timing_all(emba_ctx* ctx, int32_t on);
emba_status emba_kernel_ms_all(emba_ctx* ctx, int32_t slot, float* ms4);
/* What an event bracket costs by itself: the mean HIP-event interval around an EMPTY kernel queued behind running work (reps brackets). */
emba_status emba_bracket_overhead_us(emba_ctx* ctx, int32_t reps, float* us);
/* The clocks this run had: the device attributes (kHz), and a probe kernel — one wave per SIMD running a dependent chain of fp32 adds
 * between two reads each of the constant-rate clock (s_memrealtime) and the shader-cycle counter (s_memtime): *probe_us its duration,
 * *sclk_mhz = shader cycles / duration, *cycles_per_add the chain's cadence (8 on gfx950: a sanity check of the counter).  Any pointer may be NULL. */
emba_status emba_clock_probe(emba_ctx* ctx, double* sclk_mhz, double* probe_us, double* cycles_per_add, int32_t* clock_rate_khz,
                             int32_t* mem_clock_rate_khz, int32_t* wall_clock_rate_khz);
/* "0000:xx:00.0" of the context's device (hipDeviceGetPCIBusId): /sys/bus/pci/devices/<id>/ holds the card's own clock and power report. */
emba_status emba_device_pci_bus_id(emba_ctx* ctx, char* buf, size_t len);

/* ---- Several GPUs behind ONE host thread ------------------------------------------------------------------------
 * The reference front-end is one process that owns one LEGM (src/emba/emba.cpp:378; solver.cpp:63-353 calls it).  An emba_group is
 * that object for a multi-GPU node: n_ranks contexts on devices[0..n_ranks), events sharded by time on the global batch grid with
 * a per-pixel halo, the two exchanges of an iteration as grouped RCCL all-reduces on the contexts' own streams (ncclCommInitAll,
 * librccl bound at run time).  All ranks on ONE device (devices = {0, 0}: what a single-GPU box can test) or n_ranks = 1 exchange
 * through in-library copies and add kernels instead — same protocol, no RCCL.  Same call order as the single-GPU entry points:
 *   emba_group_set_events -> emba_group_upload_map -> { emba_group_step -> [emba_group_download] -> emba_group_solve ->
 *   emba_group_update_map -> emba_group_step ... -> emba_group_map_accept / _reject }.  emba_group_ctx gives a rank's context for
 * anything else (diagnostics, dumps).  emba_group_eval + emba_group_form are the two halves of emba_group_step with the reference's
 * call shape (solver.cpp:75,251 evaluateDataError; :114-130 formNormalEq[IRLS] + applyL2Reg), so the EMBA::LEGM adapter
 * (emba_amd/host/legm_adapter.hpp) sits on a group of any size — one rank included — without a change to solver.cpp.
 * With more than one rank every rank's launches are issued from a host thread of its own (EMBA_GROUP_NO_THREADS: from the caller's). */
typedef struct emba_group emba_group;
emba_status emba_group_create(const emba_cfg* cfg, const int32_t* devices, int32_t n_ranks, emba_group** out);   /* cfg->device, cfg->stream are ignored */
/* ... with flags: EMBA_GROUP_FORCE_RCCL — a ONE-rank group goes through RCCL too (what a one-GPU box can rehearse of that path: run-time binding of
 * librccl, communicator set-up, every collective call, world size 1); EMBA_GROUP_NO_THREADS — the caller's thread drives every rank itself. */
#define EMBA_GROUP_FORCE_RCCL 1u
#define EMBA_GROUP_NO_THREADS 2u
emba_status emba_group_create_flags(const emba_cfg* cfg, const int32_t* devices, int32_t n_ranks, uint32_t flags, emba_group** out);
/* emba_set_option on every rank's context, plus the group's own: x2_split — -1 auto (from 3 M events per rank) | 0 exchange 2 in one piece | 1 its
 * A22 | b2 rows on the side streams under the Gram kernel; group_step_fast — 1 the ranks form as resident steps where they can (emba_step_form_active) |
 * 0 the sweeping forms. */
emba_status emba_group_set_option(emba_group* g, const char* name, int32_t value);
void        emba_group_destroy(emba_group* g);
const char* emba_group_last_error(const emba_group* g);
int32_t     emba_group_size(const emba_group* g);
int32_t     emba_group_uses_rccl(const emba_group* g);
emba_ctx*   emba_group_ctx(emba_group* g, int32_t rank);
emba_status emba_group_set_events(emba_group* g, const uint16_t* x, const uint16_t* y, const uint8_t* pol, const int64_t* t_ns, size_t n);
emba_status emba_group_upload_map(emba_group* g, const double* Gx, const double* Gy);
/* The sliding-window run of emba.cpp:400-532 on a group: emba_seq_upload on EVERY rank's context — each holds its own copy of the sequence, also
 * where ranks share a device; *n_kept = n / rate.  emba_group_seq_size / _seq_free: emba_seq_size of rank 0 / emba_seq_free on every rank. */
emba_status emba_group_seq_upload(emba_group* g, const uint16_t* x, const uint16_t* y, const uint8_t* pol, const int64_t* t_ns, size_t n,
                                  int32_t sampling_rate, size_t* n_kept);
emba_status emba_group_seq_size(const emba_group* g, size_t* n);
emba_status emba_group_seq_free(emba_group* g);
/* EMBA::getEventSubset (emba.cpp:473-510): emba_seq_window on rank 0 (the search is deterministic and the copies are equal: every rank's answer). */
emba_status emba_group_seq_window(emba_group* g, int64_t t_beg_ns, int64_t t_end_ns, size_t* beg, size_t* end);
/* emba_seq_filter on EVERY rank's copy of the sequence (equal copies, a deterministic rule: equal results); stats are rank 0's.  Rank r's hot pixels:
 * emba_seq_hot_pixels(emba_group_ctx(g, r), .). */
emba_status emba_group_seq_filter(emba_group* g, double hot_sigma, int64_t refractory_ns, int64_t support_ns, int32_t sampling_rate, uint64_t* stats);
/* emba_group_set_events for the window [beg, end) of the resident sequence (emba.cpp:508-509 -> solveTimeWindow): with nb = (end - beg) / 100, rank r
 * registers the window's batches [nb r / N, nb (r + 1) / N) (the remainder on the first ranks; the last rank's range runs to `end` and so carries the
 * (end - beg) % 100 tail the library ignores) through emba_set_events_seq_shard — its halo is built on its own device, no event crosses the host. */
emba_status emba_group_set_events_seq(emba_group* g, size_t beg, size_t end);
/* The median blur of the initial map (emba.cpp:357-364): emba_median_blur3_map on every rank's replica. */
emba_status emba_group_median_blur3_map(emba_group* g);
/* evaluateDataError + formNormalEq[IRLS] + applyL2Reg over all ranks; n_inliers = total over the ranks, P = active pixels */
emba_status emba_group_step(emba_group* g, const double* knots_xyzw, int32_t K, int64_t t0_ns, int64_t dt_ns, int32_t thres_valid_pixel,
                            int32_t irls, double eta, double alpha, size_t* n_inliers, size_t* P);
/* LEGM::evaluateDataError over all ranks.  Gx / Gy: host planes to upload first, or both NULL for the resident (current or trial) map.
 * Outputs (any may be NULL): ep_out (capacity >= events used) = the residuals of all ranks merged into the reference's order, *n_inliers
 * their number, num_ev_map_out the GLOBAL count map (exact int32 exchange; without it exchange 1 is left to emba_group_form, which may
 * send saturated bytes). */
emba_status emba_group_eval(emba_group* g, const double* knots_xyzw, int32_t K, int64_t t0_ns, int64_t dt_ns, const double* Gx, const double* Gy,
                            double* ep_out, size_t* n_inliers, int32_t* num_ev_map_out);
/* The residual vector of the last emba_group_eval (ep_out NULL there, n_inliers asked for) in the reference's order, into memory the caller owns: lets a host
 * that returns it by value (VecXd LEGM::evaluateDataError) size its vector from the count and receive the residuals in it directly.  Host copies of this size go
 * through two pinned 8-MB buffers in pipelined chunks (also for emba_eval_finish / emba_get_ep).  The first such download above 1 MB (these, emba_form_finish,
 * the images) starts a few helper threads that live as long as the process and registers a pthread_atfork handler (a forked child starts from a fresh pool);
 * from 4 MB up a download also calls madvise(MADV_POPULATE_WRITE) on the caller's destination memory: embedders that fork or filter system calls should
 * expect all three. */
emba_status emba_group_get_ep(emba_group* g, double* ep_out, size_t cap, size_t* n_inliers);
/* LEGM::formNormalEq[IRLS] + applyL2Reg over all ranks on the state of the last emba_group_eval (device-resident residuals). */
emba_status emba_group_form(emba_group* g, int32_t thres_valid_pixel, int32_t irls, double eta, double alpha, size_t* n_inliers, size_t* P);
/* LEGM::applyL2Reg as a call of its own (after emba_group_form with alpha = 0): once per set of equations, on every rank's replica. */
emba_status emba_group_apply_l2(emba_group* g, double alpha);
/* emba_set_cost on every rank: the robust cost of the emba_group_form calls to come (speed only; emba_group_step declares its own). */
emba_status emba_group_set_cost(emba_group* g, int32_t irls, double eta);
emba_status emba_group_download(emba_group* g, double* A11, double* b1, uint32_t* active_idx, size_t cap_P, double* A22, double* b2);
emba_status emba_group_costs(emba_group* g, int32_t irls, double eta, double alpha, double* data_cost, double* reg_cost);
emba_status emba_group_solve(emba_group* g, double lambda, int32_t fix_first_pose, double* x1_host, double* x2_host);
/* LEGM::solveNormalEqCG over the group (round 6: any number of ranks — the pixels are sharded as in the Schur solve, one all-reduce of 3K + 2 doubles per
 * application of the matrix and one of 2 doubles per iteration; emba_cg_shard_* below are the per-rank steps). */
emba_status emba_group_solve_cg(emba_group* g, double lambda, int32_t fix_first_pose, int32_t max_iter, double tol, double* x1_host, double* x2_host,
                                int32_t* iterations, double* error);
/* emba_solve_map_only / emba_solve_poses_only over the group.  After emba_group_form every rank's pack is a replica, so each rank runs the call on its own
 * context: no record exchange, no collective, and the results are identical on every rank (x2_host / x1_host are rank 0's).  emba_group_update_map(g, NULL, ...)
 * follows emba_group_solve_map_only as it follows emba_group_solve; emba_group_last_solve_exchanged reports 0 after either. */
emba_status emba_group_solve_map_only(emba_group* g, double lambda, double* x2_host);
emba_status emba_group_solve_poses_only(emba_group* g, double lambda, int32_t fix_first_pose, double* x1_host);
/* Did the last emba_group_solve / _solve_cg run the record exchange (1), or did every rank still hold the records it had received for these equations (0)? */
emba_status emba_group_last_solve_exchanged(const emba_group* g, int32_t* exchanged);
/* x2_host == NULL: every rank applies the (all-reduced) x2 the last emba_group_solve / _solve_cg left in its own device memory. */
emba_status emba_group_update_map(emba_group* g, const double* x2_host, double damping);
emba_status emba_group_map_accept(emba_group* g);
emba_status emba_group_map_reject(emba_group* g);
emba_status emba_group_download_map(emba_group* g, double* Gx_host, double* Gy_host);
emba_status emba_group_get_map_active(emba_group* g, double* gxy_host, size_t cap_P);   /* emba_get_map_active on rank 0's replica */
emba_status emba_group_trial_reject(emba_group* g);   /* emba_trial_reject on every rank (emba_group_map_reject includes it) */

#ifdef __cplusplus
}
#endif
#endif /* EMBA_HIP_H */
