#!/usr/bin/env python3
"""Event-based mosaicing bundle adjustment of one time window — or, with --window-size, of a whole recording in sliding windows — on an MI355X, without ROS: the job of the reference's
`roslaunch emba <seq>.launch` back-end (src/emba/emba.cpp:29-330 + solver.cpp:11-368) for data already on disk.

  python examples/run_ba.py --demo out/                       # simulate a scene, perturb the trajectory, refine, write results
  python examples/run_ba.py --demo out/ --window-size 0.3 --window-stride 0.1   # the same in sliding time windows (EMBA::Run, emba.cpp:400-532)
  python examples/run_ba.py --events ev.npz --poses init_traj.txt --map-dir init_map/ --calib calib.npz --out out/
  python examples/run_ba.py --demo out/ --init-map events     # no front-end map: start from a zero map, solved for the map alone first
  python examples/run_ba.py --demo out/ --init-poses events --init-map events --window-size 0.3 --window-stride 0.1   # no front end at all: the raw poses
                                                  # come from the events by contrast maximisation on the device; --events E --calib C likewise
  python examples/run_ba.py --demo out/ --init-poses identity --init-map events --refine-contrast --contrast-levels 3,2,1,0 --window-size 0.3 --window-stride 0.1
                                                                                             # identity raw poses, the ascent coarse to fine
  python examples/run_ba.py --demo out/ --init-poses events --init-map events --refine-contrast --window-size 0.3 --window-stride 0.1   # ... and each window's
                                                  # initial control poses moved uphill on the contrast of its warped events first
  python examples/run_ba.py --demo out/ --init-poses events --init-map events --refine-contrast --contrast-prior --window-size 0.3 --window-stride 0.1
                                                  # ... against the panorama the earlier windows' events already placed
  python examples/run_ba.py --demo out/ --refine poses        # move the poses only, against the map as given (or --refine map: the map only)
  python examples/run_ba.py out/ --simulate plane.npy --poses traj.txt --calib calib.npz --sim-hz 2000 --events-out ev.npz   # panorama to events: a recording
                                                  # of the log-intensity plane along the trajectory, simulated on the device; with --demo the BA then runs on it
  python examples/run_ba.py --demo out2/ --frames out1/views --init-map frames --frames-log 0 --frames-skip-zero --frames-lo LO --frames-hi HI
                                                  # frames to panorama: the initial map is the mosaic of intensity frames along the raw trajectory (DESIGN.md
                                                  # section 19); here the frames another run wrote with --views-hz, whose tone LO HI is in out1/views/tone.txt
  python examples/run_ba.py --demo out4/ --frames out1/views --init-poses frames --init-map frames --track-levels 3,2,1 --window-size 0.5 --frames-log 0 --frames-skip-zero --frames-lo LO --frames-hi HI   # poses from the frames alone
  python -m torch.distributed.run --nproc-per-node 8 --master-addr 127.0.0.1 examples/run_ba.py ... # the window's events time-sharded
                                                  # over the GPUs of one node (RCCL); every rank runs the same LM loop, rank 0 writes
  python -m torch.distributed.run --nproc-per-node 8 --master-addr 127.0.0.1 examples/run_ba.py ... --window-size 0.3 --window-stride 0.1
                                                  # sliding windows over time shards: every rank keeps the whole sequence on its GPU and registers
                                                  # its shard of each window from it (halo built on the device); no event crosses the host per window

Inputs: events (.npz: x, y u16; polarity u8; t_ns i64), initial poses ("t tx ty tz qx qy qz qw" per line), initial map
(Gx.bin / Gy.bin raw float64, H x 2H), calibration (.npz: K [3,3], D [<=5] plumb_bob, width, height).
Outputs: <out>/refined_traj.txt, <out>/Gx.bin, <out>/Gy.bin (the files emba.cpp:300-330 writes), <out>/map_poisson_opt.pgm; with --record-data
also the reference's record_data map images (solver.cpp:173-179, 332-336, 360-364): <out>/{Gx_evo,Gy_evo,G_hsv_evo,map_poisson_evo,map_opt}/*.png; with
--views-hz (and --window-size) <out>/views/frame_%06d.pgm and times.txt, what the camera would have seen along the final trajectory, and with --view-events
<out>/views/event_frames.npy; with --frames <out>/frame_mosaic.pgm and <out>/frame_mosaic_covered.pgm, the frames stitched along
the final trajectory."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from emba_amd import LEGM, io as eio, so3, synth                      # noqa: E402
from emba_amd.legm import LinearTrajectory                            # noqa: E402
from emba_amd.solver import BASettings, LMSettings, MapRecorder, RuntimeLog, solve_time_window  # noqa: E402


def load_plane(path):
    """A log-intensity plane: a .npy of doubles, or a binary .pgm read as log(1 + v)."""
    if path.endswith(".npy"):
        return np.ascontiguousarray(np.load(path), dtype=np.float64)
    return np.log1p(eio.load_pgm(path).astype(np.float64))


def load_frames(frames_dir, sw, sh):
    """--frames DIR: times.txt ('index seconds.nanoseconds' per line) and frame_%06d.pgm of sensor size, as --views-hz writes them.  Returns (frames
    uint8 [F, sh, sw], t_ns int64 [F])."""
    idx, t_ns = [], []
    with open(os.path.join(frames_dir, "times.txt")) as fh:
        for line in fh:
            if not line.strip():
                continue
            i, stamp = line.split()
            sec, _, frac = stamp.partition(".")
            idx.append(int(i)); t_ns.append(int(sec) * 1_000_000_000 + int((frac + "000000000")[:9]))
    frames = np.zeros((len(idx), sh, sw), np.uint8)
    for k, i in enumerate(idx):
        img = eio.load_pgm(os.path.join(frames_dir, "frame_%06d.pgm" % i))
        if img.shape != (sh, sw) or img.dtype != np.uint8:
            raise ValueError(f"{frames_dir}/frame_{i:06d}.pgm: {img.shape[1]}x{img.shape[0]} {img.dtype}, the sensor is {sw}x{sh} in bytes")
        frames[k] = img
    return frames, np.array(t_ns, dtype=np.int64)


def frame_mosaic(legm, frames, t_ns, traj, skip_zero, exposure=None):
    """The frames whose times the trajectory covers, voted into the context's mosaic on the device.  Returns how many those were.
    exposure: (gain, bias) per frame of --frames-exposure, and the frames vote their compensated bytes."""
    keep = (t_ns >= traj.t0_ns) & (t_ns < traj.t0_ns + traj.dt_ns * (traj.size() - 1))
    if not keep.any():
        raise SystemExit("--frames: no frame time lies inside the trajectory's knots")
    if exposure is None:
        legm.mosaic_frames(frames[keep], t_ns[keep], traj, skip_zero=skip_zero)
    else:
        legm.mosaic_frames_exposure(frames[keep], t_ns[keep], traj, exposure[0][keep], exposure[1][keep], skip_zero=skip_zero)
    return int(keep.sum())


def refine_frames(legm, frames, t_ns, traj, t_raw, q_raw, rounds, huber_k, skip_zero, log=print, estimate=None, exposure0=None):
    """--refine-frames N: poses from frames.  Per round: the frames are stitched along the current raw trajectory, every frame is
    aligned to that mosaic's mean under its covered cells on the device, and io.fit_ctrl_poses of the aligned rotations at the frame times, merged with the
    raw poses outside the frames' span, becomes the raw trajectory.  Returns (traj, t_raw, q_raw, rows): rows holds per frame the time, the aligned
    rotation, the status and the mean cost before and after, of the last round.
    estimate (--frames-exposure bias / gain-bias: io.EXPOSURE_BIAS, or EXPOSURE_GAIN | EXPOSURE_BIAS): every frame carries a gain
    and a bias in byte units, 1 and 0 at the start.  Per round the frames are stitched with them, aligned with them estimated beside the rotation, and
    the common tone of the frames that did not end degenerate is fixed by io.exposure_gauge, before the trajectory is refitted.  The rows then end in the
    gain and the bias, and a fifth value is returned: (gain, bias) for every frame of --frames, 1 and 0 for those the trajectory does not cover.
    exposure0: (gain, bias) per frame of --frames that the rounds start from instead of 1 and 0 (--track-exposure: the tracker's)."""
    keep = (t_ns >= traj.t0_ns) & (t_ns < traj.t0_ns + traj.dt_ns * (traj.size() - 1))
    if not keep.any():
        raise SystemExit("--frames: no frame time lies inside the trajectory's knots")
    fr, ts = frames[keep], t_ns[keep]
    t_beg, dt = traj.t0_ns * 1e-9, traj.dt_ns * 1e-9
    rows = []
    gain, bias = np.ones(len(ts)), np.zeros(len(ts))
    if exposure0 is not None and estimate is not None:
        gain, bias = np.array(exposure0[0][keep], dtype=np.float64), np.array(exposure0[1][keep], dtype=np.float64)
    for rnd in range(1, rounds + 1):
        q0 = np.array([traj.evaluate(int(tn)) for tn in ts])
        if estimate is None:
            legm.mosaic_frames(fr, ts, traj, skip_zero=skip_zero)
            r = legm.align_frames(fr, q0, use_mosaic=True, lo=0.0, hi=255.0, skip_zero=skip_zero, huber_k=huber_k)
            cost = r["sums"][:, 9]
        else:
            legm.mosaic_frames_exposure(fr, ts, traj, gain, bias, skip_zero=skip_zero)
            r = legm.align_frames_exposure(fr, q0, gain, bias, estimate, use_mosaic=True, lo=0.0, hi=255.0, skip_zero=skip_zero, huber_k=huber_k)
            cost = r["sums"][:, eio.EXPOSURE_COST]
            gain, bias = eio.exposure_gauge(r["gain"], r["bias"], r["status"] != eio.ALIGN_DEGENERATE)
            log(f"refine-frames round {rnd}: gain {gain.min():.4f} ... {gain.max():.4f} (std {gain.std():.4f}), bias {bias.min():.3f} ... {bias.max():.3f} bytes")
        before, after = r["cost0"] / np.maximum(r["n0"], 1), cost / np.maximum(r["counts"][:, 0], 1)
        tf = ts * 1e-9
        outside = (t_raw < tf[0]) | (t_raw > tf[-1])
        t_all, q_all = np.concatenate([t_raw[outside], tf]), np.concatenate([q_raw[outside], r["q"]])
        order = np.argsort(t_all, kind="stable")
        t_raw, q_raw = t_all[order], q_all[order]
        traj = LinearTrajectory(eio.fit_ctrl_poses(t_raw, q_raw, t_beg, dt, traj.size()), traj.t0_ns, traj.dt_ns)
        moved = eio.rotation_angle_between(q0, r["q"])
        names = ", ".join(f"{int((r['status'] == k).sum())} {v}" for k, v in eio.ALIGN_STATUS_NAMES.items())
        log(f"refine-frames round {rnd}: {len(ts)} frames aligned to their mosaic ({names}); mean cost {before.mean():.4g} -> {after.mean():.4g}, "
            f"mean turn {moved.mean():.3e} rad, up to {int(r['iters'].max())} trials")
        rows = [(tn, q, int(st), b, a_) for tn, q, st, b, a_ in zip(ts, r["q"], r["status"], before, after)]
    if estimate is None:
        return traj, t_raw, q_raw, rows
    g_all, b_all = np.ones(len(t_ns)), np.zeros(len(t_ns))
    g_all[keep], b_all[keep] = gain, bias
    return traj, t_raw, q_raw, [row + (g, o) for row, g, o in zip(rows, gain, bias)], (g_all, b_all)


def match_settings(a):
    """--close-search and the --close-match-* flags as members of driver.SequenceSettings: only what was given."""
    given = dict(close_search=a.close_search, close_match_level=a.close_match_level, close_match_range=a.close_match_range, close_match_score=a.close_match_score,
                 close_match_per_frame=a.close_match_per_frame)
    return {k: v for k, v in given.items() if v is not None}


def track_frames(legm, frames, t_ns, traj, t_beg, t_end, a, log=print, calib=None, pairs_path=None):
    """--init-poses frames: poses from the frames alone.  The frames are tracked against their own growing mosaic on the device; the
    tracked frames' (t, q), sampled on a 5 ms grid over the span and held at both ends where the frames do not reach them, are the raw poses, and
    io.fit_ctrl_poses of them the trajectory.
    Lost frames are left out.  Returns (traj, t_raw, q_raw, rows): rows holds per frame the time, the rotation, the status, the overlap and the cost.
    --track-exposure bias / gain-bias: every frame carries a gain and a bias in byte units, estimated with its rotation, and votes its
    compensated bytes; the rows then end in the gain and the bias.
    --track-refit N: N sweeps of the refit behind the tracker; the rows then end in the refit code.
    --track-close: before any refit, pairs of tracked frames that see the same place are aligned with each other and the rotation
    graph of the kept pairs is solved with the anchor held; pairs_path takes one line per pair."""
    kw = dict(q0=a.track_q0, levels=a.track_levels, batch=a.track_batch, predict=bool(a.track_predict), skip_zero=a.frames_skip_zero,
              min_overlap=a.track_min_overlap, huber_k=a.frames_huber)
    estimate = {"none": None, "bias": eio.EXPOSURE_BIAS, "gain-bias": eio.EXPOSURE_GAIN | eio.EXPOSURE_BIAS}[a.track_exposure]
    r = legm.track_frames(frames, t_ns, **kw) if estimate is None else legm.track_frames_exposure(frames, t_ns, estimate=estimate, **kw)
    if a.track_close:      # loops closed among the tracked frames, before any refit: the mosaic in the context is the closed one
        from emba_amd.driver import SequenceSettings, close_tracked_frames
        before = r["q"]
        r = close_tracked_frames(legm, frames, t_ns, r, SequenceSettings(1.0, 1.0, track_close=True, close_window=a.close_window, close_gap=a.close_gap,
                                                                         close_angle=a.close_angle, close_per_frame=a.close_per_frame, close_huber=a.close_huber,
                                                                         close_levels=a.close_levels or (0,), close_exposure=a.close_exposure or "none",
                                                                         **match_settings(a)),
                                 calib, estimate=estimate or 0, **kw)
        g = r["graph"]
        log(f"track-close: {len(r['pairs'])} pairs, {int(r['pair_kept'].sum())} kept; "
            + (f"search {a.close_search}: {np.bincount(r['pair_source'], minlength=3).tolist()} from the window, the rotations, the appearance; " if a.close_search else "")
            + (f"graph cost {g['cost0']:.6g} -> {g['cost']:.6g} in {g['iters']} steps ({g['cg_iters']} CG iterations, {eio.GRAPH_END_NAMES[g['end']]}); "
               f"worst change against the tracker {eio.rotation_angle_between(before, r['q']).max():.3g} rad" if g else "no graph: the tracker's rotations stay"))
        if pairs_path:
            with open(pairs_path, "w") as fh:
                levelled = a.close_levels is not None or a.close_exposure is not None      # (the columns gain, bias, last level only with one of the two flags)
                fh.write("# i j status(1 converged, 2 stalled, 3 iterations, 4 degenerate) n mean_cost moved[rad] kept" + (" gain bias last_level" if levelled else "")
                         + (" source(0 window, 1 rotations, 2 appearance) match_score dx dy" if a.close_search else "") + "\n")
                if levelled and "pair_gain" not in r:      # (a flag given at its default value: the pairs went through level 0 alone, their exposure as given)
                    _, pg, pb = eio.pair_start(before, r.get("gain"), r.get("bias"), r["pairs"])
                    r = dict(r, pair_gain=pg, pair_bias=pb, pair_last_level=np.zeros(len(r["pairs"]), np.int64))
                for p, ((i, j), st, n, c, mv, kp) in enumerate(zip(r["pairs"], r["pair_status"], r["pair_n"], r["pair_cost"], r["pair_moved"], r["pair_kept"])):
                    more = f" {r['pair_gain'][p]:.9g} {r['pair_bias'][p]:.9g} {int(r['pair_last_level'][p])}" if levelled else ""
                    if a.close_search:      # (the columns source, match score, dx, dy only with --close-search)
                        more += f" {int(r['pair_source'][p])} {r['pair_match_score'][p]:.9g} {int(r['pair_match_shift'][p][0])} {int(r['pair_match_shift'][p][1])}"
                    fh.write(f"{i} {j} {int(st)} {int(n)} {c:.9g} {mv:.9g} {int(kp)}{more}\n")
    if a.track_refit:      # the sweeps behind the tracker, before the raw poses are sampled: the mosaic in the context is the refitted one
        from emba_amd.driver import SequenceSettings, refit_tracked_frames
        before = r["q"]
        r = refit_tracked_frames(legm, frames, t_ns, r, SequenceSettings(1.0, 1.0, track_refit=a.track_refit, track_refit_tol=a.track_refit_tol),
                                 estimate=estimate or 0, **kw)
        codes = [int((r["refit"] == c).sum()) for c in (eio.REFIT_MOVED, eio.REFIT_KEPT, eio.REFIT_RECOVERED, eio.REFIT_LOST)]
        log(f"track-refit: {r['sweeps_done']} of {a.track_refit} sweeps, largest rotation change per sweep {', '.join(f'{v:.3g}' for v in r['sweep'][:, 2])} rad; "
            f"{codes[0]} frames moved, {codes[1]} kept, {codes[2]} recovered, {codes[3]} lost; worst change against the tracker "
            f"{eio.rotation_angle_between(before, r['q']).max():.3g} rad")
    ok = r["status"] != eio.TRACK_LOST
    tf, qf = t_ns[ok] * 1e-9, r["q"][ok]
    # the raw poses a sliding-window run reads: the tracked rotations on a 5 ms grid over the trajectory's span (io.pose_at: interpolated between tracked
    # frames, held before the first and behind the last), so that there are more raw poses than control poses however few frames there are
    t_raw_ns = traj.t0_ns + 5_000_000 * np.arange((traj.dt_ns * (traj.size() - 1)) // 5_000_000, dtype=np.int64)
    t_raw = t_raw_ns * 1e-9
    q_raw = np.array([eio.pose_at(tf, qf, tq) for tq in t_raw])
    traj = LinearTrajectory(eio.fit_ctrl_poses(t_raw, q_raw, traj.t0_ns * 1e-9, traj.dt_ns * 1e-9, traj.size()), traj.t0_ns, traj.dt_ns)
    log(f"init-poses frames: {r['tracked']} of {len(t_ns)} frames tracked through levels {a.track_levels} (batch {a.track_batch}), {r['lost']} lost; "
        f"overlap >= {r['overlap'][1:].min() if len(t_ns) > 1 else 0.0:.3f}, up to {int(r['iters'].max()) if r['iters'].size else 0} trials per level, "
        f"{r['dropped']} votes dropped, {r['skipped']} pixels skipped")
    rows = [(int(tn), q, int(st), float(ov), float(c)) for tn, q, st, ov, c in zip(t_ns, r["q"], r["status"], r["overlap"], r["cost"])]
    if estimate is not None:
        log(f"track-exposure {a.track_exposure}: gain {r['gain'].min():.4f} ... {r['gain'].max():.4f}, bias {r['bias'].min():.3f} ... {r['bias'].max():.3f} bytes "
            f"(the anchor's tone is the gauge: gain 1, bias 0)")
        rows = [row + (float(g), float(o)) for row, g, o in zip(rows, r["gain"], r["bias"])]
    if a.track_refit:      # (the last column, behind gain and bias where they are there)
        rows = [row + (int(c),) for row, c in zip(rows, r["refit"])]
    return traj, t_raw, q_raw, rows


def simulate(a, ap):
    """--simulate: a recording from a log-intensity plane and a trajectory, on the device; with --demo, then the BA on it."""
    if not (np.isfinite(a.sim_hz) and a.sim_hz > 0):
        ap.error("--simulate needs --sim-hz, the steps per second (finite, positive)")
    if not a.events_out:
        ap.error("--simulate needs --events-out FILE")
    plane = load_plane(a.simulate)
    H, W = plane.shape
    if a.demo:      # the demo's camera and, without --poses, its trajectory
        sw, sh, dt_knots = 128, 96, 0.05
        lut = synth.pinhole_bearing_lut(sw, sh, 120.0, 120.0, 0.5 * (sw - 1), 0.5 * (sh - 1))
        truth = synth.make_trajectory(11, dt_knots=dt_knots) if not a.poses else None
    else:
        if not a.poses or not a.calib:
            ap.error("--simulate needs --poses and --calib (or --demo)")
        cal = np.load(a.calib)
        sw, sh, dt_knots, truth = int(cal["width"]), int(cal["height"]), a.dt_knots, None
        lut = eio.bearing_lut_from_calibration(cal["K"], cal["D"], sw, sh)
    if truth is None:
        t, qs = eio.load_poses(a.poses)
        t_beg = a.t_beg if a.t_beg is not None else t[0]
        t_end = a.t_end if a.t_end is not None else t[-1]
        num_cps = int(round((t_end - t_beg) / dt_knots)) + 1
        sel = (t >= t_beg) & (t <= t_end)
        truth = LinearTrajectory.from_seconds(t_beg, dt_knots, eio.fit_ctrl_poses(t[sel], qs[sel], t_beg, dt_knots, num_cps))
    # step times t0, t0 + p, ... up to t0 + (K - 1) dt - 1: the rule of --views-hz
    period = max(int(round(1e9 / a.sim_hz)), 1)
    ts = np.arange(truth.t0_ns, truth.t0_ns + truth.dt_ns * (truth.size() - 1), period, dtype=np.int64)
    if ts.size < 2:
        ap.error("--sim-hz gives fewer than two step times on this trajectory")
    c_on = a.sim_c_on if a.sim_c_on is not None else a.C_th
    c_off = a.sim_c_off if a.sim_c_off is not None else c_on
    legm = LEGM(sw, sh, lut, c_on, W, H)
    t0 = time.time()
    stats = legm.simulate_events(ts, truth.knots_xyzw, truth.t0_ns, truth.dt_ns, plane=plane, c_on=c_on, c_off=c_off)
    dt = time.time() - t0
    ev = legm.simulated_events()
    eio.save_events(a.events_out, ev)
    print(f"simulated {int(stats[0])} events ({int(stats[1])} positive) on {sw}x{sh} from a {H}x{W} plane over {ts.size - 1} steps at {a.sim_hz:g} Hz in {dt * 1e3:.1f} ms: "
          f"{int(stats[2])} (pixel, step) pairs capped, {int(stats[3])} (pixel, frame) pairs outside; written to {a.events_out}")
    if not a.demo:
        return
    # the BA on the simulated recording: device to device into the resident sequence; from a zero map (map only first) and a perturbed trajectory
    n = legm.sequence_from_simulation(a.sampling_rate)
    from emba_amd.legm import EventWindow
    import dataclasses
    rng = np.random.default_rng(5)
    knots = truth.knots_xyzw.copy()
    for i in range(1, len(knots)):
        knots[i] = so3.mul(so3.exp(rng.normal(size=3) * 0.01), knots[i])
    traj = LinearTrajectory(knots, truth.t0_ns, truth.dt_ns)
    ba = BASettings(use_IRLS=a.cost != "quadratic", cost_type=a.cost, eta=a.eta, thres_valid_pixel=a.thres_valid_pixel, alpha=a.alpha,
                    damping_factor=a.damping_factor, refine=a.refine, panorama_boundary=a.panorama_boundary)
    zero = np.zeros((H, W))
    mres = solve_time_window(legm, traj, EventWindow(0, n), zero, zero, dataclasses.replace(ba, refine="map"), LMSettings(max_num_iter=a.max_iter), verbose=a.verbose, resident=True)
    print(f"{n} simulated events resident; map-only start from a zero map: {mres.iterations} LM iterations ({mres.reason}), cost {mres.cost_min:.6e}")
    res = solve_time_window(legm, traj, EventWindow(0, n), None, None, ba, LMSettings(max_num_iter=a.max_iter), verbose=a.verbose, resident=True)
    err = lambda tr: np.degrees(np.mean([np.linalg.norm(so3.log(so3.mul(so3.inverse(p), q))) for p, q in zip(tr.knots_xyzw, truth.knots_xyzw)]))
    print(f"{res.iterations} LM iterations ({'converged' if res.converged else 'stopped'}), cost {res.cost_min:.6e}; "
          f"mean control-pose error vs the simulated trajectory: {err(traj):.4f} deg -> {err(res.traj):.4f} deg")
    eio.write_trajectory(os.path.join(a.out, "refined_traj.txt"), res.traj)
    eio.save_map(a.out, *legm.downloadMap())
    eio.save_pgm(os.path.join(a.out, "map_poisson_opt.pgm"), eio.normalize_robust(legm.reconstructIntensity(boundary=a.panorama_boundary), 0.1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("--demo", action="store_true")
    ap.add_argument("--events"); ap.add_argument("--poses"); ap.add_argument("--map-dir"); ap.add_argument("--calib")
    ap.add_argument("--dt-knots", type=float, default=0.05)
    ap.add_argument("--t-beg", type=float); ap.add_argument("--t-end", type=float)
    ap.add_argument("--C-th", type=float, default=0.2)
    ap.add_argument("--alpha", type=float, help="map L2 weight (default 5.0; 0 in --demo, where the initial map is already the true one)")
    ap.add_argument("--thres-valid-pixel", type=int, default=5)
    ap.add_argument("--damping-factor", type=float, default=1.0)
    ap.add_argument("--cost", default="quadratic", choices=["quadratic", "huber", "cauchy"])
    ap.add_argument("--eta", type=float, default=0.1)
    ap.add_argument("--max-iter", type=int, default=50)
    ap.add_argument("--verbose", action="store_true")
    ap.add_argument("--runtime-log", action="store_true", help="write the reference's run-time records under <out>/final_results (every timed phase then ends in a host synchronisation)")
    ap.add_argument("--record-data", action="store_true", help="write the reference's record_data map images (PNG, rendered on the device) under <out>/ "
                    "at every LM iteration and at the end (rank 0)")
    ap.add_argument("--window-size", type=float, help="time_window_size in seconds: refine the recording in sliding windows (EMBA::Run, emba.cpp:400-532); "
                    "the event sequence then stays on the device and the map is carried from window to window")
    ap.add_argument("--window-stride", type=float, help="sliding_window_stride in seconds (default: the window size)")
    ap.add_argument("--sampling-rate", type=int, default=1, help="event_sampling_rate: keep every n-th event (emba.cpp:281-304; with --window-size)")
    ap.add_argument("--hot-pixel-sigma", type=float, default=0.0, help="drop every event of a pixel whose event count exceeds mean + SIGMA * std over the pixels "
                    "that fired (0: off; with --window-size; the filters run on the device before the down-sampling)")
    ap.add_argument("--refractory", type=float, default=0.0, help="seconds: drop an event closer than this behind the previous event of its pixel (0: off)")
    ap.add_argument("--support-time", type=float, default=0.0, help="seconds: keep an event only if one of its eight neighbouring pixels fired at most this long "
                    "before it (0: off)")
    ap.add_argument("--median-blur", action="store_true", help="3x3 median blur of the initial map (emba.cpp:357-364; with --window-size)")
    ap.add_argument("--init-map", default="given", choices=["given", "events", "frames"], help="events: no --map-dir is needed — the run starts from a zero map, which is first "
                    "solved for alone at the initial poses (mapping with known poses), then refined jointly; --pano-h gives its size.  frames: no --map-dir is "
                    "needed — the intensity frames of --frames are stitched into the panorama along the raw trajectory on the device, and the backward "
                    "differences of that mosaic's log intensity are the initial map (DESIGN.md section 19)")
    ap.add_argument("--frames", metavar="DIR", help="intensity frames beside the events: DIR/frame_%%06d.pgm at sensor size and DIR/times.txt, exactly what --views-hz "
                    "writes.  With it <out>/frame_mosaic.pgm and <out>/frame_mosaic_covered.pgm are written: the frames stitched along the final trajectory")
    ap.add_argument("--frames-lo", type=float, default=0.0, help="the intensity a byte of 0 stands for (the tone the frames were written with)")
    ap.add_argument("--frames-hi", type=float, default=1.0, help="the intensity a byte of 255 stands for")
    ap.add_argument("--frames-eps", type=float, default=1.0 / 255.0, help="L = log(I + eps)")
    ap.add_argument("--frames-log", type=int, default=1, choices=[0, 1], help="0: the bytes are log intensity already (the frames of --views-hz): no logarithm is taken")
    ap.add_argument("--frames-skip-zero", action="store_true", help="a byte of 0 is no measurement (--views-hz writes 0 where a pixel looks past the panorama)")
    ap.add_argument("--refine-frames", type=int, default=0, metavar="N", help="with --frames and given poses: N rounds before the BA, each stitching the frames along "
                    "the current raw trajectory, aligning every frame's rotation to that mosaic on the device and fitting the raw trajectory to the aligned "
                    "rotations (DESIGN.md section 20); writes <out>/frames_aligned.txt")
    ap.add_argument("--frames-exposure", choices=("none", "bias", "gain-bias"), default="none", help="with --refine-frames: a bias, or a gain and a bias, per frame "
                    "(compensated byte = gain * byte + bias), estimated with the frame's rotation in every round and applied when the frames are stitched, the "
                    "mosaic of --init-map frames and frame_mosaic.pgm included (DESIGN.md section 22); frames_aligned.txt gains the two columns")
    ap.add_argument("--frames-huber", type=float, default=0.0, metavar="K", help="with --refine-frames: the Huber threshold of the alignment, in byte units (0: quadratic)")
    ap.add_argument("--init-poses", default="given", choices=["given", "events", "identity", "frames"], help="frames: no --poses is needed — the intensity frames of "
                    "--frames are tracked against their own growing mosaic on the device from --track-q0 on, and the tracked frames' rotations are the raw poses "
                    "(with --window-size; DESIGN.md section 21; writes <out>/frames_tracked.txt).  identity: no --poses is needed — every raw pose is the identity "
                    "(what a run without a front end always has; with --window-size).  events: no --poses is needed — the angular velocity of every slice of events is "
                    "estimated from the events alone by contrast maximisation and integrated (with --window-size; --t-beg / --t-end default to the recording's span)")
    ap.add_argument("--track-levels", default="2,1,0", help="--init-poses frames: the schedule of levels, coarse to fine, comma-separated (level l has cells 2^l pixels wide).  A level whose cells are finer than the sensor's pixels stays under-covered and loses every frame: the demo's 128 x 96 sensor on 512 x 1024 needs 3,2,1")
    ap.add_argument("--track-batch", type=int, default=1, metavar="B", help="--init-poses frames: frames aligned at once against the mosaic of the frames before them")
    ap.add_argument("--track-predict", type=int, default=1, choices=[0, 1], help="--init-poses frames: start a frame from the last two tracked frames' angular velocity")
    ap.add_argument("--track-min-overlap", type=float, default=0.3, metavar="X", help="--init-poses frames: a frame whose used pixels fall below this share is lost")
    ap.add_argument("--track-q0", default="0,0,0,1", metavar="x,y,z,w", help="--init-poses frames: the rotation of the first frame")
    ap.add_argument("--track-exposure", choices=("none", "bias", "gain-bias"), default="none", help="--init-poses frames: a bias, or a gain and a bias, per frame "
                    "estimated with its rotation inside the tracker, for frames of a camera with auto-exposure; the tracked frames vote their compensated bytes, "
                    "--init-map frames and frame_mosaic.pgm use them, and --refine-frames N --frames-exposure X starts from them (DESIGN.md section 24; "
                    "frames_tracked.txt gains the columns gain and bias)")
    ap.add_argument("--track-refit", type=int, default=0, metavar="N", help="--init-poses frames: behind the tracker (either one), N sweeps in which every frame is taken "
                    "out of the integer mosaic, aligned to the mosaic of all the other frames and voted back, before the raw poses are sampled; lost frames are "
                    "tried again; --init-map frames takes the refitted mosaic (DESIGN.md section 25; frames_tracked.txt gains the refit code as its last column: "
                    "1 anchor, 2 moved, 3 kept, 4 recovered, 5 lost).  0: off")
    ap.add_argument("--track-close", action="store_true", help="--init-poses frames: behind the tracker and before --track-refit, close loops among the tracked "
                    "frames: pairs of frames that see the same place are aligned with each other on the device and a rotation graph over all frames is solved "
                    "with the anchor held exactly; --init-map frames takes the mosaic stitched again at the new rotations (DESIGN.md section 26; writes "
                    "<out>/frames_pairs.txt: i j, the pair's code, n, the mean cost, the angle moved, kept)")
    ap.add_argument("--close-window", type=int, default=1, metavar="N", help="with --track-close: every pair of voting frames at most N frames apart is tried")
    ap.add_argument("--close-gap", type=int, default=4, metavar="N", help="... and, more than N frames apart, per frame the --close-per-frame nearest by rotation")
    ap.add_argument("--close-angle", type=float, default=0.2, metavar="RAD", help="... whose tracked rotations differ by at most RAD")
    ap.add_argument("--close-per-frame", type=int, default=2, metavar="N")
    ap.add_argument("--close-huber", type=float, default=0.0, metavar="K", help="the Huber threshold of a pair's residuals in bytes (0: quadratic)")
    ap.add_argument("--close-levels", metavar="L,L,...", help="with --track-close: the pairs are aligned coarse to fine through these levels of a pyramid of the "
                    "sensor frames (level l: the frames box-reduced by 2^l), e.g. 2,1,0 (default: level 0 alone)")
    ap.add_argument("--close-exposure", choices=("none", "bias", "gain-bias"), default=None, help="with --track-close: what of a pair's relative exposure is "
                    "estimated with its rotation (default: none, the tracker's exposure is taken as it is)")
    ap.add_argument("--close-search", choices=("rotations", "appearance", "both"), default=None, help="with --track-close: where the pairs beyond the window come "
                    "from: the tracked rotations (default), the frames' bytes alone — every frame's thumbnail compared with every other's under every shift of a "
                    "range, on the device (DESIGN.md section 28) — or both (frames_pairs.txt gains the columns source, match score, dx, dy)")
    ap.add_argument("--close-match-level", type=int, default=None, metavar="L", help="with --close-search appearance / both: the level of the thumbnails (default 2)")
    ap.add_argument("--close-match-range", default=None, metavar="RX,RY", help="... the largest shift tried, in level pixels (default 6,4)")
    ap.add_argument("--close-match-score", type=float, default=None, metavar="X", help="... the least score of a matched pair: the signed square of the correlation (default 0.5)")
    ap.add_argument("--close-match-per-frame", type=int, default=None, metavar="N", help="... matched partners kept per frame (default 2)")
    ap.add_argument("--close-calib", metavar="fu,fv,cu,cv[,k1,k2,p1,p2,k3]", help="the camera the pairs project through (default: --calib's K and D; --demo: the "
                    "demo's pinhole)")
    ap.add_argument("--track-refit-tol", type=float, default=0.0, metavar="X", help="with --track-refit: stop behind a sweep whose largest rotation change is below X rad (0: never)")
    ap.add_argument("--cmax-slice-events", type=int, default=10000, help="events per slice of the contrast maximisation (--init-poses events)")
    ap.add_argument("--cmax-omega-max", type=float, default=8.0, help="rad/s: the compass search of a slice starts with steps of half of this (--init-poses events)")
    ap.add_argument("--record-contrast", action="store_true", help="print, per window, the contrast J = sum I^2 of the panorama of the window's warped events at its "
                    "initial and at its refined control poses (with --window-size; DESIGN.md section 12)")
    ap.add_argument("--event-panorama", action="store_true", help="write <out>/event_panorama.png: the events warped along the final trajectory (with --window-size)")
    ap.add_argument("--refine-contrast", action="store_true", help="before each window's solve, move the window's initial control poses uphill on the smooth contrast of "
                    "the panorama of the window's warped events — on the events alone, the window's first pose held fixed (with --window-size; DESIGN.md section 13)")
    ap.add_argument("--contrast-iters", type=int, default=60, help="conjugate-gradient iterations of --refine-contrast per window (and per level), at the most")
    ap.add_argument("--contrast-levels", default="0", help="the schedule of --refine-contrast, coarse to fine: comma-separated levels, strictly decreasing and ending "
                    "at 0, e.g. 3,2,1,0 — level l climbs on a panorama of cells 2^l pixels wide (DESIGN.md section 14); 0: the panorama alone")
    ap.add_argument("--contrast-prior", action="store_true", help="with --refine-contrast: before a window is refined, the events no later window sees again are voted "
                    "into a prior along the trajectory as refined so far, and the window climbs against it (DESIGN.md section 15)")
    ap.add_argument("--contrast-prior-weight", type=float, default=1.0, help="the weight of that prior in the image (finite, not negative)")
    ap.add_argument("--pano-h", type=int, default=1024, help="panorama height H (the map is H x 2H) where no map is read (--init-map events without --demo)")
    ap.add_argument("--refine", default="both", choices=["both", "map", "poses"], help="what the LM steps move: map and poses (the reference), the map only, or the poses only")
    ap.add_argument("--panorama-boundary", default="dirichlet", choices=["dirichlet", "wrap"], help="the boundary of the intensity panorama (map_poisson_opt.pgm and the "
                    "recorded map_poisson images): dirichlet, the reference's flat rectangle with a dark frame, or wrap: column W-1 is the neighbour of column 0 (DESIGN.md section 16)")
    ap.add_argument("--views-hz", type=float, default=0.0, help="write <out>/views/frame_%%06d.pgm and views/times.txt: what the camera would have seen along the final "
                    "trajectory at this many frames per second, sampled from the intensity panorama under --panorama-boundary with the panorama's own tone "
                    "(with --window-size; DESIGN.md section 17; rank 0).  0: off")
    ap.add_argument("--view-events", action="store_true", help="with --views-hz: also <out>/views/event_frames.npy, the signed event counts per sensor pixel between "
                    "consecutive frames")
    ap.add_argument("--sharded", action="store_true", help="go through the multi-GPU host (ShardedLEGM / ShardedModel) even with one rank")
    ap.add_argument("--simulate", metavar="PLANE", help="simulate a recording on the device from a log-intensity plane (.npy of doubles, H x W, or a binary .pgm read as "
                    "log(1 + v)) along the trajectory of --poses (with --calib; --demo: the demo's camera and, without --poses, its trajectory), write it to "
                    "--events-out and print its stats; with --demo the BA then runs on the simulated recording (DESIGN.md section 18)")
    ap.add_argument("--sim-hz", type=float, default=0.0, help="steps per second of --simulate: step times t0, t0 + p, ... up to t0 + (K - 1) dt - 1")
    ap.add_argument("--sim-c-on", type=float, help="the threshold of positive events (default: --C-th)")
    ap.add_argument("--sim-c-off", type=float, help="the threshold of negative events (default: the positive one)")
    ap.add_argument("--events-out", help="the file --simulate writes, in the flat event format of --events")
    a = ap.parse_args()
    if a.alpha is None:
        a.alpha = 0.0 if a.demo else 5.0
    if a.simulate:
        os.makedirs(a.out, exist_ok=True)
        return simulate(a, ap)
    if not a.demo and a.init_map == "given" and not a.map_dir:
        ap.error("--map-dir is required unless --init-map events or frames is given")
    if a.init_map == "frames" and not a.frames:
        ap.error("--init-map frames needs --frames DIR")
    if a.init_map == "frames" and a.init_poses not in ("given", "frames"):
        ap.error("--init-map frames stitches the frames along the raw trajectory: it needs given poses (--poses, or --demo), not --init-poses events / identity, "
                 "whose trajectory at that point carries the timing only")
    if a.refine_frames < 0 or (a.refine_frames and not a.frames):
        ap.error("--refine-frames N (N >= 0) aligns the frames of --frames DIR")
    if a.track_exposure != "none" and a.init_poses != "frames":
        ap.error("--track-exposure estimates the exposure inside the tracker of --init-poses frames: it needs --init-poses frames")
    if (a.track_refit or a.track_refit_tol) and a.init_poses != "frames":
        ap.error("--track-refit refits the frames tracked by --init-poses frames: it needs --init-poses frames")
    if a.track_close and a.init_poses != "frames":
        ap.error("--track-close closes loops among the frames tracked by --init-poses frames: it needs --init-poses frames")
    if (a.close_levels is not None or a.close_exposure is not None) and not a.track_close:
        ap.error("--close-levels and --close-exposure say how --track-close aligns its pairs: they need --track-close")
    if any(v is not None for v in (a.close_search, a.close_match_level, a.close_match_range, a.close_match_score, a.close_match_per_frame)) and not a.track_close:
        ap.error("--close-search and --close-match-* say where --track-close finds its pairs: they need --track-close")
    if a.close_match_range is not None:
        try:
            a.close_match_range = tuple(int(x) for x in a.close_match_range.split(","))
        except ValueError:
            a.close_match_range = ()
        if len(a.close_match_range) != 2 or min(a.close_match_range) < 0:
            ap.error("--close-match-range takes RX,RY, neither negative, e.g. 6,4")
    if ((a.close_match_level is not None and not 0 <= a.close_match_level <= eio.PAIR_MAX_LEVEL) or (a.close_match_score is not None and np.isnan(a.close_match_score))
            or (a.close_match_per_frame is not None and not 1 <= a.close_match_per_frame <= eio.MATCH_MAX_PER_FRAME)):
        ap.error(f"--close-match-level takes 0 ... {eio.PAIR_MAX_LEVEL}, --close-match-score a number, --close-match-per-frame 1 ... {eio.MATCH_MAX_PER_FRAME}")
    if a.close_levels is not None:
        try:
            a.close_levels = tuple(int(x) for x in a.close_levels.split(","))
        except ValueError:
            ap.error("--close-levels takes levels separated by commas, e.g. 2,1,0")
        if not 1 <= len(a.close_levels) <= eio.PAIR_MAX_LEVELS or any(not 0 <= l <= eio.PAIR_MAX_LEVEL for l in a.close_levels):
            ap.error(f"--close-levels takes 1 ... {eio.PAIR_MAX_LEVELS} levels, each 0 ... {eio.PAIR_MAX_LEVEL}")
    if a.close_window < 0 or a.close_gap < 0 or a.close_per_frame < 0 or not a.close_angle >= 0.0 or np.isnan(a.close_huber):
        ap.error("--close-window, --close-gap, --close-per-frame and --close-angle are not negative, --close-huber is a number")
    if a.track_refit < 0 or not a.track_refit_tol >= 0.0:
        ap.error("--track-refit N and --track-refit-tol X are not negative")
    if a.frames_exposure != "none" and not a.refine_frames:
        ap.error("--frames-exposure estimates the exposure in the rounds of --refine-frames N: it needs N >= 1")
    if a.refine_frames and a.init_poses not in ("given", "frames"):
        ap.error("--refine-frames aligns the frames from the raw trajectory: it needs given poses (--poses, or --demo), not --init-poses events / identity")
    if not (np.isfinite(a.frames_huber) and a.frames_huber >= 0.0):
        ap.error("--frames-huber is finite and not negative")
    if a.frames and not (np.isfinite(a.frames_lo) and np.isfinite(a.frames_hi) and np.isfinite(a.frames_eps) and a.frames_hi > a.frames_lo):
        ap.error("--frames-lo, --frames-hi and --frames-eps are finite, and --frames-hi is above --frames-lo")
    if not a.demo and a.init_poses == "given" and not a.poses:
        ap.error("--poses is required unless --init-poses events or identity is given")
    if a.init_poses == "frames":
        if not a.frames or not a.window_size:
            ap.error("--init-poses frames tracks the frames of --frames DIR and needs --window-size (a sliding-window run makes its control poses from the raw ones)")
        try:
            a.track_levels = [int(v) for v in a.track_levels.split(",")]
            a.track_q0 = [float(v) for v in a.track_q0.split(",")]
        except ValueError:
            ap.error("--track-levels is a list of integers, --track-q0 four numbers x,y,z,w")
        if not 1 <= len(a.track_levels) <= 8 or len(a.track_q0) != 4 or a.track_batch < 1 or not 0.0 <= a.track_min_overlap <= 1.0:
            ap.error("--track-levels names 1 ... 8 levels, --track-q0 has four numbers, --track-batch >= 1, 0 <= --track-min-overlap <= 1")
    if a.init_poses != "given" and not a.window_size:
        ap.error("--init-poses events / identity needs --window-size (a sliding-window run makes its control poses from the raw ones)")
    no_front_end = a.init_poses != "given"
    try:
        a.contrast_levels = eio.check_contrast_levels([int(v) for v in a.contrast_levels.split(",")], 1 << eio.CONTRAST_MAX_LEVEL)
    except ValueError as e:
        ap.error(f"--contrast-levels: {e}")
    if (a.record_contrast or a.event_panorama or a.refine_contrast) and not a.window_size:
        ap.error("--record-contrast / --event-panorama / --refine-contrast need --window-size (they run on the resident sequence of a sliding-window run)")
    if a.contrast_prior and not a.refine_contrast:
        ap.error("--contrast-prior is the prior of --refine-contrast")
    if not (np.isfinite(a.views_hz) and a.views_hz >= 0):
        ap.error("--views-hz is finite and not negative")
    if a.views_hz > 0 and not a.window_size:
        ap.error("--views-hz needs --window-size (the views follow the trajectory of a sliding-window run)")
    if a.view_events and not a.views_hz > 0:
        ap.error("--view-events counts the events between the frames of --views-hz")
    if not (np.isfinite(a.contrast_prior_weight) and a.contrast_prior_weight >= 0):
        ap.error("--contrast-prior-weight is finite and not negative")
    os.makedirs(a.out, exist_ok=True)

    if a.demo:
        w = synth.make_scene_workload(pano_h=512, K=11, sensor=(128, 96), focal=120.0, n_steps=2000)
        rng = np.random.default_rng(5)
        knots = w.traj.knots_xyzw.copy()
        for i in range(1, len(knots)):
            knots[i] = so3.mul(so3.exp(rng.normal(size=3) * 0.01), knots[i])
        traj, truth = LinearTrajectory(knots, w.traj.t0_ns, w.traj.dt_ns), w.traj
        events, Gx, Gy, lut, sw, sh, C_th = w.events, w.Gx, w.Gy, w.lut, w.sensor_w, w.sensor_h, w.C_th
        # the front end's raw poses of a sliding-window run: the perturbed trajectory sampled every 5 ms (9 poses inside every knot interval)
        t_raw_ns = traj.t0_ns + 5_000_000 * np.arange((traj.dt_ns * (traj.size() - 1)) // 5_000_000, dtype=np.int64)
        t, qs = t_raw_ns * 1e-9, np.array([traj.evaluate(int(tn)) for tn in t_raw_ns])
        t_beg, t_end = traj.t0_ns * 1e-9, (traj.t0_ns + traj.dt_ns * (traj.size() - 1)) * 1e-9
    else:
        cal = np.load(a.calib)
        sw, sh = int(cal["width"]), int(cal["height"])
        lut = eio.bearing_lut_from_calibration(cal["K"], cal["D"], sw, sh)
        Gx, Gy = eio.load_map(a.map_dir) if a.init_map == "given" else (np.zeros((a.pano_h, 2 * a.pano_h)), np.zeros((a.pano_h, 2 * a.pano_h)))
        if no_front_end:
            # no front end: the span is the recording's, and the trajectory below only carries the timing (run_sequence makes the poses)
            whole = eio.load_events(a.events)
            t, qs = np.array([whole.t_ns[0] * 1e-9, whole.t_ns[-1] * 1e-9]), None
        else:
            t, qs = eio.load_poses(a.poses)
        t_beg = a.t_beg if a.t_beg is not None else t[0]
        t_end = a.t_end if a.t_end is not None else t[-1]
        num_cps = int(round((t_end - t_beg) / a.dt_knots)) + 1                      # trajectory.cpp:231-245
        sel = (t >= t_beg) & (t <= t_end)
        if no_front_end:
            num_cps = int(np.floor((t_end - t_beg) / a.dt_knots)) + 1               # whole knot intervals inside the recording
            traj = LinearTrajectory.from_seconds(t_beg, a.dt_knots, np.tile([0.0, 0.0, 0.0, 1.0], (num_cps, 1)))
        else:
            traj = LinearTrajectory.from_seconds(t_beg, a.dt_knots, eio.fit_ctrl_poses(t[sel], qs[sel], t_beg, a.dt_knots, num_cps))
        ev_lo, ev_hi = int(t_beg * 1e9), traj.t0_ns + traj.dt_ns * (num_cps - 1) - 1
        if no_front_end:                                                           # (the file was read above: cut the same span from it)
            keep = (whole.t_ns >= ev_lo) & (whole.t_ns <= ev_hi)
            events = type(whole)(whole.x[keep], whole.y[keep], whole.polarity[keep], whole.t_ns[keep])
        else:
            events = eio.load_events(a.events, ev_lo, ev_hi)
        t_end = t_beg + a.dt_knots * (num_cps - 1)
        truth, C_th = None, a.C_th

    if a.init_poses == "identity":      # identity raw poses every 5 ms over the span, and the identity as the trajectory the result is compared with
        t = np.arange(int(round(t_beg * 1e9)) - 10_000_000, int(round(t_end * 1e9)) + 10_000_001, 5_000_000, dtype=np.int64) * 1e-9
        qs = np.tile([0.0, 0.0, 0.0, 1.0], (len(t), 1))
        traj = LinearTrajectory(np.tile([0.0, 0.0, 0.0, 1.0], (traj.size(), 1)), traj.t0_ns, traj.dt_ns)
    H, W = Gx.shape
    if a.init_map == "events":
        Gx, Gy = np.zeros((H, W)), np.zeros((H, W))
    world, rank, local_rank = int(os.environ.get("WORLD_SIZE", "1")), int(os.environ.get("RANK", "0")), int(os.environ.get("LOCAL_RANK", "0"))
    legm = None
    if world > 1 or a.sharded:
        # one process per GPU (torchrun): kernels and RCCL collectives share one explicit torch stream
        import torch
        import torch.distributed as dist
        from emba_amd.sharded import HipEngine, ShardedLEGM, ShardedModel
        torch.cuda.set_device(local_rank)
        dev = torch.device("cuda", local_rank)
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1"); os.environ.setdefault("MASTER_PORT", "29519")
        dist.init_process_group("nccl", device_id=dev, rank=rank, world_size=world)
        tstream = torch.cuda.Stream(device=dev)
        torch.cuda.set_stream(tstream)
        legm = LEGM(sw, sh, lut, C_th, W, H, device=local_rank, stream=tstream.cuda_stream)
        count_t = torch.zeros(H * W, dtype=torch.int32, device=dev)
        pack_t = torch.zeros(9 * traj.size() ** 2 + 3 * traj.size() + 5 * H * W, dtype=torch.float64, device=dev)
        sh_ = ShardedLEGM(HipEngine(legm), dist, count_t, pack_t, sw, torch.zeros(H * W, dtype=torch.uint8, device=dev))
        sh_.force_collectives = world == 1
        model = ShardedModel(sh_, legm)
    else:
        model = legm = LEGM(sw, sh, lut, C_th, W, H)
    ba = BASettings(use_IRLS=a.cost != "quadratic", cost_type=a.cost, eta=a.eta, thres_valid_pixel=a.thres_valid_pixel, alpha=a.alpha,
                    damping_factor=a.damping_factor, refine=a.refine, panorama_boundary=a.panorama_boundary)
    if rank == 0:
        print(f"{events.size()} events, {traj.size()} control poses, panorama {H}x{W}" + (f", {world} rank(s) through the sharded host" if legm is not model else ""))
    if a.frames:
        frames, frames_t_ns = load_frames(a.frames, sw, sh)
    tracked_mosaic = False
    if a.init_poses == "frames":      # poses from the frames alone: the tracked frames' rotations are the raw poses, the tracker's mosaic stays in the context
        close_calib = None
        if a.track_close:
            if a.close_calib:
                v = [float(x) for x in a.close_calib.split(",")]
                if len(v) not in (4, 9):
                    ap.error("--close-calib takes fu,fv,cu,cv or fu,fv,cu,cv,k1,k2,p1,p2,k3")
                close_calib = eio.pair_calib(*v[:4], v[4:] or None)
            elif a.demo:
                close_calib = eio.pair_calib(120.0, 120.0, sw / 2.0, sh / 2.0)
            else:
                close_calib = eio.pair_calib(cal["K"][0, 0], cal["K"][1, 1], cal["K"][0, 2], cal["K"][1, 2], cal["D"])
        traj, t, qs, rows = track_frames(legm, frames, frames_t_ns, traj, t_beg, t_end, a, log=print if rank == 0 else (lambda *_: None), calib=close_calib,
                                         pairs_path=os.path.join(a.out, "frames_pairs.txt") if a.track_close and rank == 0 else None)
        tracked_mosaic = True
        if rank == 0:
            with open(os.path.join(a.out, "frames_tracked.txt"), "w") as fh:
                fh.write("# t[s] qx qy qz qw status(1 anchor, 2 tracked, 3 lost) overlap cost" + (" gain bias[bytes]" if a.track_exposure != "none" else "")
                         + (" refit(1 anchor, 2 moved, 3 kept, 4 recovered, 5 lost)" if a.track_refit else "") + "\n")
                for row in rows:
                    tn, q, st, ov, cost = row[:5]
                    more = "".join(f" {v:.17g}" if isinstance(v, float) else f" {v}" for v in row[5:])
                    fh.write(f"{tn // 1_000_000_000}.{tn % 1_000_000_000:09d} {q[0]:.17g} {q[1]:.17g} {q[2]:.17g} {q[3]:.17g} {st} {ov:.9g} {cost:.9g}{more}\n")
    frames_exposure = None      # (gain, bias) per frame of --frames, once --track-exposure or --frames-exposure has estimated them
    if a.init_poses == "frames" and a.track_exposure != "none":
        frames_exposure = (np.array([row[5] for row in rows]), np.array([row[6] for row in rows]))
    exposure_estimate = {"none": None, "bias": eio.EXPOSURE_BIAS, "gain-bias": eio.EXPOSURE_GAIN | eio.EXPOSURE_BIAS}[a.frames_exposure]
    if a.refine_frames:      # poses from frames: the raw trajectory is refitted to the frames' aligned rotations before anything else reads it
        refined = refine_frames(legm, frames, frames_t_ns, traj, np.asarray(t, dtype=np.float64), np.asarray(qs, dtype=np.float64), a.refine_frames,
                                a.frames_huber, a.frames_skip_zero, log=print if rank == 0 else (lambda *_: None), estimate=exposure_estimate,
                                exposure0=frames_exposure)
        traj, t, qs, rows = refined[:4]
        if exposure_estimate is not None:
            frames_exposure = refined[4]
        if rank == 0:
            with open(os.path.join(a.out, "frames_aligned.txt"), "w") as fh:
                fh.write("# t[s] qx qy qz qw status(1 converged, 2 stalled, 3 iterations, 4 degenerate) mean_cost_before mean_cost_after"
                         + (" gain bias[bytes]" if exposure_estimate is not None else "") + "\n")
                for row in rows:
                    tn, q, st, b, a_ = row[:5]
                    more = "".join(f" {v:.17g}" for v in row[5:])
                    fh.write(f"{tn // 1_000_000_000}.{tn % 1_000_000_000:09d} {q[0]:.17g} {q[1]:.17g} {q[2]:.17g} {q[3]:.17g} {st} {b:.9g} {a_:.9g}{more}\n")
    if a.init_map == "frames":      # the mosaic of the frames along the raw trajectory, on the device; its gradient map is handed on as the given map
        if tracked_mosaic and not a.refine_frames:      # the mosaic the tracker left: no second stitch
            used = int(sum(1 for row in rows if row[2] != eio.TRACK_LOST))
        else:
            used = frame_mosaic(legm, frames, frames_t_ns, traj, a.frames_skip_zero, frames_exposure)
        fm = legm.mosaic_map(lo=a.frames_lo, hi=a.frames_hi, eps=a.frames_eps, take_log=bool(a.frames_log))
        Gx, Gy = fm["Gx"], fm["Gy"]
        if rank == 0:
            print(f"initial map from {used} of {len(frames_t_ns)} frames along the raw trajectory: {legm.mosaic()['n_covered']} of {H * W} cells covered, "
                  f"mean |G| {0.5 * (np.abs(Gx).mean() + np.abs(Gy).mean()):.4g}")
    t0 = time.time()
    # the reference's run-time records (final_results/runtime_{formEqs,solveEqs,objFuncs}.txt, iterations.txt: solver.cpp:105-151, 170-178, 205-223, 271-291)
    rlog = RuntimeLog(a.out) if (a.runtime_log and rank == 0) else None
    mrec = MapRecorder(a.out) if (a.record_data and rank == 0) else None
    if a.window_size:
        from emba_amd.driver import SequenceSettings, run_sequence
        seq = SequenceSettings(time_window_size=a.window_size, sliding_window_stride=a.window_stride or a.window_size, dt_knots=traj.dt_ns * 1e-9 if a.demo else a.dt_knots,
                               event_sampling_rate=a.sampling_rate, t_start=t_beg, t_end=t_end, median_blur=a.median_blur,
                               init_map="events" if a.init_map == "events" else "given",      # (frames: the mosaic's map is a given map)
                               hot_pixel_sigma=a.hot_pixel_sigma, refractory_period=a.refractory, support_time=a.support_time,
                               init_poses="events" if a.init_poses == "events" else "given", cmax_slice_events=a.cmax_slice_events, cmax_omega_max=a.cmax_omega_max,
                               record_contrast=a.record_contrast, event_panorama=a.event_panorama, refine_contrast=a.refine_contrast,
                               contrast_iters=a.contrast_iters, contrast_levels=a.contrast_levels, contrast_prior=a.contrast_prior,
                               contrast_prior_weight=a.contrast_prior_weight, views_hz=a.views_hz if rank == 0 else 0.0, view_events=a.view_events,
                               track_refit=a.track_refit, track_refit_tol=a.track_refit_tol)
        sres = run_sequence(model, events, *((None, None) if a.init_poses == "events" else (t, qs)), *((None, None) if a.init_map == "events" else (Gx, Gy)), seq, ba, LMSettings(max_num_iter=a.max_iter), runtime_log=rlog, map_recorder=mrec, resident=True,
                            verbose=a.verbose)
        if rank == 0 and sres.filter_stats is not None:
            fs = [int(v) for v in sres.filter_stats]
            print(f"noise filters: {fs[0]} events in, {fs[1]} hot pixels ({fs[2]} events), {fs[3]} inside the refractory period, {fs[4]} without support, {fs[5]} kept")
        if rank == 0 and sres.cmax is not None:
            cm = sres.cmax
            print(f"contrast maximisation: {len(cm['omega'])} slices of {a.cmax_slice_events} events, {int(cm['evals'].sum())} evaluations, "
                  f"median |omega| {np.median(np.linalg.norm(cm['omega'], axis=1)):.3f} rad/s")
            if truth is not None:
                # the initial trajectory of the comparison at the end: the integrated estimate at the control poses' times
                tq = truth.t0_ns + truth.dt_ns * np.arange(truth.size(), dtype=np.int64)
                traj = LinearTrajectory(eio.integrate_angular_velocity(cm["omega"], cm["t_ref_ns"], tq)[1], truth.t0_ns, truth.dt_ns)
        if rank == 0:
            for wr in sres.windows:
                if wr.map_init is not None:
                    print(f"window {wr.index}: map-only start from a zero map, {wr.map_init.iterations} LM iterations ({wr.map_init.reason}), cost {wr.map_init.cost_min:.6e}")
                print(f"window {wr.index}: [{wr.t_beg_ns * 1e-9:.3f}, {wr.t_end_ns * 1e-9:.3f}] s, events [{wr.beg}, {wr.end}), control poses from {wr.idx_cp_beg}, "
                      f"{wr.result.iterations} LM iterations ({wr.result.reason or 'converged'}), cost {wr.result.cost_min:.6e}, set-up {wr.setup_ms:.2f} ms")
                if wr.refine_J_before is not None:
                    print(f"window {wr.index}: control poses refined on the events alone, smooth contrast J = {wr.refine_J_before:.6e} -> {wr.refine_J_after:.6e} "
                          f"in {wr.refine_evals} evaluations" + (f", against a prior of {wr.prior_events} earlier events" if wr.prior_events else ""))
                if wr.contrast_init is not None:
                    j0, j1 = wr.contrast_init["J"], wr.contrast_final["J"]
                    print(f"window {wr.index}: contrast of the warped events J = {j0:.6e} -> {j1:.6e} (x {j1 / max(j0, 1):.4f})")
            if sres.event_panorama is not None:
                eio.save_png(os.path.join(a.out, "event_panorama.png"), eio.normalize_robust(sres.event_panorama.astype(np.float64), 0.1))
            if sres.views is not None:
                vw = sres.views
                os.makedirs(os.path.join(a.out, "views"), exist_ok=True)
                for f, img in enumerate(vw["u8"]):
                    eio.save_pgm(os.path.join(a.out, "views", "frame_%06d.pgm" % f), img)
                with open(os.path.join(a.out, "views", "times.txt"), "w") as fh:
                    fh.write("".join("%d %d.%09d\n" % (f, tn // 1_000_000_000, tn % 1_000_000_000) for f, tn in enumerate(vw["t_ns"].tolist())))
                with open(os.path.join(a.out, "views", "tone.txt"), "w") as fh:      # the tone of the bytes, in full: --frames-lo / --frames-hi of a run on these frames
                    fh.write("%r %r\n" % (float(vw["lo"]), float(vw["hi"])))
                if vw["event_frames"] is not None:
                    np.save(os.path.join(a.out, "views", "event_frames.npy"), vw["event_frames"])
                print(f"views: {len(vw['t_ns'])} frames at {a.views_hz:g} Hz under {a.out}/views, tone [{vw['lo']:.4g}, {vw['hi']:.4g}], "
                      f"{int(vw['outside'].sum())} pixels past a pole row"
                      + (f", {int(np.abs(vw['event_frames']).sum())} net events in {len(vw['event_frames'])} event frames" if vw["event_frames"] is not None else ""))
                if vw["event_frames"] is not None and len(vw["event_frames"]) and vw["event_frames"].any():
                    # the generative model: the brightness change between two predicted frames, over C_th, is the event count it expects at that pixel
                    dv = np.diff(vw["views"], axis=0).ravel()
                    print(f"views: correlation between V[f+1] - V[f] and the signed event frames {np.corrcoef(dv, vw['event_frames'].ravel().astype(np.float64))[0, 1]:+.4f} "
                          f"(mean |dV| {np.abs(dv).mean():.4g}, C_th {C_th:g})")
        res = sres.windows[-1].result
        res = type(res)(sres.traj, res.cost_min, sum(wr.result.iterations for wr in sres.windows), all(wr.result.converged for wr in sres.windows), res.log, res.reason)
        if truth is not None:
            traj = LinearTrajectory(traj.knots_xyzw[:sres.traj.size()], traj.t0_ns, traj.dt_ns)
    else:
        if a.init_map == "events":      # mapping with known poses from the zero map, then the window as usual from the resident map
            import dataclasses
            mres = solve_time_window(model, traj, events, Gx, Gy, dataclasses.replace(ba, refine="map"), LMSettings(max_num_iter=a.max_iter), verbose=a.verbose, resident=True)
            Gx = Gy = None
            if rank == 0:
                print(f"map-only start from a zero map: {mres.iterations} LM iterations ({mres.reason}), cost {mres.cost_min:.6e}")
        res = solve_time_window(model, traj, events, Gx, Gy, ba, LMSettings(max_num_iter=a.max_iter), verbose=a.verbose, resident=True, runtime_log=rlog,
                                map_recorder=mrec)
    dt = time.time() - t0
    if mrec is not None:
        mrec.close()
        sm = mrec.summary()
        print(f"record_data: {sm['files']} PNG files in {sm['sets']} sets; rendering {sm['render_s'] * 1e3:.1f} ms (in the loop), "
              f"encoding + writing {sm['encode_s'] * 1e3:.1f} ms (writer threads)")
    if rank != 0:                                           # every rank holds the same result; rank 0 writes it
        import torch.distributed as dist
        dist.barrier(); dist.destroy_process_group()
        return
    print(f"{res.iterations} LM iterations in {dt * 1e3:.1f} ms ({'converged' if res.converged else 'stopped'}), cost {res.cost_min:.6e}")
    if truth is not None:
        # (a run from the events alone starts at the identity, wherever the camera pointed: rotations relative to the first control pose are compared then)
        rel = (lambda k: np.array([so3.mul(so3.inverse(k[0]), q) for q in k])) if no_front_end else (lambda k: k)
        err = lambda tr: np.degrees(np.mean([np.linalg.norm(so3.log(so3.mul(so3.inverse(p), q))) for p, q in zip(rel(tr.knots_xyzw), rel(truth.knots_xyzw))]))
        print(f"mean control-pose error vs ground truth: {err(traj):.4f} deg -> {err(res.traj):.4f} deg")
    eio.write_trajectory(os.path.join(a.out, "refined_traj.txt"), res.traj)
    eio.save_map(a.out, *model.downloadMap())
    # intensity panorama from the refined gradient map (solver.cpp:417-425 / 471-479), reconstructed on the device
    eio.save_pgm(os.path.join(a.out, "map_poisson_opt.pgm"), eio.normalize_robust(legm.reconstructIntensity(boundary=a.panorama_boundary), 0.1))
    if a.frames:      # the frames along the FINAL trajectory: an independent picture of the scene, to set against map_poisson_opt.pgm
        used = frame_mosaic(legm, frames, frames_t_ns, res.traj, a.frames_skip_zero, frames_exposure)
        mo = legm.mosaic()
        eio.save_pgm(os.path.join(a.out, "frame_mosaic.pgm"), np.clip(np.rint(mo["mean"]), 0, 255).astype(np.uint8))
        eio.save_pgm(os.path.join(a.out, "frame_mosaic_covered.pgm"), np.where(mo["covered"], 255, 0).astype(np.uint8))
        print(f"frame mosaic: {used} of {len(frames_t_ns)} frames along the final trajectory, {mo['n_covered']} of {H * W} cells covered")
    if legm is not model:
        import torch.distributed as dist
        dist.barrier(); dist.destroy_process_group()


if __name__ == "__main__":
    main()
