"""The caller of solve_time_window: EMBA::EMBA's preparation of its inputs and EMBA::Run, the sliding-window loop (reference src/emba/emba.cpp:281-304,
309-323, 357-364, 400-532), without ROS.  A recording longer than one time window is cut into windows of `time_window_size` that advance by
`sliding_window_stride`; the trajectory grows window by window, the map is carried from one window to the next on the device.

With a device model (emba_amd.LEGM) the whole event sequence crosses to the device once (LEGM.set_sequence: checked and down-sampled there), every window
is a range of it (LEGM.sequence_window -> EventWindow -> emba_set_events_seq) and the median blur of the initial map runs on the resident map.  The sharded
host (sharded.ShardedModel over HipEngine) does the same on every rank: each holds the whole sequence and registers its time shard of the window from it, the
per-pixel halo built on the device (emba_set_events_seq_shard).  Models without a resident sequence (the test suite's oracle model, a sharded host over an
engine that has none) get the same windows as host slices, through the numpy forms in emba_amd.io.

Time cursors are integer nanoseconds by the rostime rules of SURVEY.md Appendix A (ros::Time(double) / ros::Duration(double): io.ros_time_ns)."""
import dataclasses
from dataclasses import dataclass, field

import numpy as np

from . import io as emba_io
from . import so3
from .legm import EventWindow, LinearTrajectory
from .solver import BASettings, LMSettings, solve_time_window


@dataclass
class SequenceSettings:         # include/emba/params.h:14-61 (BA_config), docs/parameters.md; t_start / t_end: start_time_s / stop_time_s + the time offset, emba.cpp:244-249
    time_window_size: float
    sliding_window_stride: float
    dt_knots: float = 0.05
    event_sampling_rate: int = 1
    t_start: float = 0.0
    t_end: float = 0.0
    median_blur: bool = True    # emba.cpp:357-364 is unconditional in the reference; False keeps the initial map as given
    init_map: str = "given"     # "given": Gx, Gy are the front end's map.  "events": there is none (the reference's init_map_available = false, emba.cpp:333-355,
                                # fills the map with noise there) — the run starts from a zero map, and the first window is first solved for the map alone from
                                # its initial control poses (BASettings.refine = "map": well posed where the joint system with G = 0 is singular)
    # Sensor noise (no counterpart in the reference; the rule: include/emba_hip.h, emba_seq_filter).  All off by default; with any of them on the recording
    # is filtered once, BEFORE the down-sampling, on the device wherever the sequence is resident (LEGM.filter_sequence), else by io.filter_events.
    hot_pixel_sigma: float = 0.0    # a pixel is hot when its event count exceeds mean + sigma * std over the pixels that have events
    refractory_period: float = 0.0  # seconds: an event closer than this behind its pixel's previous event is dropped
    support_time: float = 0.0       # seconds: an event is kept only if one of its eight neighbours fired at most this long before it
    # The raw poses.  "given": pose_t, pose_q are a front end's.  "events": there is no front end — the angular velocity of every slice of cmax_slice_events
    # events is estimated from the events alone by contrast maximisation (the rule: include/emba_hip.h, emba_seq_cmax) after the filters and
    # the down-sampling, on the device where the sequence is resident (LEGM.estimate_angular_velocity), else by io.estimate_angular_velocity, and integrated
    # from the identity (io.integrate_angular_velocity); pose_t, pose_q may then be None.
    init_poses: str = "given"
    cmax_slice_events: int = 10000
    cmax_omega_max: float = 8.0
    # The panorama of warped events (no counterpart in the reference's back end; the rule: include/emba_hip.h, emba_seq_event_panorama), on the
    # device where the sequence is resident (LEGM.event_panorama), else by io.event_panorama.  Both off by default.
    record_contrast: bool = False   # WindowResult.contrast_init / contrast_final: J, sum, nonzero of the window's events at the segment handed to
                                    # solve_time_window and at the refined one — comparable between trajectories on the same events, which the LM cost is not
    event_panorama: bool = False    # SequenceResult.event_panorama: the image of the events the final trajectory spans, at that trajectory
    # Refinement of each window's initial control poses on the window's events alone, before solve_time_window: conjugate-gradient ascent on the smooth
    # contrast of the panorama of warped events (io.refine_contrast over LEGM.contrast_gradient; the rule: include/emba_hip.h,
    # emba_seq_contrast_gradient), the window's first pose held fixed.  Needs the sequence resident on the device.  Off by default.
    refine_contrast: bool = False
    contrast_iters: int = 60
    # The schedule of that ascent, coarse to fine (io.refine_contrast_pyramid): level l climbs on a panorama of cells 2^l pixels wide
    # (LEGM.contrast_gradient(level=l)), each level for up to contrast_iters iterations, strictly decreasing and ending at 0.  (0,): the panorama alone.
    contrast_levels: tuple = (0,)
    # The prior of that ascent (the rule: include/emba_hip.h, emba_seq_contrast_gradient_prior): before a window is refined, the events no
    # later window will see again are voted, along the trajectory as refined so far, into the priors of every level of contrast_levels
    # (LEGM.contrast_prior_add), and the window then climbs on the contrast of contrast_prior_weight times that prior plus its own events — what ties a window
    # to the panorama the windows before it placed.  Needs refine_contrast.  Off by default; the first window has no prior.
    contrast_prior: bool = False
    contrast_prior_weight: float = 1.0
    # Sensor views along the final trajectory (no counterpart in the reference; the rules: include/emba_hip.h, emba_render_views and emba_seq_event_frames;
    # DESIGN.md §17): after the last window, what the camera would have seen at views_hz frames per second over the time the trajectory covers, sampled
    # from the intensity panorama of the refined map under BASettings.panorama_boundary (SequenceResult.views) — on the device where the model has one
    # (LEGM.render_views), else by io.render_views; with view_events also the signed event counts between consecutive frames (LEGM.event_frames where the
    # sequence is resident, else io.event_frames).  0: off.
    views_hz: float = 0.0
    view_events: bool = False
    # Raw poses that come from tracked intensity frames (LEGM.track_frames / track_frames_exposure in front of run_sequence) are refitted first: track_refit
    # sweeps of LEGM.refit_frames — every frame taken out of the integer mosaic, aligned to the mosaic of the other frames and voted back (the rule:
    # include/emba_hip.h, emba_frames_refit) — ended early behind a sweep whose largest rotation change is below track_refit_tol (rad; 0:
    # never).  refit_tracked_frames below applies them.  0: off.
    track_refit: int = 0
    track_refit_tol: float = 0.0
    # ... and, before any refit, their loops are closed: track_close aligns pairs of tracked frames that see the same place with each other
    # (LEGM.pair_align) and solves the rotation graph of the kept pairs with the tracker's anchors held exactly (LEGM.rotation_graph_solve; the rules:
    # include/emba_hip.h, emba_frames_pair_align and emba_rotation_graph_solve).  The pairs are io.pair_candidates of the tracked rotations
    # under close_window, close_gap, close_angle (rad) and close_per_frame; close_huber is the pairs' Huber threshold in bytes (0: quadratic);
    # close_min_overlap the share of used pixels a kept pair needs.  close_tracked_frames below applies it.  Off by default.
    track_close: bool = False
    close_window: int = 1
    close_gap: int = 4
    close_angle: float = 0.2
    close_per_frame: int = 2
    close_huber: float = 0.0
    close_min_overlap: float = 0.3
    # How a pair is aligned (the rule: include/emba_hip.h, emba_frames_pair_align_levels): close_levels is the schedule over a pyramid of the sensor
    # frames, coarse to fine (level l: the frames box-reduced by 2^l; each 0 ... 7, at most 8), and close_exposure says what of the pair's relative exposure is
    # estimated with its rotation: "none", "bias" or "gain-bias".  With both at their defaults the pairs go through LEGM.pair_align as before; otherwise
    # through LEGM.pair_align_levels from the same starts.  The graph stays one of rotations alone.
    close_levels: tuple = (0,)
    close_exposure: str = "none"
    # Where the pairs beyond the window come from (the rule: include/emba_hip.h, emba_frames_match_search): "rotations" — io.pair_candidates of the
    # tracked rotations, as above; "appearance" — the window's neighbours plus the pairs LEGM.match_search finds more than close_gap frames apart from the frames'
    # bytes alone: level close_match_level of the pyramid, shifts up to close_match_range = (rx, ry) level pixels, per frame the close_match_per_frame partners
    # of score >= close_match_score (the signed square of the correlation), a shift scored on close_match_min_overlap of the thumbnail at the least; a matched
    # pair starts from the rotation its shift stands for (io.match_start), not from the tracked rotations; "both" — the two sets together, a pair that is in
    # both starting from the tracked rotations.
    close_search: str = "rotations"
    close_match_level: int = 2
    close_match_range: tuple = (6, 4)
    close_match_score: float = 0.5
    close_match_per_frame: int = 2
    close_match_min_overlap: float = 0.25

    def __post_init__(self):
        if self.close_search not in emba_io.MATCH_SEARCH_MODES:
            raise ValueError(f"SequenceSettings.close_search must be one of {emba_io.MATCH_SEARCH_MODES}, not {self.close_search!r}")
        self.close_match_range = tuple(int(v) for v in np.asarray(self.close_match_range).reshape(-1))
        if (len(self.close_match_range) != 2 or min(self.close_match_range) < 0 or not 0 <= int(self.close_match_level) <= emba_io.PAIR_MAX_LEVEL
                or not 1 <= int(self.close_match_per_frame) <= emba_io.MATCH_MAX_PER_FRAME or np.isnan(self.close_match_score)
                or not 0.0 <= float(self.close_match_min_overlap) <= 1.0):
            raise ValueError(f"SequenceSettings.close_match_*: a level 0 ... {emba_io.PAIR_MAX_LEVEL}, a range (rx, ry) that is not negative, 1 ... "
                             f"{emba_io.MATCH_MAX_PER_FRAME} partners per frame, a score that is a number, an overlap that is a share")
        self.close_levels = tuple(int(l) for l in np.asarray(self.close_levels).reshape(-1))
        if not 1 <= len(self.close_levels) <= emba_io.PAIR_MAX_LEVELS or any(not 0 <= l <= emba_io.PAIR_MAX_LEVEL for l in self.close_levels):
            raise ValueError(f"SequenceSettings.close_levels = {self.close_levels}: 1 ... {emba_io.PAIR_MAX_LEVELS} levels, each 0 ... {emba_io.PAIR_MAX_LEVEL}")
        if self.close_exposure not in emba_io.PAIR_EXPOSURE_MODES:
            raise ValueError(f"SequenceSettings.close_exposure must be one of {sorted(emba_io.PAIR_EXPOSURE_MODES)}, not {self.close_exposure!r}")
        if (int(self.close_window) < 0 or int(self.close_gap) < 0 or int(self.close_per_frame) < 0 or not float(self.close_angle) >= 0.0
                or not 0.0 <= float(self.close_min_overlap) <= 1.0 or np.isnan(self.close_huber)):
            raise ValueError("SequenceSettings.close_*: window, gap and per_frame are counts, the angle is not negative, the overlap a share, the threshold a number")
        if int(self.track_refit) < 0 or not float(self.track_refit_tol) >= 0.0:
            raise ValueError(f"SequenceSettings.track_refit = {self.track_refit}, track_refit_tol = {self.track_refit_tol}: sweeps and a tolerance, neither negative")
        if not (np.isfinite(self.views_hz) and self.views_hz >= 0):
            raise ValueError(f"SequenceSettings.views_hz = {self.views_hz}: frames per second, finite and not negative (0: off)")
        if self.init_poses not in ("given", "events"):
            raise ValueError(f"SequenceSettings.init_poses must be 'given' or 'events', not {self.init_poses!r}")
        self.contrast_levels = emba_io.check_contrast_levels(self.contrast_levels, 1 << emba_io.CONTRAST_MAX_LEVEL)      # (the width: checked where it is known)
        if not (np.isfinite(self.contrast_prior_weight) and self.contrast_prior_weight >= 0):
            raise ValueError(f"SequenceSettings.contrast_prior_weight = {self.contrast_prior_weight}: the weight of the prior is finite and not negative")
        if self.contrast_prior and not self.refine_contrast:
            raise ValueError("SequenceSettings.contrast_prior is the prior of the contrast refinement: it needs refine_contrast = True")
        if int(self.cmax_slice_events) < 1:
            raise ValueError(f"SequenceSettings.cmax_slice_events = {self.cmax_slice_events}: a slice has at least one event")
        if not (np.isfinite(self.cmax_omega_max) and self.cmax_omega_max > 0):
            raise ValueError("SequenceSettings.cmax_omega_max must be finite and positive")


def refit_tracked_frames(model, frames, frame_t_ns, tracked, seq, **track_kw):
    """`tracked`: what model.track_frames or model.track_frames_exposure returned for these frames under the tracker settings track_kw (levels, batch,
    skip_zero, min_weight, min_overlap, estimate, the gain bounds, the members of io.ALIGN_DEFAULTS; q0 and predict are the tracker's alone).  With
    seq.track_refit sweeps it is refitted on the device (LEGM.refit_frames) and the tracker's dict comes back with q, gain, bias, status, iters, cost, counts,
    overlap and the four stats as the refit left them, and `refit` (io.REFIT_* per frame), `sweep` and `sweeps_done` beside them; the mosaic in the context
    is the refitted one.  With track_refit = 0 `tracked` is returned as it is."""
    if not seq.track_refit:
        return tracked
    kw = {k: v for k, v in track_kw.items() if k not in ("q0", "predict", "want_pm")}
    r = model.refit_frames(frames, frame_t_ns, tracked["q"], tracked["status"], tracked.get("gain"), tracked.get("bias"), sweeps=int(seq.track_refit),
                           sweep_tol=float(seq.track_refit_tol), **kw)
    out = dict(tracked)
    out.update({k: v for k, v in r.items() if k != "pm"})
    return out


def close_tracked_frames(model, frames, frame_t_ns, tracked, seq, calib, **track_kw):
    """`tracked`: what model.track_frames or model.track_frames_exposure returned for these frames under the tracker settings track_kw (as
    refit_tracked_frames takes them); calib: the camera of the frames (io.pair_calib).  With seq.track_close: the candidates of the tracked rotations
    (io.pair_candidates), started from the tracked (q, gain, bias) (io.pair_start), are aligned on the device (LEGM.pair_align); the pairs that ended
    converged or on iterations with n / S >= close_min_overlap are the edges of the rotation graph, their information floored at io.PAIR_NOISE_FLOOR, which
    is solved with the tracker's anchors fixed (LEGM.rotation_graph_solve); the frames are then stitched again at the new rotations
    (LEGM.refit_frames, sweeps = 0), so the mosaic in the context is the closed one.  The tracker's dict comes back with the new q and, beside it, `pairs`
    [P, 2], `pair_status`, `pair_n`, `pair_cost` (mean), `pair_moved` (rad, against the pair's start), `pair_kept` and `graph` (cost0, cost, iters,
    cg_iters, end).  Without seq.track_close, or where no pair is kept, `tracked` is returned as it is (with the pairs, where there were any).  With
    seq.close_levels or seq.close_exposure off their defaults the pairs go through LEGM.pair_align_levels instead, from the same starts; a pair is kept by the
    same gate on the counts of its last level run against that level's pixels, and `pair_gain`, `pair_bias`, `pair_level_status` [P, n] and
    `pair_last_level` come back beside the rest.  The graph stays one of rotations alone.  seq.close_search says where the pairs beyond the window come
    from: "rotations" makes exactly the calls above; "appearance" and "both" add the pairs LEGM.match_search finds from the frames' bytes,
    started from io.match_start of their shifts (_matched_pairs below); everything behind the pairs is the same.  `pair_source` (0 window, 1 rotations,
    2 appearance), `pair_match_score` (io.MATCH_UNSCORED where the search did not propose the pair) and `pair_match_shift` [P, 2] come back in every mode."""
    if not seq.track_close:
        return tracked
    kw = {k: v for k, v in track_kw.items() if k not in ("q0", "predict", "want_pm")}
    S = model.sensor_w * model.sensor_h
    if seq.close_search == "rotations":
        pairs = emba_io.pair_candidates(tracked["q"], tracked["status"], window=seq.close_window, min_gap=seq.close_gap, max_angle=seq.close_angle,
                                        max_per_frame=seq.close_per_frame)
        Q0, a, b = emba_io.pair_start(tracked["q"], tracked.get("gain"), tracked.get("bias"), pairs)
        source = np.where(pairs[:, 1] - pairs[:, 0] <= int(seq.close_window), 0, 1).astype(np.int32)
        m_score, m_shift = np.full(len(pairs), emba_io.MATCH_UNSCORED), np.zeros((len(pairs), 2), np.int32)
    else:
        pairs, source, Q0, a, b, m_score, m_shift = _matched_pairs(model, frames, tracked, seq, calib, bool(kw.get("skip_zero", False)))
    align_kw = {k: v for k, v in kw.items() if k in emba_io.ALIGN_DEFAULTS}
    align_kw["huber_k"] = float(seq.close_huber)
    levelled = seq.close_levels != (0,) or seq.close_exposure != "none"
    if not levelled:
        al = model.pair_align(frames, pairs, Q0, calib, gain=a, bias=b, skip_zero=bool(kw.get("skip_zero", False)), **align_kw)
        ten, S_last = al["sums"], S
    else:      # coarse to fine, the pair's exposure estimated: the same starts, the gate on the last level run against that level's pixels
        al = model.pair_align_levels(frames, pairs, Q0, calib, levels=seq.close_levels, estimate=emba_io.PAIR_EXPOSURE_MODES[seq.close_exposure], gain=a, bias=b,
                                     skip_zero=bool(kw.get("skip_zero", False)), gain_min=kw.get("gain_min"), gain_max=kw.get("gain_max"), **align_kw)
        ten = al["sums"][:, list(emba_io.EXPOSURE_SHARED)]
        ran = np.maximum((al["level_status"] != 0).sum(axis=1) - 1, 0)      # (the levels of a pair are run in order: the last one run)
        last = np.asarray(seq.close_levels)[ran] if len(pairs) else np.zeros(0, np.int64)
        S_last = (model.sensor_w >> last) * (model.sensor_h >> last)
    n = al["counts"][:, 0]
    kept = ((al["status"] == emba_io.ALIGN_CONVERGED) | (al["status"] == emba_io.ALIGN_ITERATIONS)) & (n >= seq.close_min_overlap * S_last)
    out = dict(tracked)
    out.update(pairs=pairs, pair_status=al["status"], pair_n=n, pair_cost=ten[:, 9] / np.maximum(n, 1), pair_kept=kept,
               pair_moved=emba_io.rotation_angle_between(Q0, al["q"]) if len(pairs) else np.zeros(0), graph=None, pair_source=source,
               pair_match_score=m_score, pair_match_shift=m_shift)
    if levelled:
        out.update(pair_gain=al["gain"], pair_bias=al["bias"], pair_level_status=al["level_status"], pair_last_level=last)
    if not kept.any():
        return out
    info = emba_io.pair_information(ten, al["counts"], floor=emba_io.PAIR_NOISE_FLOOR)
    reach = _reached(tracked["status"], pairs[kept])
    kept &= reach[pairs[:, 0]] & reach[pairs[:, 1]]      # (a group of frames that no kept pair ties to an anchor stays where the tracker put it)
    if not kept.any():
        return out
    g = model.rotation_graph_solve(tracked["q"], tracked["status"], pairs[kept], al["q"][kept], info[kept])
    out["q"], out["pair_kept"], out["graph"] = g["q"], kept, {k: v for k, v in g.items() if k != "q"}
    r = model.refit_frames(frames, frame_t_ns, g["q"], tracked["status"], tracked.get("gain"), tracked.get("bias"), sweeps=0, **kw)
    out.update({k: r[k] for k in ("dropped", "skipped")})
    return out


def _matched_pairs(model, frames, tracked, seq, calib, skip_zero):
    """The pairs of close_search = "appearance" and "both" (DESIGN.md §28): the window's neighbours (source 0), with "both" the angle candidates of the
    tracked rotations (1), and the pairs LEGM.match_search finds more than close_gap frames apart (2 where nothing else proposes them).  Every pair starts from
    the tracked (q, gain, bias) but a pair of source 2, whose rotation starts from io.match_start of its shift.  (pairs [P, 2] sorted, source [P], Q0 [P, 4],
    a [P], b [P], the match score [P] (io.MATCH_UNSCORED where the search did not propose the pair) and shift [P, 2])."""
    sw, sh, level = model.sensor_w, model.sensor_h, int(seq.close_match_level)
    rx, ry = seq.close_match_range
    n_min = max(int(np.ceil(float(seq.close_match_min_overlap) * (sw >> level) * (sh >> level))), 1)
    cand = dict(window=seq.close_window, min_gap=seq.close_gap, max_angle=seq.close_angle)
    win = {tuple(p) for p in emba_io.pair_candidates(tracked["q"], tracked["status"], max_per_frame=0, **cand).tolist()}
    rot = {tuple(p) for p in emba_io.pair_candidates(tracked["q"], tracked["status"], max_per_frame=seq.close_per_frame, **cand).tolist()} if seq.close_search == "both" else win
    found = model.match_search(frames, tracked["status"], level=level, rx=rx, ry=ry, min_gap=seq.close_gap, skip_zero=skip_zero, n_min=n_min,
                               score_min=float(seq.close_match_score), k=int(seq.close_match_per_frame))
    mp, ms, md = emba_io.match_pairs(found, with_info=True)
    app = {tuple(p): (s, d) for p, s, d in zip(mp.tolist(), ms, md)}
    keys = sorted(win | rot | set(app))
    pairs = np.array(keys, dtype=np.int32).reshape(-1, 2)
    source = np.array([0 if p in win else 1 if p in rot else 2 for p in keys], dtype=np.int32)
    Q0, a, b = emba_io.pair_start(tracked["q"], tracked.get("gain"), tracked.get("bias"), pairs)
    score, shift = np.full(len(keys), emba_io.MATCH_UNSCORED), np.zeros((len(keys), 2), np.int32)
    for n, p in enumerate(keys):
        if p in app:
            score[n], shift[n] = app[p]
            if source[n] == 2:
                Q0[n] = model.match_start(shift[n, 0], shift[n, 1], level, calib, (sw, sh))
    return pairs, source, Q0, a, b, score, shift


def _reached(status, edges):
    """bool [F]: the frames an anchor reaches along the edges (graph_reach of graph_rule.h)."""
    reached = np.asarray(status) == emba_io.TRACK_ANCHOR
    grew = True
    while grew:
        grew = False
        for i, j in edges:
            if reached[i] != reached[j]:
                reached[i] = reached[j] = True
                grew = True
    return reached


@dataclass
class WindowResult:
    index: int                  # count_window_
    t_beg_ns: int
    t_end_ns: int
    beg: int                    # event subset [beg, end) of the (down-sampled) sequence
    end: int
    idx_cp_beg: int             # idx_cp_traj_beg_: first control pose of the whole trajectory this window refines
    traj_init: LinearTrajectory     # the segment handed to solve_time_window
    result: object              # its LMResult
    setup_ms: float = float("nan")  # emba_last_setup_ms of the window's registration (device models)
    map_init: object = None     # SequenceSettings.init_map = "events", first window only: the LMResult of the map-only pass that preceded `result`
    contrast_init: object = None    # SequenceSettings.record_contrast: {"J", "sum", "nonzero"} of the panorama of the window's events [beg, end) at traj_init
    contrast_final: object = None   # ... and at result.traj
    refine_J_before: object = None  # SequenceSettings.refine_contrast: the smooth contrast of the window's events at the control poses as generated ...
    refine_J_after: object = None   # ... and at the refined ones, which became traj_init
    refine_evals: object = None     # ... and the evaluations of the contrast the ascent took (over all of SequenceSettings.contrast_levels; J before and after: at level 0)
    prior_events: object = None     # SequenceSettings.contrast_prior: the events retired into the priors before this window was refined (0: it climbed without one;
                                    # with one, refine_J_before / refine_J_after are the contrast against it)


@dataclass
class SequenceResult:
    traj: LinearTrajectory      # the whole trajectory (traj_ptr_)
    windows: list = field(default_factory=list)
    n_events: int = 0           # events of the sequence after down-sampling
    filter_stats: object = None # with a noise filter on: uint64[6] — events in, hot pixels, events failing hot / refractory / support, events kept
    cmax: object = None         # SequenceSettings.init_poses = "events": what estimate_angular_velocity returned (omega, t_ref_ns, J0, J, evals) + the raw
                                # poses made of it (pose_t, pose_q)
    event_panorama: object = None   # SequenceSettings.event_panorama: int64 [H, W], the panorama of the events [windows[0].beg, windows[-1].end) warped along traj
    views: object = None        # SequenceSettings.views_hz: what sequence_views returned — t_ns [F], views [F, sh, sw], u8, outside [F], lo, hi, event_frames


def keeps_sequence(model):
    """Can `model` hold the whole sequence on the device and register windows as ranges of it?  emba_amd.LEGM can; a sharded.ShardedModel says so itself
    (has_resident_sequence: only where its engine can); anything without set_sequence cannot."""
    return hasattr(model, "set_sequence") and bool(getattr(model, "has_resident_sequence", True))


def estimate_raw_poses(model, events, seq, resident_sequence):
    """SequenceSettings.init_poses = "events": the raw poses of a run from its events alone.  events: the recording as the windows will see it (a model with
    a resident sequence asks its device instead; a ShardedModel every rank's own context — every rank holds the same sequence and the rule is deterministic
    integer arithmetic, so all get the same estimate without a collective).  The integrated trajectory is
    sampled every dt_knots / 10 over [t_start, t_end], so that every knot interval has poses to fit whatever the slices' length.  Returns the dict of the
    estimate + pose_t, pose_q."""
    m, wmax = int(seq.cmax_slice_events), float(seq.cmax_omega_max)
    if resident_sequence and hasattr(model, "estimate_angular_velocity"):
        est = model.estimate_angular_velocity(m, wmax)
    else:
        lut, sw, sh = getattr(model, "bearing_lut", None), getattr(model, "sensor_w", None), getattr(model, "sensor_h", None)
        if lut is None or not sw or not sh:
            raise ValueError("init_poses = 'events' without a resident sequence needs the camera: model.bearing_lut, model.sensor_w, model.sensor_h")
        est = emba_io.estimate_angular_velocity(events, lut, sw, sh, m, wmax)
    if not len(est["omega"]):
        raise ValueError(f"init_poses = 'events': the sequence is shorter than one slice of {m} events")
    t0, t1, step = emba_io.ros_time_ns(seq.t_start), emba_io.ros_time_ns(seq.t_end), max(int(1e9 * seq.dt_knots) // 10, 1)
    pose_t, pose_q = emba_io.integrate_angular_velocity(est["omega"], est["t_ref_ns"], np.arange(t0, t1 + step, step, dtype=np.int64))
    return dict(est, pose_t=pose_t, pose_q=pose_q)


def panorama_of_events(model, events, traj, beg, end, resident_sequence, want_image=False):
    """The panorama of warped events of [beg, end) of the run's (down-sampled) sequence along traj, as LEGM.event_panorama returns it: from the model's device
    where the sequence is resident there, else by io.event_panorama on `events` with the camera and the panorama size the model knows."""
    if resident_sequence and hasattr(model, "event_panorama"):
        return model.event_panorama(traj, beg, end, want_image=want_image)
    lut, sw, sh = getattr(model, "bearing_lut", None), getattr(model, "sensor_w", None), getattr(model, "sensor_h", None)
    if lut is None or not sw or not sh:
        raise ValueError("the panorama of warped events without a resident sequence needs the camera: model.bearing_lut, model.sensor_w, model.sensor_h")
    return emba_io.event_panorama(events, lut, sw, sh, model.W, model.H, traj, beg, end)


def view_frame_times(traj, views_hz):
    """The frame times of views_hz frames per second over the time traj covers: t0, t0 + p, t0 + 2 p, ... with p = round(1e9 / views_hz) ns (at least 1),
    up to the last time the spline accepts, t0 + (K - 1) dt - 1."""
    period = max(int(round(1e9 / float(views_hz))), 1)
    t_last = int(traj.t0_ns) + (traj.size() - 1) * int(traj.dt_ns) - 1
    return np.arange(int(traj.t0_ns), t_last + 1, period, dtype=np.int64)


def sequence_views(model, events, traj, views_hz, view_events=False, boundary="dirichlet", resident_sequence=True, panorama=None):
    """Sensor views along traj: the frames the camera would have seen at view_frame_times(traj, views_hz), sampled from the intensity
    panorama of the model's resident map under `boundary` (or from `panorama` [H, W] where given), their 8-bit form with the tone of
    normalize_robust(panorama, 0.1) — constant across frames — and, with view_events, the signed event counts of the whole (down-sampled) sequence between
    consecutive frames.  On the device where the model (or the rank's model behind a sharded host) has render_views / event_frames and, for the counts, the
    sequence is resident; else by the numpy forms of emba_amd.io with the camera the model names, which need `panorama` or a model that reconstructs one.
    Returns a dict: t_ns [F], views float64 [F, sh, sw], u8 uint8 [F, sh, sw], outside int64 [F], lo, hi, event_frames int32 [F - 1, sh, sw] or None."""
    ts = view_frame_times(traj, views_hz)
    dev = model if hasattr(model, "render_views") else getattr(model, "m", None)
    if not hasattr(dev, "render_views"):
        dev = None
    if dev is not None:
        M = None if panorama is None else np.ascontiguousarray(panorama, dtype=np.float64)
        src = dev.reconstructIntensity(boundary=boundary) if M is None else M
        lo, hi = dev.normalizeRobust(src, 0.1, with_range=True)[1]
        r = dev.render_views(ts, traj.knots_xyzw, traj.t0_ns, traj.dt_ns, plane=M, boundary=boundary, lo=lo, hi=hi, want_u8=True)
        out = dict(t_ns=ts, views=r["views"], u8=r["u8"], outside=r["outside"], lo=lo, hi=hi, event_frames=None)
    else:
        lut, sw, sh = getattr(model, "bearing_lut", None), getattr(model, "sensor_w", None), getattr(model, "sensor_h", None)
        if lut is None or not sw or not sh:
            raise ValueError("sensor views without the device need the camera: model.bearing_lut, model.sensor_w, model.sensor_h")
        if panorama is None:
            if not hasattr(model, "reconstructIntensity"):
                raise ValueError("sensor views without the device need the intensity panorama: pass panorama, or a model with reconstructIntensity")
            panorama = model.reconstructIntensity(boundary=boundary)
        M = np.asarray(panorama, dtype=np.float64)
        lo, hi = emba_io.robust_range(M, 0.1)
        pm = emba_io.view_pm(lut, traj.knots_xyzw, traj.t0_ns, traj.dt_ns, ts, M.shape[1], M.shape[0])
        v, outside = emba_io.render_views(M, pm, with_outside=True)
        shape = (ts.size, int(sh), int(sw))
        out = dict(t_ns=ts, views=v.reshape(shape), u8=emba_io.view_u8(v, lo, hi, outside=outside).reshape(shape), outside=outside.sum(axis=1).astype(np.int64),
                   lo=lo, hi=hi, event_frames=None)
    if view_events and ts.size >= 1:
        if dev is not None and resident_sequence and hasattr(dev, "event_frames"):
            out["event_frames"] = dev.event_frames(0, None, ts)[0]
        else:
            sw, sh = getattr(model, "sensor_w", None), getattr(model, "sensor_h", None)
            if events is None or not sw or not sh:
                raise ValueError("event frames without a resident sequence need the events and the sensor's size: model.sensor_w, model.sensor_h")
            out["event_frames"] = emba_io.event_frames(events.x, events.y, events.polarity, events.t_ns, ts, sw, sh)[0]
    return out


def refine_window_poses(model, seg, beg, end, resident_sequence, max_iter, levels=(0,), prior_weight=None):
    """The window's initial control poses moved uphill on the smooth contrast of the window's events [beg, end) (io.refine_contrast over the model's
    contrast_gradient), the first pose held fixed: (trajectory, J before, J after, evaluations).  Only where the sequence is resident on the model's
    device: a numpy form of pm and D of its own is out of scope (so3.spline_evaluate has no Jacobian).  The end of the ascent depends on the last bits of
    J: a model that stands for several ranks brings its own refine_contrast, which leaves every rank with the same trajectory.
    levels: the schedule, coarse to fine (io.refine_contrast_levels) — J before and after at level 0, the evaluations over all levels;
    (0,) is the ascent on the panorama itself.  prior_weight: None, or the weight of the model's priors at those levels."""
    if not (resident_sequence and hasattr(model, "contrast_gradient")):
        raise ValueError("refine_contrast needs a model with the event sequence resident on its device (LEGM.set_sequence, contrast_gradient)")
    levels = tuple(int(l) for l in levels)
    kw = {} if prior_weight is None else dict(prior_weight=float(prior_weight))      # (none: the calls made before there were priors)
    if hasattr(model, "refine_contrast"):      # a host over several ranks: one rank's loop, its result on all of them (sharded.ShardedLEGM.refine_contrast)
        return model.refine_contrast(seg, beg, end, fix_first_pose=True, max_iter=int(max_iter), levels=levels, **kw)
    return emba_io.refine_contrast_levels(model, seg, beg, end, levels, pano_w=model.W, fix_first_pose=True, max_iter=int(max_iter), **kw)


def retire_events(model, knots, t0_ns, dt_ns, retired, beg, levels):
    """SequenceSettings.contrast_prior: the events [retired, beg) of the resident sequence — those no later window sees again — voted into the model's priors
    of `levels` along the WHOLE trajectory as it stands (the control poses refined so far, and the new window's as generated).  Returns the events added:
    whole batches, so the rest of fewer than 100 events waits for the next window."""
    if beg - retired < emba_io.PANO_BATCH:
        return 0
    return int(model.contrast_prior_add(LinearTrajectory(knots.copy(), t0_ns, dt_ns), retired, beg, levels=tuple(levels))["added"])


def _contrast(r):
    return {k: r[k] for k in ("J", "sum", "nonzero")}


def run_sequence(model, events, pose_t, pose_q, Gx, Gy, seq, ba=BASettings(), lm=LMSettings(), runtime_log=None, map_recorder=None, resident=True,
                 resident_sequence=None, verbose=False):
    """model: emba_amd.LEGM (or anything solve_time_window drives).  events: the whole recording (EventPacket, sorted).  pose_t [n] seconds, pose_q [n,4]
    xyzw: the raw front-end poses (io.load_poses; both None with seq.init_poses = "events": they are estimated from the events, SequenceResult.cmax).  Gx, Gy: the initial map (both None with seq.init_map = "events").  runtime_log / map_recorder: ONE object for the run — their counters run over
    the windows like the reference's function statics.  resident: as in solve_time_window.  resident_sequence: keep the sequence on the device (default:
    wherever the model can); False registers every window from a host slice (emba_set_events) instead."""
    if seq.init_map not in ("given", "events"):
        raise ValueError(f"SequenceSettings.init_map must be 'given' or 'events', not {seq.init_map!r}")
    if (Gx is None) != (Gy is None):
        raise ValueError("pass both Gx and Gy, or neither")
    if seq.init_map == "given" and Gx is None:
        raise ValueError("no initial map: pass Gx, Gy or set SequenceSettings.init_map = 'events'")
    if seq.init_map == "events" and ba.use_CG:
        raise ValueError("init_map = 'events' starts with a map-only solve, which use_CG cannot do")
    if seq.init_poses == "given" and (pose_t is None or pose_q is None):
        raise ValueError("no raw poses: pass pose_t, pose_q or set SequenceSettings.init_poses = 'events'")
    if resident_sequence is None:
        resident_sequence = keeps_sequence(model)
    if seq.contrast_prior and not seq.refine_contrast:
        raise ValueError("contrast_prior is the prior of the contrast refinement: it needs refine_contrast")
    if seq.contrast_prior and not (resident_sequence and hasattr(model, "contrast_prior_add")):
        raise ValueError("contrast_prior needs a model with the event sequence resident on its device (LEGM.set_sequence, contrast_prior_add)")

    # event down-sampling, emba.cpp:281-304
    filter_stats = None
    if seq.hot_pixel_sigma > 0 or seq.refractory_period > 0 or seq.support_time > 0:
        # sensor noise first, then the down-sampling over the survivors
        refr_ns, supp_ns = emba_io.ros_time_ns(seq.refractory_period), emba_io.ros_time_ns(seq.support_time)
        if resident_sequence:
            model.set_sequence(events, 1)
            filter_stats = model.filter_sequence(seq.hot_pixel_sigma, refr_ns, supp_ns, seq.event_sampling_rate)
            n_seq = int(filter_stats[5])
        else:
            # (a model that does not know its sensor: any size that holds every event gives the same survivors — a pixel without events supports nobody)
            sw = getattr(model, "sensor_w", None) or int(np.max(events.x, initial=0)) + 1
            sh = getattr(model, "sensor_h", None) or int(np.max(events.y, initial=0)) + 1
            events, filter_stats, _ = emba_io.filter_events(events, sw, sh, seq.hot_pixel_sigma, refr_ns, supp_ns)
            events = emba_io.downsample_events(events, seq.event_sampling_rate)
            n_seq = events.size()
            filter_stats[5] = n_seq
    elif resident_sequence:
        n_seq = model.set_sequence(events, seq.event_sampling_rate)
    else:
        events = emba_io.downsample_events(events, seq.event_sampling_rate)
        n_seq = events.size()

    cmax = None
    if seq.init_poses == "events":
        cmax = estimate_raw_poses(model, events, seq, resident_sequence)
        pose_t, pose_q = cmax["pose_t"], cmax["pose_q"]
    pose_t = np.asarray(pose_t, dtype=np.float64)
    pose_q = np.asarray(pose_q, dtype=np.float64).reshape(-1, 4)
    pose_t_ns = np.array([emba_io.ros_time_ns(t) for t in pose_t], dtype=np.int64)      # std::map<ros::Time, SO3d>, pose_manager.cpp:41-80

    # time cursors, emba.cpp:309-323
    win_size = emba_io.ros_time_ns(seq.time_window_size)
    win_stride = emba_io.ros_time_ns(seq.sliding_window_stride)
    t_BA_end = emba_io.ros_time_ns(seq.t_end)
    t_win_beg = emba_io.ros_time_ns(seq.t_start)
    t_win_end = t_win_beg + win_size
    t_pose_beg, t_pose_end = t_win_beg, t_win_end
    first_time_window = True
    count_window = 0
    cp_stride = int(round(seq.sliding_window_stride / seq.dt_knots))                     # :322 (std::round of a positive number)
    # the whole trajectory: LinearTrajectory(config) keeps t_beg.toSec() and t_beg.toNSec(), dt_ns = int64(1e9 dt_knots)   trajectory.cpp:24-39
    traj_t_beg = (t_win_beg // 1_000_000_000) + 1e-9 * (t_win_beg % 1_000_000_000)
    traj_t0_ns, traj_dt_ns = t_win_beg, int(1e9 * seq.dt_knots)
    knots = np.zeros((0, 4))
    pose_latest = None

    # median blur of the initial map, emba.cpp:357-364
    if seq.init_map == "events":
        Gx, Gy = np.zeros((model.H, model.W)), np.zeros((model.H, model.W))            # (no blur: the blur of zeros is zeros)
    elif seq.median_blur:
        if hasattr(model, "median_blur_map") and getattr(model, "has_resident_sequence", True):      # (a ShardedModel over an engine without one: numpy)
            model.upload_map(Gx, Gy)
            model.median_blur_map()
            Gx = Gy = None                                                              # "the resident map"
        else:
            Gx, Gy = emba_io.median_blur3(Gx), emba_io.median_blur3(Gy)

    out = SequenceResult(None, [], n_seq, filter_stats, cmax)
    retired_from = retired = None      # contrast_prior: the events [retired_from, retired) are in the priors
    while t_win_end < t_BA_end + 1_000_000:                                             # :406
        # :409 getEventSubset
        if resident_sequence:
            beg, end = model.sequence_window(t_win_beg, t_win_end)
            ev_win = EventWindow(beg, end)
        else:
            beg, end = emba_io.event_window(events.t_ns, t_win_beg, t_win_end)
            ev_win = emba_io.slice_events(events, beg, end)
        # :412-413 getPoseSubset: upper_bound(t_pose_beg) ... lower_bound(t_pose_end)
        sel = (pose_t_ns > t_pose_beg) & (pose_t_ns < t_pose_end)
        # :416-417 generateCtrlPosesLong over one-knot sub-intervals
        new = emba_io.generate_ctrl_poses_long(pose_t[sel], pose_q[sel], t_pose_beg * 1e-9, t_pose_end * 1e-9, seq.dt_knots, seq.dt_knots)
        if not first_time_window:                                                       # :420-428 align to the tail of the current trajectory
            R0_inv = so3.inverse(new[0])
            new = np.array([so3.mul(pose_latest, so3.mul(R0_inv, q)) for q in new])
            new = new[1:]                                                               # :441
        idx_cp_beg = count_window * cp_stride                                           # :432
        knots = np.concatenate([knots, new])                                            # :444 pushbackCtrlPoses
        # :447 cloneSegment(idx_cp_beg, size): start = int64(1e9 (t_beg + idx dt))   trajectory.cpp:61-70, 317-330
        if not idx_cp_beg < len(knots):
            raise ValueError(f"window {count_window}: no control poses behind index {idx_cp_beg}")      # CHECK_GT, trajectory.cpp:319
        seg = LinearTrajectory.from_seconds(traj_t_beg + idx_cp_beg * seq.dt_knots, seq.dt_knots, knots[idx_cp_beg:].copy())
        # :450 solveTimeWindow; the map of windows 1, 2, ... is the one the previous window left on the device
        ba_win = dataclasses.replace(ba, first_time_window=first_time_window)
        map_init = None
        rJ0 = rJ1 = r_evals = prior_events = None
        if seq.contrast_prior:       # what no later window sees again goes to the priors, along the whole trajectory as refined so far
            if retired is None:
                retired_from = retired = beg      # (nothing in front of the first window was ever placed)
            retired += retire_events(model, knots, traj_t0_ns, traj_dt_ns, retired, beg, seq.contrast_levels)
            prior_events = retired - retired_from
        if seq.refine_contrast:      # on the events alone, before any map is solved for
            seg, rJ0, rJ1, r_evals = refine_window_poses(model, seg, beg, end, resident_sequence, seq.contrast_iters, seq.contrast_levels,
                                                         seq.contrast_prior_weight if prior_events else None)
        if first_time_window and seq.init_map == "events":
            # mapping with known poses from the zero map, at the window's initial control poses; the joint solve below then starts from the resident map
            map_init = solve_time_window(model, seg, ev_win, Gx, Gy, dataclasses.replace(ba_win, refine="map"), lm, verbose=verbose, resident=resident)
            Gx = Gy = None
        res = solve_time_window(model, seg, ev_win, Gx, Gy, ba_win, lm, verbose=verbose, resident=resident, runtime_log=runtime_log, map_recorder=map_recorder)
        Gx = Gy = None
        c_init = c_final = None
        if seq.record_contrast:      # (after the solve: the calls leave the registered window and the evaluation alone, and need neither)
            c_init = _contrast(panorama_of_events(model, events, seg, beg, end, resident_sequence))
            c_final = _contrast(panorama_of_events(model, events, res.traj, beg, end, resident_sequence))
        knots[idx_cp_beg:] = res.traj.knots_xyzw                                        # :453 replaceWith
        setup_ms = model.setup_info()["set_events_ms"] if hasattr(model, "setup_info") else float("nan")
        out.windows.append(WindowResult(count_window, t_win_beg, t_win_end, beg, end, idx_cp_beg, seg, res, setup_ms, map_init, c_init, c_final, rJ0, rJ1, r_evals, prior_events))
        # :459-460 the latest pose: the whole trajectory 1 us before the window's end
        pose_latest = so3.spline_evaluate(knots, traj_t0_ns, traj_dt_ns, t_win_end - 1000)
        # :512-532 slideWindow
        t_win_beg += win_stride
        t_pose_beg = t_win_end
        t_win_end += win_stride
        t_pose_end = t_win_end
        count_window += 1
        first_time_window = False
    out.traj = LinearTrajectory(knots, traj_t0_ns, traj_dt_ns)
    if seq.event_panorama and out.windows:
        out.event_panorama = panorama_of_events(model, events, out.traj, out.windows[0].beg, out.windows[-1].end, resident_sequence, want_image=True)["image"]
    if seq.views_hz > 0 and out.windows:
        out.views = sequence_views(model, events, out.traj, seq.views_hz, seq.view_events, ba.panorama_boundary, resident_sequence)
    return out
