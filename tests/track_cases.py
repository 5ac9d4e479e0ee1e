"""The cases of the frame-tracking tests, shared by tests/test_track_cpu.py (the numpy forms) and tests/test_gpu_track.py (the device against
them): frames made by io.render_views and io.view_u8 of exp of the smooth plane of tests/mosaic_cases.py, F = 12 of them along a rotation at a constant rate
about a fixed oblique axis, behind the wide pinhole of tests/view_cases.py.  Nothing but the frames, their times and the first rotation reaches a tracker."""
import functools

import numpy as np

import mosaic_cases as MC
import view_cases as VC
from emba_amd import io as eio
from emba_amd import so3

F = 12
SENSORS = ((20, 13), (64, 48))
PANOS = ((32, 16), (128, 64))
AXIS = np.array([0.25, 1.0, 0.15]) / np.linalg.norm([0.25, 1.0, 0.15])      # mostly yaw: the view keeps clear of the poles over all twelve frames
Q_START = so3.exp(np.array([0.1, -0.4, 0.05]))                              # frame 0's rotation: the q0 a tracker is given
T0_NS, DT_NS = 1_000_000_000, 20_000_000
# Step sizes, in level-0 cells of the panorama per frame (a cell is 2 pi / W rad of yaw), chosen on the CPU with the numpy tracker (tests/test_track_cpu.py):
#   small   half a level-0 cell per frame: inside the basin of a bilinear sample at level 0
#   large   several level-0 cells per frame, and at most half a cell of the coarsest scheduled level (2 cells of 4 on 32 x 16, 3 cells of 8 on 128 x 64)
STEP_CELLS = {"small": {(32, 16): 0.5, (128, 64): 0.5}, "large": {(32, 16): 2.0, (128, 64): 3.0}}
STEPS = ("small", "large")
SCHEDULE = {(32, 16): (2, 1, 0), (128, 64): (3, 2, 1, 0)}      # coarse to fine; 32 x 16 has levels up to 2 (level 2 is 8 x 4 cells)
MIN_OVERLAP = 0.3
SETTINGS = dict(max_iters=40, lambda0=1e-3, lambda_up=10.0, lambda_down=10.0, lambda_min=1e-9, lambda_max=1e6, tol_rot=1e-6, min_pixels=16, huber_k=0.0)
# The large cases are tracked WITHOUT prediction: with it a constant rate is predicted exactly from the third frame on; without it every frame starts a
# whole step away from where it belongs.
PREDICT = {"small": True, "large": False}

# The tracking cases: (sensor, panorama, step) -> min_weight, on which the numpy tracker under SCHEDULE keeps every frame tracked with its overlap above
# MIN_OVERLAP.  All eight combinations were run, with min_weight 256 and 32 and the schedules (0,), (1, 0), (2, 1, 0), (3, 2, 1, 0) and their coarse heads:
#   * 20 x 13 on 128 x 64: 260 pixels spread over some 670 level-0 cells, so no cell reaches one pixel's worth of weight: min_weight = 32 there.  The small step
#     still loses frames at level 0 under every schedule (the anchor alone covers too little) and is left out.
#   * everything on 32 x 16 is left out: the plane's terms of period W / 2 and W / 3 are 4 and 2.7 cells long at level 2, the coarse levels alias and end
#     up to 2 rad off, and level 0 alone drifts by 0.1 ... 0.25 rad (half a cell and more) — no yardstick a device could be held to within a factor of 2.
#     The 32 x 16 panorama still serves every test of the seam (votes, evaluation, determinism, independence), where tracking quality does not enter.
# E_NP: numpy's worst angle to the truth (rad) over the twelve frames — the measured yardstick of tests/test_gpu_track.py, which allows the device
# 2 E_NP + F tol_rot.  What is left is the drift of a frame aligned to a mosaic that is blurred by its own sixteenths-of-a-cell votes.
TRACKING = {
    ((64, 48), (128, 64), "small"): 256,
    ((64, 48), (128, 64), "large"): 256,
    ((20, 13), (128, 64), "large"): 32,
}
E_NP = {
    ((64, 48), (128, 64), "small"): 6.9498e-03,
    ((64, 48), (128, 64), "large"): 1.0900e-02,
    ((20, 13), (128, 64), "large"): 1.6349e-02,
}
# ITERS_NP: numpy's trials per level of SCHEDULE, summed over the twelve frames.  The angle to the truth does not tell the schedules apart on this plane
# (below), the trials do: a level that starts where the coarser one ended needs fewer of them (the counts fall from level to level), and a tracker that ran the
# levels in another order, or started a level anywhere but where the previous one ended, would not reproduce them — numpy under the reversed schedule differs
# from these by more than ITERS_SLACK at some level on every case (tests/test_track_cpu.py).  tests/test_gpu_track.py holds the device to them within
# ITERS_SLACK = F trials per level: both forms follow the same rule from pm that differ in their last bits, so an accept / reject decision near a tie may fall
# the other way and cost its frame a trial or two; one trial per frame is the allowance.
ITERS_NP = {
    ((64, 48), (128, 64), "small"): (317, 230, 187, 84),
    ((64, 48), (128, 64), "large"): (379, 301, 97, 54),
    ((20, 13), (128, 64), "large"): (420, 228, 171, 88),
}
ITERS_SLACK = F
# The large cases on which the schedule (0,) alone ends worse than SCHEDULE by a margin visible in numpy: none.  On 128 x 64 the plane's shortest term has a
# period of W / 3 = 43 cells, so a level-0 sample 3 cells off still has a gradient towards the minimum and (0,) ends at the same angle as the coarse-to-fine
# schedule (1.0903e-02 against 1.0900e-02 rad for 64 x 48, 1.7531e-02 against 1.6349e-02 for 20 x 13: 7 per cent, inside the factor 2 of the device's
# bound); a step large enough to leave that basin exceeds half a cell of level 3.  Both were dropped for that reason.  Larger steps and deeper schedules
# were tried as well — 6, 8, 10 and 12 cells per frame under (3, 2, 1, 0), (4, 3, 2, 1, 0) and (5, 4, 3, 2, 1, 0): wherever (0,) loses frames the coarse
# schedules lose them too, the schedules from level 4 on lose frames at every step (4 x 8 cells and fewer hold too little of this plane), and at 12 cells
# (3, 2, 1, 0) ends 3.1 rad off where (0,) ends at 1.6e-02.  On the prescribed plane numpy never shows (0,) losing to a coarse-to-fine schedule.
COARSE_BEATS_FINE = ()


def step_angle(step, pano):
    return STEP_CELLS[step][pano] * 2.0 * np.pi / pano[0]


def true_rotations(step, pano):
    """q [F, 4]: exp(f * angle * AXIS) (x) Q_START."""
    return np.array([so3.mul(so3.exp(f * step_angle(step, pano) * AXIS), Q_START) for f in range(F)])


def times():
    return T0_NS + DT_NS * np.arange(F, dtype=np.int64)


@functools.lru_cache(maxsize=None)
def case(sensor, pano, step):
    """One case, computed once: a dict of frames uint8 [F, S] rendered at q_true [F, 4], ts, lut, the schedule and predict.  Read-only."""
    W, H = pano
    inten = np.exp(MC.smooth_plane(pano))
    lo, hi = float(inten.min()), float(inten.max())
    lut = VC.lut_of(sensor)
    q_true = true_rotations(step, pano)
    pm = np.array([eio.align_warp(lut, q, W, H)[1] for q in q_true])
    views, outside = eio.render_views(inten, pm, with_outside=True)
    frames = eio.view_u8(views, lo, hi, outside=outside)
    ts = times()
    for a in (frames, q_true, ts, lut):
        a.setflags(write=False)
    return dict(frames=frames, q_true=q_true, ts=ts, lut=lut, levels=SCHEDULE[pano], predict=PREDICT[step], outside=int(outside.sum()))


def track_numpy(sensor, pano, step, levels=None, **kw):
    """io.track_frames on a case with the settings of this file."""
    c = case(sensor, pano, step)
    args = dict(q0=Q_START, levels=c["levels"] if levels is None else levels, batch=1, predict=c["predict"], skip_zero=True,
                min_weight=TRACKING.get((sensor, pano, step), 256), min_overlap=MIN_OVERLAP)
    args.update(kw)
    return eio.track_frames(c["frames"], c["ts"], c["lut"], pano[0], pano[1], **args, **SETTINGS)


def worst_angle(sensor, pano, step, q):
    return float(eio.rotation_angle_between(case(sensor, pano, step)["q_true"], q).max())
