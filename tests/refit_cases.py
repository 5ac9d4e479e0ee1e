"""The cases of the refit tests, shared by tests/test_refit_cpu.py (the numpy form) and tests/test_gpu_refit.py (the device against it):
out-and-back trajectories made with the generators of tests/track_cases.py — the constant-rate rotation of a tracking case run forward for half the frames and
then backward, so that the last frames see what the first saw — 64 x 48 frames on the 128 x 64 panorama.  A tracker runs first (numpy's or the device's),
the refit behind it; nothing but the frames, their times and the tracker's output reaches a refit."""
import functools

import numpy as np

import track_cases as TC
import track_exposure_cases as XC
import mosaic_cases as MC
import view_cases as VC
from emba_amd import io as eio
from emba_amd import so3

SENSOR, PANO = (64, 48), (128, 64)
SWEEPS = 2


def out_and_back(F):
    """The position of frame f along the rotation, in steps: 0, 1 ... F // 2, then back down to 1."""
    return np.array([f if f <= F // 2 else F - f for f in range(F)], dtype=np.float64)


def times(F):
    return TC.T0_NS + TC.DT_NS * np.arange(F, dtype=np.int64)


@functools.lru_cache(maxsize=None)
def case(step, F, ramp=False):
    """One case, computed once: frames uint8 [F, S] rendered at q_true [F, 4] as tests/track_cases.py renders them; with `ramp` every frame behind the anchor
    distorted by §24's brightness ramp stretched over the F frames (gain, bias: the truth).  Read-only."""
    W, H = PANO
    inten = np.exp(MC.smooth_plane(PANO))
    lo, hi = float(inten.min()), float(inten.max())
    lut = VC.lut_of(SENSOR)
    q_true = np.array([so3.mul(so3.exp(k * TC.step_angle(step, PANO) * TC.AXIS), TC.Q_START) for k in out_and_back(F)])
    pm = np.array([eio.align_warp(lut, q, W, H)[1] for q in q_true])
    views, outside = eio.render_views(inten, pm, with_outside=True)
    frames = eio.view_u8(views, lo, hi, outside=outside)
    gain = 1.0 + (XC.A_END - 1.0) * np.arange(F) / (F - 1)
    bias = -100.0 * (gain - 1.0)
    if ramp:
        out = np.zeros_like(frames)
        for f in range(F):
            v = frames[f].astype(np.float64)
            out[f] = np.where(frames[f] != 0, np.clip(np.rint((v - bias[f]) / gain[f]), 0.0, 255.0), 0.0).astype(np.uint8)
        frames = out
    else:
        gain, bias = np.ones(F), np.zeros(F)
    ts = times(F)
    for a in (frames, q_true, ts, lut, gain, bias):
        a.setflags(write=False)
    return dict(frames=frames, q_true=q_true, ts=ts, lut=lut, levels=TC.SCHEDULE[PANO], predict=TC.PREDICT[step], gain=gain, bias=bias, F=F)


def track_args(step, **kw):
    """The arguments of a tracker on a case, with the settings of tests/track_cases.py."""
    args = dict(q0=TC.Q_START, levels=TC.SCHEDULE[PANO], batch=1, predict=TC.PREDICT[step], skip_zero=True, min_weight=TC.TRACKING[(SENSOR, PANO, step)],
                min_overlap=TC.MIN_OVERLAP)
    args.update(kw)
    args.update(TC.SETTINGS)
    return args


def refit_args(step, estimate=0, **kw):
    """The arguments of a refit (numpy or device) behind that tracker."""
    args = dict(levels=TC.SCHEDULE[PANO], batch=1, sweeps=SWEEPS, alternate=True, recover=True, sweep_tol=0.0, estimate=estimate, skip_zero=True,
                min_weight=TC.TRACKING[(SENSOR, PANO, step)], min_overlap=TC.MIN_OVERLAP, **XC.BOUNDS)
    args.update(kw)
    args.update(TC.SETTINGS)
    return args


@functools.lru_cache(maxsize=None)
def track_numpy(step, F, ramp=False):
    """numpy's tracker on a case, computed once: io.track_frames, or with `ramp` io.track_frames_exposure with estimate = 3.  Read-only."""
    c = case(step, F, ramp)
    if ramp:
        return eio.track_frames_exposure(c["frames"], c["ts"], c["lut"], PANO[0], PANO[1], estimate=3, **XC.BOUNDS, **track_args(step))
    out = eio.track_frames(c["frames"], c["ts"], c["lut"], PANO[0], PANO[1], **track_args(step))
    out["gain"], out["bias"] = np.ones(F), np.zeros(F)
    return out


@functools.lru_cache(maxsize=None)
def refit_numpy(step, F, ramp=False):
    """io.refit_frames behind track_numpy, SWEEPS sweeps, computed once.  Read-only."""
    c, t = case(step, F, ramp), track_numpy(step, F, ramp)
    return eio.refit_frames(c["frames"], c["ts"], c["lut"], PANO[0], PANO[1], t["q"], t["status"], t["gain"], t["bias"], **refit_args(step, 3 if ramp else 0))


def worst_angle(step, F, q, ramp=False):
    return float(eio.rotation_angle_between(case(step, F, ramp)["q_true"], q).max())


def angle_after(step, F, sweep, ramp=False):
    """numpy's worst angle to the truth behind sweep `sweep` (0-based) of SWEEPS."""
    return E_REFIT_NP[(step, F, ramp)][sweep]


# The closing cases: (step, F, ramp).  Measured with numpy (tests/test_refit_cpu.py checks the figures): E_TRACK_NP the tracker's worst angle to the truth
# (rad), E_REFIT_NP the refit's behind each of the SWEEPS sweeps, ITERS_NP the refit's trials per level of the schedule summed over the frames, per sweep,
# CODES_NP every frame's refit code behind the last sweep.  Kept are the cases in which numpy ends with every frame behind the anchor moved or recovered.
CLOSING = (("small", 12, False), ("large", 12, False), ("small", 12, True))
E_TRACK_NP = {
    ("small", 12, False): 6.0554e-03,
    ("large", 12, False): 6.7968e-03,
    ("small", 12, True): 7.4995e-03,
}
E_REFIT_NP = {
    ("small", 12, False): (9.0518e-03, 1.0684e-02),
    ("large", 12, False): (1.0303e-02, 1.2471e-02),
    ("small", 12, True): (1.1292e-02, 1.3751e-02),
}
ITERS_NP = {
    ("small", 12, False): ((359, 151, 88, 47), (369, 123, 88, 48)),
    ("large", 12, False): ((282, 111, 45, 63), (243, 137, 73, 44)),
    ("small", 12, True): ((187, 166, 82, 43), (193, 170, 72, 43)),
}
CODES_NP = {key: (1,) + (2,) * 11 for key in CLOSING}      # the anchor, and eleven frames moved, behind either sweep
# numpy's worst |a - a*| and |b - b*| (bytes) on the ramp: the tracker's, then the refit's behind the last sweep
GAIN_NP = {("small", 12, True): dict(da_track=1.2003e-02, da_refit=1.8239e-02, db_track=1.159, db_refit=1.763)}
# The cases on which numpy's refit ends nearer to the truth than numpy's tracker did: none.  Also tried and not kept: F = 16 at either step (6.68e-03 ->
# 9.79e-03 -> 1.17e-02 rad small, 7.38e-03 -> 1.11e-02 -> 1.35e-02 large) and the ramp at the large step (6.86e-03 -> 8.81e-03 -> 1.09e-02).  In every case
# the tracker's error is a drift that grows from the anchor (0, 1.8, 2.7 ... 6 mrad) and the refit's is a common offset of all eleven frames (9 ... 11 mrad
# each, the spread among them 1.7 mrad): the frames are pulled into agreement with each other, and the one anchor among twelve does not hold the block in
# place.  Only the cases of IMPROVES carry the assertion E_REFIT_NP < E_TRACK_NP; the others assert the exactness properties and the device against numpy.
IMPROVES = ()
ITERS_SLACK_PER_FRAME = 1      # tests/track_cases.py's allowance: one trial per frame and level


def angle_bound(key, sweep):
    """The project's bound from tests/track_cases.py: the device may end at twice numpy's angle plus F tol_rot."""
    return 2.0 * E_REFIT_NP[key][sweep] + key[1] * TC.SETTINGS["tol_rot"]
