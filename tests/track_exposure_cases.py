"""The cases of the tests of the frame tracker with exposure, shared by tests/test_track_exposure_cpu.py (the numpy forms) and
tests/test_gpu_track_exposure.py (the device against them): the three kept cases of tests/track_cases.py, F = 12, with every frame behind the anchor distorted
by a known, slowly varying (a*_f, b*_f): v <- clamp(rint((v - b*) / a*)), §22's distortion, so that a* v + b* gives the rendered byte back.  A byte of 0 (a
pixel outside the panorama) stays 0: skip_zero tests the raw byte.  Frame 0 is left as it is: the anchor's tone is the gauge, and the truth of frame f is
a_f = a*_f, b_f = b*_f in byte units."""
import functools

import numpy as np

import track_cases as TC
from emba_amd import io as eio

F = TC.F
CASES = tuple(TC.TRACKING)      # ((sensor, pano, step), ...): 64 x 48 small with prediction, 64 x 48 large without, 20 x 13 large with min_weight = 32
BOUNDS = dict(gain_min=0.25, gain_max=4.0)
# The ramp: a* rises linearly from 1 (the anchor) to 1.3 (frame 11); b* = -100 (a* - 1) bytes.  A rendered byte v in 1 ... 255 becomes (v - b*) / a*, which
# has to stay within 1 ... 254: b* <= 1 - a* (true of -100 (a* - 1) for every a* >= 1) and b* >= 255 - 254 a* (true from a* >= 1 + 1 / 154 on; frame 1 has
# a* = 1.027).  tests/test_track_exposure_cpu.py checks that no used byte reaches 0 or 255.
A_END = 1.3
A_STAR = 1.0 + (A_END - 1.0) * np.arange(F) / (F - 1)
B_STAR = -100.0 * (A_STAR - 1.0)
A_STAR.setflags(write=False)
B_STAR.setflags(write=False)


def distort(frames_u8):
    """frames_u8 [F, S] with frame f distorted by (A_STAR[f], B_STAR[f]): v <- clamp(rint((v - b*) / a*), 0, 255) where v != 0, 0 where v == 0."""
    fr = np.asarray(frames_u8, dtype=np.uint8)
    out = np.zeros_like(fr)
    for f in range(fr.shape[0]):
        v = fr[f].astype(np.float64)
        out[f] = np.where(fr[f] != 0, np.clip(np.rint((v - B_STAR[f]) / A_STAR[f]), 0.0, 255.0), 0.0).astype(np.uint8)
    return out


@functools.lru_cache(maxsize=None)
def case(sensor, pano, step):
    """TC.case with `distorted` uint8 [F, S] and the truth `gain`, `bias` [F] (byte units) beside it.  Read-only."""
    c = dict(TC.case(sensor, pano, step))
    c["distorted"] = distort(c["frames"])
    c["gain"], c["bias"] = A_STAR, B_STAR
    c["distorted"].setflags(write=False)
    return c


def track_args(sensor, pano, step, **kw):
    """The arguments of a tracker (numpy or device, plain or with exposure) on a case, with the settings of tests/track_cases.py."""
    c = case(sensor, pano, step)
    args = dict(q0=TC.Q_START, levels=c["levels"], batch=1, predict=c["predict"], skip_zero=True, min_weight=TC.TRACKING[(sensor, pano, step)],
                min_overlap=TC.MIN_OVERLAP)
    args.update(kw)
    args.update(TC.SETTINGS)
    return args


@functools.lru_cache(maxsize=None)
def track_numpy(sensor, pano, step, estimate=3):
    """io.track_frames_exposure on the distorted frames of a case, computed once.  Read-only."""
    c = case(sensor, pano, step)
    return eio.track_frames_exposure(c["distorted"], c["ts"], c["lut"], pano[0], pano[1], estimate=estimate, **BOUNDS, **track_args(sensor, pano, step))


@functools.lru_cache(maxsize=None)
def track_numpy_plain(sensor, pano, step):
    """io.track_frames (no exposure) on the same distorted frames, computed once: the figure the feature is for."""
    c = case(sensor, pano, step)
    return eio.track_frames(c["distorted"], c["ts"], c["lut"], pano[0], pano[1], **track_args(sensor, pano, step))


def worst_angle(sensor, pano, step, q):
    return TC.worst_angle(sensor, pano, step, q)


# The recovery cases: those of CASES on which numpy alone (io.track_frames_exposure, estimate = 3) tracks every frame with no level ending degenerate.  All
# three survive; none was dropped.  Per case numpy's worst angle to the truth E_NP (rad), worst |a - a*| DA_NP and worst |b - b*| DB_NP (bytes) over the twelve
# frames, and its trials per level of the schedule summed over the frames ITERS_NP — the measured yardsticks of tests/test_gpu_track_exposure.py, which allows
# the device 2 E_NP + F tol_rot, twice DA_NP and DB_NP, and ITERS_SLACK = F trials per level (tests/track_cases.py gives the reasons).
# E_PLAIN: the worst angle of plain io.track_frames on the same distorted frames — what the tracker without exposure does to them.
E_NP = {
    ((64, 48), (128, 64), "small"): 6.7226e-03,
    ((64, 48), (128, 64), "large"): 1.1986e-02,
    ((20, 13), (128, 64), "large"): 2.1773e-02,
}
DA_NP = {
    ((64, 48), (128, 64), "small"): 1.7285e-02,
    ((64, 48), (128, 64), "large"): 6.2284e-02,
    ((20, 13), (128, 64), "large"): 5.4188e-02,
}
DB_NP = {
    ((64, 48), (128, 64), "small"): 9.9217e-01,
    ((64, 48), (128, 64), "large"): 3.0489e+00,
    ((20, 13), (128, 64), "large"): 2.5211e+00,
}
ITERS_NP = {
    ((64, 48), (128, 64), "small"): (334, 140, 91, 67),
    ((64, 48), (128, 64), "large"): (340, 209, 118, 60),
    ((20, 13), (128, 64), "large"): (330, 210, 108, 126),
}
# Plain tracking keeps every frame "tracked" on all three — it has no way to know — and ends 0.12 ... 0.25 rad from the truth: the brightness ramp is turned
# into rotation, 10 to 37 times the error of the tracker with exposure.
E_PLAIN = {
    ((64, 48), (128, 64), "small"): 2.4688e-01,
    ((64, 48), (128, 64), "large"): 1.2425e-01,
    ((20, 13), (128, 64), "large"): 1.9754e-01,
}
ITERS_SLACK = TC.ITERS_SLACK
RECOVERY = tuple(E_NP)


def angle_bound(key):
    return 2.0 * E_NP[key] + F * TC.SETTINGS["tol_rot"]
