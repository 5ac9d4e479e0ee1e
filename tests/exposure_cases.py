"""The cases of the per-frame exposure tests, shared by tests/test_exposure_cpu.py (the numpy forms) and tests/test_gpu_exposure.py (the device
against them): the sensors, panoramas, trajectory kinds, frames, start rotations and settings of tests/align_cases.py, with every frame's bytes distorted by a
known (a*, b*): v <- clamp(rint((v - b*) / a*)), so that a* v + b* gives the rendered byte back.  A byte of 0 (a pixel outside the panorama) stays 0: skip_zero
tests the raw byte."""
import functools

import numpy as np

import align_cases as AC
from emba_amd import io as eio

SENSORS, PANOS, KINDS = AC.SENSORS, AC.PANOS, AC.KINDS
F = AC.CONVERGENCE_F                        # three frames per kind
PERTURB, SETTINGS = AC.PERTURB, AC.SETTINGS
BOUNDS = dict(gain_min=0.25, gain_max=4.0)
# (a*, b*) of the three frames, b* in bytes.  A rendered byte v in 1 ... 255 becomes (v - b*) / a*, which has to stay within 1 ... 254: b* <= 1 - a* and
# b* >= 255 - 254 a*, so a* > 1 — a distortion that compresses the bytes.  tests/test_exposure_cpu.py checks that no used byte reaches 0 or 255.
DISTORTION = ((1.10, -12.0), (1.25, -40.0), (1.45, -70.0))


def distort(frames_u8, distortion=DISTORTION):
    """frames_u8 [F, S] with frame f distorted by distortion[f % len]: v <- clamp(rint((v - b*) / a*), 0, 255) where v != 0, 0 where v == 0."""
    fr = np.asarray(frames_u8, dtype=np.uint8)
    out = np.zeros_like(fr)
    for f in range(fr.shape[0]):
        a, b = distortion[f % len(distortion)]
        v = fr[f].astype(np.float64)
        out[f] = np.where(fr[f] != 0, np.clip(np.rint((v - b) / a), 0.0, 255.0), 0.0).astype(np.uint8)
    return out


def truth(c, n):
    """(a* [n], b [n]): the gain and the bias IN THE PLANE'S UNITS that undo the distortion of n frames of case c.  With I0 = lo + v' (hi - lo) / 255 of the
    distorted byte v' and v = a* v' + b*, lo + v (hi - lo) / 255 = a* I0 + (lo (1 - a*) + b* (hi - lo) / 255)."""
    d = np.array([DISTORTION[f % len(DISTORTION)] for f in range(n)])
    return d[:, 0], c["lo"] * (1.0 - d[:, 0]) + d[:, 1] * (c["hi"] - c["lo"]) / 255.0


@functools.lru_cache(maxsize=None)
def case(sensor, pano, kind, n=F):
    """AC.case with `distorted` uint8 [n, S] and the truth `gain`, `bias` [n] (plane units) beside it.  Read-only."""
    c = dict(AC.case(sensor, pano, kind, n))
    c["distorted"] = distort(c["frames"])
    c["gain"], c["bias"] = truth(c, n)
    for k in ("distorted", "gain", "bias"):
        c[k].setflags(write=False)
    return c


# The recovery cases: the (sensor, panorama) pairs on which the numpy form alone (io.align_frames_exposure, estimate = 3, from PERTURB, gain 1 and bias 0)
# ends every frame of every kind converged and, under plain io.align_frames, leaves the distorted frames further from the truth than under estimate = 3.
# Per pair numpy's worst final angle to the truth E_NP (rad), worst |a - a*| and worst |b - b| (plane units) over the kinds and frames — the measured
# yardsticks of tests/test_gpu_exposure.py, which allows the device twice each (and tol_rot on the angle).  DROPPED: the pairs left out, with the reason.
E_NP = {
    ((7, 5), (32, 16)): 3.0537e-03,
    ((7, 5), (48, 24)): 3.9226e-03,
    ((7, 5), (128, 64)): 3.0874e-03,
    ((20, 13), (32, 16)): 1.7526e-03,
    ((20, 13), (48, 24)): 1.3087e-03,
    ((20, 13), (128, 64)): 1.1140e-03,
    ((64, 48), (32, 16)): 3.8587e-04,
    ((64, 48), (48, 24)): 2.3874e-04,
}
DA_NP = {
    ((7, 5), (32, 16)): 5.2588e-03,
    ((7, 5), (48, 24)): 5.4188e-03,
    ((7, 5), (128, 64)): 4.0712e-03,
    ((20, 13), (32, 16)): 2.1964e-03,
    ((20, 13), (48, 24)): 3.3869e-03,
    ((20, 13), (128, 64)): 1.5348e-03,
    ((64, 48), (32, 16)): 5.7619e-04,
    ((64, 48), (48, 24)): 1.0630e-03,
}
DB_NP = {
    ((7, 5), (32, 16)): 7.8430e-03,
    ((7, 5), (48, 24)): 7.6813e-03,
    ((7, 5), (128, 64)): 4.0421e-03,
    ((20, 13), (32, 16)): 1.1226e-03,
    ((20, 13), (48, 24)): 3.3771e-03,
    ((20, 13), (128, 64)): 1.5492e-03,
    ((64, 48), (32, 16)): 7.4428e-04,
    ((64, 48), (48, 24)): 1.4762e-03,
}
DROPPED = {
    ((64, 48), (128, 64)): "yaw_pi, frame 0: numpy's loop ends stalled after 15 trials (1.9e-4 rad from the truth, as close as its converged neighbours)",
}
KEPT = tuple(sorted(E_NP))
