"""The cases of the sensor-view tests, shared by tests/test_views_cpu.py (the numpy forms; that numpy's own pm keeps clear of the pole rows)
and tests/test_gpu_views.py (the device against them): small sensors behind a wide pinhole, small panoramas, three kinds of trajectory and frame times on
the first knot, inside the segments and at the last time the numpy spline accepts."""
import numpy as np

from emba_amd import so3, synth

SENSORS = ((7, 5), (16, 12), (20, 13))      # sensor_w x sensor_h; the last is 260 pixels: it crosses a 256-thread workgroup
PANOS = ((32, 16), (48, 24))                # pano_w x pano_h
FRAMES = (1, 3, 65)
K, T0_NS, DT_NS = 4, 1_000_000_000, 10_000_000
T_LAST_NS = T0_NS + (K - 1) * DT_NS - 1     # so3.spline_evaluate raises from T_LAST_NS + 1 on (s + 2 > K): the limit is the numpy form's
POLE_EPS = 1e-9                             # a numpy pm_y this close to 0 or H - 1 is left out of the comparison with the device: the outside test can flip there
# The lower pole is pm_y = H: a view pitched by -1.3 rad looks 74 degrees down, and a sensor whose vertical half angle is 30 degrees or more reaches over it.
PITCH = -1.3


def lut_of(sensor):
    """A wide pinhole: focal length half the sensor's width, 90 degrees across."""
    sw, sh = sensor
    return synth.pinhole_bearing_lut(sw, sh, 0.5 * sw, 0.5 * sw, 0.5 * (sw - 1), 0.5 * (sh - 1))


def knots_of(kind):
    """K control poses: 'identity'; 'yaw_pi', turning through a yaw of pi, so the view straddles the seam; 'pitch', tilted over the lower pole and turning."""
    if kind == "identity":
        return np.tile(np.array([0.0, 0.0, 0.0, 1.0]), (K, 1))
    if kind == "yaw_pi":
        return np.array([so3.exp(np.array([0.0, np.pi - 0.05 + 0.04 * i, 0.0])) for i in range(K)])
    if kind == "pitch":
        return np.array([so3.mul(so3.exp(np.array([0.0, 0.3 * i, 0.0])), so3.exp(np.array([PITCH + 0.03 * i, 0.0, 0.0]))) for i in range(K)])
    raise ValueError(kind)


KINDS = ("identity", "yaw_pi", "pitch")


def frame_times(F):
    """F frame times: the first knot, inside the segments, the last accepted time (F = 1: inside a segment; F = 2 would be the two ends)."""
    if F == 1:
        return np.array([T0_NS + (137 * DT_NS) // 100], dtype=np.int64)
    t = T0_NS + (np.arange(F, dtype=np.int64) * (T_LAST_NS - T0_NS)) // (F - 1)
    assert t[0] == T0_NS and t[-1] == T_LAST_NS and (np.diff(t) > 0).all()
    return t


def plane_of(pano, seed=3):
    W, H = pano
    return np.random.default_rng(seed).standard_normal((H, W))


def near_pole(pm, H):
    """The pixels whose pm_y lies within POLE_EPS of row 0 or row H - 1."""
    y = pm[..., 1]
    return (np.abs(y) <= POLE_EPS) | (np.abs(y - (H - 1)) <= POLE_EPS)
