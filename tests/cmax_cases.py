"""What the contrast-maximisation tests share (tests/test_cmax_cpu.py, tests/test_gpu_cmax.py): the recordings, the simulator's true body rate and the
error bounds.  Every bound is twice the worst error the NUMPY form (emba_amd.io.estimate_angular_velocity) made on the CPU on exactly these inputs
(DESIGN.md §11 has the figures); the device form is bit-equal to it, so the margin covers nothing on the device — it only guards against reseeding."""
import numpy as np

from emba_amd import so3, synth
from emba_amd.legm import EventPacket

OMEGA_MAX = 8.0


def body_rate(traj, t_ns):
    """The true body-frame angular velocity of the linear SO(3) spline at t: log(R_i^-1 R_i+1) / dt inside knot interval i."""
    i = min(int((int(t_ns) - traj.t0_ns) // traj.dt_ns), traj.size() - 2)
    k = traj.knots_xyzw
    return so3.log(so3.mul(so3.inverse(k[i]), k[i + 1])) / (traj.dt_ns * 1e-9)


def slice_errors(omega, t_ns, m, traj):
    """|omega_s - true body rate at the middle of slice s's time span| per slice."""
    t = np.asarray(t_ns)
    return np.array([np.linalg.norm(omega[s] - body_rate(traj, (int(t[s * m]) + int(t[(s + 1) * m - 1])) // 2)) for s in range(len(omega))])


# The 64x48 default scene of synth.make_scene_workload: true body rate per knot interval about (+-1.74, 0.46, +-0.5 ... 1.0) rad/s, |w| 1.1 - 1.9 rad/s —
# 0.4 - 0.6 px of motion inside a slice of 777 events, 1.0 - 1.45 px inside one of 2000.  On this simulator's events J at the true rate lies BELOW J(0)
# (also for longer slices with 5 - 6 px of motion; cause not established), so the errors are as large as the rates or larger.  Worst error of
# the numpy form per slice length, rad/s:
SCENE_WORST = {2000: 15.154539971319863, 777: 21.916651244241176}
SCENE_BOUND = {m: 2.0 * e for m, e in SCENE_WORST.items()}


def constant_rate_events(omega, sensor=(64, 48), focal=60.0, n_points=150, n_events=6000, t_span_ns=150_000_000, seed=17):
    """Events of n_points fixed scene points seen by a camera that turns at the constant body rate omega: event k is a random point at a random time t_k,
    at the pixel its bearing exp(-omega t_k) b falls into.  Returns (EventPacket sorted by time, lut)."""
    sw, sh = sensor
    rng = np.random.default_rng(seed)
    lut = synth.pinhole_bearing_lut(sw, sh, focal, focal, sw / 2.0, sh / 2.0)
    # points spread over a field somewhat wider than the sensor's, so that some enter and leave
    P = np.stack([rng.uniform(-0.8, 0.8, n_points), rng.uniform(-0.6, 0.6, n_points), np.ones(n_points)], axis=1)
    t = np.sort(rng.integers(1_000_000_000, 1_000_000_000 + t_span_ns, size=n_events)).astype(np.int64)
    j = rng.integers(0, n_points, size=n_events)
    xs, ys, ts = [], [], []
    for tk, jk in zip(t, j):
        R = synth._quat_to_R(so3.exp(-np.asarray(omega) * ((tk - 1_000_000_000) * 1e-9)))
        b = R @ P[jk]
        if b[2] <= 0:
            continue
        x, y = int(np.rint(focal * b[0] / b[2] + sw / 2.0)), int(np.rint(focal * b[1] / b[2] + sh / 2.0))
        if 0 <= x < sw and 0 <= y < sh:
            xs.append(x); ys.append(y); ts.append(tk)
    n = len(ts)
    return EventPacket(np.array(xs, np.uint16), np.array(ys, np.uint16), rng.integers(0, 2, n).astype(np.uint8), np.array(ts, np.int64)), lut


CONST_OMEGA = np.array([0.4, -2.0, 0.9])
CONST_SLICE = 1000
CONST_WORST = 0.16842099365434116      # rad/s, worst of the three slices of 1000 events (|omega| = 2.2 rad/s: about ten pixels of motion inside a slice)
CONST_BOUND = 2.0 * CONST_WORST
