"""The event simulator without a GPU: the numpy form of emba_simulate_events (emba_amd.io: simulate_events, simulate_from_plane) against a
scalar loop that states the rule, what a recording must satisfy whatever made it, the new symbols of libemba_hip.so, and that numpy's own pm of every case
of tests/test_gpu_sim.py keeps clear of the pole rows."""
import inspect
import os

import numpy as np
import pytest

import sim_cases as SC
import view_cases as VC
from emba_amd import io as eio
from emba_amd import so3

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_new_symbols_resolve(hip_lib):
    from emba_amd import LEGM, _lib
    for name in ("emba_simulate_events", "emba_sim_size", "emba_sim_get", "emba_seq_from_sim"):
        assert hasattr(hip_lib, name) and name in _lib.SIGNATURES, name
    assert hip_lib.emba_abi_version() == 2
    blob = open(os.path.join(ROOT, "emba_amd", "libemba_hip.so"), "rb").read()
    for kernel in (b"emba_sim_count_kernel", b"emba_sim_emit_kernel", b"emba_sim_hikey_kernel", b"emba_sim_gather_kernel"):
        assert kernel in blob, kernel
    p = inspect.signature(LEGM.simulate_events).parameters
    assert list(p)[1:] == ["step_t_ns", "knots", "t0_ns", "dt_ns", "plane", "boundary", "c_on", "c_off", "max_per_step", "max_events"]
    assert (p["plane"].default, p["boundary"].default, p["c_off"].default, p["max_per_step"].default, p["max_events"].default) == (None, "dirichlet", None, 255, 0)
    p = inspect.signature(LEGM.simulated_events).parameters
    assert list(p)[1:] == ["beg", "end"] and (p["beg"].default, p["end"].default) == (0, None)
    assert inspect.signature(LEGM.sequence_from_simulation).parameters["sampling_rate"].default == 1
    p = inspect.signature(eio.simulate_events).parameters
    assert list(p) == ["views", "outside", "step_t_ns", "sensor_w", "c_on", "c_off", "max_per_step"] and (p["c_off"].default, p["max_per_step"].default) == (None, 255)


def random_samples(seed, F, sw, sh, amp, p_outside):
    """Samples that wander by a fraction of `amp` per step, a mask that takes pixels out for a few frames at a time, and step times a few ns apart (so
    that timestamps repeat within and across pixels)."""
    rng = np.random.default_rng(seed)
    S = sw * sh
    views = np.cumsum(rng.normal(0.0, amp, (F + 1, S)), axis=0)
    hold = rng.random((F + 1, S)) < 0.2
    views[1:][hold[1:]] = views[:-1][hold[1:]]                          # cur == prev: a step without a change, often with a carried difference
    outside = rng.random((F + 1, S)) < p_outside
    ts = 10**9 + np.concatenate([[0], np.cumsum(rng.integers(1, 6, F))]).astype(np.int64)
    return views, outside, ts


@pytest.mark.parametrize("cap", [1, 2, 255])
@pytest.mark.parametrize("seed,amp,p_outside", [(1, 0.08, 0.0), (2, 0.3, 0.1), (3, 1.5, 0.25)])
def test_the_numpy_form_is_the_stated_rule(seed, amp, p_outside, cap):
    """io.simulate_events against the scalar per-pixel loop of tests/sim_cases.py: the same events in the same order, the same stats."""
    sw, sh, F = 4, 3, 9
    views, outside, ts = random_samples(seed, F, sw, sh, amp, p_outside)
    ev, stats = eio.simulate_events(views, outside, ts, sw, SC.C_ON, SC.C_OFF, cap)
    (x, y, pol, t), want = SC.scalar_simulation(views.tolist(), outside.tolist(), ts.tolist(), sw, SC.C_ON, SC.C_OFF, cap)
    assert ev.x.dtype == np.uint16 and ev.y.dtype == np.uint16 and ev.polarity.dtype == np.uint8 and ev.t_ns.dtype == np.int64 and stats.dtype == np.uint64
    assert stats.tolist() == list(want), (stats, want)
    assert ev.x.tolist() == x and ev.y.tolist() == y and ev.polarity.tolist() == pol and ev.t_ns.tolist() == t
    # in time order, inside the steps
    assert (np.diff(ev.t_ns) >= 0).all() and (ev.size() == 0 or (ev.t_ns[0] >= ts[0] and ev.t_ns[-1] <= ts[-1] - 1))
    if amp > 1.0:
        assert (stats[2] > 0) == (cap < 255) and stats[0] > (100 if cap > 1 else 40) and (np.diff(ev.t_ns) == 0).any()
    if p_outside:
        assert stats[3] == outside.sum() > 0
    # c_off defaults to c_on
    a, sa = eio.simulate_events(views, outside, ts, sw, SC.C_ON, max_per_step=cap)
    b, sb = eio.simulate_events(views, outside, ts, sw, SC.C_ON, SC.C_ON, cap)
    assert np.array_equal(a.t_ns, b.t_ns) and np.array_equal(a.polarity, b.polarity) and sa.tolist() == sb.tolist()


def test_refusals_of_the_numpy_form():
    views, outside, ts = random_samples(5, 3, 2, 2, 0.3, 0.0)
    for bad in (dict(c_on=0.0), dict(c_on=np.inf), dict(c_on=0.1, c_off=-0.1), dict(c_on=0.1, c_off=np.nan), dict(c_on=0.1, max_per_step=0), dict(c_on=0.1, max_per_step=256)):
        with pytest.raises(ValueError):
            eio.simulate_events(views, outside, ts, 2, **bad)
    with pytest.raises(ValueError):
        eio.simulate_events(views, outside, ts[::-1], 2, 0.1)
    with pytest.raises(ValueError):
        eio.simulate_events(views[:1], outside[:1], ts[:1], 2, 0.1)          # F = 0
    with pytest.raises(ValueError):
        eio.simulate_events(views[:2], outside[:2], [0, 1 << 52], 2, 0.1)     # a span of 2^52
    eio.simulate_events(views[:2], outside[:2], [0, (1 << 52) - 1], 2, 0.1)


def recording(sensor, pano, kind, F, amp=1.0, cap=255):
    lut, plane, knots, ts = VC.lut_of(sensor), SC.plane_of(pano, amp), VC.knots_of(kind), SC.step_times(F)
    pm = eio.view_pm(lut, knots, VC.T0_NS, VC.DT_NS, ts, *pano)
    views, outside = eio.render_views(plane, pm, with_outside=True)
    ev, stats = eio.simulate_events(views, outside, ts, sensor[0], SC.C_ON, SC.C_OFF, cap)
    return views, outside, ts, ev, stats


@pytest.mark.parametrize("kind,cap", [("yaw_pi", 255), ("pitch", 255), ("yaw_pi", 2)])
def test_the_events_add_up_to_the_brightness_change(kind, cap):
    """Every pixel that is inside at every step and never capped: V_0 + c_on n_on - c_off n_off lies within max(c_on, c_off) of V_F — the reference, which
    the sums rebuild, is less than one threshold from the sample when the loop ends.  The same at the end of every step, with the events counted by
    io.event_frames between the step times.  (The reference is a sum of up to a few hundred thresholds: the rebuilt one differs from it by rounding, far
    below the 1e-9 allowed here on values of order 1.)"""
    sensor, pano, F = (16, 12), (48, 24), 65
    amp = SC.STEEP if cap < 255 else 1.0
    views, outside, ts, ev, stats = recording(sensor, pano, kind, F, amp, cap)
    S = sensor[0] * sensor[1]
    assert stats[0] > 500 and (stats[2] > 0) == (cap < 255) and (stats[3] > 0) == (kind == "pitch")
    edges = np.append(ts[:-1], ts[-1])      # the step times are the edges: every event lies in [ts[0], ts[F] - 1]
    on, off = ev.polarity == 1, ev.polarity == 0
    n_on, b1, a1 = eio.event_frames(ev.x[on], ev.y[on], ev.polarity[on], ev.t_ns[on], edges, *sensor, signed_polarity=False)
    n_off, b0, a0 = eio.event_frames(ev.x[off], ev.y[off], ev.polarity[off], ev.t_ns[off], edges, *sensor, signed_polarity=False)
    assert (b1, a1, b0, a0) == (0, 0, 0, 0) and int(n_on.sum()) == stats[1] and int(n_off.sum()) == stats[0] - stats[1]
    n_on, n_off = n_on.reshape(F, S), n_off.reshape(F, S)
    # which pixels were capped in which step: the scalar rule says so per pixel; here: a pixel is left out when it has max_per_step events in any step
    steady = ~outside.any(axis=0) & ((n_on + n_off).max(axis=0) < cap)
    assert steady.sum() > (S // 4 if cap == 255 else 4) and (cap == 255 or steady.sum() < S)
    bound = max(SC.C_ON, SC.C_OFF) + 1e-9
    rebuilt = views[0] + SC.C_ON * np.cumsum(n_on, axis=0) - SC.C_OFF * np.cumsum(n_off, axis=0)
    assert np.abs(rebuilt[-1] - views[-1])[steady].max() < bound
    assert np.abs(rebuilt - views[1:])[:, steady].max() < bound


def test_a_rolled_plane_under_a_yawed_trajectory():
    """A plane rolled by k columns seen along a trajectory yawed by 2 pi k / W is the same scene: the same pixels report the same polarities in the same
    order.  The yawed pm is numpy's own (another atan2), so the samples agree to rounding only: a timestamp, which truncates frac * d, may differ by 1 ns."""
    sensor, pano, F, k = (16, 12), (48, 24), 65, 7
    lut, plane, knots, ts = VC.lut_of(sensor), SC.plane_of(pano), VC.knots_of("yaw_pi"), SC.step_times(F)
    yaw = so3.exp(np.array([0.0, 2.0 * np.pi * k / pano[0], 0.0]))
    yawed = np.array([so3.mul(yaw, q) for q in knots])
    a, sa = eio.simulate_from_plane(plane, lut, knots, VC.T0_NS, VC.DT_NS, ts, sensor, SC.C_ON, SC.C_OFF)
    b, sb = eio.simulate_from_plane(np.roll(plane, k, axis=1), lut, yawed, VC.T0_NS, VC.DT_NS, ts, sensor, SC.C_ON, SC.C_OFF)
    assert sa.tolist() == sb.tolist() and sa[0] > 500
    # per pixel, in emission order (a stable sort by pixel of the time-ordered recording keeps each pixel's events in time order)
    for ev in (a, b):
        ev.pix = ev.y.astype(np.int64) * sensor[0] + ev.x
        ev.order = np.argsort(ev.pix, kind="stable")
    assert np.array_equal(a.pix[a.order], b.pix[b.order]) and np.array_equal(a.polarity[a.order], b.polarity[b.order])
    assert np.abs(np.sort(a.t_ns) - np.sort(b.t_ns)).max() <= 1
    c, _ = eio.simulate_from_plane(np.roll(plane, k + 1, axis=1), lut, yawed, VC.T0_NS, VC.DT_NS, ts, sensor, SC.C_ON, SC.C_OFF)
    assert c.size() != a.size() or not np.array_equal(c.polarity, a.polarity)      # (the test can fail)


def test_a_still_camera_reports_nothing():
    for sensor in VC.SENSORS:
        views, outside, ts, ev, stats = recording(sensor, (32, 16), "identity", 65, SC.STEEP)
        assert ev.size() == 0 and stats.tolist() == [0, 0, 0, 0] and ev.t_ns.dtype == np.int64 and not outside.any()


def test_numpys_pm_of_every_gpu_case_keeps_clear_of_the_pole_rows():
    """The outside decision is floor(pm_y) < 0 or floor(pm_y) + 1 > H - 1: it can differ between numpy's pm and the device's only where pm_y lies at row 0
    or row H - 1.  On every case of tests/test_gpu_sim.py numpy's pm_y keeps VC.POLE_EPS = 1e-9 clear of both (the device's differs from it by 1e-12 at
    the most, tests/test_gpu_views.py): no case depends on a last bit.  tests/test_gpu_sim.py compares given the device's own samples all the same."""
    seen = set()
    for sensor, pano, kind, dt_ns, ts in SC.gpu_cases():
        pm = eio.view_pm(VC.lut_of(sensor), VC.knots_of(kind), VC.T0_NS, dt_ns, ts, *pano)
        assert np.isfinite(pm).all() and not VC.near_pole(pm, pano[1]).any(), (sensor, pano, kind, ts.size)
        seen.add(kind)
    assert seen == set(VC.KINDS)
