"""The event simulator on the MI355X (include/emba_hip.h: emba_simulate_events, emba_sim_size, emba_sim_get, emba_seq_from_sim) against the
numpy form of the same rule (emba_amd.io.simulate_events).  The samples are the device's own: emba_render_views at the step times with a NaN fill gives the
views and, as the NaN cells, the outside mask (checked against its outside_out); given those, the recording and its stats are compared with array_equal,
order included — a difference is a bug in one of the two forms, never a tolerance.  Then the capacity limit, every refusal, the resident map as the source,
the way into the resident sequence, and what a call leaves alone."""
import ctypes as C

import numpy as np
import pytest

import sim_cases as SC
import view_cases as VC
from emba_amd import io as eio
from emba_amd import synth
from emba_amd.legm import EventWindow

pytestmark = pytest.mark.gpu
ERR_INVALID_ARG, ERR_TIME_RANGE, ERR_STATE, ERR_CAPACITY = 1, 4, 5, 6
_dp, _u8p, _u16p, _i64p, _u64p = (C.POINTER(t) for t in (C.c_double, C.c_uint8, C.c_uint16, C.c_int64, C.c_uint64))


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from emba_amd import build
    build.build_hip()
    return True


@pytest.fixture(scope="module")
def scene():
    return synth.make_scene_workload()          # 64x48 on 256x512, K = 6: 38 965 events


def make_legm(sensor, pano, lut=None):
    from emba_amd import LEGM
    return LEGM(sensor[0], sensor[1], VC.lut_of(sensor) if lut is None else lut, 0.2, pano[0], pano[1], device=0)


def ptr(a, ty):
    return None if a is None else a.ctypes.data_as(ty)


def device_samples(m, ts, knots, t0, dt, plane=None, boundary="dirichlet"):
    """The samples the simulator sees, through emba_render_views: views [F + 1, S] and the outside mask."""
    r = m.render_views(ts, knots, t0, dt, plane=plane, boundary=boundary, fill=np.nan)
    views = r["views"].reshape(ts.size, -1)
    outside = np.isnan(views)
    assert np.array_equal(outside.sum(axis=1), r["outside"])      # (the planes are finite: a NaN is the fill)
    return views, outside


def same_recording(got, want):
    return (np.array_equal(got.t_ns, want.t_ns) and np.array_equal(got.x, want.x) and np.array_equal(got.y, want.y) and np.array_equal(got.polarity, want.polarity)
            and got.t_ns.dtype == np.int64 and got.x.dtype == np.uint16 and got.polarity.dtype == np.uint8)


def check_against_numpy(m, sensor, ts, knots, dt, plane, cap=255, what=""):
    views, outside = device_samples(m, ts, knots, VC.T0_NS, dt, plane)
    want, want_stats = eio.simulate_events(views, outside, ts, sensor[0], SC.C_ON, SC.C_OFF, cap)
    stats = m.simulate_events(ts, knots, VC.T0_NS, dt, plane=plane, c_on=SC.C_ON, c_off=SC.C_OFF, max_per_step=cap)
    print(f"{what}: stats {stats.tolist()} numpy {want_stats.tolist()}")
    assert stats.dtype == np.uint64 and stats.tolist() == want_stats.tolist(), what
    assert m.simulated_size() == want.size()
    assert same_recording(m.simulated_events(), want), what
    return want, stats


@pytest.mark.parametrize("pano", VC.PANOS, ids=lambda p: f"pano{p[1]}x{p[0]}")
@pytest.mark.parametrize("sensor", VC.SENSORS, ids=lambda s: f"sensor{s[0]}x{s[1]}")
def test_recordings_against_the_numpy_form(gpu, sensor, pano):
    S = sensor[0] * sensor[1]
    plane, steep = SC.plane_of(pano), SC.plane_of(pano, SC.STEEP)
    m = make_legm(sensor, pano)
    m.set_option("poison", 1)      # an event that is read before it is written shows
    for kind in VC.KINDS:
        knots = VC.knots_of(kind)
        for F in SC.STEPS:
            ts = SC.step_times(F)
            want, stats = check_against_numpy(m, sensor, ts, knots, VC.DT_NS, plane, what=f"{kind}, F = {F}")
            if kind == "identity":      # a still camera: no event, through every call
                assert stats.tolist() == [0, 0, 0, 0] and m.simulated_size() == 0 and m.simulated_events().size() == 0 and m.simulated_events(0, 0).size() == 0
                assert m.sequence_from_simulation() == 0 and m.sequence_size() == 0
            else:
                assert stats[0] >= 3 * S and 0 < stats[1] < stats[0] and stats[2] == 0      # several events per pixel, both polarities
                assert (stats[3] > 0) == (kind == "pitch")
                assert (np.diff(want.t_ns) >= 0).all() and want.t_ns[0] >= ts[0] and want.t_ns[-1] <= ts[-1] - 1
    # the cap at 1 and at 2 on the steep plane: what is left over is carried into the next step
    for cap in (1, 2):
        for kind in ("yaw_pi", "pitch"):
            _, stats = check_against_numpy(m, sensor, SC.step_times(3), VC.knots_of(kind), VC.DT_NS, steep, cap=cap, what=f"{kind}, steep, cap {cap}")
            assert stats[2] > 0 and stats[0] > S
    m.close()


def test_a_chunk_longer_than_2_32_ns_takes_two_sorts(gpu):
    sensor, pano = VC.SENSORS[1], VC.PANOS[0]
    m = make_legm(sensor, pano)
    ts = SC.step_times(3, SC.LONG_DT_NS)
    assert ts[-1] - ts[0] > 1 << 32
    want, stats = check_against_numpy(m, sensor, ts, VC.knots_of("yaw_pi"), SC.LONG_DT_NS, SC.plane_of(pano), what="6 s")
    assert stats[0] > 500 and (want.t_ns - ts[0] >= 1 << 32).any() and (want.t_ns - ts[0] < 1 << 32).any()
    m.close()


def test_steps_across_a_chunk_edge(gpu):
    """260 pixels, three steps more than one chunk of 32 MiB of samples holds: the pixels' state, the frame between the chunks and the recording's growth."""
    sensor, pano = VC.SENSORS[2], VC.PANOS[0]
    S = sensor[0] * sensor[1]
    F = SC.chunk_edge_steps(S)
    assert F * S * 8 > SC.CHUNK_BYTES >= (F - 3) * S * 8 > SC.CHUNK_BYTES - S * 8
    m = make_legm(sensor, pano)
    m.set_option("poison", 1)
    ts = SC.step_times(F)
    want, stats = check_against_numpy(m, sensor, ts, VC.knots_of("pitch"), VC.DT_NS, SC.plane_of(pano, SC.STEEP), what=f"pitch, F = {F}")
    assert stats[0] > 100_000 and stats[3] > 0 and (want.t_ns >= ts[F - 3]).sum() >= 10      # events in the second chunk too
    _, outside = device_samples(m, ts, VC.knots_of("pitch"), VC.T0_NS, VC.DT_NS, SC.plane_of(pano))
    assert (outside[:-1] & ~outside[1:]).any() and (~outside[:-1] & outside[1:]).any()      # pixels leave over the pole row and come back: disarmed, armed again
    m.close()


def test_capacity(gpu):
    from emba_amd import EmbaError
    sensor, pano = (16, 12), (32, 16)
    m = make_legm(sensor, pano)
    plane, ts = SC.plane_of(pano), SC.step_times(3)
    first, _ = check_against_numpy(m, sensor, ts, VC.knots_of("pitch"), VC.DT_NS, plane, what="pitch")
    want, want_stats = check_against_numpy(m, sensor, ts, VC.knots_of("yaw_pi"), VC.DT_NS, plane, what="yaw_pi")
    n = want.size()
    assert n > 100 and n != first.size()
    m.simulate_events(ts, VC.knots_of("yaw_pi"), VC.T0_NS, VC.DT_NS, plane=plane, c_on=SC.C_ON, c_off=SC.C_OFF, max_events=n)      # exactly enough
    assert same_recording(m.simulated_events(), want)
    # one below: refused, stats[0] is the number needed, the recording before is still there
    first_stats = m.simulate_events(ts, VC.knots_of("pitch"), VC.T0_NS, VC.DT_NS, plane=plane, c_on=SC.C_ON, c_off=SC.C_OFF)
    stats = np.full(4, 77, np.uint64)
    knots = VC.knots_of("yaw_pi")
    st = m._L.emba_simulate_events(m._ctx, ptr(plane, _dp), 0, ptr(ts, _i64p), 3, ptr(knots, _dp), VC.K, VC.T0_NS, VC.DT_NS, SC.C_ON, SC.C_OFF, 255, n - 1, ptr(stats, _u64p))
    assert st == ERR_CAPACITY and stats.tolist() == [n, 77, 77, 77]
    assert m.simulated_size() == first.size() == first_stats[0] and same_recording(m.simulated_events(), first)
    with pytest.raises(EmbaError) as ei:
        m.simulate_events(ts, knots, VC.T0_NS, VC.DT_NS, plane=plane, c_on=SC.C_ON, c_off=SC.C_OFF, max_events=1)
    assert ei.value.status == ERR_CAPACITY and ei.value.needed == n
    assert same_recording(m.simulated_events(), first)
    assert same_recording(m.simulated_events(5, 17), type(first)(first.x[5:17], first.y[5:17], first.polarity[5:17], first.t_ns[5:17]))
    m.close()


def test_refusals(gpu, scene):
    sensor, pano = (16, 12), (32, 16)
    m = make_legm(sensor, pano)
    plane, knots, ts = SC.plane_of(pano), VC.knots_of("yaw_pi"), SC.step_times(3)
    stats = np.full(4, 55, np.uint64)
    x, y, pol, t = np.full(8, 3, np.uint16), np.full(8, 4, np.uint16), np.full(8, 5, np.uint8), np.full(8, 6, np.int64)
    n_out = C.c_size_t(99)

    def sim(plane=plane, boundary=0, ts=ts, F=None, knots=knots, K=VC.K, t0=VC.T0_NS, dt=VC.DT_NS, c_on=SC.C_ON, c_off=SC.C_OFF, cap=255, max_events=0):
        return m._L.emba_simulate_events(m._ctx, ptr(plane, _dp), boundary, ptr(ts, _i64p), (ts.size - 1) if F is None else F, ptr(knots, _dp), K, t0, dt, c_on, c_off, cap,
                                         max_events, ptr(stats, _u64p))

    def get(beg, end):
        return m._L.emba_sim_get(m._ctx, beg, end, ptr(x, _u16p), ptr(y, _u16p), ptr(pol, _u8p), ptr(t, _i64p))

    def untouched():
        return (stats == 55).all() and (x == 3).all() and (y == 4).all() and (pol == 5).all() and (t == 6).all() and n_out.value == 99

    def refusals(have):
        """Every refusal, with the outputs pre-filled; `have`: the recording (or None) that must still be there afterwards."""
        assert sim(knots=None) == ERR_INVALID_ARG and untouched()
        assert sim(ts=None, F=3) == ERR_INVALID_ARG and untouched()
        assert sim(F=0) == ERR_INVALID_ARG and untouched()
        assert sim(K=1) == ERR_INVALID_ARG and untouched()
        assert sim(dt=0) == ERR_INVALID_ARG and untouched()
        assert sim(ts=np.array([ts[0], ts[2], ts[1], ts[3]], np.int64)) == ERR_INVALID_ARG and untouched()      # going back
        assert sim(ts=np.array([ts[0], ts[1], ts[1], ts[3]], np.int64)) == ERR_INVALID_ARG and untouched()      # repeated
        for bad in (0.0, -0.1, np.inf, np.nan):
            assert sim(c_on=bad) == ERR_INVALID_ARG and untouched() and sim(c_off=bad) == ERR_INVALID_ARG and untouched()
        assert sim(cap=0) == ERR_INVALID_ARG and untouched() and sim(cap=256) == ERR_INVALID_ARG and untouched()
        for bad in ([VC.T0_NS, VC.T0_NS + 5, VC.T_LAST_NS + 1], [VC.T0_NS - 1, VC.T0_NS + 5, VC.T_LAST_NS]):      # behind the last knot's span, in front of the first knot
            assert sim(ts=np.array(bad, np.int64)) == ERR_TIME_RANGE and untouched()
        assert sim(plane=None) == ERR_STATE and untouched()                        # no plane and no map
        assert sim(plane=None, boundary=7) == ERR_INVALID_ARG and untouched()      # ... and no such boundary
        if have is None:
            assert get(0, 0) == ERR_STATE and untouched()
            assert m._L.emba_sim_size(m._ctx, C.byref(n_out)) == ERR_STATE and untouched()
            assert m._L.emba_seq_from_sim(m._ctx, 1, C.byref(n_out)) == ERR_STATE and untouched()
        else:
            assert get(0, have.size() + 1) == ERR_INVALID_ARG and get(5, 4) == ERR_INVALID_ARG and untouched()
            assert m.simulated_size() == have.size() and same_recording(m.simulated_events(), have)

    refusals(None)
    # a resident sequence, a registered window and an evaluation: what a refusal must leave alone
    w = scene
    m2 = make_legm((64, 48), (512, 256), lut=w.lut)
    n = m2.set_sequence(w.events)
    m2.set_events(EventWindow(0, n))
    m2.upload_map(w.Gx, w.Gy)
    first = m2.step(w.traj, w.thres_valid_pixel, w.alpha)
    bad_ts = np.array([w.traj.t0_ns - 1, w.traj.t0_ns + 10], np.int64)
    from emba_amd import EmbaError
    with pytest.raises(EmbaError) as ei:
        m2.simulate_events(bad_ts, w.traj.knots_xyzw, w.traj.t0_ns, w.traj.dt_ns, plane=w.Gx, c_on=0.1)
    assert ei.value.status == ERR_TIME_RANGE and m2.sequence_size() == n
    assert m2.step(w.traj, w.thres_valid_pixel, w.alpha) == first
    m2.close()
    # the context is still usable, and with a recording the refusals leave it alone
    have, _ = check_against_numpy(m, sensor, ts, knots, VC.DT_NS, plane, what="after the refusals")
    stats[:] = 55
    refusals(have)
    assert get(2, 10) == 0 and np.array_equal(t, have.t_ns[2:10]) and np.array_equal(x, have.x[2:10]) and np.array_equal(pol, have.polarity[2:10])
    assert m._L.emba_sim_get(m._ctx, 0, have.size(), None, None, None, None) == 0
    m.close()


def solved_step(m, w):
    """One evaluation, the equations, a solve and the trial map of emba_update_map on the scene."""
    m.evaluateDataError(w.traj, w.Gx, w.Gy)
    m.formNormalEq(None, w.K, None, w.thres_valid_pixel)
    m.applyL2Reg(w.alpha)
    _, x2 = m.solveNormalEq(1e-2, fix_first_pose=True)
    m.updateMap(x2, 1.0)


def test_the_resident_map_as_the_source(gpu, scene):
    """plane_host = NULL: the recording is that of the M emba_reconstruct_intensity_bc gives for the map the next evaluation reads, handed in as a plane —
    under both boundaries."""
    w = scene
    m = make_legm((64, 48), (512, 256), lut=w.lut)
    m.set_events(w.events)
    solved_step(m, w)
    t_end = w.traj.t0_ns + w.traj.dt_ns * (w.K - 1) - 1
    ts = w.traj.t0_ns + (np.arange(5, dtype=np.int64) * (t_end - w.traj.t0_ns)) // 4
    args = (ts, w.traj.knots_xyzw, w.traj.t0_ns, w.traj.dt_ns)
    sizes = []
    for boundary in ("dirichlet", "wrap"):
        M = m.reconstructIntensity(boundary=boundary)
        c_on = 0.02 * float(M.max() - M.min())
        s_map = m.simulate_events(*args, boundary=boundary, c_on=c_on, c_off=0.8 * c_on)
        from_map = m.simulated_events()
        s_plane = m.simulate_events(*args, plane=M, c_on=c_on, c_off=0.8 * c_on)
        assert s_map.tolist() == s_plane.tolist() and s_map[0] > 1000 and same_recording(from_map, m.simulated_events())
        views, outside = device_samples(m, ts, w.traj.knots_xyzw, w.traj.t0_ns, w.traj.dt_ns, boundary=boundary)
        want, want_stats = eio.simulate_events(views, outside, ts, 64, c_on, 0.8 * c_on)
        assert same_recording(from_map, want) and want_stats.tolist() == s_map.tolist()
        sizes.append(int(s_map[0]))
    m.rejectMap()
    m.close()


@pytest.mark.parametrize("rate", [1, 3])
def test_the_recording_becomes_the_resident_sequence(gpu, rate):
    sensor, pano = VC.SENSORS[2], VC.PANOS[1]
    m = make_legm(sensor, pano)
    m.simulate_events(SC.step_times(65), VC.knots_of("yaw_pi"), VC.T0_NS, VC.DT_NS, plane=SC.plane_of(pano), c_on=SC.C_ON, c_off=SC.C_OFF)
    rec = m.simulated_events()
    assert rec.size() > 1000
    n_kept = m.sequence_from_simulation(rate)
    fresh = make_legm(sensor, pano)
    assert fresh.set_sequence(rec, rate) == n_kept == rec.size() // rate == m.sequence_size()
    assert same_recording(m.sequence_events(0, n_kept), fresh.sequence_events(0, n_kept))
    assert same_recording(m.simulated_events(), rec)      # the simulated recording itself stays
    # the sequence is a sequence like any other: its windows register
    m.set_events(EventWindow(0, n_kept))
    fresh.set_events(EventWindow(0, n_kept))
    assert m.event_counts() == fresh.event_counts()
    m.close()
    fresh.close()


def test_a_call_in_between_changes_nothing(gpu, scene):
    """The panorama of warped events and a step evaluation after emba_simulate_events (both sources), emba_sim_get and emba_sim_size: bit-equal to the same
    calls on a context that never made them."""
    w = scene
    t_end = w.traj.t0_ns + w.traj.dt_ns * (w.K - 1) - 1
    ts = w.traj.t0_ns + (np.arange(4, dtype=np.int64) * (t_end - w.traj.t0_ns)) // 3
    got = []
    for between in (False, True):
        m = make_legm((64, 48), (512, 256), lut=w.lut)
        n = m.set_sequence(w.events)
        m.set_events(EventWindow(0, n))
        m.upload_map(w.Gx, w.Gy)
        first = m.step(w.traj, w.thres_valid_pixel, w.alpha)
        if between:
            s = m.simulate_events(ts[:2], w.traj.knots_xyzw[:3], w.traj.t0_ns, 4 * w.traj.dt_ns, plane=w.Gx, c_on=0.05, c_off=0.04, max_per_step=3)      # (other knots than the calls around it)
            assert s[0] > 0 and m.simulated_events().size() == s[0]
        pano = m.event_panorama(w.traj, 300, 20000, signed=True, want_pm=True)
        if between:
            M = m.reconstructIntensity(boundary="wrap")
            s = m.simulate_events(ts, w.traj.knots_xyzw, w.traj.t0_ns, w.traj.dt_ns, boundary="wrap", c_on=0.05 * float(M.max() - M.min()))
            assert s[0] > 0 and m.simulated_size() == s[0] and m.sequence_size() == n
        second = m.step(w.traj, w.thres_valid_pixel, w.alpha)
        got.append((first, pano, second, m.get_ep(), m.last_counts(), m.event_counts()))
        m.close()
    a, b = got
    assert a[0] == b[0] and a[2] == b[2] and a[4] == b[4] and a[5] == b[5] and a[0][0] > 1000
    assert np.array_equal(a[3].view(np.uint64), b[3].view(np.uint64))
    assert np.array_equal(a[1]["image"], b[1]["image"]) and np.array_equal(a[1]["pm"].view(np.uint64), b[1]["pm"].view(np.uint64))
    assert all(a[1][k] == b[1][k] for k in ("J", "sum", "nonzero", "dropped"))
