"""Sensor views along the trajectory on the MI355X (include/emba_hip.h: emba_render_views, emba_seq_event_frames) against the numpy forms of
the same rules (emba_amd.io: render_views, view_u8, view_pm, event_frames).  Given the call's own pm_out the frames and their bytes are compared with
array_equal — a difference is a bug in one of the two forms, never a tolerance; pm_out and the frames against numpy's own pm under the suite's assert_close,
less the pixels whose numpy pm_y lies within 1e-9 of row 0 or row H - 1 (tests/test_views_cpu.py: on these cases there is none).  The event frames are
integers.  Then the resident map as the source, what a call leaves alone, and every refusal."""
import ctypes as C

import numpy as np
import pytest

import view_cases as VC
from emba_amd import io as eio
from emba_amd import synth
from emba_amd.legm import EventPacket, EventWindow
from helpers import assert_close

pytestmark = pytest.mark.gpu
ERR_INVALID_ARG, ERR_TIME_RANGE, ERR_STATE = 1, 4, 5
LEFT_OUT_CAP = 1e-3        # at most 0.1 % of a frame's pixels may be left out of the comparison with numpy's own pm
FILL = -3.5
_dp, _u8p, _i32p, _i64p, _u64p = (C.POINTER(t) for t in (C.c_double, C.c_uint8, C.c_int32, C.c_int64, C.c_uint64))


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


def raw_render(m, plane, boundary, ts, knots, t0, dt, fill, lo, hi, views, u8, outside, pm, K=None):
    """emba_render_views itself, on the caller's (pre-filled) arrays: the status."""
    return m._L.emba_render_views(m._ctx, ptr(plane, _dp), boundary, ptr(ts, _i64p), ts.size, ptr(knots, _dp), knots.shape[0] if K is None else K, t0, dt, fill, lo, hi,
                                  ptr(views, _dp), ptr(u8, _u8p), ptr(outside, _u64p), ptr(pm, _dp))


@pytest.mark.parametrize("pano", VC.PANOS, ids=lambda p: f"pano{p[1]}x{p[0]}")
@pytest.mark.parametrize("sensor", VC.SENSORS, ids=lambda s: f"sensor{s[0]}x{s[1]}")
def test_views_against_the_numpy_forms(gpu, sensor, pano):
    W, H = pano
    S = sensor[0] * sensor[1]
    lut, plane = VC.lut_of(sensor), VC.plane_of(pano)
    m = make_legm(sensor, pano)
    m.set_option("poison", 1)      # a cell of a frame that is read before it is written shows
    for kind in VC.KINDS:
        knots = VC.knots_of(kind)
        for F in VC.FRAMES:
            ts = VC.frame_times(F)
            lo, hi = (0.5, 0.5) if (kind == "identity" and F == 3) else (-2.0, 1.5)      # one case at lo == hi
            r = m.render_views(ts, knots, VC.T0_NS, VC.DT_NS, plane=plane, fill=FILL, lo=lo, hi=hi, want_u8=True, want_pm=True)
            what = f"{kind}, F = {F}"
            assert r["views"].shape == (F, sensor[1], sensor[0]) and r["u8"].shape == r["views"].shape and r["pm"].shape == (F, S, 2) and r["outside"].shape == (F,)
            # 1. given the device's pm: the same bits
            v_np, out_np = eio.render_views(plane, r["pm"], fill=FILL, with_outside=True)
            assert np.array_equal(r["views"].reshape(F, S).view(np.uint64), v_np.view(np.uint64)), what
            assert np.array_equal(r["u8"].reshape(F, S), eio.view_u8(v_np, lo, hi, outside=out_np)), what
            assert np.array_equal(r["outside"], out_np.sum(axis=1)), what
            # 2. against numpy's own pm, less the pixels numpy puts within 1e-9 of a pole row
            pm_np = eio.view_pm(lut, knots, VC.T0_NS, VC.DT_NS, ts, W, H)
            left_out = VC.near_pole(pm_np, H)
            assert (left_out.sum(axis=1) <= LEFT_OUT_CAP * S).all(), what
            keep = ~left_out
            assert_close(r["pm"][keep], pm_np[keep], f"view_pm against numpy's ({what})")
            v_own, out_own = eio.render_views(plane, pm_np, fill=FILL, with_outside=True)
            assert_close(r["views"].reshape(F, S)[keep], v_own[keep], f"views against numpy's own pm ({what})")
            # 3. the outside pixels, under the same exclusion
            assert np.array_equal(r["outside"] - (out_np & left_out).sum(axis=1), (out_own & keep).sum(axis=1)), what
            if kind == "pitch":
                assert (r["outside"] > 0).all() and (r["outside"] < S).all() and (r["views"] == FILL).any() and (r["u8"].reshape(F, S)[out_np] == 0).all()
            else:
                assert not r["outside"].any()
            if kind == "yaw_pi":
                assert (r["pm"][..., 0] < 1.0).any() or (r["pm"][..., 0] >= W - 1.0).any()      # patches that cross the seam themselves
    # outputs asked for one at a time give the same as all together
    ts, knots = VC.frame_times(3), VC.knots_of("pitch")
    every = m.render_views(ts, knots, VC.T0_NS, VC.DT_NS, plane=plane, fill=FILL, lo=-2.0, hi=1.5, want_u8=True, want_pm=True)
    outside = np.full(3, 99, np.uint64)
    assert raw_render(m, plane, 0, ts, knots, VC.T0_NS, VC.DT_NS, FILL, 0.0, 1.0, None, None, outside, None) == 0 and np.array_equal(outside.astype(np.int64), every["outside"])
    u8 = np.full((3, S), 7, np.uint8)
    assert raw_render(m, plane, 0, ts, knots, VC.T0_NS, VC.DT_NS, FILL, -2.0, 1.5, None, u8, None, None) == 0 and np.array_equal(u8, every["u8"].reshape(3, S))
    m.close()


def test_time_range_and_the_other_refusals_of_render_views(gpu):
    from emba_amd import EmbaError
    sensor, pano = (16, 12), (32, 16)
    S = 16 * 12
    m = make_legm(sensor, pano)
    plane, knots = VC.plane_of(pano), VC.knots_of("yaw_pi")
    views, u8, outside, pm = np.full((3, S), 4.25), np.full((3, S), 9, np.uint8), np.full(3, 5, np.uint64), np.full((3, S, 2), -1.5)

    def untouched():
        return (views == 4.25).all() and (u8 == 9).all() and (outside == 5).all() and (pm == -1.5).all()
    args = (FILL, -2.0, 1.5, views, u8, outside, pm)
    # one frame beyond the last time the numpy spline accepts; one in front of the first knot
    with pytest.raises(ValueError):
        eio.view_pm(VC.lut_of(sensor), knots, VC.T0_NS, VC.DT_NS, [VC.T_LAST_NS + 1], *pano)
    for bad_t in (VC.T_LAST_NS + 1, VC.T0_NS - 1):
        ts = np.array([VC.T0_NS, bad_t, VC.T_LAST_NS], np.int64)
        assert raw_render(m, plane, 0, ts, knots, VC.T0_NS, VC.DT_NS, *args) == ERR_TIME_RANGE and untouched()
        with pytest.raises(EmbaError) as ei:
            m.render_views(ts, knots, VC.T0_NS, VC.DT_NS, plane=plane)
        assert ei.value.status == ERR_TIME_RANGE
    ts = np.array([VC.T0_NS, VC.T0_NS + 5, VC.T_LAST_NS], np.int64)
    assert raw_render(m, plane, 0, ts, knots, VC.T0_NS, VC.DT_NS, *args, K=1) == ERR_INVALID_ARG and untouched()          # K < 2
    assert raw_render(m, plane, 0, ts, knots, VC.T0_NS, 0, *args) == ERR_INVALID_ARG and untouched()                        # dt = 0
    assert raw_render(m, plane, 0, ts, None, VC.T0_NS, VC.DT_NS, *args, K=4) == ERR_INVALID_ARG and untouched()             # knots NULL
    assert m._L.emba_render_views(m._ctx, ptr(plane, _dp), 0, None, 3, ptr(knots, _dp), 4, VC.T0_NS, VC.DT_NS, FILL, -2.0, 1.5, ptr(views, _dp), None, None, None) == ERR_INVALID_ARG
    assert raw_render(m, plane, 0, ts, knots, VC.T0_NS, VC.DT_NS, FILL, np.nan, 1.5, views, u8, outside, pm) == ERR_INVALID_ARG and untouched()   # the tone's limits
    assert raw_render(m, None, 0, ts, knots, VC.T0_NS, VC.DT_NS, *args) == ERR_STATE and untouched()                        # no plane and no map
    assert raw_render(m, None, 7, ts, knots, VC.T0_NS, VC.DT_NS, *args) == ERR_INVALID_ARG and untouched()                  # ... and no such boundary
    # F = 0, and every output NULL: nothing happens
    assert raw_render(m, plane, 0, ts[:0], knots, VC.T0_NS, VC.DT_NS, *args) == 0 and untouched()
    assert raw_render(m, plane, 0, ts, knots, VC.T0_NS, VC.DT_NS, FILL, -2.0, 1.5, None, None, None, None) == 0
    r0 = m.render_views(ts[:0], knots, VC.T0_NS, VC.DT_NS, plane=plane, want_u8=True, lo=0.0, hi=1.0, want_pm=True)
    assert r0["views"].shape == (0, 12, 16) and r0["pm"].shape == (0, S, 2)
    # the context is still usable
    assert raw_render(m, plane, 0, ts, knots, VC.T0_NS, VC.DT_NS, *args) == 0 and not untouched()
    assert np.array_equal(views, eio.render_views(plane, pm, fill=FILL)) and not outside.any()
    with pytest.raises(ValueError):
        m.render_views(ts, knots, VC.T0_NS, VC.DT_NS, plane=plane[:, :-1])
    with pytest.raises(ValueError):
        m.render_views(ts, knots, VC.T0_NS, VC.DT_NS, plane=plane, boundary="periodic")
    m.close()


def solved_step(m, w):
    """One evaluation, the equations, a solve and the trial map of emba_update_map on the scene."""
    m.evaluateDataError(w.traj, w.Gx, w.Gy)
    m.formNormalEq(None, w.K, None, w.thres_valid_pixel)
    m.applyL2Reg(w.alpha)
    _, x2 = m.solveNormalEq(1e-2, fix_first_pose=True)
    m.updateMap(x2, 1.0)


def test_the_resident_map_as_the_source(gpu, scene):
    """plane_host = NULL after emba_update_map: the frames are samples of the M emba_reconstruct_intensity_bc gives for the map the next evaluation reads,
    under both boundaries, and the default tone is normalizeRobust's of that M."""
    w = scene
    m = make_legm((64, 48), (512, 256), lut=w.lut)
    m.set_events(w.events)
    solved_step(m, w)
    t_end = w.traj.t0_ns + w.traj.dt_ns * (w.K - 1) - 1
    ts = np.array([w.traj.t0_ns, (w.traj.t0_ns + t_end) // 2, t_end], np.int64)
    M = {}
    for boundary in ("dirichlet", "wrap"):
        M[boundary] = m.reconstructIntensity(boundary=boundary)
        r = m.render_views(ts, w.traj.knots_xyzw, w.traj.t0_ns, w.traj.dt_ns, boundary=boundary, want_u8=True, want_pm=True)
        v_np, out_np = eio.render_views(M[boundary], r["pm"], with_outside=True)
        assert np.array_equal(r["views"].reshape(3, -1), v_np) and not r["outside"].any() and np.abs(v_np).max() > 0
        lo, hi = m.normalizeRobust(M[boundary], with_range=True)[1]
        assert np.array_equal(r["u8"].reshape(3, -1), eio.view_u8(v_np, lo, hi, outside=out_np)) and len(np.unique(r["u8"])) > 20
        # a plane given by the caller goes before the map
        ones = m.render_views(ts, w.traj.knots_xyzw, w.traj.t0_ns, w.traj.dt_ns, plane=np.ones((256, 512)), boundary=boundary)
        assert (ones["views"] == 1.0).all()
    assert not np.array_equal(M["dirichlet"], M["wrap"])
    m.rejectMap()
    m.close()


def test_a_call_in_between_changes_nothing(gpu, scene):
    """The panorama of warped events and a step evaluation after emba_render_views (both sources) and emba_seq_event_frames: bit-equal to the same calls on a
    context that never made them."""
    w = scene
    t_end = w.traj.t0_ns + w.traj.dt_ns * (w.K - 1) - 1
    ts = np.array([w.traj.t0_ns, t_end], np.int64)
    got = []
    for between in (False, True):
        m = make_legm((64, 48), (512, 256), lut=w.lut)
        n = m.set_sequence(w.events)
        m.set_events(EventWindow(0, n))
        m.upload_map(w.Gx, w.Gy)
        first = m.step(w.traj, w.thres_valid_pixel, w.alpha)
        if between:
            m.render_views(ts, w.traj.knots_xyzw[:3], w.traj.t0_ns, 4 * w.traj.dt_ns, plane=w.Gx, want_u8=True, lo=-1.0, hi=1.0, want_pm=True)      # (other knots than the calls around it)
            m.event_frames(100, n - 50, np.array([w.traj.t0_ns, (w.traj.t0_ns + t_end) // 2, t_end], np.int64))
        pano = m.event_panorama(w.traj, 300, 20000, signed=True, want_pm=True)
        if between:
            m.render_views(ts, w.traj.knots_xyzw, w.traj.t0_ns, w.traj.dt_ns, boundary="wrap")
            m.event_frames(0, n, np.array([t_end - 5, t_end], np.int64), signed_polarity=False)
        second = m.step(w.traj, w.thres_valid_pixel, w.alpha)
        got.append((first, pano, second, m.get_ep(), m.last_counts(), m.event_counts()))
        m.close()
    a, b = got
    assert a[0] == b[0] and a[2] == b[2] and a[4] == b[4] and a[5] == b[5] and a[0][0] > 1000
    assert np.array_equal(a[3].view(np.uint64), b[3].view(np.uint64))
    assert np.array_equal(a[1]["image"], b[1]["image"]) and np.array_equal(a[1]["pm"].view(np.uint64), b[1]["pm"].view(np.uint64))
    assert all(a[1][k] == b[1][k] for k in ("J", "sum", "nonzero", "dropped"))


def synthetic_events(n, sensor, seed):
    rng = np.random.default_rng(seed)
    t = 10**9 + np.sort(rng.integers(0, 40_000, n)).astype(np.int64)      # repeated timestamps among them
    return EventPacket(rng.integers(0, sensor[0], n).astype(np.uint16), rng.integers(0, sensor[1], n).astype(np.uint16), rng.integers(0, 2, n).astype(np.uint8), t)


@pytest.mark.parametrize("F", [1, 2, 65])
@pytest.mark.parametrize("n,sensor", [(300, (7, 5)), (2000, (20, 13))], ids=["300ev_7x5", "2000ev_20x13"])
def test_event_frames_are_the_numpy_integers(gpu, n, sensor, F):
    ev = synthetic_events(n, sensor, seed=n + F)
    m = make_legm(sensor, (32, 16))
    m.set_option("poison", 1)
    assert m.set_sequence(ev) == n
    # the edges take in exact event timestamps: the first edge is event n / 10's own time, the last one event 9 n / 10's
    inner = np.unique(ev.t_ns[n // 10: 9 * n // 10])
    edges = inner[(np.arange(F + 1) * (inner.size - 1)) // F]
    assert edges.size == F + 1 and (np.diff(edges) > 0).all() and edges[0] == ev.t_ns[n // 10] and edges[-1] == ev.t_ns[9 * n // 10 - 1]
    for signed in (True, False):
        for beg, end in ((0, n), (n // 20 + 3, n - n // 20 - 4)):      # the whole sequence, and a range inside it that is no multiple of 100
            frames, before, after = m.event_frames(beg, end, edges, signed_polarity=signed)
            want, wb, wa = eio.event_frames(ev.x[beg:end], ev.y[beg:end], ev.polarity[beg:end], ev.t_ns[beg:end], edges, sensor[0], sensor[1], signed)
            assert frames.dtype == np.int32 and frames.shape == (F, sensor[1], sensor[0]) and np.array_equal(frames, want)
            assert (before, after) == (wb, wa) and before > 0 and after > 0
            assert int(np.abs(frames).sum()) <= end - beg - before - after
            if not signed:
                assert int(frames.sum()) == end - beg - before - after and (frames >= 0).all()
            else:
                assert (frames < 0).any()
    m.close()


def test_refusals_of_event_frames(gpu):
    from emba_amd import EmbaError
    sensor, n = (7, 5), 300
    ev = synthetic_events(n, sensor, seed=1)
    m = make_legm(sensor, (32, 16))
    frames, before, after = np.full((2, 35), 11, np.int32), C.c_uint64(77), C.c_uint64(78)

    def call(beg, end, edges, F=None):
        e = np.ascontiguousarray(edges, dtype=np.int64)
        return m._L.emba_seq_event_frames(m._ctx, beg, end, ptr(e, _i64p), e.size - 1 if F is None else F, 1, ptr(frames, _i32p), C.byref(before), C.byref(after))

    def untouched():
        return (frames == 11).all() and before.value == 77 and after.value == 78
    good = [10**9, 10**9 + 20_000, 10**9 + 40_000]
    assert call(0, 0, good) == ERR_STATE and untouched()                       # no resident sequence
    with pytest.raises(EmbaError) as ei:
        m.event_frames(0, 0, good)
    assert ei.value.status == ERR_STATE
    m.set_sequence(ev)
    assert call(0, n + 1, good) == ERR_INVALID_ARG and untouched()             # end > n
    assert call(5, 4, good) == ERR_INVALID_ARG and untouched()                 # beg > end
    assert call(0, n, [good[0], good[0], good[2]]) == ERR_INVALID_ARG and untouched()      # an edge repeated
    assert call(0, n, [good[0], good[2], good[1]]) == ERR_INVALID_ARG and untouched()      # an edge going back
    assert m._L.emba_seq_event_frames(m._ctx, 0, n, None, 2, 1, ptr(frames, _i32p), C.byref(before), C.byref(after)) == ERR_INVALID_ARG and untouched()
    assert m._L.emba_seq_event_frames(m._ctx, 0, n, ptr(np.array(good, np.int64), _i64p), 2, 1, None, None, None) == 0 and untouched()      # nothing asked for
    # the context is still usable: an empty range, F = 0, and the call itself
    assert call(17, 17, good) == 0 and not frames.any() and (before.value, after.value) == (0, 0)
    fr, b, a = m.event_frames(0, n, [10**9 + 20_000])
    assert fr.shape == (0, 5, 7) and b + a == n and b == int((ev.t_ns < 10**9 + 20_000).sum())
    assert call(0, n, good) == 0
    want, wb, wa = eio.event_frames(ev.x, ev.y, ev.polarity, ev.t_ns, good, 7, 5, True)
    assert np.array_equal(frames.reshape(2, 5, 7), want) and (before.value, after.value) == (wb, wa)
    m.free_sequence()
    assert call(0, 0, good) == ERR_STATE
    m.close()
