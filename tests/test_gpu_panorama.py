"""The panorama of warped events on the MI355X (include/emba_hip.h: emba_seq_event_panorama) against the numpy form of the same rule
(emba_amd.io.event_panorama).  The votes are integers: given the call's own pm_out the image, J, sum, nonzero and dropped are compared with array_equal — a
difference is a bug in one of the two forms, never a tolerance.  pm_out itself is compared with the oracle's pm under the suite's element bound, and the
device image with the image of the oracle's pm by its L1 distance.  Then ranges, the wrap, the poles, contention, the statuses and the driver."""
import ctypes as C

import numpy as np
import pytest

from emba_amd import io as eio
from emba_amd import so3, synth
from emba_amd.driver import SequenceSettings, run_sequence
from emba_amd.legm import EventPacket, EventWindow, LinearTrajectory
from emba_amd.solver import BASettings, LMSettings
from helpers import assert_close_elementwise

pytestmark = pytest.mark.gpu
ERR_INVALID_ARG, ERR_TIME_RANGE, ERR_STATE = 1, 4, 5
W, H = 512, 256

# L1 distance between the device's image and the image of the oracle's pm as a share of the total votes (256 per event), measured once on the MI355X on
# synth.make_scene_workload(): 0.  The device's pm differs from the oracle's in the last bits (ocml's atan2 / asin / sin / cos against
# glibc's: at most 5.7e-14 px here); a vote moves only where a coordinate lies that close to a sixteenth of a pixel, and on this recording none does.  The
# asserted bound is ten times the measurement — here: equality — and never above 1e-3: a half-pixel or axis error moves essentially every vote, a share
# of order one.
DEVICE_SHARE_MEASURED = 0.0
DEVICE_SHARE_BOUND = min(10.0 * DEVICE_SHARE_MEASURED, 1e-3)


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


@pytest.fixture(scope="module")
def oracle_pm(scene, oracle_mod):
    """pm of every used event of the scene along its trajectory, by the oracle: computed once, never written."""
    ev = scene.events
    o = oracle_mod.OracleLEGM(scene.sensor_w, scene.sensor_h, W, H, scene.lut, scene.C_th)
    pm = o.count_map(scene.traj.knots_xyzw, scene.traj.t0_ns, scene.traj.dt_ns, ev.x, ev.y, ev.t_ns, want_pm=True)[2][:ev.size() // 100 * 100]
    pm.setflags(write=False)
    return pm


def make_legm(lut, sensor=(64, 48)):
    from emba_amd import LEGM
    return LEGM(sensor[0], sensor[1], lut, 0.2, W, H, device=0)


def turned(traj, w):
    """The trajectory with every control pose turned by exp(w) in the world frame."""
    return LinearTrajectory(np.array([so3.mul(so3.exp(np.asarray(w, dtype=np.float64)), q) for q in traj.knots_xyzw]), traj.t0_ns, traj.dt_ns)


def assert_exact(got, ev, beg, end, signed):
    """Everything the call returned equals the numpy rule applied to the call's own pm."""
    want = eio.event_panorama(ev, None, 64, 48, W, H, None, beg, end, signed, pm=got["pm"])
    assert got["image"].shape == (H, W) and np.array_equal(got["image"], want["image"])
    for k in ("J", "sum", "nonzero", "dropped"):
        assert got[k] == want[k], (k, got[k], want[k])
    return want


@pytest.mark.parametrize("signed", [False, True])
def test_exact_accumulation(gpu, scene, signed):
    m = make_legm(scene.lut)
    n = m.set_sequence(scene.events)
    got = m.event_panorama(scene.traj, 0, n, signed=signed, want_pm=True)
    assert got["pm"].shape == (n // 100 * 100, 2) and np.isfinite(got["pm"]).all()
    assert_exact(got, scene.events, 0, n, signed)
    assert got["dropped"] == 0 and got["nonzero"] > 1000 and got["J"] > 0
    if signed:
        assert (got["image"] < 0).any() and abs(got["sum"]) < 256 * got["pm"].shape[0]
    else:
        assert got["sum"] == 256 * got["pm"].shape[0] and (got["image"] >= 0).all()
    # the scalars alone, and the image alone: the same numbers
    lean = m.event_panorama(scene.traj, 0, n, signed=signed, want_image=False)
    assert lean["image"] is None and lean["pm"] is None and all(lean[k] == got[k] for k in ("J", "sum", "nonzero", "dropped"))
    img = np.empty((H, W), np.int32)
    knots = np.ascontiguousarray(scene.traj.knots_xyzw)
    st = m._L.emba_seq_event_panorama(m._ctx, 0, n, knots.ctypes.data_as(C.POINTER(C.c_double)), 6, scene.traj.t0_ns, scene.traj.dt_ns, int(signed),
                                      img.ctypes.data_as(C.POINTER(C.c_int32)), None, None, None, None, None)
    assert st == 0 and np.array_equal(img, got["image"])
    m.close()


def test_pm_against_the_oracle(gpu, scene, oracle_pm):
    m = make_legm(scene.lut)
    n = m.set_sequence(scene.events)
    pm = m.event_panorama(scene.traj, 0, n, want_image=False, want_pm=True)["pm"]
    e = assert_close_elementwise(pm, oracle_pm, "pano_pm against the oracle's pm")
    print(f"pm_out against the oracle: worst element {e:.3e} relative, max |diff| {np.abs(pm - oracle_pm).max():.3e} px")
    m.close()


def test_a_range_inside_the_sequence(gpu, scene, oracle_mod):
    """[300, 2850): 2500 events are used, in the range's own batches [300 + 100 b, 400 + 100 b) — the same result, bit for bit, as a fresh upload of that
    slice, and the pm the oracle gives the slice (whose batches begin at the slice's first event)."""
    beg, end = 300, 2850
    ev = scene.events
    m = make_legm(scene.lut)
    m.set_sequence(ev)
    got = m.event_panorama(scene.traj, beg, end, want_pm=True)
    assert got["pm"].shape == (2500, 2) and got["sum"] == 256 * 2500
    assert_exact(got, ev, beg, end, False)
    sl = eio.slice_events(ev, beg, end)
    o = oracle_mod.OracleLEGM(64, 48, W, H, scene.lut, scene.C_th)
    pm_o = o.count_map(scene.traj.knots_xyzw, scene.traj.t0_ns, scene.traj.dt_ns, sl.x, sl.y, sl.t_ns, want_pm=True)[2][:2500]
    assert_close_elementwise(got["pm"], pm_o, "pano_pm of a range against the oracle's pm of the slice")
    # the batch grid of the whole sequence, which begins at event 0
    pm_grid0 = o.count_map(scene.traj.knots_xyzw, scene.traj.t0_ns, scene.traj.dt_ns, ev.x, ev.y, ev.t_ns, want_pm=True)[2][beg:beg + 2500]
    assert np.array_equal(pm_grid0, pm_o)      # here the two grids coincide (300 is a multiple of 100) ...
    got2 = m.event_panorama(scene.traj, beg + 37, end, want_pm=True)      # ... and here they do not: 337 + 100 b
    sl2 = eio.slice_events(ev, beg + 37, end)
    pm_o2 = o.count_map(scene.traj.knots_xyzw, scene.traj.t0_ns, scene.traj.dt_ns, sl2.x, sl2.y, sl2.t_ns, want_pm=True)[2][:2500]
    assert got2["pm"].shape == (2500, 2)
    assert_close_elementwise(got2["pm"], pm_o2, "pano_pm of an off-grid range against the oracle's pm of the slice")
    assert not np.array_equal(got2["pm"][:2400], got["pm"][37:2437])      # (the same events under the other grid's midpoints)
    m2 = make_legm(scene.lut)
    m2.set_sequence(sl)
    fresh = m2.event_panorama(scene.traj, 0, None, want_pm=True)
    assert np.array_equal(fresh["pm"].view(np.uint64), got["pm"].view(np.uint64)) and np.array_equal(fresh["image"], got["image"])
    assert all(fresh[k] == got[k] for k in ("J", "sum", "nonzero", "dropped"))
    m.close(); m2.close()


def test_wrap_across_column_zero(gpu, scene):
    """The trajectory yawed by pi: the view straddles azimuth +-pi, column W - 1 | column 0."""
    m = make_legm(scene.lut)
    n = m.set_sequence(scene.events)
    got = m.event_panorama(turned(scene.traj, [0.0, np.pi, 0.0]), 0, n, want_pm=True)
    assert_exact(got, scene.events, 0, n, False)
    img = got["image"]
    assert img[:, 0].any() and img[:, W - 1].any() and not img[:, W // 2].any()
    assert (got["pm"][:, 0] < 1.0).any() and (got["pm"][:, 0] >= W - 1.0).any()      # events whose 2x2 patch itself crosses the seam
    assert got["sum"] == 256 * got["pm"].shape[0] and got["dropped"] == 0           # nothing is lost at the seam
    m.close()


def test_dropped_rows_at_the_pole(gpu):
    """20 000 uniform events under poses pitched to the poles.  At the lower pole (pm_y in [H - 1, H]) the row below the last one has no cell: its votes
    are dropped and counted; at the upper pole pm_y >= 0, row -1 is never asked for and nothing is lost."""
    n = 20_000
    rng = np.random.default_rng(5)
    lut = synth.pinhole_bearing_lut(64, 48, 60.0, 60.0, 32.0, 24.0)
    ev = EventPacket(rng.integers(0, 64, n).astype(np.uint16), rng.integers(0, 48, n).astype(np.uint16), rng.integers(0, 2, n).astype(np.uint8),
                     10**9 + 5000 * np.arange(n, dtype=np.int64))
    m = make_legm(lut)
    m.set_sequence(ev)
    for pitch, lower in ((-np.pi / 2 + 0.1, True), (np.pi / 2 - 0.1, False)):
        traj = LinearTrajectory(np.array([so3.exp([pitch, 0.02 * i, 0.0]) for i in range(4)]), 10**9, 50_000_000)
        got = m.event_panorama(traj, 0, n, want_pm=True)
        want = assert_exact(got, ev, 0, n, False)
        print("pitch", pitch, "dropped", got["dropped"], "pm_y", got["pm"][:, 1].min(), got["pm"][:, 1].max())
        assert got["dropped"] == want["dropped"]
        if lower:
            assert got["dropped"] > 0 and got["pm"][:, 1].max() >= H - 1 and got["sum"] < 256 * n and got["image"][H - 1].any()
        else:
            assert got["dropped"] == 0 and got["pm"][:, 1].min() < 1.0 and got["sum"] == 256 * n and got["image"][0].any()
    m.close()


def test_contention_on_one_patch(gpu):
    """100 000 events at one sensor pixel under one pose: every add of the launch goes to the same four cells."""
    n = 100_000
    lut = synth.pinhole_bearing_lut(64, 48, 60.0, 60.0, 32.0, 24.0)
    ev = EventPacket(np.full(n, 40, np.uint16), np.full(n, 13, np.uint16), (np.arange(n) % 2).astype(np.uint8), 10**9 + 1000 * np.arange(n, dtype=np.int64))
    q = so3.exp([0.03, 0.4, -0.02])
    traj = LinearTrajectory(np.tile(q, (3, 1)), 10**9, 100_000_000)
    m = make_legm(lut)
    m.set_sequence(ev)
    got = m.event_panorama(traj, 0, n, want_pm=True)
    assert (got["pm"] == got["pm"][0]).all()
    img = got["image"]
    ys, xs = np.nonzero(img)
    assert got["nonzero"] == len(ys) and 1 <= len(ys) <= 4 and ys.max() - ys.min() <= 1 and xs.max() - xs.min() <= 1
    assert got["sum"] == 256 * n == int(img.sum()) and got["dropped"] == 0
    assert_exact(got, ev, 0, n, False)
    signed = m.event_panorama(traj, 0, n, signed=True)
    assert signed["sum"] == 0 and signed["J"] == 0 and signed["nonzero"] == 0      # as many events of either polarity
    m.close()


def test_statuses_and_what_a_call_leaves_alone(gpu, scene):
    from emba_amd import EmbaError
    ev, traj = scene.events, scene.traj
    m = make_legm(scene.lut)
    with pytest.raises(EmbaError) as ei:                              # no sequence
        m.event_panorama(traj, 0, 0)
    assert ei.value.status == ERR_STATE
    n = m.set_sequence(ev)
    for beg, end in ((5, 4), (0, n + 1)):
        with pytest.raises(EmbaError) as ei:
            m.event_panorama(traj, beg, end)
        assert ei.value.status == ERR_INVALID_ARG
    with pytest.raises(EmbaError) as ei:                              # K = 1
        m.event_panorama(LinearTrajectory(traj.knots_xyzw[:1], traj.t0_ns, traj.dt_ns), 0, n)
    assert ei.value.status == ERR_INVALID_ARG
    with pytest.raises(EmbaError) as ei:                              # dt = 0
        m.event_panorama(LinearTrajectory(traj.knots_xyzw, traj.t0_ns, 0), 0, n)
    assert ei.value.status == ERR_INVALID_ARG
    with pytest.raises(EmbaError) as ei:                              # the last batches lie behind the last knot of a spline of three
        m.event_panorama(LinearTrajectory(traj.knots_xyzw[:3], traj.t0_ns, traj.dt_ns), 0, n)
    assert ei.value.status == ERR_TIME_RANGE
    with pytest.raises(EmbaError) as ei:                              # ... and every batch in front of a spline that begins later
        m.event_panorama(LinearTrajectory(traj.knots_xyzw, traj.t0_ns + 10**9, traj.dt_ns), 0, 1000)
    assert ei.value.status == ERR_TIME_RANGE
    ok = m.event_panorama(LinearTrajectory(traj.knots_xyzw[:3], traj.t0_ns, traj.dt_ns), 0, 2000)      # the same three knots span the first events
    assert ok["J"] > 0
    for beg, end in ((77, 77), (500, 599), (n, n)):                   # an empty range, less than a batch
        r = m.event_panorama(traj, beg, end, want_pm=True)
        assert r["J"] == 0 and r["sum"] == 0 and r["nonzero"] == 0 and r["dropped"] == 0 and not r["image"].any() and r["pm"].shape == (0, 2)
    # with every output NULL nothing happens (the arguments are still checked); the registered window and the last evaluation are left alone
    m.set_events(EventWindow(0, n))
    ep = m.evaluateDataError(traj, scene.Gx, scene.Gy)
    counts, evc = m.last_counts(), m.event_counts()
    knots = np.ascontiguousarray(traj.knots_xyzw)
    kp = knots.ctypes.data_as(C.POINTER(C.c_double))
    assert m._L.emba_seq_event_panorama(m._ctx, 0, n, kp, 6, traj.t0_ns, traj.dt_ns, 0, None, None, None, None, None, None) == 0
    assert m._L.emba_seq_event_panorama(m._ctx, 0, n, kp, 1, traj.t0_ns, traj.dt_ns, 0, None, None, None, None, None, None) == ERR_INVALID_ARG
    a = m.event_panorama(turned(traj, [0.0, 1.0, 0.0]), 300, 20000, signed=True, want_pm=True)
    assert a["J"] > 0
    assert m.last_counts() == counts and m.event_counts() == evc and m.n_events == n
    assert np.array_equal(m.evaluateDataError(traj, None, None), ep)      # the window is still registered, the map still resident
    m.free_sequence()
    with pytest.raises(EmbaError) as ei:
        m.event_panorama(traj, 0, 0)
    assert ei.value.status == ERR_STATE
    m.close()


def test_device_image_against_the_oracle(gpu, scene, oracle_pm):
    m = make_legm(scene.lut)
    n = m.set_sequence(scene.events)
    got = m.event_panorama(scene.traj, 0, n)
    ref = eio.event_panorama(scene.events, None, 64, 48, W, H, None, 0, n, pm=oracle_pm)
    total = 256 * oracle_pm.shape[0]
    share = int(np.abs(got["image"] - ref["image"]).sum()) / total
    print(f"device image against the image of the oracle's pm: L1 distance {share!r} of the total votes, bound {DEVICE_SHARE_BOUND!r}; J device {got['J']} oracle {ref['J']}")
    assert share <= DEVICE_SHARE_BOUND <= 1e-3
    m.close()


def test_poisoned_workspace(gpu, scene):
    """Option poison on a fresh context: every new allocation reads as 0xFF bytes, so a cell, slot or counter that is read before it is written shows."""
    m = make_legm(scene.lut)
    m.set_option("poison", 1)
    n = m.set_sequence(scene.events)
    for signed in (False, True):
        got = m.event_panorama(scene.traj, 0, n, signed=signed, want_pm=True)
        assert_exact(got, scene.events, 0, n, signed)
    m.close()


def test_chunks_and_the_driver(gpu, scene):
    m = make_legm(scene.lut)
    n = m.set_sequence(scene.events)
    one = m.event_panorama(scene.traj, 150, n, signed=True, want_pm=True)
    for chunk in (1000, 20000):
        cut = m.event_panorama(scene.traj, 150, n, signed=True, want_pm=True, _chunk_events=chunk)
        assert np.array_equal(cut["image"], one["image"]) and np.array_equal(cut["pm"], one["pm"])
        assert all(cut[k] == one[k] for k in ("J", "sum", "nonzero", "dropped"))
    lean = m.event_panorama(scene.traj, 150, n, signed=True, want_image=False, _chunk_events=7000)
    assert lean["image"] is None and lean["J"] == one["J"]
    with pytest.raises(ValueError):
        m.event_panorama(scene.traj, 0, n, _chunk_events=150)
    m.close()
    # the sliding-window driver on the device model
    w = scene
    m = make_legm(w.lut)
    t0, t1 = w.traj.t0_ns * 1e-9, (w.traj.t0_ns + w.traj.dt_ns * (w.K - 1)) * 1e-9
    t_raw_ns = w.traj.t0_ns + 5_000_000 * np.arange((w.traj.dt_ns * (w.K - 1)) // 5_000_000, dtype=np.int64)
    pose_t, pose_q = t_raw_ns * 1e-9, np.array([w.traj.evaluate(int(tn)) for tn in t_raw_ns])
    seq = SequenceSettings(time_window_size=0.15, sliding_window_stride=0.1, dt_knots=0.05, t_start=t0, t_end=t1, median_blur=False, record_contrast=True,
                           event_panorama=True)
    res = run_sequence(m, w.events, pose_t, pose_q, w.Gx, w.Gy, seq, BASettings(alpha=0.0), LMSettings(max_num_iter=3))
    assert len(res.windows) == 2
    for wr in res.windows:
        for got, traj in ((wr.contrast_init, wr.traj_init), (wr.contrast_final, wr.result.traj)):
            want = m.event_panorama(traj, wr.beg, wr.end, want_image=False)
            assert got == {k: want[k] for k in ("J", "sum", "nonzero")} and got["J"] > 0
        print(f"window {wr.index}: J {wr.contrast_init['J']} -> {wr.contrast_final['J']}")
    want = m.event_panorama(res.traj, res.windows[0].beg, res.windows[-1].end)
    assert res.event_panorama.shape == (H, W) and np.array_equal(res.event_panorama, want["image"]) and want["J"] > 0
    m.close()
