"""Sensor views along the trajectory without a GPU: the numpy forms of emba_render_views and emba_seq_event_frames (emba_amd.io: view_pm,
render_views, view_u8, event_frames) against what they state, the new symbols of libemba_hip.so, and that numpy's own pm of every case of
tests/test_gpu_views.py keeps clear of the pole rows, so that the comparison there leaves out no pixel on numpy's account."""
import inspect
import os

import numpy as np
import pytest

import view_cases as VC
from emba_amd import io as eio
from emba_amd import so3
from helpers import assert_close

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_new_symbols_resolve(hip_lib):
    from emba_amd import LEGM, _lib
    for name in ("emba_render_views", "emba_seq_event_frames"):
        assert hasattr(hip_lib, name) and name in _lib.SIGNATURES, name
    assert hip_lib.emba_abi_version() == 2
    blob = open(os.path.join(ROOT, "emba_amd", "libemba_hip.so"), "rb").read()
    assert b"emba_view_kernel" in blob and b"emba_event_frames_kernel" in blob
    p = inspect.signature(LEGM.render_views).parameters
    assert list(p)[1:] == ["frame_t_ns", "knots", "t0_ns", "dt_ns", "plane", "boundary", "fill", "lo", "hi", "want_u8", "want_pm"]
    assert (p["plane"].default, p["boundary"].default, p["fill"].default, p["lo"].default, p["hi"].default) == (None, "dirichlet", 0.0, None, None)
    assert p["want_u8"].default is False and p["want_pm"].default is False
    p = inspect.signature(LEGM.event_frames).parameters
    assert list(p)[1:] == ["beg", "end", "edge_t_ns", "signed_polarity"] and p["signed_polarity"].default is True


def test_linear_planes_reproduce_pm():
    """A plane that is linear in the column gives pm_x back wherever the 2x2 patch does not straddle the seam, one that is linear in the row gives pm_y, to
    1e-12; a pixel outside reads the fill."""
    W, H = 48, 24
    rng = np.random.default_rng(11)
    pm = np.stack([rng.uniform(0.0, W - 1.0, 4000), rng.uniform(0.0, H - 1.0, 4000)], axis=1)      # ix + 1 <= W - 1: away from the seam
    col = np.tile(np.arange(W, dtype=np.float64), (H, 1))
    row = np.tile(np.arange(H, dtype=np.float64)[:, None], (1, W))
    vx, out = eio.render_views(col, pm, fill=-7.0, with_outside=True)
    vy = eio.render_views(row, pm, fill=-7.0)
    assert not out.any() and vx.shape == (4000,)
    assert np.abs(vx - pm[:, 0]).max() <= 1e-12 and np.abs(vy - pm[:, 1]).max() <= 1e-12
    # pm_y is linear across the seam as well (the row plane has no seam); the column plane there mixes columns W - 1 and 0
    seam = np.stack([rng.uniform(W - 1.0, W + 1.0, 500), rng.uniform(0.0, H - 1.0, 500)], axis=1)
    assert np.abs(eio.render_views(row, seam) - seam[:, 1]).max() <= 1e-12
    ax = seam[:, 0] - np.floor(seam[:, 0])
    left = np.floor(seam[:, 0]) % W
    assert np.abs(eio.render_views(col, seam) - ((1.0 - ax) * left + ax * ((left + 1) % W))).max() <= 1e-12
    # outside: iy = -1, iy = H - 1 (no row below), not finite; iy = H - 2 is the last pair
    edge = np.array([[3.0, -0.25], [3.0, H - 1.0], [3.0, H - 0.5], [np.nan, 3.0], [3.0, np.inf], [2.0 ** 31, 3.0], [3.5, H - 1.5], [3.0, 0.0]])
    v, out = eio.render_views(row, edge, fill=-7.0, with_outside=True)
    assert out.tolist() == [True] * 6 + [False] * 2 and (v[:6] == -7.0).all() and v[6] == H - 1.5 and v[7] == 0.0
    assert eio.render_views(row, edge.reshape(2, 4, 2)).shape == (2, 4)
    assert np.isnan(eio.render_views(row, edge, fill=np.nan)[:6]).all()


def test_the_stated_formula_per_pixel():
    """render_views against the formula of include/emba_hip.h, one pixel at a time in python floats: the same bits."""
    W, H = 32, 16
    plane = VC.plane_of((W, H))
    rng = np.random.default_rng(5)
    pm = np.stack([rng.uniform(-3.0, W + 3.0, 600), rng.uniform(-1.0, H + 1.0, 600)], axis=1)
    got, out = eio.render_views(plane, pm, fill=0.25, with_outside=True)
    n_out = 0
    for (x, y), g, o in zip(pm.tolist(), got.tolist(), out.tolist()):
        ix, iy = int(np.floor(x)), int(np.floor(y))
        if iy < 0 or iy + 1 > H - 1:
            assert o and g == 0.25
            n_out += 1
            continue
        ax, ay = x - ix, y - iy
        c0, c1 = ix % W, (ix + 1) % W
        want = (1 - ay) * ((1 - ax) * plane[iy, c0] + ax * plane[iy, c1]) + ay * ((1 - ax) * plane[iy + 1, c0] + ax * plane[iy + 1, c1])
        assert not o and g == float(want)
    assert 50 < n_out < 300


def test_view_u8_is_normalize_robust_with_given_limits():
    a = np.random.default_rng(2).standard_normal((24, 48)) * 3.0
    srt = np.sort(a, axis=None)
    n = a.size
    i_min = int(np.float32(np.float32(0.5) * np.float32(0.1) / np.float32(100.0)) * np.float32(n))
    i_max = int(np.float32(np.float32(1.0) - np.float32(0.5) * np.float32(0.1) / np.float32(100.0)) * np.float32(n))
    lo, hi = srt[i_min], srt[min(i_max, n - 1)]
    assert np.array_equal(eio.view_u8(a, lo, hi), eio.normalize_robust(a, 0.1))
    assert eio.view_u8([2.0, 5.4, 400.0, -9.0, np.nan], 3.0, 3.0).tolist() == [0, 2, 255, 0, 0]                 # lo == hi: scale 1
    assert eio.view_u8([-7.0, -1.0, 0.0, 1.0, 9.0], -1.0, 1.0).tolist() == [0, 0, 128, 255, 255]                # below lo, above hi, 127.5 to the even 128
    assert eio.view_u8([0.0, 1.0], -1.0, 1.0, outside=np.array([True, False])).tolist() == [0, 255]


def yawed(knots, a):
    q = so3.exp(np.array([0.0, float(a), 0.0]))
    return np.array([so3.mul(q, k) for k in knots])


@pytest.mark.parametrize("k", [1, 5, 31, -7])
def test_rolled_plane_under_a_yawed_trajectory(k):
    """The plane rolled by k columns seen along the trajectory yawed by 2 pi k / W gives the same frames: the columns wrap, whatever the seam."""
    W, H = 32, 16
    sensor = (16, 12)
    lut, plane, ts = VC.lut_of(sensor), VC.plane_of((W, H)), VC.frame_times(3)
    for kind in VC.KINDS:
        knots = VC.knots_of(kind)
        pm0 = eio.view_pm(lut, knots, VC.T0_NS, VC.DT_NS, ts, W, H)
        pm1 = eio.view_pm(lut, yawed(knots, 2.0 * np.pi * k / W), VC.T0_NS, VC.DT_NS, ts, W, H)
        assert pm0.shape == (3, 16 * 12, 2)
        v0, o0 = eio.render_views(plane, pm0, with_outside=True)
        v1, o1 = eio.render_views(np.roll(plane, k, axis=1), pm1, with_outside=True)
        assert np.array_equal(o0, o1)
        assert_close(v1, v0, f"views of the plane rolled by {k} under the yawed trajectory ({kind})")
        if kind == "yaw_pi":
            assert (pm0[..., 0] < 1.0).any() or (pm0[..., 0] >= W - 1.0).any()      # the view does straddle the seam


def test_view_pm_is_the_event_panorama_projection():
    """view_pm at a batch's midpoint is event_panorama_pm of that batch's pixels: the same spline, the same projection."""
    from emba_amd.legm import EventPacket, LinearTrajectory
    sensor, (W, H) = (16, 12), (48, 24)
    lut, knots = VC.lut_of(sensor), VC.knots_of("pitch")
    S = sensor[0] * sensor[1]
    xs, ys = (np.arange(100) % 16).astype(np.uint16), (np.arange(100) // 16).astype(np.uint16)
    t = np.full(100, VC.T0_NS + 12_345_678, np.int64)
    ev = EventPacket(xs, ys, np.ones(100, np.uint8), t)
    pm_e = eio.event_panorama_pm(ev, lut, 16, 12, W, H, LinearTrajectory(knots, VC.T0_NS, VC.DT_NS))
    pm_v = eio.view_pm(lut, knots, VC.T0_NS, VC.DT_NS, [VC.T0_NS + 12_345_678], W, H)
    assert pm_v.shape == (1, S, 2) and np.array_equal(pm_v[0, :100], pm_e)
    with pytest.raises(ValueError):
        eio.view_pm(lut, knots, VC.T0_NS, VC.DT_NS, [VC.T_LAST_NS + 1], W, H)
    with pytest.raises(ValueError):
        eio.view_pm(lut, knots, VC.T0_NS, VC.DT_NS, [VC.T0_NS - 1], W, H)
    assert eio.view_pm(lut, knots, VC.T0_NS, VC.DT_NS, [VC.T0_NS, VC.T_LAST_NS], W, H).shape == (2, S, 2)


def test_gpu_cases_keep_clear_of_the_pole_rows():
    """Every case of tests/test_gpu_views.py in numpy alone: no pm_y within POLE_EPS of row 0 or row H - 1, so the comparison with the device leaves out no
    pixel on numpy's account; the pitched trajectory does carry part of every view over the pole and leaves part inside, the others none."""
    for sensor in VC.SENSORS:
        lut = VC.lut_of(sensor)
        for W, H in VC.PANOS:
            for kind in VC.KINDS:
                for F in VC.FRAMES:
                    pm = eio.view_pm(lut, VC.knots_of(kind), VC.T0_NS, VC.DT_NS, VC.frame_times(F), W, H)
                    assert np.isfinite(pm).all() and not VC.near_pole(pm, H).any(), (sensor, W, H, kind, F)
                    out = eio.render_views(VC.plane_of((W, H)), pm, with_outside=True)[1].sum(axis=1)
                    if kind == "pitch":
                        assert (out > 0).all() and (out < sensor[0] * sensor[1]).all(), (sensor, W, H, F, out)
                    else:
                        assert not out.any()


def loop_frames(x, y, pol, t, edges, sw, sh, signed):
    F = len(edges) - 1
    fr = np.zeros((F, sh, sw), np.int64)
    before = after = 0
    for xi, yi, pi, ti in zip(x.tolist(), y.tolist(), pol.tolist(), t.tolist()):
        if ti < edges[0]:
            before += 1
        elif ti >= edges[F]:
            after += 1
        else:
            f = max(j for j in range(F) if edges[j] <= ti)
            fr[f, yi, xi] += -1 if (signed and pi == 0) else 1
    return fr, before, after


@pytest.mark.parametrize("signed", [True, False])
def test_event_frames_against_a_loop(signed):
    rng = np.random.default_rng(17)
    n, sw, sh = 1500, 7, 5
    x, y = rng.integers(0, sw, n).astype(np.uint16), rng.integers(0, sh, n).astype(np.uint16)
    pol = rng.integers(0, 2, n).astype(np.uint8)
    t = np.sort(rng.integers(1000, 9000, n)).astype(np.int64)
    # the edges take in exact timestamps; [4000, 4001) and a gap hold few or no events; the last edge is an event's own time
    edges = np.array([int(t[100]), int(t[400]), 4000, 4001, int(t[900]), int(t[900]) + 1, int(t[1400])], dtype=np.int64)
    assert (np.diff(edges) > 0).all()
    got, before, after = eio.event_frames(x, y, pol, t, edges, sw, sh, signed)
    want, wb, wa = loop_frames(x, y, pol, t, edges, sw, sh, signed)
    assert got.dtype == np.int32 and got.shape == (6, sh, sw) and np.array_equal(got, want) and (before, after) == (wb, wa)
    assert before > 0 and after > 0
    if signed:
        assert (got < 0).any()
    else:
        assert int(got.sum()) + before + after == n


def test_event_frames_edge_cases():
    x = np.array([1, 1, 2, 0], np.uint16); y = np.array([0, 0, 1, 1], np.uint16); pol = np.array([1, 0, 1, 1], np.uint8)
    t = np.array([10, 20, 20, 30], np.int64)
    fr, b, a = eio.event_frames(x, y, pol, t, [10, 20, 30], 3, 2)
    assert (b, a) == (0, 1)                                  # t == edge[F] is excluded
    assert fr[0, 0, 1] == 1 and fr[0].sum() == 1             # t == edge[0] belongs to frame 0
    assert fr[1, 0, 1] == -1 and fr[1, 1, 2] == 1            # t == edge[1] belongs to frame 1
    fr, b, a = eio.event_frames(x, y, pol, t, [0, 5, 6, 100], 3, 2, signed_polarity=False)
    assert not fr[0].any() and not fr[1].any() and fr[2].sum() == 4 and (b, a) == (0, 0)      # empty frames
    fr, b, a = eio.event_frames(x, y, pol, t, [20], 3, 2)    # F = 0: one edge
    assert fr.shape == (0, 2, 3) and (b, a) == (1, 3)
    fr, b, a = eio.event_frames(x[:0], y[:0], pol[:0], t[:0], [0, 5], 3, 2)
    assert fr.shape == (1, 2, 3) and not fr.any() and (b, a) == (0, 0)
    for bad in ([5, 5], [5, 4], []):
        with pytest.raises(ValueError):
            eio.event_frames(x, y, pol, t, bad, 3, 2)


def test_the_driver_takes_the_numpy_forms_without_a_device():
    """driver.sequence_views on a model that only names its camera: frame times every 1 / views_hz from the first knot to the last accepted time, frames
    and tone by the numpy forms from the panorama it is given, event frames of the intervals between consecutive frames.  Off by default."""
    from types import SimpleNamespace
    from emba_amd.driver import SequenceSettings, sequence_views, view_frame_times
    from emba_amd.legm import EventPacket, LinearTrajectory
    kw = dict(time_window_size=0.1, sliding_window_stride=0.1)
    assert SequenceSettings(**kw).views_hz == 0 and SequenceSettings(**kw).view_events is False
    with pytest.raises(ValueError):
        SequenceSettings(views_hz=-1.0, **kw)
    sensor, (W, H) = (16, 12), (48, 24)
    traj = LinearTrajectory(VC.knots_of("yaw_pi"), VC.T0_NS, VC.DT_NS)
    ts = view_frame_times(traj, 1000.0)                       # 1 ms: 30 frames over the 30 ms - 1 ns the spline accepts
    assert ts[0] == VC.T0_NS and (np.diff(ts) == 1_000_000).all() and ts[-1] <= VC.T_LAST_NS < ts[-1] + 1_000_000 and ts.size == 30
    assert view_frame_times(traj, 1.0).tolist() == [VC.T0_NS] and view_frame_times(traj, 100.0).tolist() == [VC.T0_NS + 10_000_000 * i for i in range(3)]
    model = SimpleNamespace(bearing_lut=VC.lut_of(sensor), sensor_w=16, sensor_h=12, W=W, H=H)
    M = VC.plane_of((W, H))
    rng = np.random.default_rng(4)
    n = 800
    ev = EventPacket(rng.integers(0, 16, n).astype(np.uint16), rng.integers(0, 12, n).astype(np.uint16), rng.integers(0, 2, n).astype(np.uint8),
                     VC.T0_NS + np.sort(rng.integers(0, 30_000_000, n)).astype(np.int64))
    with pytest.raises(ValueError):
        sequence_views(model, ev, traj, 1000.0, resident_sequence=False)      # no panorama, and nothing that reconstructs one
    r = sequence_views(model, ev, traj, 1000.0, view_events=True, resident_sequence=False, panorama=M)
    assert np.array_equal(r["t_ns"], ts) and r["views"].shape == (30, 12, 16) and r["u8"].dtype == np.uint8 and r["event_frames"].shape == (29, 12, 16)
    pm = eio.view_pm(model.bearing_lut, traj.knots_xyzw, VC.T0_NS, VC.DT_NS, ts, W, H)
    assert np.array_equal(r["views"].reshape(30, -1), eio.render_views(M, pm)) and not r["outside"].any()
    assert (r["lo"], r["hi"]) == eio.robust_range(M, 0.1) and np.array_equal(r["u8"], eio.view_u8(r["views"], r["lo"], r["hi"]))
    assert np.array_equal(r["event_frames"], eio.event_frames(ev.x, ev.y, ev.polarity, ev.t_ns, ts, 16, 12)[0]) and r["event_frames"].any()
    assert sequence_views(model, None, traj, 1000.0, panorama=M)["event_frames"] is None
