"""Contrast maximisation on the MI355X (include/emba_hip.h: emba_seq_cmax, emba_seq_cmax_objective) against the numpy form of the same rule
(emba_amd.io.cmax_objective / estimate_angular_velocity): J, the image of warped events and every result of the search are integers or exact doubles,
so everything is compared with array_equal — a difference is a bug in one of the two forms, never a tolerance.  Then the error paths, the estimate against
the simulator's true body rate, and a whole sliding-window run started without front-end poses."""
import numpy as np
import pytest

import cmax_cases as CC
from emba_amd import io as eio
from emba_amd import so3, synth
from emba_amd.driver import SequenceSettings, run_sequence
from emba_amd.legm import EventPacket
from emba_amd.solver import BASettings, LMSettings

pytestmark = pytest.mark.gpu
ERR_INVALID_ARG, ERR_STATE, ERR_CAPACITY = 1, 5, 6


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from emba_amd import build
    build.build_hip()
    return True


@pytest.fixture(scope="module")
def scene():
    return synth.make_scene_workload()          # the 64x48 default scene: 38 965 events


@pytest.fixture(scope="module")
def scene_reference(scene):
    """The numpy estimates on the scene, computed once: {slice_events: estimate}."""
    return {m: eio.estimate_angular_velocity(scene.events, scene.lut, 64, 48, m, CC.OMEGA_MAX) for m in (2000, 777)}


def make_legm(sw, sh, lut):
    from emba_amd import LEGM
    return LEGM(sw, sh, lut, 0.2, 512, 256, device=0)


# small, a negative component, zero, large enough that every event but the reference leaves the grid, and far too large
CANDIDATES = np.array([[0.0, 0.0, 0.0], [0.05, 0.4, -0.02], [-3.0, 1.5, 0.7], [0.0, 0.0, -6.0], [900.0, 0.0, 0.0], [0.0, -4000.0, 300.0]])


@pytest.mark.parametrize("sensor", [(64, 48), (63, 47)])
def test_objective_and_image_equal_numpy(gpu, scene, sensor):
    """Ranges of 1, 255, 256, 257 and 2000 events (one event per lane and fewer, a second sweep, many), at the head, inside and at the tail of the sequence;
    63x47: the scene's events that lie on the smaller sensor, whose pinhole centre falls between pixels."""
    sw, sh = sensor
    ev = scene.events
    keep = (ev.x < sw) & (ev.y < sh)
    ev = EventPacket(ev.x[keep], ev.y[keep], ev.polarity[keep], ev.t_ns[keep])
    lut = synth.pinhole_bearing_lut(sw, sh, 60.0, 60.0, sw / 2.0, sh / 2.0)
    m = make_legm(sw, sh, lut)
    assert m.cmax_grid() == eio.cmax_grid(sw, sh) == (0, sw, sh)
    n = m.set_sequence(ev)
    pin = eio.cmax_pinhole_fit(lut, sw, sh)
    for beg, length in ((0, 1), (5, 255), (1000, 256), (4321, 257), (n - 2000, 2000), (n - 1, 1), (77, 0)):
        J, iwe = m.cmax_objective(CANDIDATES, beg, beg + length)
        Jn, iwen = eio.cmax_objective(ev, lut, sw, sh, CANDIDATES, beg, beg + length, pinhole=pin)
        assert J.dtype == np.uint64 and iwe.dtype == np.uint32
        assert np.array_equal(iwe, iwen), (beg, length)
        assert np.array_equal(J, Jn), (beg, length)
        if length:
            # an event's four votes are 256 in all, less what falls outside the grid (the fitted f is a few ulps off 60: an unwarped event at
            # the border may already lose a sliver)
            assert J[0] > 0 and (iwe.reshape(len(CANDIDATES), -1).sum(axis=1) <= 256 * length).all() and iwe[0].sum() > 255 * length
        if length > 1:
            assert len(set(J.tolist())) > 2                        # the candidates are told apart
    # (t_ref is the range's own first timestamp, so the reference event never moves and J > 0 for every omega; under the two huge candidates all the
    # other events turn behind the plane or leave the grid unless they share the reference's instant)
    # J without the image
    J2, none = m.cmax_objective(CANDIDATES, 1000, 1256, want_iwe=False)
    assert none is None and np.array_equal(J2, eio.cmax_objective(ev, lut, sw, sh, CANDIDATES, 1000, 1256, want_iwe=False, pinhole=pin)[0])
    m.close()


@pytest.mark.parametrize("sensor,shift", [((130, 100), 0), ((160, 120), 1), ((240, 180), 1)])
def test_objective_on_larger_sensors(gpu, sensor, shift):
    """A few thousand uniform random events.  130x100 (13 000 cells: they still fit 64 KiB, shift 0) is the largest grid the tests sweep; 160x120 and 240x180
    take shift 1 — cells of two pixels, 160x120 with whole border cells and an even grid, 240x180 the benchmark's sensor."""
    sw, sh = sensor
    rng = np.random.default_rng(31)
    n = 5000
    ev = EventPacket(rng.integers(0, sw, n).astype(np.uint16), rng.integers(0, sh, n).astype(np.uint16), rng.integers(0, 2, n).astype(np.uint8),
                     np.sort(rng.integers(10**9, 10**9 + 40_000_000, size=n)).astype(np.int64))
    lut = synth.pinhole_bearing_lut(sw, sh, 0.8 * sw, 0.8 * sw, sw / 2.0 - 0.5, sh / 2.0 + 0.25)
    m = make_legm(sw, sh, lut)
    assert m.cmax_grid() == eio.cmax_grid(sw, sh) and m.cmax_grid()[0] == shift
    m.set_sequence(ev)
    for beg, end in ((0, n), (123, 4000)):
        J, iwe = m.cmax_objective(CANDIDATES, beg, end)
        Jn, iwen = eio.cmax_objective(ev, lut, sw, sh, CANDIDATES, beg, end)
        assert np.array_equal(iwe, iwen) and np.array_equal(J, Jn)
        assert 250 * (end - beg) < iwe[0].sum() <= 256 * (end - beg)      # unwarped: all but slivers at the border inside the grid
    m.close()


@pytest.mark.parametrize("slice_events", [2000, 777])
def test_search_equals_numpy(gpu, scene, scene_reference, slice_events):
    m = make_legm(64, 48, scene.lut)
    m.set_sequence(scene.events)
    got, want = m.estimate_angular_velocity(slice_events, CC.OMEGA_MAX), scene_reference[slice_events]
    assert got["omega"].shape == (scene.events.size() // slice_events, 3)
    for k in ("evals", "J0", "J", "t_ref_ns"):
        assert np.array_equal(got[k], want[k]), k
    assert np.array_equal(got["omega"].view(np.uint64), want["omega"].view(np.uint64))      # bit-equal doubles
    assert (got["J"] >= got["J0"]).all() and (got["evals"] > 1).all()
    m.close()


def test_search_after_filter_and_down_sampling(gpu, scene):
    """The estimate runs on the sequence as it stands: down-sampled at the upload, then filtered."""
    m = make_legm(64, 48, scene.lut)
    m.set_sequence(scene.events, 2)
    stats = m.filter_sequence(0.0, 20_000_000, 0, 1)
    ev = eio.downsample_events(scene.events, 2)
    ev, _, _ = eio.filter_events(ev, 64, 48, 0.0, 20_000_000, 0)
    assert int(stats[5]) == ev.size() < scene.events.size() // 2
    got, want = m.estimate_angular_velocity(3000, 4.0), eio.estimate_angular_velocity(ev, scene.lut, 64, 48, 3000, 4.0)
    for k in ("omega", "evals", "J0", "J", "t_ref_ns"):
        assert np.array_equal(got[k], want[k]), k
    m.close()


def test_error_paths(gpu, scene):
    import ctypes as C
    from emba_amd import EmbaError
    m = make_legm(64, 48, scene.lut)
    with pytest.raises(EmbaError) as ei:                              # no sequence
        m.estimate_angular_velocity(2000, 8.0)
    assert ei.value.status == ERR_STATE
    with pytest.raises(EmbaError) as ei:
        m.cmax_objective(CANDIDATES, 0, 0)
    assert ei.value.status == ERR_STATE
    assert m.cmax_grid() == (0, 64, 48)                               # (the grid needs none)
    n = m.set_sequence(scene.events)
    for bad in ((0, 8.0), (-1, 8.0), (2000, 0.0), (2000, -2.0), (2000, float("inf")), (2000, float("nan")), (1 << 24, 8.0)):
        with pytest.raises(EmbaError) as ei:
            m.estimate_angular_velocity(*bad)
        assert ei.value.status == ERR_INVALID_ARG, bad
    for beg, end in ((5, 4), (0, n + 1)):
        with pytest.raises(EmbaError) as ei:
            m.cmax_objective(CANDIDATES, beg, end)
        assert ei.value.status == ERR_INVALID_ARG
    with pytest.raises(EmbaError) as ei:
        m.cmax_objective([[0.0, float("nan"), 0.0]], 0, 10)
    assert ei.value.status == ERR_INVALID_ARG
    # capacity: 19 slices into arrays of 18; the count is set all the same
    ns, omega = C.c_size_t(0), np.zeros((18, 3))
    st = m._L.emba_seq_cmax(m._ctx, 2000, 8.0, omega.ctypes.data_as(C.POINTER(C.c_double)), None, None, None, None, 18, C.byref(ns))
    assert st == ERR_CAPACITY and ns.value == 19 and not omega.any()
    # fewer events than one slice: EMBA_OK, nothing estimated
    none = m.estimate_angular_velocity(n + 1, 8.0)
    assert none["omega"].shape == (0, 3) and none["t_ref_ns"].size == 0
    # a slice of one instant: omega = 0 after the one evaluation of J(0)
    still = EventPacket(scene.events.x[:300], scene.events.y[:300], scene.events.polarity[:300], np.full(300, 5_000, np.int64))
    m.set_sequence(still)
    one = m.estimate_angular_velocity(150, 8.0)
    assert np.array_equal(one["omega"], np.zeros((2, 3))) and np.array_equal(one["evals"], [1, 1]) and np.array_equal(one["J"], one["J0"]) and (one["J0"] > 0).all()
    m.free_sequence()
    with pytest.raises(EmbaError) as ei:
        m.estimate_angular_velocity(150, 8.0)
    assert ei.value.status == ERR_STATE
    m.close()


@pytest.mark.parametrize("slice_events", [2000, 777])
def test_estimate_against_the_true_body_rate(gpu, scene, slice_events):
    """|omega_s - the simulator's body rate at the middle of slice s| <= twice the worst error the numpy form made on the CPU (cmax_cases.SCENE_WORST,
    DESIGN.md §11).  The scene turns at 1.1 - 1.9 rad/s (0.4 - 1.45 px inside a slice); on its events the objective is larger at omega = 0 than at the true
    rate (cause not established), so the bound is several times the rate itself: it records what the estimator does on this recording, not that it is good
    on it."""
    m = make_legm(64, 48, scene.lut)
    m.set_sequence(scene.events)
    got = m.estimate_angular_velocity(slice_events, CC.OMEGA_MAX)
    err = CC.slice_errors(got["omega"], scene.events.t_ns, slice_events, scene.traj)
    print(f"slice_events {slice_events}: worst {err.max()!r} median {np.median(err)!r} rad/s, bound {CC.SCENE_BOUND[slice_events]!r}")
    assert err.max() <= CC.SCENE_BOUND[slice_events]
    m.close()


def test_whole_run_without_front_end_poses(gpu):
    """The demo recording of examples/run_ba.py (128x96, 0.5 s) refined in sliding windows from its events alone: init_poses = "events" and
    init_map = "events".  The run completes, no window ends above its initial cost, and the integrated initial poses and the refined trajectory both have
    a finite rotation error against truth (relative to the first control pose: the estimate starts at the identity) — figures in DESIGN.md §11, no bound."""
    w = synth.make_scene_workload(pano_h=512, K=11, sensor=(128, 96), focal=120.0, n_steps=2000)
    from emba_amd import LEGM
    m = LEGM(w.sensor_w, w.sensor_h, w.lut, w.C_th, w.pano_w, w.pano_h, device=0)
    t0, t1 = w.traj.t0_ns * 1e-9, (w.traj.t0_ns + w.traj.dt_ns * (w.K - 1)) * 1e-9
    seq = SequenceSettings(time_window_size=0.3, sliding_window_stride=0.1, dt_knots=0.05, t_start=t0, t_end=t1, init_map="events", init_poses="events")
    res = run_sequence(m, w.events, None, None, None, None, seq, BASettings(alpha=0.0), LMSettings(max_num_iter=10))
    assert len(res.windows) == 3 and res.cmax is not None and len(res.cmax["omega"]) == w.events.size() // 10000
    want = eio.estimate_angular_velocity(w.events, w.lut, w.sensor_w, w.sensor_h, 10000, 8.0)
    assert np.array_equal(res.cmax["omega"], want["omega"]) and np.array_equal(res.cmax["evals"], want["evals"])
    for wr in res.windows:
        assert wr.result.log and wr.result.cost_min <= wr.result.log[0][2]
    tq = w.traj.t0_ns + w.traj.dt_ns * np.arange(res.traj.size(), dtype=np.int64)
    _, q_init = eio.integrate_angular_velocity(res.cmax["omega"], res.cmax["t_ref_ns"], tq)

    def err_deg(knots):
        rel = lambda k: [so3.mul(so3.inverse(k[0]), q) for q in k]
        return float(np.degrees(np.mean([np.linalg.norm(so3.log(so3.mul(so3.inverse(p), q))) for p, q in zip(rel(knots), rel(w.traj.knots_xyzw))])))
    e_init, e_ref = err_deg(q_init), err_deg(res.traj.knots_xyzw)
    print(f"mean control-pose error vs truth: integrated initial poses {e_init:.4f} deg, refined {e_ref:.4f} deg")
    assert np.isfinite(e_init) and np.isfinite(e_ref) and np.isfinite(res.traj.knots_xyzw).all()
    m.close()
