"""Contrast maximisation without a GPU: the numpy form of the rule (emba_amd.io: cmax_objective, estimate_angular_velocity, integrate_angular_velocity),
the HIP-free rule header (emba_amd/csrc/cmax_rule.h through tests/cpp/cmax_rule_test.cpp), the new symbols of libemba_hip.so, and the sliding-window
driver started without front-end poses on the oracle model."""
import os
import subprocess

import numpy as np
import pytest

import cmax_cases as CC
from emba_amd import io as eio
from emba_amd import so3, synth
from emba_amd.driver import SequenceSettings, run_sequence
from emba_amd.legm import EventPacket
from emba_amd.solver import BASettings, LMSettings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cmax_rule_on_the_cpu(tmp_path):
    """emba_amd/csrc/cmax_rule.h (plain C++17, no HIP): tests/cpp/cmax_rule_test.cpp checks shift and grid of 64x48, 240x180, 346x260 and 640x480, the slice
    count, the argument checks, the search's schedule against its evaluation cap, and the pinhole fit on known pinholes; the fit it prints is compared
    here with io.cmax_pinhole_fit bit for bit, and the grids with io.cmax_grid."""
    exe = str(tmp_path / "cmax_rule_test")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-ffp-contract=off", os.path.join(ROOT, "tests", "cpp", "cmax_rule_test.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout[-3000:], r.stderr)
    lines = r.stdout.strip().splitlines()
    assert r.returncode == 0 and lines[-1] == "OK cmax_rule", r.stdout[-3000:] + r.stderr
    fit = [float(v) for v in [l for l in lines if l.startswith("FIT ")][0].split()[1:]]
    assert tuple(fit) == eio.cmax_pinhole_fit(synth.pinhole_bearing_lut(63, 47, 60.0, 60.0, 31.5, 23.5), 63, 47)
    assert [eio.cmax_grid(w, h) for w, h in ((64, 48), (240, 180), (346, 260), (640, 480))] == [(0, 64, 48), (1, 120, 90), (2, 87, 65), (3, 80, 60)]


def test_new_symbols_resolve(hip_lib):
    assert hasattr(hip_lib, "emba_seq_cmax") and hasattr(hip_lib, "emba_seq_cmax_objective")
    from emba_amd import LEGM
    assert callable(LEGM.estimate_angular_velocity) and callable(LEGM.cmax_objective)
    blob = open(os.path.join(ROOT, "emba_amd", "libemba_hip.so"), "rb").read()
    assert b"emba_cmax_search_kernel" in blob and b"emba_cmax_objective_kernel" in blob


def test_objective_by_hand():
    """Three events on a 4x3 sensor, f = 1, centre (1.5, 1): the votes of the rule written out."""
    lut = synth.pinhole_bearing_lut(4, 3, 1.0, 1.0, 1.5, 1.0)
    assert eio.cmax_pinhole_fit(lut, 4, 3) == (1.0, 1.5, 1.0)
    ev = EventPacket(np.array([0, 0, 3], np.uint16), np.array([0, 0, 2], np.uint16), np.zeros(3, np.uint8), np.array([10, 20, 30], np.int64))
    J, iwe = eio.cmax_objective(ev, lut, 4, 3, [[0, 0, 0]])
    want = np.zeros((3, 4), np.uint32)
    want[0, 0], want[2, 3] = 512, 256                          # unwarped events sit on their pixels with the whole vote
    assert np.array_equal(iwe[0], want) and J[0] == 512 * 512 + 256 * 256
    # a rotation about the optical axis by 2 atan(wz dt / 2): with wz dt / 2 = 1 a quarter turn, x' = -y, y' = x about the centre (1.5, 1)
    ev = EventPacket(np.array([1, 2], np.uint16), np.array([1, 1], np.uint16), np.zeros(2, np.uint8), np.array([0, 2_000_000_000], np.int64))
    J, iwe = eio.cmax_objective(ev, lut, 4, 3, [[0, 0, 1.0]])
    # the first event is the reference: not moved.  The second: (0.5, 0, 1) turned a quarter about z is (0, 0.5, 1): u = 1.5, v = 1.5 -> wx = wy = 8: 64 each on (1,1), (2,1), (1,2), (2,2)
    want = np.zeros((3, 4), np.uint32)
    want[1, 1] = 256 + 64; want[1, 2] = 64; want[2, 1] = 64; want[2, 2] = 64
    assert np.array_equal(iwe[0], want) and J[0] == 320 * 320 + 3 * 64 * 64
    # every event leaves the grid / turns behind the plane: J = 0
    ev = EventPacket(np.array([3, 0], np.uint16), np.array([1, 1], np.uint16), np.zeros(2, np.uint8), np.array([0, 1_000_000_000], np.int64))
    J, iwe = eio.cmax_objective(ev, lut, 4, 3, [[0, 2.0, 0]], beg=1, end=2)
    assert J[0] == 256 * 256                                    # (a range of one event: dt = 0, never moved)
    J, _ = eio.cmax_objective(ev, lut, 4, 3, [[0, 2.0, 0], [0, -2.0, 0], [0, 200.0, 0]])
    assert J[0] != J[1] and J[2] == 256 * 256                   # a half-turn-and-more about y: only the reference event still votes
    assert eio.cmax_objective(ev, lut, 4, 3, [[1, 2, 3]], beg=1, end=1)[0][0] == 0
    with pytest.raises(ValueError):
        eio.cmax_objective(ev, lut, 4, 3, [[0, 0, 0]], beg=2, end=1)
    with pytest.raises(ValueError):
        eio.cmax_objective(ev, lut, 4, 3, [[np.nan, 0, 0]])


def test_numpy_rule_recovers_a_constant_rate():
    """Scene points seen by a camera turning at a constant body rate: every slice's estimate lies within twice the error measured once on this input
    (cmax_cases.CONST_WORST), the objective rose, and the search kept to its schedule."""
    ev, lut = CC.constant_rate_events(CC.CONST_OMEGA)
    est = eio.estimate_angular_velocity(ev, lut, 64, 48, CC.CONST_SLICE, CC.OMEGA_MAX)
    ns = ev.size() // CC.CONST_SLICE
    assert ns == 3 and est["omega"].shape == (ns, 3) and est["t_ref_ns"].shape == (ns + 1,)
    err = np.linalg.norm(est["omega"] - CC.CONST_OMEGA, axis=1)
    print("errors (rad/s):", err, "bound", CC.CONST_BOUND)
    assert err.max() <= CC.CONST_BOUND
    assert (est["J"] > est["J0"]).all() and (est["evals"] % 6 == 1).all() and (est["evals"] <= 1 + 6 * eio.CMAX_MAX_ITER).all()
    assert np.array_equal(est["t_ref_ns"][:ns], ev.t_ns[0:ns * CC.CONST_SLICE:CC.CONST_SLICE]) and est["t_ref_ns"][ns] == ev.t_ns[ns * CC.CONST_SLICE - 1]
    assert np.array_equal(est["omega"] * 4096.0 / CC.OMEGA_MAX, np.rint(est["omega"] * 4096.0 / CC.OMEGA_MAX))      # exact multiples of the last step
    # fewer events than one slice: nothing is estimated; a slice of one instant: omega = 0 after one evaluation
    few = eio.estimate_angular_velocity(ev, lut, 64, 48, ev.size() + 1, CC.OMEGA_MAX)
    assert few["omega"].shape == (0, 3) and few["t_ref_ns"].size == 0
    still = EventPacket(ev.x[:50], ev.y[:50], ev.polarity[:50], np.full(50, 7, np.int64))
    one = eio.estimate_angular_velocity(still, lut, 64, 48, 50, CC.OMEGA_MAX)
    assert np.array_equal(one["omega"], np.zeros((1, 3))) and one["evals"][0] == 1 and one["J"][0] == one["J0"][0] > 0
    for bad in ((0, 8.0), (-5, 8.0), (10, 0.0), (10, -1.0), (10, np.inf), (10, np.nan), (1 << 24, 8.0)):
        with pytest.raises(ValueError):
            eio.estimate_angular_velocity(ev, lut, 64, 48, *bad)


def test_integration_against_so3():
    rng = np.random.default_rng(4)
    omega = rng.normal(size=(5, 3))
    t_ref = np.array([100, 150, 230, 300, 420, 470], np.int64) * 1_000_000
    pt, pq = eio.integrate_angular_velocity(omega, t_ref)
    assert np.array_equal(pt, t_ref * 1e-9) and np.array_equal(pq[0], [0, 0, 0, 1])
    q = np.array([0.0, 0.0, 0.0, 1.0])
    for s in range(5):
        q = so3.mul(q, so3.exp(omega[s] * ((t_ref[s + 1] - t_ref[s]) * 1e-9)))
        assert np.allclose(pq[s + 1], q, atol=1e-15)
        # body frame: the relative rotation over the slice is exp(omega dt) on the right
        assert np.allclose(so3.log(so3.mul(so3.inverse(pq[s]), pq[s + 1])), omega[s] * ((t_ref[s + 1] - t_ref[s]) * 1e-9), atol=1e-13)
    # at given times: inside a slice, at a boundary, in front of the first slice and behind the last estimated event (first / last velocity)
    tq = np.array([175, 230, 60, 500], np.int64) * 1_000_000
    _, qq = eio.integrate_angular_velocity(omega, t_ref, tq)
    assert np.allclose(qq[0], so3.mul(pq[1], so3.exp(omega[1] * 0.025)), atol=1e-15) and np.allclose(qq[1], pq[2], atol=1e-15)
    assert np.allclose(qq[2], so3.exp(omega[0] * -0.040), atol=1e-15) and np.allclose(qq[3], so3.mul(pq[4], so3.exp(omega[4] * 0.080)), atol=1e-15)
    # a constant rate is one rotation about one axis
    _, pq = eio.integrate_angular_velocity(np.tile([0.0, 0.5, 0.0], (4, 1)), np.arange(5, dtype=np.int64) * 10**9)
    assert np.allclose(so3.log(pq[-1]), [0, 2.0, 0], atol=1e-13)
    with pytest.raises(ValueError):
        eio.integrate_angular_velocity(omega, t_ref[:-1])
    with pytest.raises(ValueError):
        eio.integrate_angular_velocity(np.zeros((0, 3)), np.zeros(0, np.int64))


def test_sequence_settings_validation():
    s = SequenceSettings(0.1, 0.05)
    assert s.init_poses == "given" and s.cmax_slice_events == 10000 and s.cmax_omega_max == 8.0
    SequenceSettings(0.1, 0.05, init_poses="events", cmax_slice_events=1, cmax_omega_max=0.5)
    for kw in (dict(init_poses="cmax"), dict(cmax_slice_events=0), dict(cmax_omega_max=0.0), dict(cmax_omega_max=float("nan")), dict(cmax_omega_max=float("inf"))):
        with pytest.raises(ValueError):
            SequenceSettings(0.1, 0.05, **kw)


def test_run_sequence_without_front_end_poses_on_the_oracle_model(oracle_mod):
    """run_sequence(init_poses = "events") through the numpy path: the oracle model has no resident sequence, the camera comes from its attributes.  The run
    completes, keeps the estimate on the result, starts from exactly the poses io.integrate_angular_velocity makes of it, and no window ends above its
    initial cost."""
    from helpers import OracleModel
    w = synth.make_scene_workload(n_steps=1000)
    om = OracleModel(oracle_mod, w)
    t0, t1 = w.traj.t0_ns * 1e-9, (w.traj.t0_ns + w.traj.dt_ns * (w.K - 1)) * 1e-9
    seq = SequenceSettings(time_window_size=0.15, sliding_window_stride=0.1, dt_knots=0.05, t_start=t0, t_end=t1, median_blur=False, init_poses="events",
                           cmax_slice_events=2000, cmax_omega_max=CC.OMEGA_MAX)
    with pytest.raises(ValueError):                      # (no camera on the model, no resident sequence: nothing to estimate with)
        run_sequence(om, w.events, None, None, w.Gx, w.Gy, seq, BASettings(alpha=0.0), LMSettings(max_num_iter=3), resident=False)
    with pytest.raises(ValueError):                      # init_poses = "given" still wants its poses
        run_sequence(om, w.events, None, None, w.Gx, w.Gy, SequenceSettings(0.15, 0.1, t_start=t0, t_end=t1), BASettings(alpha=0.0), LMSettings(max_num_iter=3), resident=False)
    om.bearing_lut, om.sensor_w, om.sensor_h = w.lut, w.sensor_w, w.sensor_h
    res = run_sequence(om, w.events, None, None, w.Gx, w.Gy, seq, BASettings(alpha=0.0), LMSettings(max_num_iter=3), resident=False)
    want = eio.estimate_angular_velocity(w.events, w.lut, w.sensor_w, w.sensor_h, 2000, CC.OMEGA_MAX)
    for k in ("omega", "t_ref_ns", "J0", "J", "evals"):
        assert np.array_equal(res.cmax[k], want[k]), k
    assert len(res.windows) == 2 and np.isfinite(res.traj.knots_xyzw).all()
    first = res.windows[0].traj_init.knots_xyzw
    assert np.allclose(np.linalg.norm(first, axis=1), 1.0)
    for wr in res.windows:
        assert wr.result.log and wr.result.cost_min <= wr.result.log[0][2]      # (log[0][2]: the cost at the window's initial poses)


def test_sharded_hosts_forward_the_estimate_or_fall_back_to_numpy():
    """ShardedModel -> ShardedLEGM -> engine: an engine with a resident sequence is asked itself (every rank its own: equal copies, a deterministic rule);
    over an engine without one the driver takes the numpy path with the camera the rank's model knows, and says so where it knows none."""
    from types import SimpleNamespace
    from emba_amd.driver import estimate_raw_poses, keeps_sequence
    from emba_amd.sharded import HipEngine, ShardedLEGM, ShardedModel
    ev, lut = CC.constant_rate_events(CC.CONST_OMEGA)
    want = eio.estimate_angular_velocity(ev, lut, 64, 48, CC.CONST_SLICE, CC.OMEGA_MAX)
    calls = []

    class DeviceEngine:                                   # what HipEngine forwards to: a model that keeps the sequence
        def bind_exchange(self, count, pack):
            pass

        def set_sequence(self, events, sampling_rate=1):
            return events.size()

        def estimate_angular_velocity(self, slice_events, omega_max):
            calls.append((slice_events, omega_max))
            return want

    class Engine:                                         # no resident sequence
        def bind_exchange(self, count, pack):
            pass
    dist = SimpleNamespace(get_rank=lambda: 1, get_world_size=lambda: 3)
    seq = SequenceSettings(0.1, 0.1, t_start=1.0, t_end=1.15, init_poses="events", cmax_slice_events=CC.CONST_SLICE, cmax_omega_max=CC.OMEGA_MAX)
    host = ShardedModel(ShardedLEGM(DeviceEngine(), dist, None, None, 64), SimpleNamespace(H=4, W=8))
    got = estimate_raw_poses(host, None, seq, keeps_sequence(host))
    assert calls == [(CC.CONST_SLICE, CC.OMEGA_MAX)] and got["omega"] is want["omega"] and len(got["pose_t"]) == len(got["pose_q"]) > 10
    eng = HipEngine.__new__(HipEngine)                    # (its constructor wants a context on a GPU: the forwarding method alone)
    eng.m = DeviceEngine()
    assert eng.estimate_angular_velocity(5, 2.0) is want and calls[-1] == (5, 2.0)
    legm = SimpleNamespace(H=4, W=8, bearing_lut=lut, sensor_w=64, sensor_h=48)
    host = ShardedModel(ShardedLEGM(Engine(), dist, None, None, 64), legm)
    assert not keeps_sequence(host)
    got = estimate_raw_poses(host, ev, seq, False)
    assert np.array_equal(got["omega"], want["omega"]) and np.array_equal(got["evals"], want["evals"])
    with pytest.raises(ValueError):
        estimate_raw_poses(ShardedModel(ShardedLEGM(Engine(), dist, None, None, 64), SimpleNamespace(H=4, W=8)), ev, seq, False)
