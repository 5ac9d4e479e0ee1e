"""The sliding-window driver (emba_amd/driver.py, restating EMBA::EMBA + EMBA::Run, emba.cpp:281-304, 357-364, 400-532) and the numpy forms of its
three sequence-level rules (emba_amd/io.py), on the CPU: against the loop-for-loop restatements of tests/sequence_ref.py, and end to end on the oracle
model.  tests/test_gpu_sequence.py runs the same on the device forms."""
import re

import numpy as np
import pytest

import sequence_ref as SR
from emba_amd import io as eio, so3, synth
from emba_amd.driver import SequenceSettings, run_sequence
from emba_amd.legm import EventPacket, LinearTrajectory
from emba_amd.solver import BASettings, LMSettings, MapRecorder, RuntimeLog, solve_time_window
from helpers import OracleModel
from test_lm_solver_cpu import perturbed

MS = 1_000_000


# ---- inputs shared with tests/test_gpu_sequence.py -------------------------------------------------------------------------------
def window_cases(t):
    """(t_beg_ns, t_end_ns) pairs around sorted timestamps t: before, inside, across either end and past the data, margins on and off a probe."""
    t0, t1 = int(t[0]), int(t[-1])
    span = max(t1 - t0, 10 * MS)
    cases = [(t0 - 50 * MS, t0 - 10 * MS), (t0 - 50 * MS, t0 + span // 2), (t0 + span // 4, t0 + 3 * span // 4), (t0 + span // 2, t1 + 50 * MS),
             (t1 + 10 * MS, t1 + 50 * MS), (t0 - 5 * MS, t1 + 5 * MS), (t0, t1), (t0 + span // 3, t0 + span // 3 + MS), (t0 + span // 3, t0 + span // 3 + 2 * MS),
             (t0 - MS, t0 + span // 5), (t1 - MS, t1 + 3 * MS)]
    for j in (100, 200, 300):       # the margins land exactly on a probe's timestamp (strict comparisons)
        if j < len(t):
            cases += [(int(t[j]) - MS, t1 + 5 * MS), (t0 - 5 * MS, int(t[j]) + MS), (int(t[j]) - MS - 1, int(t[j]) + MS + 1)]
    return cases


def timestamp_sets():
    rng = np.random.default_rng(11)
    sets = {}
    for n in (1000, 1234, 57, 100, 99, 101):
        sets[f"n{n}"] = np.sort(rng.integers(10**9, 10**9 + 400 * MS, size=n)).astype(np.int64)
    ties = np.sort(rng.integers(10**9, 10**9 + 400 * MS, size=1500)).astype(np.int64)
    ties[95:106] = ties[100]            # ties in timestamps across a multiple of 100
    ties[400:420] = ties[400]
    sets["ties"] = ties
    return sets


def blur_planes():
    rng = np.random.default_rng(3)
    planes = {}
    for shape in ((1, 7), (7, 1), (2, 2), (75, 150)):
        a = rng.normal(size=shape)
        planes["normal%dx%d" % shape] = a
        b = rng.integers(-2, 3, size=shape).astype(np.float64)       # repeated values ...
        b[b == 0] = np.where(rng.random(int((b == 0).sum())) < 0.5, -0.0, 0.0)   # ... and both zeros
        planes["repeats%dx%d" % shape] = b
        planes["tiny%dx%d" % shape] = a * 1e-30 + 1.0                     # values that collapse in float32
    return planes


def expect_window(t, tb, te):
    try:
        return SR.event_subset(t, tb, te)
    except SR.NoEvents:
        return None


def raw_poses(traj, step_ns=5 * MS):
    """The front end's poses: the trajectory sampled every 5 ms (9 poses strictly inside every 50-ms knot interval, fitCtrlPoses needs 2)."""
    n = (traj.dt_ns * (traj.size() - 1)) // step_ns
    t_ns = traj.t0_ns + step_ns * np.arange(n, dtype=np.int64)
    return t_ns * 1e-9, np.array([so3.spline_evaluate(traj.knots_xyzw, traj.t0_ns, traj.dt_ns, int(t)) for t in t_ns])


def three_window_case():
    """0.1 ... 0.7 s at dt_knots 0.05 (K = 13); windows of 0.3 s every 0.15 s: cp_stride 3, 7 control poses per window, 3 windows."""
    w = synth.make_scene_workload(K=13, n_steps=2000)
    pose_t, pose_q = raw_poses(perturbed(w))
    seq = SequenceSettings(time_window_size=0.3, sliding_window_stride=0.15, dt_knots=0.05, event_sampling_rate=1, t_start=0.1, t_end=0.7, median_blur=True)
    return w, pose_t, pose_q, seq


# ---- 1. the three rules ---------------------------------------------------------------------------------------------------------------
def test_event_window_matches_the_restatement():
    n_ok = n_none = 0
    for name, t in timestamp_sets().items():
        rng = np.random.default_rng(len(t))
        cases = window_cases(t) + [tuple(sorted(int(v) for v in rng.integers(int(t[0]) - 20 * MS, int(t[-1]) + 20 * MS, size=2))) for _ in range(60)]
        for tb, te in cases:
            want = expect_window(t, tb, te)
            if want is None:
                n_none += 1
                with pytest.raises(ValueError, match="no events"):
                    eio.event_window(t, tb, te)
            else:
                n_ok += 1
                assert eio.event_window(t, tb, te) == want, (name, tb, te)
    assert n_ok > 100 and n_none > 20


def test_downsample_matches_the_restatement():
    rng = np.random.default_rng(2)
    for n in (0, 1, 6, 1000, 1001, 1006):
        ev = EventPacket(rng.integers(0, 64, n).astype(np.uint16), rng.integers(0, 48, n).astype(np.uint16), rng.integers(0, 2, n).astype(np.uint8),
                         np.sort(rng.integers(0, 10**9, n)).astype(np.int64))
        for rate in (0, 1, 2, 3, 7):
            got = eio.downsample_events(ev, rate)
            want = SR.downsample(ev.x, ev.y, ev.polarity, ev.t_ns, rate)
            assert got.size() == (n // rate if rate >= 2 else n)
            for g, o in zip((got.x, got.y, got.polarity, got.t_ns), want):
                assert np.array_equal(g, o), (n, rate)


def test_median_blur3_matches_the_restatement():
    for name, a in blur_planes().items():
        want = SR.median_blur3(a)
        assert np.array_equal(eio.median_blur3(a), want), name           # (== : -0.0 and +0.0 count as equal)
        assert np.array_equal(SR.median_blur3_fast(a), want), name
        assert eio.median_blur3(a).dtype == np.float64
    a = blur_planes()["normal75x150"]
    assert not np.array_equal(eio.median_blur3(a), a) and np.isin(eio.median_blur3(a), a.astype(np.float32).astype(np.float64)).all()


def test_ros_time_ns():
    assert eio.ros_time_ns(0.1) == 100 * MS and eio.ros_time_ns(0.3) == 300 * MS and eio.ros_time_ns(1e-3) == MS and eio.ros_time_ns(1e-6) == 1000
    assert eio.ros_time_ns(1468939802.884364206) == 1468939802884364128      # nsec = round((t - floor(t)) * 1e9) of the nearest double
    assert eio.ros_time_ns(1.9999999999) == 2_000_000_000                     # carry


# ---- 2. one window == today's direct call ----------------------------------------------------------------------------------------------
def test_one_window_sequence_equals_the_direct_call(oracle_mod):
    w = synth.make_scene_workload(n_steps=1000)                              # K = 6: 0.1 ... 0.35 s
    pose_t, pose_q = raw_poses(perturbed(w))
    ba, lm = BASettings(alpha=1.0), LMSettings(max_num_iter=8)
    seq = SequenceSettings(time_window_size=0.35 - 0.1, sliding_window_stride=0.35 - 0.1, dt_knots=0.05, t_start=0.1, t_end=0.35, median_blur=False)
    ms = OracleModel(oracle_mod, w)
    rs = run_sequence(ms, w.events, pose_t, pose_q, w.Gx, w.Gy, seq, ba, lm, resident=False)
    assert len(rs.windows) == 1
    beg, end = rs.windows[0].beg, rs.windows[0].end
    assert (beg, end) == SR.event_subset(w.events.t_ns, 100 * MS, 350 * MS) and end - beg > 10000
    t_b, t_e = eio.ros_time_ns(0.1) * 1e-9, (eio.ros_time_ns(0.1) + eio.ros_time_ns(0.35 - 0.1)) * 1e-9
    sel = (pose_t > t_b) & (pose_t < t_e)
    traj = LinearTrajectory.from_seconds(0.1, 0.05, eio.generate_ctrl_poses_long(pose_t[sel], pose_q[sel], t_b, t_e, 0.05, 0.05))
    assert traj.size() == 6 and traj.t0_ns == rs.traj.t0_ns and traj.dt_ns == rs.traj.dt_ns
    md = OracleModel(oracle_mod, w)
    rd = solve_time_window(md, traj, eio.slice_events(w.events, beg, end), w.Gx, w.Gy, ba, lm)
    assert rs.windows[0].result.log == rd.log and len(rd.log) >= 2 and any(e[4] for e in rd.log)
    assert np.array_equal(rs.traj.knots_xyzw, rd.traj.knots_xyzw)
    for a, b in zip(ms.downloadMap(), md.downloadMap()):
        assert np.array_equal(a, b)


# ---- 3. three overlapping windows -------------------------------------------------------------------------------------------------------
class Spy(OracleModel):
    """Records what the driver hands the model window by window: the map at every registration, fix_first_pose and x1 of every solve."""

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.maps, self.solves, self.win = [], [], -1

    def set_events(self, ev):
        self.win += 1
        self.maps.append(None if self.cur is None else (self.cur[0].copy(), self.cur[1].copy()))
        super().set_events(ev)

    def solveNormalEq(self, lam, fix_first_pose=False):
        x1, x2 = super().solveNormalEq(lam, fix_first_pose)
        self.solves.append((self.win, bool(fix_first_pose), np.array(x1)))
        return x1, x2


def test_three_overlapping_windows_on_the_oracle(oracle_mod, tmp_path, monkeypatch):
    w, pose_t, pose_q, seq = three_window_case()
    rendered = []
    monkeypatch.setattr(Spy, "renderMapImages", lambda self, pct, poisson=True: rendered.append(1) or
                        {k: np.zeros((4, 8, 3) if k == "G_hsv" else (4, 8), np.uint8) for k in ("Gx", "Gy", "G_hsv", "map_poisson")}, raising=False)
    m = Spy(oracle_mod, w)
    rl, mr = RuntimeLog(str(tmp_path)), MapRecorder(str(tmp_path))
    ba, lm = BASettings(alpha=1.0), LMSettings(max_num_iter=10)
    r = run_sequence(m, w.events, pose_t, pose_q, w.Gx, w.Gy, seq, ba, lm, runtime_log=rl, map_recorder=mr, resident=False)
    mr.close()
    n_win = len(r.windows)
    assert n_win == 3                                                                   # the loop runs exactly three windows
    for k, win in enumerate(r.windows):                                                 # ... and none of them is degenerate
        assert any(e[4] for e in win.result.log), f"window {k} accepted no LM step"
        assert win.index == k and win.idx_cp_beg == 3 * k and win.traj_init.size() == 7
        assert (win.t_beg_ns, win.t_end_ns) == ((100 + 150 * k) * MS, (400 + 150 * k) * MS)
        assert (win.beg, win.end) == SR.event_subset(w.events.t_ns, win.t_beg_ns, win.t_end_ns) and win.end - win.beg > 5000
        assert win.traj_init.t0_ns == int(1e9 * (0.1 + 3 * k * 0.05)) and win.traj_init.dt_ns == 50 * MS
    assert r.windows[0].beg == 0 and r.windows[1].beg < r.windows[0].end                # they overlap
    assert r.traj.size() == 7 + 2 * 3 and r.traj.t0_ns == 100 * MS
    assert np.allclose(np.linalg.norm(r.traj.knots_xyzw, axis=1), 1.0, atol=1e-12)
    # control poses in front of a window are not touched by it: what window k - 1 left there is in the final trajectory, bit for bit
    for k in (1, 2):
        prev = r.windows[k - 1]
        assert np.array_equal(r.traj.knots_xyzw[prev.idx_cp_beg:3 * k], prev.result.traj.knots_xyzw[:3 * k - prev.idx_cp_beg])
        # ... and the overlap enters window k as window k - 1 left it
        assert np.array_equal(r.windows[k].traj_init.knots_xyzw[:4], prev.result.traj.knots_xyzw[3:7])
    assert np.array_equal(r.traj.knots_xyzw[6:], r.windows[2].result.traj.knots_xyzw)
    # first_time_window for window 0 only: the first pose is held there and free afterwards
    for k in range(3):
        s = [(f, x1) for (wi, f, x1) in m.solves if wi == k]
        assert s and all(f == (k == 0) for f, _ in s)
        if k:
            assert any(np.abs(x1[0:3]).max() > 0 for _, x1 in s)
        else:
            assert all(np.array_equal(x1[0:3], np.zeros(3)) for _, x1 in s)
    assert np.array_equal(r.windows[0].result.traj.knots_xyzw[0], r.windows[0].traj_init.knots_xyzw[0])
    # the map is carried: window 0 starts from the blurred initial map, window k + 1 from what window k left
    assert m.maps[0] is None
    for k in (1, 2):
        fresh = OracleModel(oracle_mod, w)
        win = r.windows[k]
        fresh.set_events(eio.slice_events(w.events, win.beg, win.end))
        ep = fresh.evaluateDataError(win.traj_init, *m.maps[k])
        cost = fresh.dataCost() + fresh.regCost(ba.alpha)
        assert win.result.log[0][2] == cost and ep.size > 0
    fresh = OracleModel(oracle_mod, w)
    fresh.set_events(eio.slice_events(w.events, r.windows[0].beg, r.windows[0].end))
    fresh.evaluateDataError(r.windows[0].traj_init, SR.median_blur3_fast(w.Gx), SR.median_blur3_fast(w.Gy))
    assert r.windows[0].result.log[0][2] == fresh.dataCost() + fresh.regCost(ba.alpha)
    # ONE log / recorder for the run
    it = (tmp_path / "final_results" / "iterations.txt").read_text()
    assert re.findall(r"^window #(\d+)$", it, flags=re.M) == ["1", "2", "3"]
    wins = sorted({re.match(r"win_(\d{4})_", p.name).group(1) for p in (tmp_path / "map_opt").iterdir()})
    assert wins == ["0000", "0001", "0002"] and rendered
    n_solves = int((tmp_path / "final_results" / "runtime_solveEqs.txt").read_text().splitlines()[-1].split("count_solveEqs = ")[1].split()[0])
    assert n_solves == sum(win.result.iterations for win in r.windows)


def test_host_slices_with_down_sampling(oracle_mod):
    """rate 2 on the host path: the windows are cut from the down-sampled sequence."""
    w, pose_t, pose_q, seq = three_window_case()
    seq.event_sampling_rate = 2
    r = run_sequence(OracleModel(oracle_mod, w), w.events, pose_t, pose_q, w.Gx, w.Gy, seq, BASettings(alpha=1.0), LMSettings(max_num_iter=2), resident=False)
    t2 = SR.downsample(w.events.x, w.events.y, w.events.polarity, w.events.t_ns, 2)[3]
    assert r.n_events == w.events.size() // 2 and len(r.windows) == 3
    for win in r.windows:
        assert (win.beg, win.end) == SR.event_subset(t2, win.t_beg_ns, win.t_end_ns)


# ---- 4. the host spline evaluation ---------------------------------------------------------------------------------------------------
def test_host_spline_evaluation_matches_the_reference_build(oracle_mod):
    """so3.spline_evaluate (what pose_latest is taken with, emba.cpp:459-460) against basalt's So3Spline<2>::evaluate — the reference build under
    oracle/_ref where it exists, else the oracle's restatement, which tests/test_oracle_pinned.py pins to that build bit for bit.  Bound: the two sides
    evaluate the same formula in fp64 with differently ordered products and one extra normalisation — a few dozen roundings of 1.1e-16 on values of
    magnitude <= pi; 1e-13 leaves two orders of magnitude."""
    O = oracle_mod
    use_ref = O.ref_available()
    traj = perturbed(synth.make_scene_workload(K=13, n_steps=10), sigma=0.2)
    t0, dt, K = traj.t0_ns, traj.dt_ns, traj.size()
    times = [t0 + dt * s for s in range(K - 1)] + [t0 + dt * s + dt // 2 for s in range(K - 1)] + [t0 + dt * s + 12345677 for s in range(K - 1)]
    times += [t0 + dt * (K - 1) - 1000, t0 + dt * (K - 1) - 1, t0 + dt * 7 - 1000]          # 1 us before the last knot (pose_latest) and before an inner one
    for t in times:
        q_ref = O.spline_eval(traj.knots_xyzw, t0, dt, t, use_ref=use_ref)[0]
        q = so3.spline_evaluate(traj.knots_xyzw, t0, dt, t)
        assert min(np.abs(q - q_ref).max(), np.abs(q + q_ref).max()) < 1e-13, t
        assert np.array_equal(q, traj.evaluate(t))
    assert np.array_equal(so3.spline_evaluate(traj.knots_xyzw, t0, dt, t0 + 3 * dt), so3.normalize(so3.mul(traj.knots_xyzw[3], so3.exp(np.zeros(3)))))
    for t in (t0 - 1, t0 + dt * (K - 1)):
        with pytest.raises(ValueError):
            so3.spline_evaluate(traj.knots_xyzw, t0, dt, t)
