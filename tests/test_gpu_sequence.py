"""The device forms of the sliding-window run (include/emba_hip.h: emba_seq_*, emba_set_events_seq, emba_median_blur3[_map]) on the MI355X: against
the loop-for-loop restatements of tests/sequence_ref.py, against the oracle on the host slice of every window, and the three-window run of
emba_amd/driver.py against the same driver on the oracle model."""
import os
import subprocess
import sys

import numpy as np
import pytest

import sequence_ref as SR
from emba_amd import io as eio
from emba_amd.driver import run_sequence
from emba_amd.legm import EventPacket, EventWindow
from emba_amd.solver import BASettings, LMSettings
from helpers import OracleModel, assert_close_elementwise, oracle_run, small_workload
from test_sequence_cpu import MS, blur_planes, expect_window, three_window_case, timestamp_sets, window_cases

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_INVALID_ARG, ERR_STATE = 1, 5


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from emba_amd import build
    build.build_hip()
    return True


def make_legm(w, **options):
    from emba_amd import LEGM
    m = LEGM(w.sensor_w, w.sensor_h, w.lut, w.C_th, w.pano_w, w.pano_h, device=0)
    for k, v in options.items():
        m.set_option(k, v)
    return m


def packet(n, sw, sh, seed, t_span=400 * MS):
    rng = np.random.default_rng(seed)
    return EventPacket(rng.integers(0, sw, n).astype(np.uint16), rng.integers(0, sh, n).astype(np.uint16), rng.integers(0, 2, n).astype(np.uint8),
                       np.sort(rng.integers(10**9, 10**9 + t_span, size=n)).astype(np.int64))


# ---- 5. median blur -------------------------------------------------------------------------------------------------------------------
def test_median_blur3_equals_the_restatement(gpu):
    from emba_amd import EmbaError
    w = small_workload(n_events=2000)
    m = make_legm(w)
    for name, a in blur_planes().items():
        assert np.array_equal(m.medianBlur3(a), SR.median_blur3(a)), name               # exact (== : -0.0 and +0.0 count as equal)
    big = np.random.default_rng(8).normal(size=(1024, 2048))
    big[100:140, 200:260] = 0.25                                                        # a flat patch: repeated values
    assert np.array_equal(m.medianBlur3(big), SR.median_blur3_fast(big))
    # the resident map, both planes, in place
    with pytest.raises(EmbaError) as ei:
        m.median_blur_map()
    assert ei.value.status == ERR_STATE                                                 # no map resident
    m.upload_map(w.Gx, w.Gy)
    m.median_blur_map()
    gx, gy = m.downloadMap()
    assert np.array_equal(gx, SR.median_blur3_fast(w.Gx)) and np.array_equal(gy, SR.median_blur3_fast(w.Gy)) and not np.array_equal(gx, w.Gx)
    m.median_blur_map()                                                                 # a second pass blurs the blurred map
    assert np.array_equal(m.downloadMap()[0], SR.median_blur3_fast(SR.median_blur3_fast(w.Gx)))
    # a trial map pending: EMBA_ERR_STATE, and the maps are untouched
    m.set_events(w.events)
    m.evaluateDataError(w.traj, None, None)
    m.formNormalEq(None, w.K, None, w.thres_valid_pixel)
    m.applyL2Reg(w.alpha)
    x1, x2 = m.solveNormalEq(1e-2, fix_first_pose=True)
    m.updateMap(x2, 1.0)
    trial = m.downloadMap()
    with pytest.raises(EmbaError) as ei:
        m.median_blur_map()
    assert ei.value.status == ERR_STATE
    assert np.array_equal(m.downloadMap()[0], trial[0])
    m.rejectMap()
    m.median_blur_map()
    assert np.array_equal(m.downloadMap()[1], SR.median_blur3_fast(SR.median_blur3_fast(SR.median_blur3_fast(w.Gy))))


# ---- 6. the resident sequence ------------------------------------------------------------------------------------------------------------
def test_sequence_upload_down_samples_like_the_restatement(gpu):
    w = small_workload(n_events=2000)
    m = make_legm(w)
    assert m.sequence_size() == 0
    ev = packet(250_007, w.sensor_w, w.sensor_h, seed=21)
    for rate in (1, 2, 3, 7, 0):
        kept = m.set_sequence(ev, rate)
        want = SR.downsample(ev.x, ev.y, ev.polarity, ev.t_ns, rate)
        assert kept == len(want[3]) == m.sequence_size() == (ev.size() // rate if rate >= 2 else ev.size())
        got = m.sequence_events(0, kept)
        for g, o in zip((got.x, got.y, got.polarity, got.t_ns), want):
            assert np.array_equal(g, o), rate
        part = m.sequence_events(1000, 1357)
        assert np.array_equal(part.t_ns, want[3][1000:1357]) and np.array_equal(part.x, want[0][1000:1357])
    # several upload chunks (the staging buffers take 2^19 events each), the last one ragged
    ev = packet((1 << 20) + 12_345, w.sensor_w, w.sensor_h, seed=22)
    kept = m.set_sequence(ev, 3)
    want = SR.downsample(ev.x, ev.y, ev.polarity, ev.t_ns, 3)
    got = m.sequence_events(0, kept)
    for g, o in zip((got.x, got.y, got.polarity, got.t_ns), want):
        assert np.array_equal(g, o)
    m.free_sequence()
    assert m.sequence_size() == 0


def test_sequence_upload_validates_every_raw_event(gpu):
    """An error code from a reduction: nothing here reads or writes out of bounds."""
    from emba_amd import EmbaError
    w = small_workload(n_events=2000)
    m = make_legm(w)
    n = (1 << 20) + 5000                                   # three chunks
    good = packet(n, w.sensor_w, w.sensor_h, seed=23)
    for where in (3, (1 << 19) - 1, 1 << 19, n - 1):      # first chunk, either side of a chunk boundary, last event
        for kind in ("x", "y", "t"):
            ev = EventPacket(good.x.copy(), good.y.copy(), good.polarity, good.t_ns.copy())
            if kind == "x":
                ev.x[where] = w.sensor_w
            elif kind == "y":
                ev.y[where] = w.sensor_h + 7
            else:
                ev.t_ns[where] = ev.t_ns[where - 1] - 1
            with pytest.raises(EmbaError) as ei:
                m.set_sequence(ev, 2)                      # (an odd index is not even kept at rate 2: every RAW event is checked)
            assert ei.value.status == ERR_INVALID_ARG and str(where) in str(ei.value), (where, kind)
            assert m.sequence_size() == 0
    assert m.set_sequence(good, 2) == n // 2               # the context is usable afterwards
    equal_t = EventPacket(good.x, good.y, good.polarity, good.t_ns.copy())
    equal_t.t_ns[100:200] = equal_t.t_ns[100]              # equal timestamps are sorted
    assert m.set_sequence(equal_t, 1) == n


def test_sequence_window_equals_the_restatement(gpu):
    from emba_amd import EmbaError
    w = small_workload(n_events=2000)
    m = make_legm(w)
    assert m.sequence_window(0, 10 * MS) == (0, 0) == SR.event_subset(np.zeros(0, np.int64), 0, 10 * MS)     # no sequence: the empty range
    sets = dict(timestamp_sets())
    sets["n250k"] = packet(250_007, w.sensor_w, w.sensor_h, seed=24).t_ns
    n_ok = n_none = 0
    for name, t in sets.items():
        n = len(t)
        rng = np.random.default_rng(n)
        ev = EventPacket(rng.integers(0, w.sensor_w, n).astype(np.uint16), rng.integers(0, w.sensor_h, n).astype(np.uint16), np.zeros(n, np.uint8), t)
        assert m.set_sequence(ev, 1) == n
        n_rand = 300 if name == "n250k" else 40
        cases = window_cases(t) + [tuple(sorted(int(v) for v in rng.integers(int(t[0]) - 20 * MS, int(t[-1]) + 20 * MS, size=2))) for _ in range(n_rand)]
        for tb, te in cases:
            want = expect_window(t, tb, te)
            if want is None:
                n_none += 1
                with pytest.raises(EmbaError) as ei:
                    m.sequence_window(tb, te)
                assert ei.value.status == ERR_INVALID_ARG and "no events" in str(ei.value)
            else:
                n_ok += 1
                assert m.sequence_window(tb, te) == want, (name, tb, te)
    assert n_ok > 400 and n_none > 20


# ---- 7. a window of the resident sequence is the window emba_set_events builds from the host slice ---------------------------------------
def check_window_against_oracle(m, oracle_mod, w, beg, end):
    import dataclasses
    from test_gpu_parity import compare_event_state, compare_normal_eq
    ev = w.events
    ws = dataclasses.replace(w, events=eio.slice_events(ev, beg, end))
    o = oracle_run(oracle_mod, ws, dump=True)
    nem = np.zeros((w.pano_h, w.pano_w), dtype=np.int32)
    ep = m.evaluateDataError(w.traj, w.Gx, w.Gy, None, True, nem)
    used = ((end - beg) // 100) * 100
    assert m.event_counts()[0] == used and m.n_events == end - beg
    assert np.array_equal(nem, o["num_ev_map"]) and ep.shape == o["ep"].shape
    assert_close_elementwise(ep, o["ep"], "ep")
    compare_event_state(m.dump_state(), o["dump"], used)
    m.formNormalEq(None, w.K, nem, w.thres_valid_pixel)
    ne = m.applyL2Reg(w.alpha)
    compare_normal_eq(ne, o["ne"])
    for k in ("A11", "b1", "A22", "b2"):
        assert_close_elementwise(ne[k], o["ne"][k], k)


@pytest.mark.parametrize("poison", [0, 1])
def test_window_of_the_resident_sequence_matches_the_oracle_on_the_slice(gpu, oracle_mod, poison):
    w = small_workload(n_events=60_050)
    m = make_legm(w, poison=poison)
    assert m.set_sequence(w.events, 1) == 60_050
    t = w.events.t_ns
    beg, end = m.sequence_window(int(t[10_000]) - MS, int(t[40_000]) + MS)
    assert (beg, end) == SR.event_subset(t, int(t[10_000]) - MS, int(t[40_000]) + MS) and beg > 0 and end - beg >= 29_000
    m.set_events(EventWindow(beg, end))
    assert m.setup_info()["set_events_ms"] > 0 and m.setup_info()["entries"] == end - beg
    check_window_against_oracle(m, oracle_mod, w, beg, end)
    # a second, overlapping window on the same context
    beg2, end2 = m.sequence_window(int(t[25_000]) - MS, int(t[-1]) + 5 * MS)
    assert beg < beg2 < end < end2 == 60_050                                            # (runs to the ragged end of the sequence: 50 events are dropped, quirk Q1)
    m.set_events(EventWindow(beg2, end2))
    check_window_against_oracle(m, oracle_mod, w, beg2, end2)
    # a plain emba_set_events in between leaves the sequence as it was
    m.set_events(eio.slice_events(w.events, 300, 20_300))
    check_window_against_oracle(m, oracle_mod, w, 300, 20_300)
    assert m.sequence_size() == 60_050
    m.set_events(EventWindow(beg, end))
    check_window_against_oracle(m, oracle_mod, w, beg, end)
    from emba_amd import EmbaError
    for bad in ((end, beg), (0, 60_051)):
        with pytest.raises(EmbaError) as ei:
            m.set_events(EventWindow(*bad))
        assert ei.value.status == ERR_INVALID_ARG


# ---- 8. the three-window run ----------------------------------------------------------------------------------------------------------------
def test_three_window_run_on_the_device_matches_the_oracle_run(gpu, oracle_mod):
    """resident sequence + device blur + rate 2 against the same driver on host slices + numpy blur + the oracle.  Bounds: those of
    test_lm_solver_device_matches_oracle_loop, per window."""
    w, pose_t, pose_q, seq = three_window_case()
    seq.event_sampling_rate = 2
    ba, lm = BASettings(alpha=1.0), LMSettings(max_num_iter=10)
    om = OracleModel(oracle_mod, w)
    ro = run_sequence(om, w.events, pose_t, pose_q, w.Gx, w.Gy, seq, ba, lm, resident=False)
    m = make_legm(w)
    rg = run_sequence(m, w.events, pose_t, pose_q, w.Gx, w.Gy, seq, ba, lm, resident=True)
    assert len(ro.windows) == len(rg.windows) == 3 and rg.n_events == ro.n_events == w.events.size() // 2 == m.sequence_size()
    worst = []
    for k, (g, o) in enumerate(zip(rg.windows, ro.windows)):
        assert (g.beg, g.end) == (o.beg, o.end), k
        assert any(e[4] for e in o.result.log), f"window {k} accepted no LM step on the oracle"
        rel = max([abs(a[3] / b[3] - 1) for a, b in zip(g.result.log, o.result.log)] + [abs(a[2] / b[2] - 1) for a, b in zip(g.result.log, o.result.log)])
        dk = np.abs(g.result.traj.knots_xyzw - o.result.traj.knots_xyzw).max()
        worst.append((k, rel, dk))
        print(f"window {k}: events [{g.beg}, {g.end}) iterations {g.result.iterations}/{o.result.iterations} worst relative cost difference {rel:.3e} "
              f"worst control-pose difference {dk:.3e} set-up {g.setup_ms:.3f} ms")
    gmap, omap = m.downloadMap(), om.downloadMap()
    dmap = max(np.abs(d - o).max() / np.abs(o).max() for d, o in zip(gmap, omap))
    print(f"map: worst difference / max|map| {dmap:.3e}; whole trajectory {np.abs(rg.traj.knots_xyzw - ro.traj.knots_xyzw).max():.3e}")
    for k, (g, o) in enumerate(zip(rg.windows, ro.windows)):
        assert [e[4] for e in g.result.log] == [e[4] for e in o.result.log], f"window {k}: accept/reject sequence differs"
        assert g.result.iterations == o.result.iterations and g.result.converged == o.result.converged
        for a, b in zip(g.result.log, o.result.log):
            assert a[3] == pytest.approx(b[3], rel=1e-7) and a[2] == pytest.approx(b[2], rel=1e-7), k
        assert g.setup_ms > 0
    assert rg.traj.size() == 13 and np.abs(rg.traj.knots_xyzw - ro.traj.knots_xyzw).max() < 1e-7
    for d, o in zip(gmap, omap):
        assert np.abs(d - o).max() < 1e-7 * np.abs(o).max()
    # the host-slice path of the same device model (resident_sequence=False) cuts the same windows
    m2 = make_legm(w)
    rh = run_sequence(m2, w.events, pose_t, pose_q, w.Gx, w.Gy, seq, ba, LMSettings(max_num_iter=2), resident=True, resident_sequence=False)
    assert [(x.beg, x.end) for x in rh.windows] == [(x.beg, x.end) for x in rg.windows] and m2.sequence_size() == 0


# ---- 9. the command line ----------------------------------------------------------------------------------------------------------------------
def test_run_ba_demo_in_sliding_windows(gpu, tmp_path):
    out = tmp_path / "out"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "run_ba.py"), "--demo", str(out), "--window-size", "0.3", "--window-stride", "0.1",
                        "--max-iter", "6"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [l for l in r.stdout.splitlines() if l.startswith("window ")]
    assert len(lines) == 3, r.stdout                                                    # 0.1 ... 0.6 s: [0.1, 0.4], [0.2, 0.5], [0.3, 0.6]
    traj = np.loadtxt(out / "refined_traj.txt")
    assert traj.shape == (11, 8) and np.allclose(np.linalg.norm(traj[:, 4:], axis=1), 1.0, atol=1e-5)
    assert np.allclose(traj[:, 0], 0.1 + 0.05 * np.arange(11), atol=1e-6)
    assert (out / "Gx.bin").stat().st_size == 512 * 1024 * 8
