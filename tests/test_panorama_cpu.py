"""The panorama of warped events without a GPU: the HIP-free rule header (emba_amd/csrc/panorama_rule.h through tests/cpp/panorama_rule_test.cpp), the numpy
form of the rule (emba_amd.io: pano_votes, event_panorama), the new symbol of libemba_hip.so, the contrast on a recording whose motion is known, the numpy
form's own pm against the oracle's, and the sliding-window driver recording the contrast on the oracle model."""
import os
import subprocess

import numpy as np
import pytest

import cmax_cases as CC
from emba_amd import io as eio
from emba_amd import so3, synth
from emba_amd.driver import SequenceSettings, run_sequence
from emba_amd.legm import EventPacket, LinearTrajectory
from emba_amd.solver import BASettings, LMSettings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# L1 distance between the image made of io.event_panorama's own pm and the image made of the oracle's pm, as a share of the total votes (256 per event),
# measured once on synth.make_scene_workload(): 0 — the two pm differ by at most 5.7e-14 px (numpy's quaternion product and rotation matrix
# against the oracle's Sophus order of operations), and on this recording no coordinate lies that close to a sixteenth of a pixel, so no vote moves.  The
# asserted bound is ten times the measurement — here: equality — and never above 1e-3: a half-pixel or axis error moves essentially every vote, a share
# of order one.
ORACLE_SHARE_MEASURED = 0.0
ORACLE_SHARE_BOUND = min(10.0 * ORACLE_SHARE_MEASURED, 1e-3)


def plain_loop(pm, pol, W, H, signed):
    """The stated formula, one event at a time in python ints: (image [H, W], dropped votes)."""
    img = [[0] * W for _ in range(H)]
    dropped = 0
    for (px, py), p in zip(pm.tolist(), pol.tolist()):
        if not (np.isfinite(px) and np.isfinite(py)):
            continue
        ix, iy = int(np.floor(px)), int(np.floor(py))
        wx, wy = int(np.floor((px - ix) * 16)), int(np.floor((py - iy) * 16))
        sgn = -1 if (signed and p == 0) else 1
        for cx, cy, w in ((ix, iy, (16 - wx) * (16 - wy)), (ix + 1, iy, wx * (16 - wy)), (ix, iy + 1, (16 - wx) * wy), (ix + 1, iy + 1, wx * wy)):
            if w == 0:
                continue
            if 0 <= cy < H:
                img[cy][cx % W] += sgn * w
            else:
                dropped += 1
    return np.array(img, dtype=np.int64), dropped


def test_panorama_rule_on_the_cpu(tmp_path):
    """emba_amd/csrc/panorama_rule.h (plain C++17, no HIP): tests/cpp/panorama_rule_test.cpp checks pano_vote — the weights sum to 256, pm_x in [W - 1, W)
    votes into column 0 and pm_x in [-1, 0) into column W - 1, rows -1 and H are dropped, an integer pm puts 256 into one cell, NaN / inf vote nowhere — the
    batch count and the argument checks with nn = 2^23 (a number passed to the rule function: nothing of that size is allocated).  The votes it prints are
    compared here with io.pano_votes."""
    exe = str(tmp_path / "panorama_rule_test")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-ffp-contract=off", os.path.join(ROOT, "tests", "cpp", "panorama_rule_test.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout[-3000:], r.stderr)
    lines = r.stdout.strip().splitlines()
    assert r.returncode == 0 and lines[-1] == "OK panorama_rule", r.stdout[-3000:] + r.stderr
    votes = [l for l in lines if l.startswith("VOTE ")]
    assert len(votes) == 8
    for l in votes:
        head, cells, weights = l[5:].split("|")
        px, py, W, H = head.split()
        cell, w = eio.pano_votes([[float(px), float(py)]], int(W), int(H))
        assert cell[0].tolist() == [int(v) for v in cells.split()] and w[0].tolist() == [int(v) for v in weights.split()], l
    # the numpy form's own limits
    cell, w = eio.pano_votes([[np.nan, 1.0], [1.0, np.inf], [2.0 ** 31, 0.0], [5.0, 5.0]], 512, 256)
    assert (cell[:3] == -1).all() and (w[:3] == 0).all() and w[3].tolist() == [256, 0, 0, 0]
    assert eio.PANO_MAX_EVENTS == 1 << 23 and eio.PANO_BATCH == 100


def test_new_symbol_resolves(hip_lib):
    assert hasattr(hip_lib, "emba_seq_event_panorama")
    from emba_amd import LEGM
    from emba_amd.sharded import HipEngine, ShardedLEGM, ShardedModel
    assert all(callable(getattr(k, "event_panorama")) for k in (LEGM, HipEngine, ShardedLEGM, ShardedModel))
    blob = open(os.path.join(ROOT, "emba_amd", "libemba_hip.so"), "rb").read()
    assert b"emba_pano_vote_kernel" in blob and b"emba_pano_reduce_kernel" in blob and b"emba_pano_reduce_final_kernel" in blob


@pytest.mark.parametrize("signed", [False, True])
def test_numpy_form_given_pm_equals_the_plain_loop(signed):
    """500 random pm over the panorama and a margin around it (wrapped columns, dropped rows), a few on integers, on the edges and not finite."""
    W, H, n = 512, 256, 500
    rng = np.random.default_rng(23)
    pm = np.stack([rng.uniform(-3.0, W + 3.0, n), rng.uniform(-3.0, H + 3.0, n)], axis=1)
    pm[:8] = [[0.0, 0.0], [W - 0.5, 10.0], [-0.25, 10.5], [W, H], [77.0, -1.0], [77.5, H - 0.5], [np.nan, 3.0], [3.0, np.inf]]
    pm[8:40] = np.floor(pm[8:40])                                   # integers: the whole vote in one cell
    pm[40:60] = pm[0:20]                                            # several events in the same cells
    ev = EventPacket(np.zeros(n, np.uint16), np.zeros(n, np.uint16), rng.integers(0, 2, n).astype(np.uint8), np.arange(n, dtype=np.int64))
    got = eio.event_panorama(ev, None, 64, 48, W, H, None, 0, n, signed, pm=pm)
    want, dropped = plain_loop(pm, ev.polarity, W, H, signed)
    assert got["image"].dtype == np.int64 and np.array_equal(got["image"], want)
    assert got["dropped"] == dropped > 0
    assert got["J"] == int((want * want).sum()) and got["sum"] == int(want.sum()) and got["nonzero"] == int(np.count_nonzero(want))
    finite = int(np.isfinite(pm).all(axis=1).sum())
    if signed:
        assert (want < 0).any() and abs(got["sum"]) < 256 * finite
    else:
        assert (want >= 0).all() and got["sum"] <= 256 * finite and got["sum"] > 200 * finite       # 256 per event, less the dropped votes
    # a range inside the packet, a tail that is ignored, and the arguments
    part = eio.event_panorama(ev, None, 64, 48, W, H, None, 100, 399, signed, pm=pm[100:300])
    assert np.array_equal(part["image"], plain_loop(pm[100:300], ev.polarity[100:300], W, H, signed)[0])
    none = eio.event_panorama(ev, None, 64, 48, W, H, None, 7, 106, signed, pm=np.zeros((0, 2)))
    assert none["J"] == 0 and none["nonzero"] == 0 and not none["image"].any() and none["pm"].shape == (0, 2)
    for bad in (dict(beg=5, end=4), dict(beg=0, end=n + 1)):
        with pytest.raises(ValueError):
            eio.event_panorama(ev, None, 64, 48, W, H, None, signed=signed, pm=pm, **bad)
    with pytest.raises(ValueError):
        eio.event_panorama(ev, None, 64, 48, W, H, None, 0, n, signed, pm=pm[:400])       # pm of another range
    with pytest.raises(ValueError):
        eio.event_panorama(ev, None, 64, 48, W, H, None, 0, n, signed)                    # neither pm nor a trajectory


def constant_rate_trajectory(omega):
    """Control poses exp(omega (t_i - 1 s)) every 50 ms from 1 s on: the rotation cmax_cases.constant_rate_events turns its camera by, exactly (one axis)."""
    return LinearTrajectory(np.array([so3.exp(np.asarray(omega) * (0.05 * i)) for i in range(4)]), 1_000_000_000, 50_000_000)


def test_the_contrast_orders_trajectories():
    """Scene points seen by a camera turning at the constant rate CONST_OMEGA (64x48, focal 60, about 3000 events), voted onto a 256x512 panorama along the
    true trajectory, along one at half the rate and along the identity: J(w) > J(w / 2) > J(0).  The values: DESIGN.md §12."""
    ev, lut = CC.constant_rate_events(CC.CONST_OMEGA)
    assert 2500 < ev.size() < 3500
    J = []
    for w in (CC.CONST_OMEGA, CC.CONST_OMEGA / 2, np.zeros(3)):
        r = eio.event_panorama(ev, lut, 64, 48, 512, 256, constant_rate_trajectory(w))
        assert r["pm"].shape == (ev.size() // 100 * 100, 2) and r["dropped"] == 0 and r["sum"] == 256 * r["pm"].shape[0]
        J.append(r["J"])
    print("J(w), J(w / 2), J(0):", J, "ratio", J[0] / J[2])
    assert J[0] > J[1] > J[2]
    # a midpoint outside the knots is refused
    with pytest.raises(ValueError):
        eio.event_panorama(ev, lut, 64, 48, 512, 256, LinearTrajectory(constant_rate_trajectory(CC.CONST_OMEGA).knots_xyzw[:3], 1_000_000_000, 50_000_000))


def test_own_pm_against_the_oracle(oracle_mod):
    """synth.make_scene_workload() (64x48, 256x512, K = 6, 38 965 events): the image of io.event_panorama's own pm against the image of the pm
    OracleLEGM.count_map returns.  The L1 distance as a share of the total votes is printed and bounded by ORACLE_SHARE_BOUND."""
    w = synth.make_scene_workload()
    ev = w.events
    assert ev.size() == 38965
    o = oracle_mod.OracleLEGM(w.sensor_w, w.sensor_h, w.pano_w, w.pano_h, w.lut, w.C_th)
    pm_o = o.count_map(w.traj.knots_xyzw, w.traj.t0_ns, w.traj.dt_ns, ev.x, ev.y, ev.t_ns, want_pm=True)[2]
    nn = ev.size() // 100 * 100
    own = eio.event_panorama(ev, w.lut, w.sensor_w, w.sensor_h, w.pano_w, w.pano_h, w.traj)
    ref = eio.event_panorama(ev, w.lut, w.sensor_w, w.sensor_h, w.pano_w, w.pano_h, None, pm=pm_o[:nn])
    total = 256 * nn
    assert ref["dropped"] == 0 and ref["sum"] == total      # (this trajectory keeps the view off the poles)
    share = int(np.abs(own["image"] - ref["image"]).sum()) / total
    print(f"L1 distance {share!r} of the total votes (max |pm - oracle pm| {np.abs(own['pm'] - pm_o[:nn]).max():.3e} px), bound {ORACLE_SHARE_BOUND!r}; "
          f"J own {own['J']} oracle {ref['J']}")
    assert share <= ORACLE_SHARE_BOUND <= 1e-3


def test_run_sequence_records_the_contrast_on_the_oracle_model(oracle_mod):
    """run_sequence(record_contrast = True, event_panorama = True) on the oracle model (no resident sequence: the numpy form with the camera the model
    names): every window's contrast_init / contrast_final are io.event_panorama's values at traj_init / result.traj over the window's events, and the
    run's image is the one of the final trajectory over all the windows' events.  Off by default: the fields stay None."""
    from helpers import OracleModel
    w = synth.make_scene_workload(n_steps=1000)
    om = OracleModel(oracle_mod, w)
    t0, t1 = w.traj.t0_ns * 1e-9, (w.traj.t0_ns + w.traj.dt_ns * (w.K - 1)) * 1e-9
    t_raw_ns = w.traj.t0_ns + 5_000_000 * np.arange((w.traj.dt_ns * (w.K - 1)) // 5_000_000, dtype=np.int64)
    pose_t, pose_q = t_raw_ns * 1e-9, np.array([w.traj.evaluate(int(tn)) for tn in t_raw_ns])
    kw = dict(time_window_size=0.15, sliding_window_stride=0.1, dt_knots=0.05, t_start=t0, t_end=t1, median_blur=False)
    assert SequenceSettings(**kw).record_contrast is False and SequenceSettings(**kw).event_panorama is False
    seq = SequenceSettings(record_contrast=True, event_panorama=True, **kw)
    args = (om, w.events, pose_t, pose_q, w.Gx, w.Gy)
    with pytest.raises(ValueError):                      # (no camera on the model, no resident sequence)
        run_sequence(*args, seq, BASettings(alpha=0.0), LMSettings(max_num_iter=2), resident=False)
    om.bearing_lut, om.sensor_w, om.sensor_h = w.lut, w.sensor_w, w.sensor_h
    res = run_sequence(*args, seq, BASettings(alpha=0.0), LMSettings(max_num_iter=2), resident=False)
    assert len(res.windows) == 2
    for wr in res.windows:
        for got, traj in ((wr.contrast_init, wr.traj_init), (wr.contrast_final, wr.result.traj)):
            want = eio.event_panorama(w.events, w.lut, w.sensor_w, w.sensor_h, w.pano_w, w.pano_h, traj, wr.beg, wr.end)
            assert got == {k: want[k] for k in ("J", "sum", "nonzero")} and got["J"] > 0
    want = eio.event_panorama(w.events, w.lut, w.sensor_w, w.sensor_h, w.pano_w, w.pano_h, res.traj, res.windows[0].beg, res.windows[-1].end)
    assert res.event_panorama.shape == (w.pano_h, w.pano_w) and np.array_equal(res.event_panorama, want["image"]) and res.event_panorama.any()
    off = run_sequence(*args, SequenceSettings(**kw), BASettings(alpha=0.0), LMSettings(max_num_iter=2), resident=False)
    assert off.event_panorama is None and all(wr.contrast_init is None and wr.contrast_final is None for wr in off.windows)


def test_sharded_hosts_forward_the_panorama():
    """ShardedModel -> ShardedLEGM -> HipEngine -> the rank's model: the call and its arguments arrive unchanged; over an engine without a resident sequence
    the driver takes the numpy form."""
    from types import SimpleNamespace
    from emba_amd.driver import panorama_of_events
    from emba_amd.sharded import HipEngine, ShardedLEGM, ShardedModel
    calls = []

    class Device:
        def bind_exchange(self, count, pack):
            pass

        def set_sequence(self, events, sampling_rate=1):
            return events.size()

        def event_panorama(self, traj, beg=0, end=None, signed=False, want_image=True, want_pm=False):
            calls.append((traj, beg, end, signed, want_image, want_pm))
            return dict(J=7)
    dist = SimpleNamespace(get_rank=lambda: 0, get_world_size=lambda: 2)
    host = ShardedModel(ShardedLEGM(Device(), dist, None, None, 64), SimpleNamespace(H=4, W=8))
    assert host.event_panorama("traj", 3, 900, True, False, True) == dict(J=7) and calls == [("traj", 3, 900, True, False, True)]
    eng = HipEngine.__new__(HipEngine)                    # (its constructor wants a context on a GPU: the forwarding method alone)
    eng.m = Device()
    assert eng.event_panorama("traj", 1, 2) == dict(J=7) and calls[-1] == ("traj", 1, 2, False, True, False)
    assert panorama_of_events(host, None, "traj", 0, 500, True) == dict(J=7) and calls[-1] == ("traj", 0, 500, False, False, False)
    ev, lut = CC.constant_rate_events(CC.CONST_OMEGA)
    traj = constant_rate_trajectory(CC.CONST_OMEGA)
    legm = SimpleNamespace(H=256, W=512, bearing_lut=lut, sensor_w=64, sensor_h=48)

    class Engine:
        def bind_exchange(self, count, pack):
            pass
    host = ShardedModel(ShardedLEGM(Engine(), dist, None, None, 64), legm)
    got = panorama_of_events(host, ev, traj, 100, 1300, False)
    assert got["J"] == eio.event_panorama(ev, lut, 64, 48, 512, 256, traj, 100, 1300)["J"]
