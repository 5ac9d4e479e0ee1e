"""Tracked frames refitted against the mosaic of the other frames on the MI355X (include/emba_hip.h: emba_frames_refit) against the numpy form
of the same rule (emba_amd.io: refit_frames, refit_start, track_votes_exposure, exposure_step) and against the trackers it stands behind.  The seam is
pm_out: fed the device's pm and (gain, bias), numpy gives every level's sums and both counters as equal integers — behind the build, behind every sweep,
and with every frame taken out and put back.  Then the first step against its own rule, the closing cases within the figures recorded on the CPU
(tests/refit_cases.py), determinism, a lost frame recovered, a black frame, the chunk edge, every refusal and what a call leaves alone."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import refit_cases as RC
import track_cases as TC
import track_exposure_cases as XC
import view_cases as VC
from emba_amd import _lib
from emba_amd import io as eio
from emba_amd import so3, synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_INVALID_ARG = 1
_dp, _u8p, _i32p, _i64p, _u64p = (C.POINTER(t) for t in (C.c_double, C.c_uint8, C.c_int32, C.c_int64, C.c_uint64))
SENSOR, PANO = RC.SENSOR, RC.PANO
W, H = PANO
STEP, F = "small", 12
LEVELS = TC.SCHEDULE[PANO]
SMALL = dict(max_iters=6)      # a few trials are enough wherever the outcome of the alignment is not what is tested


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from emba_amd import build
    build.build_hip()
    return True


def make_legm(sensor=SENSOR, pano=PANO, lut=None):
    from emba_amd import LEGM
    return LEGM(sensor[0], sensor[1], VC.lut_of(sensor) if lut is None else lut, 0.2, pano[0], pano[1], device=0)


def ptr(a, ty):
    return None if a is None else a.ctypes.data_as(ty)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def levels_of(m, levels):
    return {l: m.track_level(l) for l in eio.track_vote_levels(levels)}


def same_planes(a, b):
    return a.keys() == b.keys() and all(np.array_equal(a[l][0], b[l][0]) and np.array_equal(a[l][1], b[l][1]) for l in a)


def track(m, key, **kw):
    """The device's tracker on a case of tests/refit_cases.py: the plain one, or on the ramp the one with exposure; gain and bias beside q either way."""
    step, F_, ramp = key
    c = RC.case(*key)
    a = RC.track_args(step, want_pm=True)
    a.update(kw)
    fr = c["frames"].reshape(-1, SENSOR[1], SENSOR[0])
    if ramp:
        return m.track_frames_exposure(fr, c["ts"], estimate=3, **XC.BOUNDS, **a)
    r = m.track_frames(fr, c["ts"], **a)
    r["gain"], r["bias"] = np.ones(F_), np.zeros(F_)
    return r


def refit(m, key, t, status=None, frames=None, q=None, **kw):
    step, F_, ramp = key
    c = RC.case(*key)
    a = RC.refit_args(step, 3 if ramp else 0, want_pm=True)
    a.update(kw)
    fr = c["frames"] if frames is None else frames
    return m.refit_frames(fr.reshape(-1, SENSOR[1], SENSOR[0]), c["ts"], t["q"] if q is None else q, t["status"] if status is None else status, t["gain"], t["bias"], **a)


def invariant(m, frames, r, levels=LEVELS):
    """Every level's sums and both counters are io.track_votes_exposure of pm_out with gain_out / bias_out, as equal integers; stats agree."""
    want = eio.track_votes_exposure(frames, np.nan_to_num(r["pm"]), r["status"], r["gain"], r["bias"], W, H, levels, skip_zero=True)
    votes = int(np.isin(r["status"], (eio.TRACK_ANCHOR, eio.TRACK_TRACKED)).sum())
    return (same_planes(want["planes"], levels_of(m, levels)) and (want["dropped"], want["skipped"]) == (r["dropped"], r["skipped"])
            and (r["tracked"], r["lost"]) == (votes, len(r["status"]) - votes) and np.isnan(r["pm"][~np.isin(r["status"], (1, 2))]).all())


KEY = (STEP, F, False)
RAMP = (STEP, F, True)


@pytest.mark.parametrize("batch", (1, 3))
@pytest.mark.parametrize("key", (KEY, RAMP), ids=("plain", "exposure"))
def test_sweeps_0_is_the_trackers_planes(gpu, key, batch):
    """Behind either tracker, sweeps = 0 builds that tracker's planes at every level and its counters, bit for bit, and returns what it was given: the vote
    kernel with its sign is the trackers' vote kernel."""
    m = make_legm()
    t = track(m, key, batch=batch)
    planes = levels_of(m, LEVELS)
    m.mosaic_clear()
    r = refit(m, key, t, sweeps=0, batch=batch)
    assert same_planes(planes, levels_of(m, LEVELS)) and (r["dropped"], r["skipped"], r["tracked"], r["lost"]) == (t["dropped"], t["skipped"], t["tracked"], t["lost"])
    assert np.array_equal(bits(r["pm"]), bits(t["pm"])) and np.array_equal(bits(r["q"]), bits(t["q"])) and np.array_equal(bits(r["gain"]), bits(t["gain"]))
    assert r["sweeps_done"] == 0 and r["refit"].tolist() == [eio.REFIT_ANCHOR] + [0] * (F - 1) and not r["iters"].any()
    assert invariant(m, RC.case(*key)["frames"], r)
    m.close()


@pytest.mark.parametrize("alternate", (True, False), ids=("alternate", "forward"))
def test_the_invariant_behind_one_and_two_sweeps(gpu, alternate):
    """Behind one and behind two sweeps, at batch 1 and at batch 3, forward and alternating: the level sums are the votes of pm_out, as equal integers."""
    m = make_legm()
    c = RC.case(*RAMP)
    t = track(m, RAMP)
    for sweeps, batch in ((1, 1), (2, 3)):
        r = refit(m, RAMP, t, sweeps=sweeps, batch=batch, alternate=alternate, **SMALL)
        assert r["sweeps_done"] == sweeps and r["sweep"].shape == (sweeps, 4) and invariant(m, c["frames"], r), (sweeps, batch)
        assert (r["refit"][1:] == eio.REFIT_MOVED).all() and r["refit"][0] == eio.REFIT_ANCHOR and r["sweep"][-1, 0] == F - 1
        assert not np.array_equal(bits(r["q"][1:]), bits(t["q"][1:])) and np.array_equal(bits(r["q"][0]), bits(t["q"][0]))
        change = eio.rotation_angle_between(t["q"], r["q"]).max()
        if sweeps == 1:
            assert abs(r["sweep"][0, 2] - change) < 1e-12 and abs(r["sweep"][0, 3] - r["cost"].sum()) <= 1e-9 * r["cost"].sum()
    m.close()


@pytest.mark.parametrize("batch", (1, 3))
def test_unvote_is_exact(gpu, batch):
    """min_overlap = 1: every frame fails its verdict, keeps what it had and votes back what it took out — q, gains and every plane bit-identical to before."""
    m = make_legm()
    t = track(m, RAMP, batch=batch)
    planes = levels_of(m, LEVELS)
    r = refit(m, RAMP, t, sweeps=2, batch=batch, min_overlap=1.0, **SMALL)
    assert (t["status"][1:] == eio.TRACK_TRACKED).all()
    assert r["refit"].tolist() == [eio.REFIT_ANCHOR] + [eio.REFIT_KEPT] * (F - 1) and (r["overlap"][1:] < 1.0).all() and r["iters"][1:].any(axis=1).all()
    for k in ("q", "gain", "bias", "pm"):
        assert np.array_equal(bits(r[k]), bits(t[k])), k
    assert same_planes(planes, levels_of(m, LEVELS)) and (r["dropped"], r["skipped"]) == (t["dropped"], t["skipped"]) and np.array_equal(r["status"], t["status"])
    assert r["sweep"][:, 2].tolist() == [0.0, 0.0] and r["sweep"][:, 0].tolist() == [0.0, 0.0]
    m.close()


def test_the_first_step(gpu):
    """Level 1 alone, max_iters = 1, batch = 1, one forward sweep: frame 1 is the first to move.  The planes it is aligned against are those of a sweeps = 0
    call with frame 1 marked lost; emba_track_exposure_eval there plus io.exposure_step gives the step it takes."""
    m = make_legm()
    c = RC.case(*RAMP)
    fr = c["frames"].reshape(F, SENSOR[1], SENSOR[0])
    t = track(m, RAMP, levels=(1,))
    one = refit(m, RAMP, t, sweeps=1, levels=(1,), max_iters=1)
    st = t["status"].copy()
    st[1] = eio.TRACK_LOST
    without = refit(m, RAMP, t, status=st, sweeps=0, levels=(1,))
    assert without["lost"] == 1 and invariant(m, c["frames"], without, (1,))
    e = m.track_exposure_eval(fr[1:2], t["q"][1:2], t["gain"][1], t["bias"][1], level=1, min_weight=TC.TRACKING[(SENSOR, PANO, STEP)], skip_zero=True)
    x = eio.exposure_step(e["sums"][0], TC.SETTINGS["lambda0"], 3)
    got = so3.log(so3.mul(one["q"][1], so3.inverse(t["q"][1])))
    assert x is not None and one["iters"][1, 0] == 1 and one["refit"][1] == eio.REFIT_MOVED
    print("first step", got, x)
    # whether the trial is taken is decided from the evaluation at the stepped state, not from what the device reported
    trial = so3.mul(so3.exp(x[:3]), t["q"][1])
    e1 = m.track_exposure_eval(fr[1:2], trial[None], t["gain"][1] + x[3], t["bias"][1] + x[4], level=1, min_weight=TC.TRACKING[(SENSOR, PANO, STEP)], skip_zero=True)
    cost0, n0, cost1, n1 = e["sums"][0][eio.EXPOSURE_COST], e["counts"][0, 0], e1["sums"][0][eio.EXPOSURE_COST], e1["counts"][0, 0]
    taken = n1 >= TC.SETTINGS["min_pixels"] and cost1 / n1 < cost0 / n0 and XC.BOUNDS["gain_min"] <= t["gain"][1] + x[3] <= XC.BOUNDS["gain_max"]
    assert abs(cost1 / n1 - cost0 / n0) > 1e-9 * cost0 / n0, "the two mean costs tie: the case does not decide the branch"
    if not taken:      # the trial is rejected: the frame stays where it was
        assert np.array_equal(bits(one["q"][1]), bits(t["q"][1])) and bits(one["gain"][1]) == bits(t["gain"][1]) and bits(one["bias"][1]) == bits(t["bias"][1])
        m.close()
        return
    assert np.all(np.abs(got - x[:3]) <= 1e-7 * np.abs(x[:3]).max() + 1e-9), (got, x)
    assert abs(one["gain"][1] - (t["gain"][1] + x[3])) <= 1e-7 * abs(x[3]) + 1e-12 and abs(one["bias"][1] - (t["bias"][1] + x[4])) <= 1e-7 * abs(x[4]) + 1e-10
    m.close()


@pytest.mark.parametrize("key", RC.CLOSING, ids=lambda k: f"{k[0]}-F{k[1]}{'-ramp' if k[2] else ''}")
def test_the_closing_cases(gpu, key):
    """The device's tracker, then one and two sweeps: no frame kept or lost, the codes numpy's, the worst angle to the truth within 2 E_REFIT_NP + F tol_rot
    behind either sweep, the trials per level of the last sweep within one per frame of numpy's, and the invariant."""
    step, F_, ramp = key
    m = make_legm()
    c = RC.case(*key)
    t = track(m, key)
    assert (t["status"][1:] == eio.TRACK_TRACKED).all()
    for sweeps in (1, 2):
        r = refit(m, key, t, sweeps=sweeps)
        e_dev = RC.worst_angle(step, F_, r["q"], ramp)
        print(key, "sweeps", sweeps, "E_dev", e_dev, "bound", RC.angle_bound(key, sweeps - 1), "iters", r["iters"].sum(axis=0).tolist(), "numpy", RC.ITERS_NP[key][sweeps - 1])
        assert tuple(r["refit"].tolist()) == RC.CODES_NP[key] and not np.isin(r["refit"], (eio.REFIT_KEPT, eio.REFIT_LOST)).any()
        assert e_dev <= RC.angle_bound(key, sweeps - 1)
        assert np.all(np.abs(r["iters"].sum(axis=0) - np.array(RC.ITERS_NP[key][sweeps - 1])) <= RC.ITERS_SLACK_PER_FRAME * F_)
        assert invariant(m, c["frames"], r)
    m.close()


def test_determinism_recovery_and_a_black_frame(gpu):
    """The same call twice gives the same bits.  A frame marked lost by hand, reported anywhere, is recovered from between its neighbours, and the planes gain
    exactly its votes; without `recover` it stays out; a black frame stays lost and casts no vote."""
    m = make_legm()
    c = RC.case(*KEY)
    t = track(m, KEY)
    a, b = refit(m, KEY, t, sweeps=2, batch=3, **SMALL), refit(m, KEY, t, sweeps=2, batch=3, **SMALL)
    for k in ("q", "gain", "bias", "cost", "overlap", "pm", "sweep"):
        assert np.array_equal(bits(a[k]), bits(b[k])), k
    assert all(np.array_equal(a[k], b[k]) for k in ("status", "refit", "iters", "counts"))
    st = t["status"].copy()
    st[5] = eio.TRACK_LOST
    q_in = t["q"].copy()
    q_in[5] = TC.Q_START
    without = refit(m, KEY, t, status=st, q=q_in, sweeps=0)
    planes0 = levels_of(m, LEVELS)
    r = refit(m, KEY, t, status=st, q=q_in, sweeps=1, min_overlap=TC.MIN_OVERLAP)
    assert r["refit"][5] == eio.REFIT_RECOVERED and r["status"][5] == eio.TRACK_TRACKED and r["sweep"][0, 1] == 1 and (r["tracked"], r["lost"]) == (F, 0)
    assert eio.rotation_angle_between(c["q_true"][5], r["q"][5])[0] <= RC.angle_bound(KEY, 0) and invariant(m, c["frames"], r)
    # frame 5 alone is recovered where every other frame is held in place: the planes gain exactly its votes
    hold = refit(m, KEY, t, status=np.where(np.arange(F) == 5, eio.TRACK_LOST, eio.TRACK_ANCHOR), q=q_in, sweeps=1)
    assert hold["refit"].tolist() == [eio.REFIT_ANCHOR] * 5 + [eio.REFIT_RECOVERED] + [eio.REFIT_ANCHOR] * 6
    mine = eio.track_votes_exposure(c["frames"][5:6], hold["pm"][5:6], [eio.TRACK_TRACKED], hold["gain"][5:6], hold["bias"][5:6], W, H, LEVELS, skip_zero=True)
    now = levels_of(m, LEVELS)
    assert all(np.array_equal(now[l][k] - planes0[l][k], mine["planes"][l][k]) for l in now for k in (0, 1))
    assert hold["dropped"] - without["dropped"] == mine["dropped"] and hold["skipped"] - without["skipped"] == mine["skipped"]
    off = refit(m, KEY, t, status=st, q=q_in, sweeps=1, recover=False, **SMALL)
    assert off["refit"][5] == eio.REFIT_LOST and np.array_equal(bits(off["q"][5]), bits(q_in[5])) and np.isnan(off["pm"][5]).all() and invariant(m, c["frames"], off)
    black = c["frames"].copy()
    black[5] = 0
    r = refit(m, KEY, t, status=st, q=q_in, frames=black, sweeps=1, **SMALL)
    assert r["refit"][5] == eio.REFIT_LOST and r["status"][5] == eio.TRACK_LOST and np.array_equal(bits(r["q"][5]), bits(q_in[5])) and r["overlap"][5] == 0.0
    assert invariant(m, black, r) and (r["tracked"], r["lost"]) == (F - 1, 1)
    m.close()


def test_chunk_edge(gpu):
    """F = 65 535 + 3 frames of the 7 x 5 sensor, batch = 1000, one sweep of one trial: the frames behind the chunk edge are uploaded, taken out, aligned and
    voted back like the others.  Level 0's sums are the votes of pm_out (checked on the whole call through the total weight, and on the last chunk's frames
    through the difference to a call that marks them lost)."""
    sensor, pano = (7, 5), (32, 16)
    n = 65535 + 3
    m = make_legm(sensor, pano)
    rng = np.random.default_rng(65538)
    base = rng.integers(40, 200, (1, 5, 7))
    frames = np.clip(base + rng.integers(-3, 4, (n, 5, 7)), 1, 255).astype(np.uint8)
    ts = 1_000_000 * np.arange(n, dtype=np.int64)
    q = np.tile(TC.Q_START, (n, 1))
    st = np.full(n, eio.TRACK_TRACKED, np.int32)
    st[0] = eio.TRACK_ANCHOR
    kw = dict(levels=(0,), batch=1000, skip_zero=True, min_weight=1, min_overlap=0.0, estimate=0, want_pm=True, **dict(TC.SETTINGS, max_iters=1, min_pixels=3))
    r = m.refit_frames(frames, ts, q, st, sweeps=1, **kw)
    assert r["sweeps_done"] == 1 and (r["tracked"], r["lost"]) == (n, 0) and set(r["refit"][1:].tolist()) <= {eio.REFIT_MOVED, eio.REFIT_KEPT}
    assert (r["iters"][1:, 0] <= 1).all() and (r["counts"][1:].sum(axis=1) == 35).all() and not r["counts"][0].any() and not np.isnan(r["pm"]).any()
    sw, sv = m.track_level(0)
    cell, w = eio.pano_votes(r["pm"].reshape(-1, 2), pano[0], pano[1])
    assert int(sw.sum()) == int(w[cell >= 0].sum()) and r["dropped"] == int(np.count_nonzero((cell < 0) & (w != 0)))
    st2 = st.copy()
    st2[65535:] = eio.TRACK_LOST
    m.refit_frames(frames, ts, r["q"], st2, sweeps=0, **kw)
    sw2, sv2 = m.track_level(0)
    tail = eio.track_votes_exposure(frames[65535:].reshape(3, -1), r["pm"][65535:], [2, 2, 2], np.ones(3), np.zeros(3), pano[0], pano[1], (0,), skip_zero=True)
    assert np.array_equal(sw - sw2, tail["planes"][0][0]) and np.array_equal(sv - sv2, tail["planes"][0][1])
    m.close()


def test_refusals_and_what_a_call_leaves_alone(gpu):
    """Every refusal leaves the outputs, the mosaic and the level planes untouched; a successful call leaves the resident map, the window and the last
    evaluation as they were."""
    w = synth.make_scene_workload()          # 64x48 on 256x512
    S, n = 64 * 48, 4
    m = make_legm((64, 48), (512, 256), lut=w.lut)
    m.set_events(w.events)
    m.upload_map(w.Gx, w.Gy)
    first = m.step(w.traj, w.thres_valid_pixel, w.alpha)
    ep0, map0 = m.get_ep(), m.downloadMap()
    frames = np.random.default_rng(3).integers(1, 256, (n, 48, 64)).astype(np.uint8)
    ts = np.array([10, 20, 30, 40], np.int64)
    good = m.track_frames_exposure(frames, ts, levels=(2, 0), batch=2, max_iters=2)
    before = [m.track_level(l) for l in (2, 0)]
    L = m._L
    out = dict(q=np.full((n, 4), 3.5), gain=np.full(n, 9.5), bias=np.full(n, 8.5), status=np.full(n, 9, np.int32), refit=np.full(n, 9, np.int32),
               iters=np.full((n, 2), 8, np.int32), cost=np.full(n, 1.5), counts=np.full((n, 4), 77, np.uint64), overlap=np.full(n, 2.5), sweep=np.full((2, 4), 7.5),
               done=np.full(1, 6, np.int32), stats=np.full(4, 55, np.uint64), pm=np.full((n, S, 2), -1.5))
    vals = dict(q=3.5, gain=9.5, bias=8.5, status=9, refit=9, iters=8, cost=1.5, counts=77, overlap=2.5, sweep=7.5, done=6, stats=55, pm=-1.5)

    def untouched():
        now = [m.track_level(l) for l in (2, 0)]
        return all((out[k] == v).all() for k, v in vals.items()) and all(np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1]) for x, y in zip(before, now))

    q_ok, st_ok = good["q"].copy(), good["status"].copy()
    st_ok[st_ok == eio.TRACK_LOST] = eio.TRACK_TRACKED      # (random frames: whatever the tracker made of them, the refit is given voting frames)
    ones, zeros = np.ones(n), np.zeros(n)

    def call(fr=frames, t=ts, F_=n, q=q_ok, gain=ones, bias=zeros, st=st_ok, null_settings=False, n_levels=2, levels=(2, 0), batch=2, min_weight=256, min_overlap=0.5,
             estimate=3, gain_min=0.25, gain_max=4.0, sweeps=2, sweep_tol=0.0, **kw):
        s = dict(dict(eio.ALIGN_DEFAULTS, max_iters=2), **kw)
        lv = list(levels) + [0] * (8 - len(levels))
        cs = _lib.EmbaRefitSettings(_lib.EmbaTrackExposureSettings(
            _lib.EmbaTrackSettings(n_levels, (C.c_int32 * 8)(*lv), batch, 1, 1, min_weight, min_overlap,
                                   _lib.EmbaAlignSettings(int(s["max_iters"]), int(s["min_pixels"]), s["lambda0"], s["lambda_up"], s["lambda_down"], s["lambda_min"],
                                                          s["lambda_max"], s["tol_rot"], s["huber_k"])), estimate, gain_min, gain_max), sweeps, 1, 1, sweep_tol)
        return L.emba_frames_refit(m._ctx, ptr(fr, _u8p), ptr(t, _i64p), F_, ptr(q, _dp), ptr(gain, _dp), ptr(bias, _dp), ptr(st, _i32p),
                                   None if null_settings else C.addressof(cs), ptr(out["q"], _dp), ptr(out["gain"], _dp), ptr(out["bias"], _dp), ptr(out["status"], _i32p),
                                   ptr(out["refit"], _i32p), ptr(out["iters"], _i32p), ptr(out["cost"], _dp), ptr(out["counts"], _u64p), ptr(out["overlap"], _dp),
                                   ptr(out["sweep"], _dp), ptr(out["done"], _i32p), ptr(out["stats"], _u64p), ptr(out["pm"], _dp))

    nan, inf = float("nan"), float("inf")
    bad_q, nan_q = q_ok.copy(), q_ok.copy()
    bad_q[2] = 0.0
    nan_q[1, 2] = nan
    bad = lambda v, i=1: np.array([1.0 if k != i else v for k in range(n)])      # noqa: E731
    bad_st = lambda v: np.array([1, 2, v, 2], np.int32)      # noqa: E731
    refused = [dict(fr=None), dict(t=None), dict(null_settings=True), dict(F_=1 << 31), dict(n_levels=0), dict(n_levels=9), dict(levels=(8, 0)), dict(levels=(-1, 0)),
               dict(batch=0), dict(min_overlap=nan), dict(min_overlap=1.5), dict(min_weight=0), dict(t=np.array([10, 20, 20, 40], np.int64)), dict(max_iters=-1),
               dict(lambda_up=1.0), dict(lambda0=0.0), dict(min_pixels=2), dict(tol_rot=-1.0), dict(huber_k=nan), dict(estimate=4), dict(estimate=-1), dict(gain_min=0.0),
               dict(gain_min=1.5), dict(gain_max=0.5), dict(gain_max=inf),
               dict(q=None), dict(gain=None), dict(bias=None), dict(st=None), dict(sweeps=-1), dict(sweep_tol=-1.0), dict(sweep_tol=nan), dict(st=bad_st(0)), dict(st=bad_st(4)),
               dict(st=np.full(n, 3, np.int32)), dict(q=bad_q), dict(q=nan_q), dict(gain=bad(nan)), dict(gain=bad(inf)), dict(gain=bad(0.2)), dict(gain=bad(4.5)),
               dict(bias=bad(nan)), dict(bias=bad(inf)), dict(F_=0)]
    for kw in refused:
        assert call(**kw) == ERR_INVALID_ARG and untouched(), kw
    many = (1 << 36) // S + 1
    assert call(F_=many, t=np.arange(many, dtype=np.int64)) == ERR_INVALID_ARG and untouched()
    assert b"2^36" in L.emba_last_error(m._ctx)
    # the call itself still goes, with an anchor or without one, and leaves the step path alone
    assert call(st=np.full(n, 2, np.int32)) == 0 and out["refit"].min() >= eio.REFIT_MOVED
    assert call() == 0 and not untouched()
    assert out["stats"][0] + out["stats"][1] == n and out["done"][0] == 2 and out["refit"][0] == eio.REFIT_ANCHOR and set(out["status"].tolist()) <= {1, 2, 3}
    again = m.step(w.traj, w.thres_valid_pixel, w.alpha)
    assert again == first and np.array_equal(bits(m.get_ep()), bits(ep0))
    map1 = m.downloadMap()
    assert np.array_equal(bits(map0[0]), bits(map1[0])) and np.array_equal(bits(map0[1]), bits(map1[1]))
    m.close()


def test_run_ba_refits_the_tracked_frames(gpu, tmp_path):
    """examples/run_ba.py --demo with --views-hz writes frames; a second run takes them with --init-poses frames --track-refit 1 --init-map frames: it runs to the
    end, frames_tracked.txt gains the refit code as its last column, and the flag is refused without --init-poses frames."""
    out1, out2 = tmp_path / "out1", tmp_path / "out2"
    exe = [sys.executable, os.path.join(ROOT, "examples", "run_ba.py")]
    r = subprocess.run(exe + ["--demo", str(out1), "--views-hz", "50", "--window-size", "0.5", "--max-iter", "3"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    lo, hi = open(out1 / "views" / "tone.txt").read().split()
    n_frames = len(open(out1 / "views" / "times.txt").read().splitlines())
    common = ["--frames", str(out1 / "views"), "--init-poses", "frames", "--init-map", "frames", "--track-levels", "3,2,1", "--track-batch", "2", "--track-predict", "1",
              "--track-min-overlap", "0.3", "--track-q0", "0,0,0,1", "--window-size", "0.5", "--frames-log", "0", "--frames-lo", lo, "--frames-hi", hi,
              "--frames-skip-zero", "--max-iter", "3"]
    r = subprocess.run(exe + ["--demo", str(out2)] + common + ["--track-refit", "1", "--track-refit-tol", "1e-9"], capture_output=True, text=True, timeout=600)
    print(r.stdout[-3000:])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "init-poses frames:" in r.stdout and "track-refit: 1 of 1 sweeps" in r.stdout and "initial map from" in r.stdout
    lines = open(out2 / "frames_tracked.txt").read().splitlines()
    assert lines[0].startswith("#") and "refit(" in lines[0]
    rows = [l.split() for l in lines if l and not l.startswith("#")]
    assert len(rows) == n_frames and all(len(x) == 9 for x in rows)
    status, code = [int(x[5]) for x in rows], [int(x[8]) for x in rows]
    assert status[0] == 1 and code[0] == eio.REFIT_ANCHOR and set(code[1:]) <= {2, 3, 4, 5} and eio.REFIT_MOVED in code
    assert all((c in (eio.REFIT_MOVED, eio.REFIT_KEPT, eio.REFIT_RECOVERED)) == (st == 2) for st, c in zip(status[1:], code[1:]))
    assert (out2 / "refined_traj.txt").exists()
    r = subprocess.run(exe + ["--demo", str(tmp_path / "out3"), "--window-size", "0.5", "--track-refit", "1"], capture_output=True, text=True, timeout=600)
    assert r.returncode != 0 and "--track-refit" in r.stderr
