"""The numpy form of the refit (emba_amd.io.refit_frames, refit_start, refit_batches) on a CPU: the planes as exact integers through un-vote
and vote, sweeps = 0 against the tracker's planes, a sweep that keeps every frame, a hand-marked lost frame recovered, a black frame, determinism, and the
figures recorded in tests/refit_cases.py."""
import numpy as np
import pytest

import refit_cases as RC
import track_cases as TC
from emba_amd import io as eio

W, H = RC.PANO
STEP, F = "small", 12
SMALL = dict(max_iters=6)      # a few trials are enough wherever the outcome of the alignment is not what is tested


def planes_equal(a, b):
    return a.keys() == b.keys() and all(np.array_equal(a[l][0], b[l][0]) and np.array_equal(a[l][1], b[l][1]) for l in a)


def votes_of(c, pm, status, gain, bias):
    return eio.track_votes_exposure(c["frames"], pm, status, gain, bias, W, H, c["levels"], True)


def refit(c, t, status=None, frames=None, **kw):
    a = RC.refit_args(STEP, **kw)
    return eio.refit_frames(c["frames"] if frames is None else frames, c["ts"], c["lut"], W, H, t["q"], t["status"] if status is None else status, t["gain"], t["bias"], **a)


def test_batches_and_start():
    assert eio.refit_batches(7, 3) == [(0, 1), (1, 3), (4, 3)] and eio.refit_batches(1, 5) == [(0, 1)] and eio.refit_batches(0, 1) == []
    t = RC.track_numpy(STEP, F)
    ts = RC.case(STEP, F)["ts"]
    st = t["status"].copy()
    st[3:6] = eio.TRACK_LOST
    g, b = np.linspace(1.0, 2.0, F), np.linspace(0.0, -50.0, F)
    q, a_, b_ = eio.refit_start(st, ts, t["q"], g, b, 2)
    assert np.array_equal(q, t["q"][2]) and a_ == g[2] and b_ == b[2]
    for f in (3, 4, 5):      # between frames 2 and 6, the times evenly spaced: the exposure is linear, the rotation lies between the two
        q, a_, b_ = eio.refit_start(st, ts, t["q"], g, b, f)
        frac = (f - 2) / 4.0
        assert abs(a_ - (g[2] + frac * (g[6] - g[2]))) < 1e-14 and abs(b_ - (b[2] + frac * (b[6] - b[2]))) < 1e-12
        whole = eio.rotation_angle_between(t["q"][2], t["q"][6])[0]
        assert abs(eio.rotation_angle_between(t["q"][2], q)[0] - frac * whole) < 1e-12
    st[6:] = eio.TRACK_LOST
    q, a_, b_ = eio.refit_start(st, ts, t["q"], g, b, 9)
    assert np.array_equal(q, t["q"][2]) and a_ == g[2]
    assert eio.refit_start(np.full(F, eio.TRACK_LOST), ts, t["q"], g, b, 4) is None


def test_sweeps_0_is_the_trackers_planes_and_unvote_leaves_the_others():
    c, t = RC.case(STEP, F), RC.track_numpy(STEP, F)
    r = refit(c, t, sweeps=0)
    assert planes_equal(r["planes"], t["planes"]) and np.array_equal(r["q"], t["q"]) and r["sweeps_done"] == 0
    assert r["refit"].tolist() == [eio.REFIT_ANCHOR] + [0] * (F - 1)
    whole = votes_of(c, t["pm"], t["status"], t["gain"], t["bias"])
    assert planes_equal(r["planes"], whole["planes"]) and (r["dropped"], r["skipped"]) == (whole["dropped"], whole["skipped"])
    # frame f taken out of the uint64 sums: the vote of the other frames, as equal integers — also from planes that were offset to wrap
    for f in (1, 6, F - 1):
        st = t["status"].copy()
        st[f] = eio.TRACK_LOST
        others = votes_of(c, t["pm"], st, t["gain"], t["bias"])
        one = votes_of(c, t["pm"], np.where(np.arange(F) == f, eio.TRACK_TRACKED, eio.TRACK_LOST), t["gain"], t["bias"])
        for l in others["planes"]:
            for k in (0, 1):
                assert np.array_equal(whole["planes"][l][k] - one["planes"][l][k], others["planes"][l][k])
                off = np.uint64(2**64 - 5)
                assert np.array_equal((whole["planes"][l][k] + off) - one["planes"][l][k] - off, others["planes"][l][k])


def test_sweeps_0_behind_the_tracker_with_exposure():
    """On the ramp: sweeps = 0 at the tracker's (q, a, b) builds the tracker's compensated planes, as equal integers, at batch 1 and 3."""
    key = (STEP, F, True)
    c, t = RC.case(*key), RC.track_numpy(*key)
    assert t["gain"].max() > 1.1
    for batch in (1, 3):
        r = eio.refit_frames(c["frames"], c["ts"], c["lut"], W, H, t["q"], t["status"], t["gain"], t["bias"], **RC.refit_args(STEP, 3, sweeps=0, batch=batch))
        assert planes_equal(r["planes"], t["planes"]) and np.array_equal(r["gain"], t["gain"]) and np.array_equal(r["bias"], t["bias"])
    for bad in (dict(gain=np.where(np.arange(F) == 3, np.nan, t["gain"])), dict(bias=np.where(np.arange(F) == 3, np.inf, t["bias"])),
                dict(gain=np.where(np.arange(F) == 3, 9.0, t["gain"]))):
        with pytest.raises(ValueError):
            eio.refit_frames(c["frames"], c["ts"], c["lut"], W, H, t["q"], t["status"], bad.get("gain", t["gain"]), bad.get("bias", t["bias"]), **RC.refit_args(STEP, 3, sweeps=0))


def test_a_sweep_that_keeps_every_frame_changes_nothing():
    """min_overlap = 1 on frames of which some pixels see no other frame (they are masked once the frame has left the planes): every verdict fails, every
    frame votes back what it took out."""
    c, t = RC.case(STEP, F), RC.track_numpy(STEP, F)
    for batch in (1, 3):
        r = refit(c, t, sweeps=1, min_overlap=1.0, batch=batch, **SMALL)
        assert r["refit"].tolist() == [eio.REFIT_ANCHOR] + [eio.REFIT_KEPT] * (F - 1)
        assert np.array_equal(r["q"].view(np.uint64), t["q"].view(np.uint64)) and planes_equal(r["planes"], t["planes"])
        assert r["sweep"][0, 2] == 0.0 and r["sweep"][0, 0] == 0 and (r["overlap"][1:] < 1.0).all() and (r["counts"][1:, 1] + r["counts"][1:, 2] > 0).all()


def test_a_lost_frame_is_recovered_and_a_black_frame_stays_lost():
    c, t = RC.case(STEP, F), RC.track_numpy(STEP, F)
    st = t["status"].copy()
    st[5] = eio.TRACK_LOST
    q_in = t["q"].copy()
    q_in[5] = TC.Q_START      # what a lost frame reports is not where it starts
    r = eio.refit_frames(c["frames"], c["ts"], c["lut"], W, H, q_in, st, **RC.refit_args(STEP, sweeps=1))
    assert r["refit"][5] == eio.REFIT_RECOVERED and r["status"][5] == eio.TRACK_TRACKED and r["sweep"][0, 1] == 1
    assert eio.rotation_angle_between(c["q_true"][5], r["q"][5])[0] < 2.0 * RC.E_REFIT_NP[(STEP, F, False)][0]
    assert planes_equal(r["planes"], votes_of(c, r["pm"], r["status"], r["gain"], r["bias"])["planes"])
    off = eio.refit_frames(c["frames"], c["ts"], c["lut"], W, H, q_in, st, **RC.refit_args(STEP, sweeps=1, recover=False, **SMALL))
    assert off["refit"][5] == eio.REFIT_LOST and np.array_equal(off["q"][5], q_in[5]) and np.isnan(off["pm"][5]).all()
    black = c["frames"].copy()
    black[5] = 0
    r = eio.refit_frames(black, c["ts"], c["lut"], W, H, q_in, st, **RC.refit_args(STEP, sweeps=1, **SMALL))
    assert r["refit"][5] == eio.REFIT_LOST and r["status"][5] == eio.TRACK_LOST and np.array_equal(r["q"][5], q_in[5]) and np.isnan(r["pm"][5]).all()
    assert planes_equal(r["planes"], eio.track_votes_exposure(black, r["pm"], r["status"], r["gain"], r["bias"], W, H, c["levels"], True)["planes"])


def test_refusals():
    c, t = RC.case(STEP, F), RC.track_numpy(STEP, F)
    for kw in (dict(sweeps=-1), dict(sweep_tol=-1.0), dict(sweep_tol=float("nan")), dict(estimate=4)):
        with pytest.raises(ValueError):
            refit(c, t, **kw)
    for st in (np.full(F, eio.TRACK_LOST), np.where(np.arange(F) == 2, 7, t["status"])):
        with pytest.raises(ValueError):
            refit(c, t, status=st)


@pytest.mark.parametrize("key", RC.CLOSING, ids=lambda k: f"{k[0]}-F{k[1]}{'-ramp' if k[2] else ''}")
def test_the_closing_cases_are_as_recorded(key):
    """The figures of tests/refit_cases.py, and the invariant behind the last sweep.  Whether the refit ends nearer to the truth is measured, not assumed:
    only the cases of RC.IMPROVES assert it."""
    step, F_, ramp = key
    c, t, r = RC.case(*key), RC.track_numpy(*key), RC.refit_numpy(*key)
    e_track, e_refit = RC.worst_angle(step, F_, t["q"], ramp), RC.worst_angle(step, F_, r["q"], ramp)
    print(key, "E_TRACK", e_track, "E_REFIT", e_refit, "iters", r["iters_sweeps"].tolist(), "codes", r["refit"].tolist(), "sweep", r["sweep"].tolist())
    assert (t["status"][1:] == eio.TRACK_TRACKED).all()
    assert abs(e_track / RC.E_TRACK_NP[key] - 1.0) < 1e-3 and abs(e_refit / RC.E_REFIT_NP[key][-1] - 1.0) < 1e-3
    assert tuple(map(tuple, r["iters_sweeps"].tolist())) == RC.ITERS_NP[key]
    assert all(tuple(codes) == RC.CODES_NP[key] for codes in r["refit_sweeps"].tolist()) and r["sweeps_done"] == RC.SWEEPS
    assert np.isin(r["refit"][1:], (eio.REFIT_MOVED, eio.REFIT_RECOVERED)).all()
    want = eio.track_votes_exposure(c["frames"], r["pm"], r["status"], r["gain"], r["bias"], W, H, c["levels"], True)
    assert planes_equal(r["planes"], want["planes"]) and (r["dropped"], r["skipped"]) == (want["dropped"], want["skipped"])
    if key in RC.IMPROVES:
        assert RC.E_REFIT_NP[key][-1] < RC.E_TRACK_NP[key]
    if ramp:
        g = RC.GAIN_NP[key]
        assert abs(np.abs(r["gain"] - c["gain"]).max() / g["da_refit"] - 1.0) < 1e-3 and abs(np.abs(t["gain"] - c["gain"]).max() / g["da_track"] - 1.0) < 1e-3


def test_determinism():
    c, t = RC.case(STEP, F), RC.track_numpy(STEP, F)
    a, b = refit(c, t, sweeps=1, batch=3, **SMALL), refit(c, t, sweeps=1, batch=3, **SMALL)
    assert np.array_equal(a["q"].view(np.uint64), b["q"].view(np.uint64)) and planes_equal(a["planes"], b["planes"]) and np.array_equal(a["refit"], b["refit"])
