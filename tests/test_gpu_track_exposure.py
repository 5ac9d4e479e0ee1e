"""The frame tracker with a per-frame exposure on the MI355X (include/emba_hip.h: emba_frames_track_exposure, emba_track_exposure_eval) against
the numpy forms of the same rule (emba_amd.io: track_exposure_terms, exposure_sums, exposure_step, track_predict, track_votes_exposure) and against the
entry points it extends.  The seam is pm_out: fed the device's pm, numpy gives the counts and every level's sums as equal integers and the residuals bit for
bit; the 21 sums are held to the suite's standing bound, 1e-5 relative to sum |terms| with a floor of 1e-12 of the array's scale.  Then what is shared bit
for bit with emba_track_eval, emba_frames_exposure_eval and emba_frames_track, determinism and independence, the loop against its own rule, a lost frame,
the chunk edge, recovery within the figures recorded on the CPU (tests/track_exposure_cases.py), every refusal, what a call leaves alone, and
examples/run_ba.py --track-exposure."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import track_cases as TC
import track_exposure_cases as XC
import view_cases as VC
from emba_amd import _lib
from emba_amd import io as eio
from emba_amd import so3, synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_INVALID_ARG, ERR_STATE = 1, 5
SUM_REL, SUM_FLOOR = 1e-5, 1e-12      # README: Jacobian-derived quantities
_dp, _u8p, _i32p, _i64p, _u64p = (C.POINTER(t) for t in (C.c_double, C.c_uint8, C.c_int32, C.c_int64, C.c_uint64))
SHARED = list(eio.EXPOSURE_SHARED)


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from emba_amd import build
    build.build_hip()
    return True


def make_legm(sensor, pano, lut=None):
    from emba_amd import LEGM
    return LEGM(sensor[0], sensor[1], VC.lut_of(sensor) if lut is None else lut, 0.2, pano[0], pano[1], device=0)


def ptr(a, ty):
    return None if a is None else a.ctypes.data_as(ty)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


FLOATS, INTS, SCALARS = ("q", "cost", "overlap"), ("status", "iters", "counts"), ("tracked", "lost", "dropped", "skipped")


def same_result(a, b, with_exposure=True):
    keys = FLOATS + (("gain", "bias") if with_exposure else ())
    return (all(np.array_equal(bits(a[k]), bits(b[k])) for k in keys) and all(np.array_equal(a[k], b[k]) for k in INTS) and all(a[k] == b[k] for k in SCALARS)
            and (a["pm"] is None or b["pm"] is None or np.array_equal(bits(a["pm"]), bits(b["pm"]))))


def args_of(sensor, pano, step, **kw):
    return XC.track_args(sensor, pano, step, **dict(dict(want_pm=True), **kw))


def track_x(m, sensor, pano, step, frames=None, estimate=3, **kw):
    c = XC.case(sensor, pano, step)
    fr = c["distorted"] if frames is None else frames
    a = args_of(sensor, pano, step)
    a.update(kw)
    return m.track_frames_exposure(fr.reshape(-1, sensor[1], sensor[0]), c["ts"][:len(fr)], estimate=estimate, **XC.BOUNDS, **a)


def track_plain(m, sensor, pano, step, frames=None, **kw):
    c = XC.case(sensor, pano, step)
    fr = c["distorted"] if frames is None else frames
    a = args_of(sensor, pano, step)
    a.update(kw)
    return m.track_frames(fr.reshape(-1, sensor[1], sensor[0]), c["ts"][:len(fr)], **a)


def sums_distance(got, want, scale):
    allow = SUM_REL * scale + SUM_FLOOR * max(float(np.abs(want).max()), 1e-300)
    return float((np.abs(got - want) / allow).max())


def levels_of(m, levels):
    return {l: m.track_level(l) for l in eio.track_vote_levels(levels)}


def same_planes(a, b):
    return a.keys() == b.keys() and all(np.array_equal(a[l][0], b[l][0]) and np.array_equal(a[l][1], b[l][1]) for l in a)


@pytest.mark.parametrize("sensor", ((20, 13), (64, 48)), ids=lambda s: f"sensor{s[0]}x{s[1]}")
def test_the_evaluation(gpu, sensor):
    """emba_track_exposure_eval at every level of (3, 2, 1, 0) for skip_zero x huber_k x a non-trivial (a, b): numpy from the device's pm gives equal counts, the
    residuals bit for bit and the 21 sums within 1e-5 of sum |terms|; at a = 1, b = 0 the ten shared sums and the residuals are emba_track_eval's bits; level 0
    is emba_frames_exposure_eval(use_mosaic, lo 0, hi 255) bit for bit."""
    pano, step = (128, 64), "large"
    c = XC.case(sensor, pano, step)
    S = sensor[0] * sensor[1]
    m = make_legm(sensor, pano)
    m.set_option("poison", 1)
    fr = c["distorted"].copy()
    fr.reshape(-1)[::11] = 0      # bytes for skip_zero to skip inside the panorama
    r = track_x(m, sensor, pano, step, frames=fr, batch=3, min_weight=32, max_iters=4)
    assert r["tracked"] > 1
    planes = levels_of(m, c["levels"])
    rng = np.random.default_rng(24)
    n = 4
    q = np.array([so3.mul(so3.exp(0.02 * rng.standard_normal(3)), x) for x in c["q_true"][:n]])
    gain, bias = 0.8 + 0.6 * rng.random(n), -20.0 + 30.0 * rng.random(n)
    frs = fr[:n].reshape(n, sensor[1], sensor[0])
    worst, seen = 0.0, np.zeros(4, np.int64)
    for l in (3, 2, 1, 0):
        for mw in (32, 256):
            for skip_zero in (False, True):
                for hk in (0.0, 3.0):
                    what = f"{sensor}, level {l}, min_weight {mw}, skip_zero {skip_zero}, huber_k {hk}"
                    g = m.track_exposure_eval(frs, q, gain, bias, level=l, min_weight=mw, skip_zero=skip_zero, huber_k=hk, want_pm=True, want_resid=True)
                    for f in range(n):
                        t = eio.track_exposure_terms(fr[f], g["pm"][f], c["lut"], q[f], planes[l][0], planes[l][1], gain[f], bias[f], mw, skip_zero, hk)
                        s, cnt, scale = eio.exposure_sums(t, with_scale=True)
                        assert np.array_equal(g["counts"][f], cnt) and cnt.sum() == S, what
                        assert np.array_equal(bits(g["resid"][f]), bits(t["r"])), what
                        d = sums_distance(g["sums"][f], s, scale)
                        worst = max(worst, d)
                        assert d <= 1.0, (what, f, d)
                        seen += cnt
                    # unit exposure: emba_track_eval's bits
                    one = m.track_exposure_eval(frs, q, 1.0, 0.0, level=l, min_weight=mw, skip_zero=skip_zero, huber_k=hk, want_pm=True, want_resid=True)
                    ref = m.track_eval(frs, q, level=l, min_weight=mw, skip_zero=skip_zero, huber_k=hk, want_pm=True, want_resid=True)
                    assert np.array_equal(bits(one["sums"][:, SHARED]), bits(ref["sums"])) and np.array_equal(one["counts"], ref["counts"]), what
                    assert np.array_equal(bits(one["resid"]), bits(ref["resid"])) and np.array_equal(bits(one["pm"]), bits(ref["pm"])), what
                    if l == 0:
                        x = m.exposure_eval(frs, q, gain, bias, use_mosaic=True, min_weight=mw, lo=0.0, hi=255.0, skip_zero=skip_zero, huber_k=hk, want_pm=True,
                                            want_resid=True)
                        assert all(np.array_equal(bits(g[k]), bits(x[k])) for k in ("sums", "resid", "pm")) and np.array_equal(g["counts"], x["counts"]), what
    print(f"{sensor}: worst |sums_device - sums_numpy| = {worst * SUM_REL:.3e} of sum |terms| (allowed {SUM_REL:.0e}); classes seen {seen.tolist()}")
    assert seen[0] > 0 and seen[2] > 0 and seen[3] > 0
    m.close()


def test_estimate_zero_is_emba_frames_track(gpu):
    """estimate = 0: emba_frames_track's bits in every output and every level plane as integers, at batch = 1 and batch = 2; the same call twice gives the same
    bits; a frame's outputs do not depend on the later frames of its batch."""
    sensor, pano, step = (64, 48), (128, 64), "large"
    c = XC.case(sensor, pano, step)
    m = make_legm(sensor, pano)
    for batch in (1, 2):
        p = track_plain(m, sensor, pano, step, batch=batch)
        lp = levels_of(m, c["levels"])
        e = track_x(m, sensor, pano, step, estimate=0, batch=batch)
        le = levels_of(m, c["levels"])
        assert same_result(e, p, with_exposure=False), batch
        assert (e["gain"] == 1.0).all() and (e["bias"] == 0.0).all()
        assert same_planes(lp, le) and lp[0][0].sum() > 0, batch
    a = track_x(m, sensor, pano, step, batch=4)
    la = levels_of(m, c["levels"])
    m.align_frames_eval(c["frames"][:2].reshape(2, 48, 64), c["q_true"][:2], use_mosaic=True)      # an unrelated stage in between
    b = track_x(m, sensor, pano, step, batch=4)
    assert same_result(a, b) and same_planes(la, levels_of(m, c["levels"]))
    assert not np.array_equal(a["gain"][1:], np.ones(XC.F - 1))
    # batches [1, 5) [5, 9) [9, 12) against a call that ends inside the second batch
    short = track_x(m, sensor, pano, step, batch=4, frames=c["distorted"][:7])
    for k in FLOATS + ("gain", "bias"):
        assert np.array_equal(bits(short[k]), bits(a[k][:7])), k
    assert np.array_equal(short["iters"], a["iters"][:7]) and np.array_equal(short["status"], a["status"][:7])
    m.close()


def test_the_loop_and_the_votes(gpu):
    """batch = 1: every frame starts at io.track_predict of the device's earlier q_out and at the gain and bias of the frame before it;
    emba_track_exposure_eval there plus io.exposure_step reproduces the first step.  The level sums are io.track_votes_exposure at pm_out with the
    reported (gain, bias), as integers."""
    sensor, pano, step = (64, 48), (128, 64), "small"
    c = XC.case(sensor, pano, step)
    fr = c["distorted"].reshape(XC.F, 48, 64)
    m = make_legm(sensor, pano)
    lam0 = TC.SETTINGS["lambda0"]
    for predict in (True, False):
        one = track_x(m, sensor, pano, step, levels=(1,), predict=predict, max_iters=1)
        want = eio.track_votes_exposure(c["distorted"], np.nan_to_num(one["pm"]), one["status"], one["gain"], one["bias"], 128, 64, (1,), skip_zero=True)
        assert (want["dropped"], want["skipped"]) == (one["dropped"], one["skipped"]) and same_planes(want["planes"], levels_of(m, (1,)))
        moved = 0
        for f in range(1, XC.F):
            track_x(m, sensor, pano, step, levels=(1,), predict=predict, max_iters=1, frames=c["distorted"][:f])      # the mosaic frame f was aligned against
            start = eio.track_predict(one["q"][f - 2] if f >= 2 else None, c["ts"][f - 2] if f >= 2 else None, one["q"][f - 1], c["ts"][f - 1], c["ts"][f], predict)
            a0, b0 = one["gain"][f - 1], one["bias"][f - 1]
            e = m.track_exposure_eval(fr[f:f + 1], start[None], a0, b0, level=1)
            x = eio.exposure_step(e["sums"][0], lam0, 3)
            assert one["iters"][f, 0] == 1 and one["status"][f] == eio.TRACK_TRACKED and x is not None
            got = so3.log(so3.mul(one["q"][f], so3.inverse(start)))
            if np.abs(got).max() < 1e-12:      # the trial was rejected: the outputs are the start
                assert bits(one["gain"][f]) == bits(a0) and bits(one["bias"][f]) == bits(b0)
                continue
            moved += 1
            assert np.all(np.abs(got - x[:3]) <= 1e-7 * np.abs(x[:3]).max() + 1e-9), (predict, f, got, x)
            assert abs(one["gain"][f] - (a0 + x[3])) <= 1e-7 * abs(x[3]) + 1e-12 and abs(one["bias"][f] - (b0 + x[4])) <= 1e-7 * abs(x[4]) + 1e-10, (predict, f)
        assert moved >= XC.F // 2, (predict, moved)
    # the full schedule, batch 3: the sums are the compensated votes
    r = track_x(m, sensor, pano, step, batch=3)
    want = eio.track_votes_exposure(c["distorted"], np.nan_to_num(r["pm"]), r["status"], r["gain"], r["bias"], 128, 64, c["levels"], skip_zero=True)
    assert (want["dropped"], want["skipped"]) == (r["dropped"], r["skipped"]) and same_planes(want["planes"], levels_of(m, c["levels"]))
    raw = eio.track_votes(c["distorted"], np.nan_to_num(r["pm"]), r["status"], 128, 64, c["levels"], skip_zero=True)
    assert not np.array_equal(raw["planes"][0][1], want["planes"][0][1])
    mos = m.mosaic()
    assert np.array_equal(mos["sum_w"], want["planes"][0][0]) and np.array_equal(mos["sum_v"], want["planes"][0][1])
    m.close()


def test_a_lost_frame(gpu):
    """A black frame is lost and casts no vote; it reports its predicted rotation and its start gain and bias; the next frame starts with the bits of a call
    that never saw it."""
    sensor, pano, step = (64, 48), (128, 64), "small"
    c = XC.case(sensor, pano, step)
    fr = c["distorted"].copy()
    fr[5] = 0
    m = make_legm(sensor, pano)
    r = track_x(m, sensor, pano, step, frames=fr, levels=(1, 0))
    assert r["status"][5] == eio.TRACK_LOST and (np.delete(r["status"], 5)[1:] == eio.TRACK_TRACKED).all() and (r["tracked"], r["lost"]) == (XC.F - 1, 1)
    assert r["overlap"][5] == 0.0 and r["counts"][5, 0] == 0 and np.isnan(r["pm"][5]).all()
    pred5 = eio.track_predict(r["q"][3], c["ts"][3], r["q"][4], c["ts"][4], c["ts"][5])
    assert eio.rotation_angle_between(pred5, r["q"][5])[0] < 1e-12
    assert bits(r["gain"][5]) == bits(r["gain"][4]) and bits(r["bias"][5]) == bits(r["bias"][4]) and r["gain"][4] != 1.0
    want = eio.track_votes_exposure(fr, np.nan_to_num(r["pm"]), r["status"], r["gain"], r["bias"], 128, 64, (1, 0), skip_zero=True)
    assert same_planes(want["planes"], levels_of(m, (1, 0)))
    keep = np.arange(XC.F) != 5
    a = args_of(sensor, pano, step, levels=(1, 0), want_pm=False)
    r2 = m.track_frames_exposure(fr[keep].reshape(-1, 48, 64), c["ts"][keep], estimate=3, **XC.BOUNDS, **a)
    for k in ("q", "gain", "bias", "cost"):
        assert np.array_equal(bits(r2[k]), bits(r[k][keep])), k
    assert (r2["lost"], r2["tracked"]) == (0, XC.F - 1)
    m.close()


def test_chunk_edge(gpu):
    """F = 65 535 + 3 frames of the 7 x 5 sensor, batch = 1000, max_iters = 1: the chunk ends a batch, so the frames up to the edge are those of a call that
    ends there, bit for bit, and the frames behind the edge start from the non-unit gain and bias carried across it."""
    sensor, pano = (7, 5), (32, 16)
    F = 65535 + 3
    m = make_legm(sensor, pano)
    rng = np.random.default_rng(65538)
    base = rng.integers(40, 200, (1, 5, 7))
    frames = np.clip(base + rng.integers(-3, 4, (F, 5, 7)), 1, 255).astype(np.uint8)
    frames[1:] = np.clip(np.rint((frames[1:].astype(np.float64) + 12.0) / 1.25), 1, 255).astype(np.uint8)      # every frame behind the anchor: a* = 1.25, b* = -12
    ts = 1_000_000 * np.arange(F, dtype=np.int64)
    kw = dict(q0=TC.Q_START, levels=(1,), batch=1000, skip_zero=True, min_weight=1, min_overlap=0.0, estimate=3, **XC.BOUNDS,
              **dict(TC.SETTINGS, max_iters=1, min_pixels=3))
    big = m.track_frames_exposure(frames, ts, **kw)
    assert big["tracked"] + big["lost"] == F and set(big["status"].tolist()) <= {1, 2, 3} and big["status"][0] == 1 and big["tracked"] > 1
    small = m.track_frames_exposure(frames[:65535], ts[:65535], **kw)
    for k in ("q", "gain", "bias", "cost", "overlap"):
        assert np.array_equal(bits(big[k][:65535]), bits(small[k])), k
    assert np.array_equal(big["status"][:65535], small["status"]) and np.array_equal(big["iters"][:65535], small["iters"])
    assert np.abs(np.linalg.norm(big["q"], axis=1) - 1.0).max() < 1e-9 and (big["counts"][1:].sum(axis=1) == 35).all()
    # across the edge: the three frames behind it are one batch, started at the last tracked frame in front of the edge; a lost one among them reports that start
    last = int(np.flatnonzero((big["status"][:65535] == eio.TRACK_TRACKED) | (big["status"][:65535] == eio.TRACK_ANCHOR))[-1])
    a0, b0 = big["gain"][last], big["bias"][last]
    assert a0 != 1.0 and b0 != 0.0
    e = m.track_exposure_eval(frames[65535:], np.tile(big["q"][last], (3, 1)), a0, b0, level=1, min_weight=1, skip_zero=True)      # (predict is on: only the exposure is checked)
    for f in range(65535, F):
        if big["status"][f] == eio.TRACK_LOST:
            assert bits(big["gain"][f]) == bits(a0) and bits(big["bias"][f]) == bits(b0)
    assert e["counts"].sum(axis=1).tolist() == [35, 35, 35]
    m.close()


@pytest.mark.parametrize("key", XC.RECOVERY, ids=lambda k: f"{k[0][0]}x{k[0][1]}-on-{k[1][0]}x{k[1][1]}-{k[2]}")
def test_recovery(gpu, key):
    """Every frame tracked; the angle within 2 E_NP + F tol_rot, the gain within twice numpy's worst |a - a*|, the bias within twice numpy's worst |b - b*|, the
    trials per level within F of numpy's; plain emba_frames_track on the same frames ends beyond that angle bound."""
    sensor, pano, step = key
    c = XC.case(*key)
    m = make_legm(sensor, pano)
    r = track_x(m, sensor, pano, step, want_pm=False)
    e, da, db = XC.worst_angle(*key, r["q"]), float(np.abs(r["gain"] - c["gain"]).max()), float(np.abs(r["bias"] - c["bias"]).max())
    bound = XC.angle_bound(key)
    print(f"{key}: angle {e:.4e} rad (bound {bound:.4e}), |a - a*| {da:.4e} (bound {2 * XC.DA_NP[key]:.4e}), |b - b*| {db:.4e} (bound {2 * XC.DB_NP[key]:.4e}), "
          f"iters {r['iters'].sum(axis=0).tolist()} (numpy {XC.ITERS_NP[key]})")
    assert r["status"].tolist() == [eio.TRACK_ANCHOR] + [eio.TRACK_TRACKED] * (XC.F - 1) and (r["tracked"], r["lost"]) == (XC.F, 0)
    assert r["gain"][0] == 1.0 and r["bias"][0] == 0.0
    assert e <= bound, (key, e, bound)
    assert da <= 2.0 * XC.DA_NP[key] and db <= 2.0 * XC.DB_NP[key], (key, da, db)
    assert np.abs(r["iters"].sum(axis=0) - np.array(XC.ITERS_NP[key])).max() <= XC.ITERS_SLACK, (key, r["iters"].sum(axis=0), XC.ITERS_NP[key])
    p = track_plain(m, sensor, pano, step, want_pm=False)
    ep = XC.worst_angle(*key, p["q"])
    print(f"{key}: plain emba_frames_track ends {ep:.4e} rad from the truth (numpy {XC.E_PLAIN[key]:.4e})")
    assert ep > bound, (key, ep, bound)
    m.close()


def test_degenerate_bounds_refusals_and_what_a_call_leaves_alone(gpu):
    """Under estimate = 3 a constant-byte frame is degenerate and therefore lost; the gain bounds reject; every refusal leaves the outputs, the mosaic and the
    level planes untouched; a successful call leaves the resident map, the window and the last evaluation as they were."""
    sensor, pano, step = (64, 48), (128, 64), "small"
    c = XC.case(sensor, pano, step)
    m1 = make_legm(sensor, pano)
    fr = c["distorted"][:4].copy()
    fr[2] = 77
    r = track_x(m1, sensor, pano, step, frames=fr, levels=(1, 0))
    assert r["status"].tolist() == [1, 2, 3, 2] and r["counts"][2, 0] > 0      # used pixels, and yet no way to tell a gain from a bias
    assert track_x(m1, sensor, pano, step, frames=fr, levels=(1, 0), estimate=0)["status"][2] == eio.TRACK_TRACKED
    # bounds that the truth lies outside of: every trial that moves the gain past them is rejected
    a = args_of(sensor, pano, step, want_pm=False)
    tight = m1.track_frames_exposure(c["distorted"].reshape(-1, 48, 64), c["ts"], estimate=3, gain_min=0.95, gain_max=1.05, **a)
    assert tight["gain"].max() <= 1.05 and tight["gain"].min() >= 0.95 and track_x(m1, sensor, pano, step, want_pm=False)["gain"].max() > 1.2
    m1.close()

    w = synth.make_scene_workload()          # 64x48 on 256x512
    S, F = 64 * 48, 4
    m = make_legm((64, 48), (512, 256), lut=w.lut)
    m.set_events(w.events)
    m.upload_map(w.Gx, w.Gy)
    first = m.step(w.traj, w.thres_valid_pixel, w.alpha)
    ep0, map0 = m.get_ep(), m.downloadMap()
    frames = np.random.default_rng(3).integers(1, 256, (F, 48, 64)).astype(np.uint8)
    ts = np.array([10, 20, 30, 40], np.int64)
    good = m.track_frames_exposure(frames, ts, levels=(2, 0), batch=2, max_iters=2)
    assert good["tracked"] + good["lost"] == F
    before = [m.track_level(l) for l in (2, 0)]
    L = m._L
    out = dict(q=np.full((F, 4), 3.5), gain=np.full(F, 9.5), bias=np.full(F, 8.5), status=np.full(F, 9, np.int32), iters=np.full((F, 2), 8, np.int32), cost=np.full(F, 1.5),
               counts=np.full((F, 4), 77, np.uint64), overlap=np.full(F, 2.5), stats=np.full(4, 55, np.uint64), pm=np.full((F, S, 2), -1.5), sums=np.full((F, 21), 4.25),
               resid=np.full((F, S), 6.5))

    def untouched():
        vals = dict(q=3.5, gain=9.5, bias=8.5, status=9, iters=8, cost=1.5, counts=77, overlap=2.5, stats=55, pm=-1.5, sums=4.25, resid=6.5)
        same = all((out[k] == v).all() for k, v in vals.items())
        now = [m.track_level(l) for l in (2, 0)]
        return same and all(np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1]) for x, y in zip(before, now))

    q0 = np.array([0.0, 0.0, 0.0, 1.0])

    def call(fr=frames, t=ts, F_=F, q=q0, null_settings=False, n_levels=2, levels=(2, 0), batch=2, min_weight=256, min_overlap=0.5, estimate=3, gain_min=0.25, gain_max=4.0,
             **kw):
        s = dict(eio.ALIGN_DEFAULTS, **kw)
        lv = list(levels) + [0] * (8 - len(levels))
        cs = _lib.EmbaTrackExposureSettings(
            _lib.EmbaTrackSettings(n_levels, (C.c_int32 * 8)(*lv), batch, 1, 1, min_weight, min_overlap,
                                   _lib.EmbaAlignSettings(int(s["max_iters"]), int(s["min_pixels"]), s["lambda0"], s["lambda_up"], s["lambda_down"], s["lambda_min"],
                                                          s["lambda_max"], s["tol_rot"], s["huber_k"])), estimate, gain_min, gain_max)
        return L.emba_frames_track_exposure(m._ctx, ptr(fr, _u8p), ptr(t, _i64p), F_, ptr(q, _dp), None if null_settings else C.addressof(cs), ptr(out["q"], _dp),
                                            ptr(out["gain"], _dp), ptr(out["bias"], _dp), ptr(out["status"], _i32p), ptr(out["iters"], _i32p), ptr(out["cost"], _dp),
                                            ptr(out["counts"], _u64p), ptr(out["overlap"], _dp), ptr(out["stats"], _u64p), ptr(out["pm"], _dp))

    ones, zeros = np.ones(F), np.zeros(F)

    def call_eval(fr=frames, F_=F, q=np.tile(q0, (F, 1)), gain=ones, bias=zeros, level=2, min_weight=256, huber_k=0.0):
        return L.emba_track_exposure_eval(m._ctx, ptr(fr, _u8p), F_, ptr(q, _dp), ptr(gain, _dp), ptr(bias, _dp), level, min_weight, 1, huber_k, ptr(out["sums"], _dp),
                                          ptr(out["counts"], _u64p), ptr(out["pm"], _dp), ptr(out["resid"], _dp))

    nan, inf = float("nan"), float("inf")
    refused = [dict(fr=None), dict(t=None), dict(q=None), dict(null_settings=True), dict(F_=1 << 31), dict(n_levels=0), dict(n_levels=9), dict(levels=(8, 0)),
               dict(levels=(-1, 0)), dict(batch=0), dict(min_overlap=nan), dict(min_overlap=1.5), dict(min_overlap=-0.5), dict(min_weight=0),
               dict(t=np.array([10, 20, 20, 40], np.int64)), dict(t=np.array([10, 20, 15, 40], np.int64)), dict(q=np.zeros(4)), dict(q=np.array([0.0, nan, 0.0, 1.0])),
               dict(q=np.array([inf, 0.0, 0.0, 1.0])), dict(max_iters=-1), dict(lambda_up=1.0), dict(lambda0=0.0), dict(min_pixels=2), dict(tol_rot=-1.0), dict(lambda_max=nan),
               dict(huber_k=nan),
               dict(estimate=4), dict(estimate=-1), dict(gain_min=0.0), dict(gain_min=-1.0), dict(gain_min=1.5), dict(gain_max=0.5), dict(gain_min=nan), dict(gain_max=inf)]
    for kw in refused:
        assert call(**kw) == ERR_INVALID_ARG and untouched(), kw
    many = (1 << 36) // S + 1
    assert call(F_=many, t=np.arange(many, dtype=np.int64)) == ERR_INVALID_ARG and untouched()
    assert b"2^36" in L.emba_last_error(m._ctx)
    bad_q = np.tile(q0, (F, 1))
    bad_q[2] = 0.0
    bad = lambda v, i=1: np.array([1.0 if k != i else v for k in range(F)])
    for kw in (dict(fr=None), dict(q=None), dict(F_=1 << 31), dict(level=8), dict(level=-1), dict(min_weight=0), dict(huber_k=nan), dict(q=bad_q), dict(gain=None),
               dict(bias=None), dict(gain=bad(nan)), dict(gain=bad(inf)), dict(gain=bad(0.0)), dict(gain=bad(-1.0)), dict(bias=bad(nan)), dict(bias=bad(inf))):
        assert call_eval(**kw) == ERR_INVALID_ARG and untouched(), kw
    assert call_eval(level=1) == ERR_STATE and untouched()      # level 1 was not voted into
    # the calls themselves still go, and leave the step path alone
    assert call() == 0 and call_eval() == 0 and not untouched()
    assert out["stats"][0] + out["stats"][1] == F and (out["counts"].sum(axis=1) == S).all() and out["gain"][0] == 1.0 and out["bias"][0] == 0.0
    again = m.step(w.traj, w.thres_valid_pixel, w.alpha)
    assert again == first and np.array_equal(bits(m.get_ep()), bits(ep0))
    map1 = m.downloadMap()
    assert np.array_equal(bits(map0[0]), bits(map1[0])) and np.array_equal(bits(map0[1]), bits(map1[1]))
    m.close()


def test_run_ba_tracks_frames_under_per_frame_exposures(gpu, tmp_path):
    """examples/run_ba.py --demo with --views-hz writes frames; they are put under per-frame exposures (frame 0 left alone) and a second run takes them with
    --init-poses frames --init-map frames --track-exposure gain-bias: it runs to the end, frames_tracked.txt has the columns gain and bias, and the gains
    follow the ramp."""
    out1, out2 = tmp_path / "out1", tmp_path / "out2"
    exe = [sys.executable, os.path.join(ROOT, "examples", "run_ba.py")]
    r = subprocess.run(exe + ["--demo", str(out1), "--views-hz", "50", "--window-size", "0.5", "--max-iter", "3"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    lo, hi = open(out1 / "views" / "tone.txt").read().split()
    names = sorted(p for p in os.listdir(out1 / "views") if p.endswith(".pgm"))
    n_frames = len(open(out1 / "views" / "times.txt").read().splitlines())
    assert len(names) == n_frames
    a_star = 1.0 + 0.3 * np.arange(n_frames) / max(n_frames - 1, 1)
    for f, name in enumerate(names[1:], start=1):
        img = eio.load_pgm(str(out1 / "views" / name))
        v = img.astype(np.float64)
        d = np.where(img != 0, np.clip(np.rint((v + 100.0 * (a_star[f] - 1.0)) / a_star[f]), 1.0, 255.0), 0.0).astype(np.uint8)
        eio.save_pgm(str(out1 / "views" / name), d)
    common = ["--frames", str(out1 / "views"), "--init-poses", "frames", "--init-map", "frames", "--track-levels", "3,2,1", "--track-batch", "2", "--track-predict", "1",
              "--track-min-overlap", "0.3", "--track-q0", "0,0,0,1", "--window-size", "0.5", "--frames-log", "0", "--frames-lo", lo, "--frames-hi", hi,
              "--frames-skip-zero", "--max-iter", "3"]
    r = subprocess.run(exe + ["--demo", str(out2)] + common + ["--track-exposure", "gain-bias"], capture_output=True, text=True, timeout=600)
    print(r.stdout[-3000:])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "init-poses frames:" in r.stdout and "initial map from" in r.stdout and "track-exposure gain-bias" in r.stdout
    rows = [l.split() for l in open(out2 / "frames_tracked.txt").read().splitlines() if l and not l.startswith("#")]
    assert len(rows) == n_frames and all(len(x) == 10 for x in rows)
    status = [int(x[5]) for x in rows]
    gain, bias = np.array([float(x[8]) for x in rows]), np.array([float(x[9]) for x in rows])
    assert status[0] == 1 and set(status[1:]) <= {2, 3} and 2 in status and gain[0] == 1.0 and bias[0] == 0.0
    assert gain[-1] > 1.1 and bias[-1] < -5.0      # the ramp ends at a* = 1.3, b* = -30: the exposures were estimated, not left at 1 and 0
    assert (out2 / "refined_traj.txt").exists() and (out2 / "frame_mosaic.pgm").exists()
    # --track-exposure is refused without --init-poses frames
    r = subprocess.run(exe + ["--demo", str(tmp_path / "out3"), "--window-size", "0.5", "--track-exposure", "bias"], capture_output=True, text=True, timeout=600)
    assert r.returncode != 0 and "--track-exposure" in r.stderr
