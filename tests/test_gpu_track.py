"""Intensity frames tracked against their own growing mosaic on the MI355X (include/emba_hip.h: emba_frames_track, emba_track_eval, emba_track_level_get;
DESIGN.md §21) against the numpy forms of the same rule (emba_amd.io: track_votes, track_terms, track_predict, track_frames).  The seam is pm_out: fed the
device's pm, numpy gives every level's sums as equal integers, the counts as equal integers and the residuals bit for bit; the sums of the normal equations
are held to the suite's standing bound, 1e-5 relative to sum |terms| with a floor of 1e-12 of the array's scale.  Then level 0 against emba_frames_align_eval
on the mosaic, determinism, independence of a batch's frames, the loop against its own rule, tracking within 2 E_NP + F tol_rot on the CPU-chosen cases, a
lost frame, the chunk edge, every refusal, what a call leaves alone, and examples/run_ba.py --init-poses frames."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import track_cases as TC
import view_cases as VC
from emba_amd import _lib
from emba_amd import io as eio
from emba_amd import so3, synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_INVALID_ARG, ERR_STATE = 1, 5
SUM_REL, SUM_FLOOR = 1e-5, 1e-12      # README: Jacobian-derived quantities
_dp, _u8p, _i32p, _i64p, _u64p = (C.POINTER(t) for t in (C.c_double, C.c_uint8, C.c_int32, C.c_int64, C.c_uint64))


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


def same_result(a, b):
    return (all(np.array_equal(bits(a[k]), bits(b[k])) for k in ("q", "cost", "overlap")) and all(np.array_equal(a[k], b[k]) for k in ("status", "iters", "counts"))
            and all(a[k] == b[k] for k in ("tracked", "lost", "dropped", "skipped")) and (a["pm"] is None or np.array_equal(bits(a["pm"]), bits(b["pm"]))))


def track(m, sensor, pano, step, frames=None, **kw):
    c = TC.case(sensor, pano, step)
    args = dict(q0=TC.Q_START, levels=c["levels"], batch=1, predict=c["predict"], skip_zero=True, min_weight=TC.TRACKING.get((sensor, pano, step), 256),
                min_overlap=TC.MIN_OVERLAP, want_pm=True, **TC.SETTINGS)
    args.update(kw)
    fr = c["frames"] if frames is None else frames
    return m.track_frames(fr.reshape(-1, sensor[1], sensor[0]), c["ts"][:len(fr)], **args)


def sums_distance(got, want, scale):
    allow = SUM_REL * scale + SUM_FLOOR * max(float(np.abs(want).max()), 1e-300)
    return float((np.abs(got - want) / allow).max())


@pytest.mark.parametrize("pano", TC.PANOS, ids=lambda p: f"pano{p[1]}x{p[0]}")
@pytest.mark.parametrize("sensor", TC.SENSORS, ids=lambda s: f"sensor{s[0]}x{s[1]}")
def test_the_seam(gpu, sensor, pano):
    """The level sums are io.track_votes of pm_out and the statuses; emba_track_eval at every level is io.track_terms of its own pm_out and those sums."""
    W, H = pano
    c = TC.case(sensor, pano, "small")
    m = make_legm(sensor, pano)
    m.set_option("poison", 1)
    fr = c["frames"].copy()
    fr.reshape(-1)[::11] = 0      # bytes for skip_zero to skip inside the panorama
    fr[7] = 0                     # ... and a frame that is lost
    r = track(m, sensor, pano, "small", frames=fr, batch=3, min_weight=32, max_iters=4)
    assert r["status"][0] == eio.TRACK_ANCHOR and r["status"][7] == eio.TRACK_LOST and r["tracked"] + r["lost"] == TC.F
    assert np.isnan(r["pm"][r["status"] == eio.TRACK_LOST]).all() and not np.isnan(r["pm"][r["status"] != eio.TRACK_LOST]).any()
    want = eio.track_votes(fr, np.nan_to_num(r["pm"]), r["status"], W, H, c["levels"], skip_zero=True)
    assert (want["dropped"], want["skipped"]) == (r["dropped"], r["skipped"])
    planes = {}
    for l in eio.track_vote_levels(c["levels"]):
        planes[l] = m.track_level(l)
        assert np.array_equal(planes[l][0], want["planes"][l][0]) and np.array_equal(planes[l][1], want["planes"][l][1]), l
        assert planes[l][0].sum() > 0
    mos = m.mosaic(min_weight=32)      # level 0's planes are the mosaic's sums
    assert np.array_equal(mos["sum_w"], planes[0][0]) and np.array_equal(mos["sum_v"], planes[0][1])
    rng = np.random.default_rng(21)
    q = np.array([so3.mul(so3.exp(0.02 * rng.standard_normal(3)), x) for x in c["q_true"][:5]])
    frs = fr[:5].reshape(5, sensor[1], sensor[0])
    worst, seen = 0.0, np.zeros(4, np.int64)
    for l in eio.track_vote_levels(c["levels"]):
        for mw in (256, 32):
            for skip_zero in (False, True):
                for hk in (0.0, 3.0):
                    what = f"{sensor} on {pano}, level {l}, min_weight {mw}, skip_zero {skip_zero}, huber_k {hk}"
                    g = m.track_eval(frs, q, level=l, min_weight=mw, skip_zero=skip_zero, huber_k=hk, want_pm=True, want_resid=True)
                    for f in range(5):
                        t = eio.track_terms(fr[f], g["pm"][f], c["lut"], q[f], planes[l][0], planes[l][1], mw, skip_zero, hk)
                        s, n, scale = eio.align_sums(t, with_scale=True)
                        assert np.array_equal(g["counts"][f], n) and n.sum() == sensor[0] * sensor[1], what
                        assert np.array_equal(bits(g["resid"][f]), bits(t["r"])), what
                        d = sums_distance(g["sums"][f], s, scale)
                        worst = max(worst, d)
                        assert d <= 1.0, (what, f, d)
                        seen += n
    print(f"{sensor} on {pano}: worst |sums_device - sums_numpy| = {worst * SUM_REL:.3e} of sum |terms| (allowed {SUM_REL:.0e}); classes seen {seen.tolist()}")
    assert seen[0] > 0 and seen[2] > 0 and seen[3] > 0
    # a level the call did not vote into
    r = track(m, sensor, pano, "small", levels=(1,), max_iters=1)
    m.track_level(1), m.track_level(0)
    for call in (lambda: m.track_level(2), lambda: m.track_eval(frs, q, level=2)):
        with pytest.raises(Exception) as e:
            call()
        assert getattr(e.value, "status", None) == ERR_STATE
    m.close()


def test_level_0_against_the_alignment_stage(gpu):
    """emba_track_eval(level 0) and emba_frames_align_eval(use_mosaic, lo 0, hi 255) at the same rotations: the same counts, residuals and pm, bit for bit."""
    sensor, pano = (64, 48), (128, 64)
    c = TC.case(sensor, pano, "small")
    m = make_legm(sensor, pano)
    track(m, sensor, pano, "small", max_iters=3)
    rng = np.random.default_rng(22)
    q = np.array([so3.mul(so3.exp(0.03 * rng.standard_normal(3)), x) for x in c["q_true"]])
    fr = c["frames"].reshape(TC.F, 48, 64)
    for mw in (256, 1000):
        for skip_zero in (False, True):
            for hk in (0.0, 2.0):
                a = m.track_eval(fr, q, level=0, min_weight=mw, skip_zero=skip_zero, huber_k=hk, want_pm=True, want_resid=True)
                b = m.align_frames_eval(fr, q, use_mosaic=True, min_weight=mw, lo=0.0, hi=255.0, skip_zero=skip_zero, huber_k=hk, want_pm=True, want_resid=True)
                assert np.array_equal(a["counts"], b["counts"]) and np.array_equal(bits(a["resid"]), bits(b["resid"])) and np.array_equal(bits(a["pm"]), bits(b["pm"]))
                assert a["counts"][:, 0].min() > 0
    m.close()


def test_determinism_and_independence(gpu):
    """The same call twice gives the same bits in every output; a frame's q_out under batch = B does not depend on which later frames share its batch."""
    sensor, pano = (64, 48), (128, 64)
    c = TC.case(sensor, pano, "large")
    m = make_legm(sensor, pano)
    a = track(m, sensor, pano, "large", batch=4)
    la = [m.track_level(l) for l in (3, 2, 1, 0)]
    m.align_frames_eval(c["frames"][:2].reshape(2, 48, 64), c["q_true"][:2], use_mosaic=True)      # an unrelated stage in between
    b = track(m, sensor, pano, "large", batch=4)
    assert same_result(a, b)
    for (w0, v0), l in zip(la, (3, 2, 1, 0)):
        w1, v1 = m.track_level(l)
        assert np.array_equal(w0, w1) and np.array_equal(v0, v1)
    # batches [1, 5) [5, 9) [9, 12) against a call that ends inside the second batch: frames 0 ... 6 have the same frames before their batches
    short = track(m, sensor, pano, "large", batch=4, frames=c["frames"][:7])
    assert np.array_equal(bits(short["q"]), bits(a["q"][:7])) and np.array_equal(short["iters"], a["iters"][:7]) and np.array_equal(bits(short["cost"]), bits(a["cost"][:7]))
    # ... and batch = 1 is another tracker: its frames see the frame just before them
    one = track(m, sensor, pano, "large", batch=1)
    assert np.array_equal(bits(one["q"][:2]), bits(a["q"][:2])) and not np.array_equal(bits(one["q"]), bits(a["q"]))
    m.close()


def test_the_loop_against_its_own_rule(gpu):
    """batch = 1: every frame's start is io.track_predict of the device's earlier q_out; emba_track_eval there plus io.align_step reproduces the first step."""
    sensor, pano = (64, 48), (128, 64)
    c = TC.case(sensor, pano, "small")
    fr = c["frames"].reshape(TC.F, 48, 64)
    m = make_legm(sensor, pano)
    for predict in (True, False):
        one = track(m, sensor, pano, "small", levels=(1,), predict=predict, max_iters=1)
        moved = 0
        for f in range(1, TC.F):
            # the mosaic frame f was aligned against: that of the frames before it
            track(m, sensor, pano, "small", levels=(1,), predict=predict, max_iters=1, frames=c["frames"][:f])
            start = eio.track_predict(one["q"][f - 2] if f >= 2 else None, c["ts"][f - 2] if f >= 2 else None, one["q"][f - 1], c["ts"][f - 1], c["ts"][f], predict)
            e = m.track_eval(fr[f:f + 1], start[None], level=1)
            delta = eio.align_step(e["sums"][0, :6], e["sums"][0, 6:9], TC.SETTINGS["lambda0"])
            assert one["iters"][f, 0] == 1 and one["status"][f] == eio.TRACK_TRACKED
            got = so3.log(so3.mul(one["q"][f], so3.inverse(start)))
            if np.abs(got).max() < 1e-12:      # the trial was rejected: q_out is the start
                continue
            moved += 1
            assert np.all(np.abs(got - delta) <= 1e-7 * np.abs(delta).max() + 1e-9), (predict, f, got, delta)
        assert moved >= TC.F // 2, (predict, moved)
    m.close()


@pytest.mark.parametrize("key", list(TC.TRACKING), ids=lambda k: f"{k[0][0]}x{k[0][1]}-on-{k[1][0]}x{k[1][1]}-{k[2]}")
def test_tracking(gpu, key):
    """Every frame tracked; the worst angle to the truth within 2 E_NP + F tol_rot — both forms follow the same rule to the same minimiser within tol_rot per
    frame, and the factor 2 absorbs a different accept / reject path (numpy's own pm differs from the device's in the last bits)."""
    sensor, pano, step = key
    m = make_legm(sensor, pano)
    bound = 2.0 * TC.E_NP[key] + TC.F * TC.SETTINGS["tol_rot"]
    for batch in (1,) if step == "large" else (1, 2):      # (without prediction a batch of two starts its second frame two steps away)
        r = track(m, sensor, pano, step, batch=batch, want_pm=False)
        e = TC.worst_angle(sensor, pano, step, r["q"])
        print(f"{key}, batch {batch}: angle to the truth {e:.4e} rad (bound {bound:.4e}), overlap >= {r['overlap'][1:].min():.3f}, iters {r['iters'].sum(axis=0).tolist()}")
        assert r["status"].tolist() == [eio.TRACK_ANCHOR] + [eio.TRACK_TRACKED] * (TC.F - 1) and (r["tracked"], r["lost"]) == (TC.F, 0)
        assert (r["overlap"][1:] >= TC.MIN_OVERLAP).all()
        assert e <= bound, (key, batch, e, bound)
        if batch == 1:      # the trials per level are numpy's: the levels ran in the schedule's order, each from where the one before it ended
            assert np.abs(r["iters"].sum(axis=0) - np.array(TC.ITERS_NP[key])).max() <= TC.ITERS_SLACK, (key, r["iters"].sum(axis=0), TC.ITERS_NP[key])
    if key in TC.COARSE_BEATS_FINE:
        r0 = track(m, sensor, pano, step, levels=(0,), want_pm=False)
        assert TC.worst_angle(sensor, pano, step, r0["q"]) > bound
    # the mosaic is there for emba_mosaic_get / emba_mosaic_map as it stands
    mos = m.mosaic()
    assert mos["n_covered"] > 0 and np.array_equal(mos["sum_w"], m.track_level(0)[0])
    m.close()


def test_a_lost_frame(gpu):
    """A black frame in the middle with skip_zero is lost, casts no vote, and the next frame predicts across it."""
    sensor, pano = (64, 48), (128, 64)
    c = TC.case(sensor, pano, "small")
    fr = c["frames"].copy()
    fr[5] = 0
    m = make_legm(sensor, pano)
    r = track(m, sensor, pano, "small", frames=fr, levels=(1, 0))
    assert r["status"][5] == eio.TRACK_LOST and (np.delete(r["status"], 5)[1:] == eio.TRACK_TRACKED).all() and (r["tracked"], r["lost"]) == (TC.F - 1, 1)
    assert r["overlap"][5] == 0.0 and r["counts"][5, 0] == 0 and np.isnan(r["pm"][5]).all()
    pred5 = eio.track_predict(r["q"][3], c["ts"][3], r["q"][4], c["ts"][4], c["ts"][5])
    assert eio.rotation_angle_between(pred5, r["q"][5])[0] < 1e-12      # q_out of a lost frame is its prediction
    planes = [m.track_level(l) for l in (1, 0)]
    # ... the sums are those of the other frames alone
    want = eio.track_votes(fr, np.nan_to_num(r["pm"]), r["status"], 128, 64, (1, 0), skip_zero=True)
    for (w, v), l in zip(planes, (1, 0)):
        assert np.array_equal(w, want["planes"][l][0]) and np.array_equal(v, want["planes"][l][1])
    # frame 6 started from frames 3 and 4 across the gap: a call without frame 5 at all (its time left out too) gives frame 6 the same bits
    keep = np.arange(TC.F) != 5
    r2 = m.track_frames(fr[keep].reshape(-1, 48, 64), c["ts"][keep], q0=TC.Q_START, levels=(1, 0), skip_zero=True, min_overlap=TC.MIN_OVERLAP, **TC.SETTINGS)
    assert np.array_equal(bits(r2["q"]), bits(r["q"][keep])) and (r2["lost"], r2["tracked"]) == (0, TC.F - 1)
    m.close()


def test_chunk_edge(gpu):
    """F = 65 535 + 40 frames of the 7 x 5 sensor, batch = 1000 (it does not divide the chunk), max_iters = 1: the chunk ends a batch, so the frames up to the
    edge are those of a call that ends there, bit for bit, and every frame has a verdict."""
    sensor, pano = (7, 5), (32, 16)
    F = 65535 + 40
    m = make_legm(sensor, pano)
    rng = np.random.default_rng(65575)
    frames = rng.integers(1, 256, (F, 5, 7)).astype(np.uint8)
    ts = 1_000_000 * np.arange(F, dtype=np.int64)
    kw = dict(q0=TC.Q_START, levels=(1,), batch=1000, skip_zero=True, min_weight=1, min_overlap=0.0, **dict(TC.SETTINGS, max_iters=1, min_pixels=3))
    big = m.track_frames(frames, ts, **kw)
    assert big["tracked"] + big["lost"] == F and set(big["status"].tolist()) <= {1, 2, 3} and big["status"][0] == 1 and big["tracked"] > 1
    small = m.track_frames(frames[:65535], ts[:65535], **kw)
    for k in ("q", "cost", "overlap"):
        assert np.array_equal(bits(big[k][:65535]), bits(small[k])), k
    assert np.array_equal(big["status"][:65535], small["status"]) and np.array_equal(big["iters"][:65535], small["iters"])
    assert np.abs(np.linalg.norm(big["q"], axis=1) - 1.0).max() < 1e-9 and (big["counts"][1:].sum(axis=1) == 35).all()
    m.close()


def test_every_refusal_and_what_a_call_leaves_alone(gpu):
    """Every refusal leaves the mosaic, the level planes and all outputs untouched; a successful call leaves the resident map, the window and the last
    evaluation as they were."""
    w = synth.make_scene_workload()          # 64x48 on 256x512
    S, F = 64 * 48, 4
    m = make_legm((64, 48), (512, 256), lut=w.lut)
    m.set_events(w.events)
    m.upload_map(w.Gx, w.Gy)
    first = m.step(w.traj, w.thres_valid_pixel, w.alpha)
    ep0, map0 = m.get_ep(), m.downloadMap()
    frames = np.random.default_rng(3).integers(1, 256, (F, 48, 64)).astype(np.uint8)
    ts = np.array([10, 20, 30, 40], np.int64)
    good = m.track_frames(frames, ts, levels=(2, 0), batch=2, max_iters=2)
    assert good["tracked"] + good["lost"] == F
    before = [m.track_level(l) for l in (2, 0)]
    L = m._L
    out = dict(q=np.full((F, 4), 3.5), status=np.full(F, 9, np.int32), iters=np.full((F, 2), 8, np.int32), cost=np.full(F, 1.5), counts=np.full((F, 4), 77, np.uint64),
               overlap=np.full(F, 2.5), stats=np.full(4, 55, np.uint64), pm=np.full((F, S, 2), -1.5), sums=np.full((F, 10), 4.25), resid=np.full((F, S), 6.5))

    def untouched():
        vals = dict(q=3.5, status=9, iters=8, cost=1.5, counts=77, overlap=2.5, stats=55, pm=-1.5, sums=4.25, resid=6.5)
        same = all((out[k] == v).all() for k, v in vals.items())
        now = [m.track_level(l) for l in (2, 0)]
        return same and all(np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) for a, b in zip(before, now))

    q0 = np.array([0.0, 0.0, 0.0, 1.0])

    def call(fr=frames, t=ts, F_=F, q=q0, null_settings=False, n_levels=2, levels=(2, 0), batch=2, min_weight=256, min_overlap=0.5, **kw):
        s = dict(eio.ALIGN_DEFAULTS, **kw)
        lv = list(levels) + [0] * (8 - len(levels))
        cs = _lib.EmbaTrackSettings(n_levels, (C.c_int32 * 8)(*lv), batch, 1, 1, min_weight, min_overlap,
                                    _lib.EmbaAlignSettings(int(s["max_iters"]), int(s["min_pixels"]), s["lambda0"], s["lambda_up"], s["lambda_down"], s["lambda_min"],
                                                           s["lambda_max"], s["tol_rot"], s["huber_k"]))
        return L.emba_frames_track(m._ctx, ptr(fr, _u8p), ptr(t, _i64p), F_, ptr(q, _dp), None if null_settings else C.addressof(cs), ptr(out["q"], _dp),
                                   ptr(out["status"], _i32p), ptr(out["iters"], _i32p), ptr(out["cost"], _dp), ptr(out["counts"], _u64p), ptr(out["overlap"], _dp),
                                   ptr(out["stats"], _u64p), ptr(out["pm"], _dp))

    def call_eval(fr=frames, F_=F, q=np.tile(q0, (F, 1)), level=2, min_weight=256, huber_k=0.0):
        return L.emba_track_eval(m._ctx, ptr(fr, _u8p), F_, ptr(q, _dp), level, min_weight, 1, huber_k, ptr(out["sums"], _dp), ptr(out["counts"], _u64p), ptr(out["pm"], _dp),
                                 ptr(out["resid"], _dp))

    nan, inf = float("nan"), float("inf")
    refused = [dict(fr=None), dict(t=None), dict(q=None), dict(null_settings=True), dict(F_=1 << 31), dict(n_levels=0), dict(n_levels=9), dict(levels=(8, 0)),
               dict(levels=(-1, 0)), dict(batch=0), dict(min_overlap=nan), dict(min_overlap=1.5), dict(min_overlap=-0.5), dict(min_weight=0),
               dict(t=np.array([10, 20, 20, 40], np.int64)), dict(t=np.array([10, 20, 15, 40], np.int64)), dict(q=np.zeros(4)), dict(q=np.array([0.0, nan, 0.0, 1.0])),
               dict(q=np.array([inf, 0.0, 0.0, 1.0])), dict(max_iters=-1), dict(lambda_up=1.0), dict(lambda0=0.0), dict(min_pixels=2), dict(tol_rot=-1.0), dict(lambda_max=nan),
               dict(huber_k=nan)]
    for kw in refused:
        assert call(**kw) == ERR_INVALID_ARG and untouched(), kw
    # F * S >= 2^36 votes: 22 369 622 frames of 3072 pixels (the times are read before the bound is, the frames never)
    many = (1 << 36) // S + 1
    assert call(F_=many, t=np.arange(many, dtype=np.int64)) == ERR_INVALID_ARG and untouched()
    assert b"2^36" in L.emba_last_error(m._ctx)
    bad_q = np.tile(q0, (F, 1))
    bad_q[2] = 0.0
    for kw in (dict(fr=None), dict(q=None), dict(F_=1 << 31), dict(level=8), dict(level=-1), dict(min_weight=0), dict(huber_k=nan), dict(q=bad_q)):
        assert call_eval(**kw) == ERR_INVALID_ARG and untouched(), kw
    assert call_eval(level=1) == ERR_STATE and untouched()      # level 1 was not voted into
    assert L.emba_track_level_get(m._ctx, 1, None, None) == ERR_STATE and L.emba_track_level_get(m._ctx, 9, None, None) == ERR_INVALID_ARG
    # a panorama whose size a level does not divide
    # a panorama whose size a level does not divide (36 x 18: level 2), and one where a level leaves a single row (32 x 16: level 4); both after a call
    # that went through, so that there are planes and outputs to leave untouched
    for pano, ok_lv, bad_lvs in (((36, 18), (1,), ((2,), (1, 5))), ((32, 16), (3, 0), ((4,), (3, 4)))):
        m2 = make_legm((7, 5), pano)
        f2, t2 = np.full((2, 5, 7), 9, np.uint8), np.array([1, 2], np.int64)
        assert m2.track_frames(f2, t2, levels=ok_lv)["status"][0] == eio.TRACK_ANCHOR
        before2 = [m2.track_level(l) for l in eio.track_vote_levels(ok_lv)]
        o2 = dict(q=np.full((2, 4), 3.5), status=np.full(2, 9, np.int32), stats=np.full(4, 55, np.uint64))
        for lv in bad_lvs:
            cs = _lib.EmbaTrackSettings(len(lv), (C.c_int32 * 8)(*(list(lv) + [0] * (8 - len(lv)))), 1, 1, 1, 256, 0.5, _lib.EmbaAlignSettings(30, 16, 1e-3, 10.0, 10.0, 1e-9, 1e6, 1e-6, 0.0))
            st = m2._L.emba_frames_track(m2._ctx, ptr(f2, _u8p), ptr(t2, _i64p), 2, ptr(q0, _dp), C.addressof(cs), ptr(o2["q"], _dp), ptr(o2["status"], _i32p), None, None, None,
                                         None, ptr(o2["stats"], _u64p), None)
            assert st == ERR_INVALID_ARG and (o2["q"] == 3.5).all() and (o2["status"] == 9).all() and (o2["stats"] == 55).all(), (pano, lv)
            now2 = [m2.track_level(l) for l in eio.track_vote_levels(ok_lv)]
            assert all(np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1]) and x[0].sum() > 0 for x, y in zip(before2, now2)), (pano, lv)
        m2.close()
    # the calls themselves still go, and leave the step path alone
    assert call() == 0 and call_eval() == 0 and not untouched()
    assert out["stats"][0] + out["stats"][1] == F and (out["counts"].sum(axis=1) == S).all()
    again = m.step(w.traj, w.thres_valid_pixel, w.alpha)
    assert again == first and np.array_equal(bits(m.get_ep()), bits(ep0))
    map1 = m.downloadMap()
    assert np.array_equal(bits(map0[0]), bits(map1[0])) and np.array_equal(bits(map0[1]), bits(map1[1]))
    m.close()


def test_run_ba_tracks_the_frames_of_another_run(gpu, tmp_path):
    """examples/run_ba.py --demo with --views-hz writes frames; a second run takes them as --frames with --init-poses frames --init-map frames: no poses and
    no map are given, the raw poses are the tracked frames' and the initial map is the mosaic the tracker left.  It runs to the end and writes
    frames_tracked.txt."""
    out1, out2 = tmp_path / "out1", tmp_path / "out2"
    exe = [sys.executable, os.path.join(ROOT, "examples", "run_ba.py")]
    r = subprocess.run(exe + ["--demo", str(out1), "--views-hz", "50", "--window-size", "0.5", "--max-iter", "3"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    lo, hi = open(out1 / "views" / "tone.txt").read().split()
    n_frames = len(open(out1 / "views" / "times.txt").read().splitlines())
    r = subprocess.run(exe + ["--demo", str(out2), "--frames", str(out1 / "views"), "--init-poses", "frames", "--init-map", "frames", "--track-levels", "3,2,1", "--track-batch", "2",
                              "--track-predict", "1", "--track-min-overlap", "0.3", "--track-q0", "0,0,0,1", "--window-size", "0.5", "--frames-log", "0", "--frames-lo", lo,
                              "--frames-hi", hi, "--frames-skip-zero", "--max-iter", "3"], capture_output=True, text=True, timeout=600)
    print(r.stdout[-3000:])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "init-poses frames:" in r.stdout and "initial map from" in r.stdout
    rows = [l.split() for l in open(out2 / "frames_tracked.txt").read().splitlines() if l and not l.startswith("#")]
    assert len(rows) == n_frames and all(len(x) == 8 for x in rows)
    status = [int(x[5]) for x in rows]
    assert status[0] == 1 and set(status[1:]) <= {2, 3} and 2 in status
    qn = np.array([[float(v) for v in x[1:5]] for x in rows])
    assert np.abs(np.linalg.norm(qn, axis=1) - 1.0).max() < 1e-9 and np.array_equal(qn[0], [0.0, 0.0, 0.0, 1.0])
    assert (out2 / "refined_traj.txt").exists()
    # --init-poses frames refuses without --frames and without --window-size
    for extra in (["--window-size", "0.5"], ["--frames", str(out1 / "views")]):
        r = subprocess.run(exe + ["--demo", str(tmp_path / "out3"), "--init-poses", "frames"] + extra, capture_output=True, text=True, timeout=600)
        assert r.returncode != 0 and "--init-poses frames" in r.stderr
