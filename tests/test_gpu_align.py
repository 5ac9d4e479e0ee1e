"""Intensity frames aligned to a panorama plane on the MI355X (include/emba_hip.h: emba_frames_align_eval, emba_frames_align) against the numpy
forms of the same rule (emba_amd.io: align_terms, align_sums, align_step, align_frames).  The seam is pm_out: fed the device's pm, numpy gives the counts as
equal integers and the residuals bit for bit; the sums are Jacobian-derived and held to the suite's standing bound for such quantities, 1e-5 relative to
sum |terms| of each sum with a floor of 1e-12 of the array's scale.  Then determinism, the loop against the evaluation and against io.align_step,
convergence on the CPU-chosen cases within 2 E_NP + tol_rot, the mosaic as the plane, the chunk edge, the statuses, every refusal, what a call leaves
alone, and examples/run_ba.py --refine-frames."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import align_cases as AC
import view_cases as VC
from emba_amd import _lib
from emba_amd import io as eio
from emba_amd import so3, synth
from emba_amd.legm import LinearTrajectory

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_INVALID_ARG, ERR_STATE = 1, 5
SUM_REL, SUM_FLOOR = 1e-5, 1e-12      # README: Jacobian-derived quantities
_dp, _u8p, _i32p, _u64p = (C.POINTER(t) for t in (C.c_double, C.c_uint8, C.c_int32, C.c_uint64))


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from emba_amd import build
    build.build_hip()
    return True


@pytest.fixture(scope="module")
def scene():
    return synth.make_scene_workload()          # 64x48 on 256x512, K = 6: 38 965 events


def make_legm(sensor, pano, lut=None):
    from emba_amd import LEGM
    return LEGM(sensor[0], sensor[1], VC.lut_of(sensor) if lut is None else lut, 0.2, pano[0], pano[1], device=0)


def ptr(a, ty):
    return None if a is None else a.ctypes.data_as(ty)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def numpy_eval(c, q, pm, valid, skip_zero, huber_k, frames=None):
    """io.align_terms / align_sums of every frame from the device's pm: (sums [F, 10], counts [F, 4], scale [F, 10], resid [F, S])."""
    out = [[], [], [], []]
    frames = c["frames"] if frames is None else frames
    for f in range(len(q)):
        t = eio.align_terms(frames[f], pm[f], c["lut"], q[f], c["I"], valid, c["lo"], c["hi"], skip_zero, huber_k)
        s, n, scale = eio.align_sums(t, with_scale=True)
        for o, v in zip(out, (s, n, scale, t["r"])):
            o.append(v)
    return [np.array(o) for o in out]


def sums_distance(got, want, scale):
    """The worst |got - want| over its allowance SUM_REL * sum |terms| + SUM_FLOOR * max |want|: at most 1 where the bound holds."""
    allow = SUM_REL * scale + SUM_FLOOR * max(float(np.abs(want).max()), 1e-300)
    return float((np.abs(got - want) / allow).max())


@pytest.mark.parametrize("kind", AC.KINDS)
@pytest.mark.parametrize("pano", AC.PANOS, ids=lambda p: f"pano{p[1]}x{p[0]}")
@pytest.mark.parametrize("sensor", AC.SENSORS, ids=lambda s: f"sensor{s[0]}x{s[1]}")
def test_every_evaluation_against_the_numpy_forms(gpu, sensor, pano, kind):
    sw_, sh_ = sensor
    m = make_legm(sensor, pano)
    m.set_option("poison", 1)      # a cell that is read before it is written shows
    worst, seen = 0.0, np.zeros(4, np.int64)
    for F in AC.FRAMES:
        c = AC.case(sensor, pano, kind, F)
        k = AC.huber_split(c)
        fr = c["frames"].copy()      # a rendered frame holds the byte 0 almost only where it looks past the panorama: every 11th byte is zeroed, so that
        fr.reshape(-1)[::11] = 0     # skip_zero has pixels to skip inside the panorama
        for valid in (None, c["valid"]):
            for skip_zero in (False, True):
                for huber_k in (0.0, k):
                    what = f"{sensor} on {pano}, {kind}, F = {F}, mask = {valid is not None}, skip_zero = {skip_zero}, huber_k = {huber_k}"
                    g = m.align_frames_eval(fr.reshape(F, sh_, sw_), c["q_start"], c["I"], valid, lo=c["lo"], hi=c["hi"], skip_zero=skip_zero,
                                            huber_k=huber_k, want_pm=True, want_resid=True)
                    sums, counts, scale, resid = numpy_eval(c, c["q_start"], g["pm"], valid, skip_zero, huber_k, frames=fr)
                    assert np.array_equal(g["counts"], counts), what
                    assert (g["counts"].sum(axis=1) == sw_ * sh_).all(), what
                    assert np.array_equal(bits(g["resid"]), bits(resid)), what
                    d = sums_distance(g["sums"], sums, scale)
                    worst = max(worst, d)
                    assert d <= 1.0, (what, d)
                    seen += counts.sum(axis=0)
                    if huber_k > 0 and counts[0, 0] > 8:
                        assert not np.array_equal(g["sums"][0], last[0]), what      # the weight changes the sums
                    last = g["sums"]
    print(f"{sensor} on {pano}, {kind}: worst |sums_device - sums_numpy| = {worst * SUM_REL:.3e} of sum |terms| (allowed {SUM_REL:.0e})")
    assert seen[0] > 0 and seen[2] > 0 and seen[3] > 0 and (kind != "pitch" or seen[1] > 0)
    m.close()


def test_the_sums_are_deterministic(gpu):
    """The same call twice, and once more after an unrelated stage ran in between: bit-equal sums (64 x 48: twelve workgroups per frame)."""
    sensor, pano = (64, 48), (128, 64)
    c = AC.case(sensor, pano, "pitch", 65)
    m = make_legm(sensor, pano)
    fr = c["frames"].reshape(65, 48, 64)
    call = lambda: m.align_frames_eval(fr, c["q_start"], c["I"], c["valid"], lo=c["lo"], hi=c["hi"], skip_zero=True, huber_k=0.05)
    a, b = call(), call()
    m.mosaic_frames(fr, c["ts"], LinearTrajectory(np.ascontiguousarray(VC.knots_of("pitch")), VC.T0_NS, VC.DT_NS), skip_zero=True)
    m.render_views(c["ts"], VC.knots_of("yaw_pi"), VC.T0_NS, VC.DT_NS, plane=c["I"])
    d = call()
    assert np.abs(a["sums"]).max() > 0
    for other in (b, d):
        assert np.array_equal(bits(a["sums"]), bits(other["sums"])) and np.array_equal(a["counts"], other["counts"])
    # ... and a frame's sums do not depend on the frames around it
    one = m.align_frames_eval(fr[17:18], c["q_start"][17:18], c["I"], c["valid"], lo=c["lo"], hi=c["hi"], skip_zero=True, huber_k=0.05)
    assert np.array_equal(bits(one["sums"][0]), bits(a["sums"][17]))
    m.close()


@pytest.mark.parametrize("sensor,pano", [((20, 13), (48, 24)), ((64, 48), (128, 64))])
def test_the_loop_is_consistent_with_the_evaluation(gpu, sensor, pano):
    m = make_legm(sensor, pano)
    m.set_option("poison", 1)
    for kind in AC.KINDS:
        c = AC.case(sensor, pano, kind, 3)
        fr = c["frames"].reshape(3, sensor[1], sensor[0])
        kw = dict(lo=c["lo"], hi=c["hi"], skip_zero=True)
        start = m.align_frames_eval(fr, c["q_start"], c["I"], **kw)
        # max_iters = 0: nothing moves
        r0 = m.align_frames(fr, c["q_start"], c["I"], **kw, **dict(AC.SETTINGS, max_iters=0))
        assert np.array_equal(bits(r0["q"]), bits(c["q_start"])) and (r0["status"] == eio.ALIGN_ITERATIONS).all() and (r0["iters"] == 0).all()
        assert np.array_equal(bits(r0["cost0"]), bits(start["sums"][:, 9])) and np.array_equal(bits(r0["sums"]), bits(start["sums"]))
        assert np.array_equal(r0["n0"], start["counts"][:, 0]) and np.array_equal(r0["counts"], start["counts"])
        # max_iters = 1: the step of io.align_step on the device's own start sums, within the solver bound on delta
        r1 = m.align_frames(fr, c["q_start"], c["I"], **kw, **dict(AC.SETTINGS, max_iters=1))
        assert (r1["iters"] == 1).all() and np.array_equal(bits(r1["cost0"]), bits(start["sums"][:, 9]))
        for f in range(3):
            delta = eio.align_step(start["sums"][f, :6], start["sums"][f, 6:9], AC.SETTINGS["lambda0"])
            got = so3.log(so3.mul(r1["q"][f], so3.inverse(c["q_start"][f])))
            if np.array_equal(r1["q"][f], c["q_start"][f]):      # the trial was rejected: its mean cost at numpy's trial is not lower either
                continue
            assert np.all(np.abs(got - delta) <= 1e-9 * np.abs(delta).max() + 1e-7 * np.abs(delta)), (kind, f, got, delta)
        assert any(not np.array_equal(r1["q"][f], c["q_start"][f]) for f in range(3)), kind
        # any number of iterations: the sums and counts are the evaluation's at q_out, bit for bit
        for iters in (1, 5, AC.SETTINGS["max_iters"]):
            r = m.align_frames(fr, c["q_start"], c["I"], **kw, **dict(AC.SETTINGS, max_iters=iters))
            e = m.align_frames_eval(fr, r["q"], c["I"], **kw)
            assert np.array_equal(bits(r["sums"]), bits(e["sums"])) and np.array_equal(r["counts"], e["counts"]), (kind, iters)
    m.close()


@pytest.mark.parametrize("pano", AC.PANOS, ids=lambda p: f"pano{p[1]}x{p[0]}")
@pytest.mark.parametrize("sensor", AC.SENSORS, ids=lambda s: f"sensor{s[0]}x{s[1]}")
def test_convergence_on_the_cpu_chosen_cases(gpu, sensor, pano):
    """Every frame ends converged or stalled, none degenerate; no frame's mean cost rises; the angle to the truth is within 2 E_NP + tol_rot of the pair: both
    forms stop within tol_rot of the same minimiser, whose distance from the truth belongs to the bytes' quantisation, and the factor 2 absorbs a different
    accept / reject path."""
    m = make_legm(sensor, pano)
    F = AC.CONVERGENCE_F
    bound = 2.0 * AC.E_NP[(sensor, pano)] + AC.SETTINGS["tol_rot"]
    for kind in AC.KINDS:
        c = AC.case(sensor, pano, kind, F)
        r = m.align_frames(c["frames"].reshape(F, sensor[1], sensor[0]), c["q_start"], c["I"], lo=c["lo"], hi=c["hi"], skip_zero=True, **AC.SETTINGS)
        err = eio.rotation_angle_between(c["q_true"], r["q"])
        print(f"{sensor} on {pano}, {kind}: angle to the truth {err.max():.4e} rad (bound {bound:.4e}), status {r['status'].tolist()}, iters {r['iters'].tolist()}")
        assert set(r["status"].tolist()) <= {eio.ALIGN_CONVERGED, eio.ALIGN_STALLED}, (kind, r["status"])
        assert (r["sums"][:, 9] / r["counts"][:, 0] <= r["cost0"] / r["n0"]).all(), kind
        assert err.max() <= bound, (kind, err, bound)
    m.close()


def test_the_mosaic_as_the_plane(gpu):
    """mosaic_frames at the true rotations, then align_frames(use_mosaic) from the perturbed ones: within 2 E_NP_MOSAIC + tol_rot."""
    sensor, pano = AC.MOSAIC_PAIR
    F = AC.CONVERGENCE_F
    m = make_legm(sensor, pano)
    bound = 2.0 * AC.E_NP_MOSAIC + AC.SETTINGS["tol_rot"]
    for kind in AC.KINDS:
        c = AC.case(sensor, pano, kind, F)
        fr = c["frames"].reshape(F, sensor[1], sensor[0])
        m.mosaic_frames(fr, c["ts"], LinearTrajectory(np.ascontiguousarray(VC.knots_of(kind)), VC.T0_NS, VC.DT_NS), skip_zero=True)
        before = m.mosaic()
        r = m.align_frames(fr, c["q_start"], use_mosaic=True, skip_zero=True, **AC.SETTINGS)
        # the same plane handed over by the caller gives the same bits
        r2 = m.align_frames(fr, c["q_start"], before["mean"], before["covered"], skip_zero=True, **AC.SETTINGS)
        assert np.array_equal(bits(r["q"]), bits(r2["q"])) and np.array_equal(bits(r["sums"]), bits(r2["sums"]))
        after = m.mosaic()
        assert np.array_equal(after["sum_w"], before["sum_w"]) and np.array_equal(after["sum_v"], before["sum_v"])
        err = eio.rotation_angle_between(c["q_true"], r["q"])
        print(f"mosaic as the plane, {kind}: angle to the truth {err.max():.4e} rad (bound {bound:.4e}), status {r['status'].tolist()}")
        assert set(r["status"].tolist()) <= {eio.ALIGN_CONVERGED, eio.ALIGN_STALLED} and (r["counts"][:, 2] > 0).all()
        assert err.max() <= bound, (kind, err)
    m.close()


def test_chunk_edge(gpu):
    """F = 65 535 + 3 frames of the 7 x 5 sensor: two chunks.  The frames on both sides of the cut give the counts and sums of the same frames in a small
    call, bit for bit."""
    sensor, pano = (7, 5), (32, 16)
    F = 65535 + 3
    c = AC.case(sensor, pano, "yaw_pi", 3)
    m = make_legm(sensor, pano)
    m.set_option("poison", 1)
    rng = np.random.default_rng(65538)
    frames = rng.integers(0, 256, (F, 5, 7)).astype(np.uint8)
    q = rng.standard_normal((F, 4))
    q /= np.linalg.norm(q, axis=1)[:, None]
    kw = dict(valid=c["valid"], lo=c["lo"], hi=c["hi"], skip_zero=True, huber_k=0.1)
    big = m.align_frames_eval(frames, q, c["I"], **kw)
    edge = slice(65535 - 4, 65535 + 3)
    small = m.align_frames_eval(frames[edge], q[edge], c["I"], **kw)
    assert np.array_equal(bits(big["sums"][edge]), bits(small["sums"])) and np.array_equal(big["counts"][edge], small["counts"])
    first = m.align_frames_eval(frames[:2], q[:2], c["I"], **kw)
    assert np.array_equal(bits(big["sums"][:2]), bits(first["sums"])) and np.array_equal(big["counts"][:2], first["counts"])
    assert (big["counts"].sum(axis=1) == 35).all() and big["counts"][:, 0].sum() > F and np.abs(small["sums"]).max() > 0
    m.close()


def test_statuses(gpu):
    sensor, pano = (20, 13), (48, 24)
    c = AC.case(sensor, pano, "yaw_pi", 3)
    fr = c["frames"].reshape(3, 13, 20)
    m = make_legm(sensor, pano)
    # a frame looking wholly past the mask is degenerate and keeps its q; the frame next to it is not touched by that
    hidden = np.zeros(c["I"].shape, bool)
    r = m.align_frames(fr, c["q_start"], c["I"], hidden, lo=c["lo"], hi=c["hi"], **AC.SETTINGS)
    assert (r["status"] == eio.ALIGN_DEGENERATE).all() and np.array_equal(bits(r["q"]), bits(c["q_start"])) and (r["iters"] == 0).all()
    assert (r["counts"][:, 0] == 0).all() and (r["counts"][:, 2] > 0).all()
    H, W = c["I"].shape
    pm0 = m.align_frames_eval(fr[:1], c["q_start"][:1], c["I"], lo=c["lo"], hi=c["hi"], want_pm=True)["pm"][0]
    half = np.ones((H, W), bool)
    cols = np.unique(np.floor(pm0[:, 0]).astype(np.int64) % W)
    half[:, cols] = False
    half[:, (cols + 1) % W] = False      # frame 0 sees masked cells only; the mask is the same for all three, so test what numpy says of each
    r = m.align_frames(fr, c["q_start"], c["I"], half, lo=c["lo"], hi=c["hi"], **AC.SETTINGS)
    assert r["status"][0] == eio.ALIGN_DEGENERATE and np.array_equal(r["q"][0], c["q_start"][0])
    # max_iters exhausted
    r = m.align_frames(fr, c["q_start"], c["I"], lo=c["lo"], hi=c["hi"], **dict(AC.SETTINGS, max_iters=2))
    assert (r["status"] == eio.ALIGN_ITERATIONS).all() and (r["iters"] == 2).all()
    # lambda_max = lambda0: a rejection at lambda0 stalls its frame; no frame is degenerate
    r = m.align_frames(fr, c["q_start"], c["I"], lo=c["lo"], hi=c["hi"], **dict(AC.SETTINGS, lambda0=1e-3, lambda_max=1e-3, lambda_min=0.0))
    assert set(r["status"].tolist()) <= {eio.ALIGN_CONVERGED, eio.ALIGN_STALLED, eio.ALIGN_ITERATIONS}
    # F = 0 launches nothing
    r = m.align_frames(fr[:0], c["q_start"][:0], c["I"], **AC.SETTINGS)
    assert r["q"].shape == (0, 4)
    assert m.align_frames_eval(fr[:0], c["q_start"][:0], c["I"])["sums"].shape == (0, 10)
    m.close()


def test_every_refusal_by_status(gpu, scene):
    w = scene
    S = 64 * 48
    m = make_legm((64, 48), (512, 256), lut=w.lut)
    m.set_events(w.events)
    m.upload_map(w.Gx, w.Gy)
    first = m.step(w.traj, w.thres_valid_pixel, w.alpha)
    ep0 = m.get_ep()
    L = m._L
    F = 3
    frames = np.random.default_rng(3).integers(0, 256, (F, 48, 64)).astype(np.uint8)
    q = np.tile(np.array([0.0, 0.0, 0.0, 1.0]), (F, 1))
    plane = np.random.default_rng(4).standard_normal((256, 512))
    out = dict(sums=np.full((F, 10), 4.25), counts=np.full((F, 4), 77, np.uint64), pm=np.full((F, S, 2), -1.5), resid=np.full((F, S), 2.5), q=np.full((F, 4), 3.5),
               status=np.full(F, 9, np.int32), iters=np.full(F, 8, np.int32), cost0=np.full(F, 1.5), n0=np.full(F, 55, np.uint64))
    good = dict(eio.ALIGN_DEFAULTS)

    def untouched():
        return ((out["sums"] == 4.25).all() and (out["counts"] == 77).all() and (out["pm"] == -1.5).all() and (out["resid"] == 2.5).all() and (out["q"] == 3.5).all()
                and (out["status"] == 9).all() and (out["iters"] == 8).all() and (out["cost0"] == 1.5).all() and (out["n0"] == 55).all())

    def call_eval(fr=frames, F_=F, q_=q, pl=plane, use_mosaic=0, min_weight=256, fill=0.0, lo=0.0, hi=1.0, huber_k=0.0):
        return L.emba_frames_align_eval(m._ctx, ptr(fr, _u8p), F_, ptr(q_, _dp), ptr(pl, _dp), None, use_mosaic, min_weight, fill, lo, hi, 1, huber_k,
                                        ptr(out["sums"], _dp), ptr(out["counts"], _u64p), ptr(out["pm"], _dp), ptr(out["resid"], _dp))

    def call_loop(fr=frames, F_=F, q_=q, pl=plane, use_mosaic=0, min_weight=256, fill=0.0, lo=0.0, hi=1.0, null_settings=False, **kw):
        s = dict(good, **kw)
        cs = _lib.EmbaAlignSettings(int(s["max_iters"]), int(s["min_pixels"]), s["lambda0"], s["lambda_up"], s["lambda_down"], s["lambda_min"], s["lambda_max"],
                                    s["tol_rot"], s["huber_k"])
        return L.emba_frames_align(m._ctx, ptr(fr, _u8p), F_, ptr(q_, _dp), ptr(pl, _dp), None, use_mosaic, min_weight, fill, lo, hi, 1,
                                   None if null_settings else C.addressof(cs), ptr(out["q"], _dp), ptr(out["sums"], _dp), ptr(out["counts"], _u64p),
                                   ptr(out["status"], _i32p), ptr(out["iters"], _i32p), ptr(out["cost0"], _dp), ptr(out["n0"], _u64p))

    def unchanged(st, want):
        again = m.step(w.traj, w.thres_valid_pixel, w.alpha)      # the context still evaluates its window
        return st == want and untouched() and again == first and np.array_equal(bits(m.get_ep()), bits(ep0))

    nan, inf = float("nan"), float("inf")
    bad_q = []
    for v in (nan, inf):
        b = q.copy()
        b[1, 2] = v
        bad_q.append(b)
    z = q.copy()
    z[2] = 0.0
    bad_q.append(z)
    for call in (call_eval, call_loop):
        assert unchanged(call(fr=None), ERR_INVALID_ARG) and unchanged(call(q_=None), ERR_INVALID_ARG)
        assert unchanged(call(F_=1 << 31), ERR_INVALID_ARG)
        for lo, hi in ((nan, 1.0), (0.0, inf), (-inf, 1.0), (1.0, 1.0), (2.0, 1.0)):
            assert unchanged(call(lo=lo, hi=hi), ERR_INVALID_ARG), (lo, hi)
        for b in bad_q:
            assert unchanged(call(q_=b), ERR_INVALID_ARG)
        assert unchanged(call(pl=None), ERR_INVALID_ARG)                                    # neither a plane nor the mosaic
        assert unchanged(call(pl=None, use_mosaic=1, min_weight=0), ERR_INVALID_ARG)
        assert unchanged(call(pl=None, use_mosaic=1, fill=nan), ERR_INVALID_ARG)
        assert unchanged(call(pl=None, use_mosaic=1), ERR_STATE)                            # nothing accumulated
    assert unchanged(call_eval(huber_k=nan), ERR_INVALID_ARG) and unchanged(call_loop(huber_k=nan), ERR_INVALID_ARG)
    assert unchanged(call_loop(null_settings=True), ERR_INVALID_ARG)
    for kw in (dict(max_iters=-1), dict(lambda_up=1.0), dict(lambda_down=0.5), dict(lambda_up=nan), dict(lambda0=0.0), dict(lambda0=-1.0), dict(lambda0=nan),
               dict(min_pixels=2), dict(tol_rot=-1.0), dict(lambda_min=-1.0), dict(lambda_max=nan)):
        assert unchanged(call_loop(**kw), ERR_INVALID_ARG), kw
    # F = 0: nothing launched, nothing written
    assert unchanged(call_eval(F_=0, fr=None, q_=None), 0) and unchanged(call_loop(F_=0, fr=None, q_=None), 0)
    # the calls themselves still go
    assert call_eval() == 0 and call_loop() == 0 and not untouched()
    assert (out["counts"].sum(axis=1) == S).all() and set(out["status"].tolist()) <= {1, 2, 3, 4}
    m.close()


def test_a_call_in_between_changes_nothing(gpu, scene):
    """The two calls between two steps and a mosaic change neither the step's ep nor the mosaic's sums."""
    w = scene
    t_end = w.traj.t0_ns + w.traj.dt_ns * (w.K - 1) - 1
    ts = np.array([w.traj.t0_ns, t_end], np.int64)
    frames = np.random.default_rng(9).integers(0, 256, (2, 48, 64)).astype(np.uint8)
    q = np.array([w.traj.evaluate(int(t)) for t in ts])
    plane = np.random.default_rng(10).random((256, 512)) * 255.0
    got = []
    for between in (False, True):
        m = make_legm((64, 48), (512, 256), lut=w.lut)
        m.set_events(w.events)
        m.upload_map(w.Gx, w.Gy)
        first = m.step(w.traj, w.thres_valid_pixel, w.alpha)
        m.mosaic_frames(frames, ts, w.traj, skip_zero=True)
        if between:
            m.align_frames_eval(frames, q, plane, want_pm=True, want_resid=True)
            m.align_frames(frames, q, plane, max_iters=3)
            m.align_frames_eval(frames, q, use_mosaic=True)
            m.align_frames(frames, q, use_mosaic=True, min_weight=1, fill=-3.0, max_iters=3, huber_k=4.0)
        mosaic = m.mosaic()
        second = m.step(w.traj, w.thres_valid_pixel, w.alpha)
        got.append((first, second, m.get_ep(), m.last_counts(), m.event_counts(), m.downloadMap(), mosaic))
        m.close()
    a, b = got
    assert a[0] == b[0] and a[1] == b[1] and a[3] == b[3] and a[4] == b[4] and a[0][0] > 1000
    assert np.array_equal(bits(a[2]), bits(b[2]))
    assert np.array_equal(bits(a[5][0]), bits(b[5][0])) and np.array_equal(bits(a[5][1]), bits(b[5][1]))
    for k in ("sum_w", "sum_v", "covered"):
        assert np.array_equal(a[6][k], b[6][k])
    assert np.array_equal(bits(a[6]["mean"]), bits(b[6]["mean"])) and a[6]["n_covered"] == b[6]["n_covered"]


def test_run_ba_refines_the_frames_of_another_run(gpu, tmp_path):
    """examples/run_ba.py --demo with --views-hz writes frames; a second run takes them as --frames with --refine-frames 1 and writes frames_aligned.txt."""
    out1, out2 = tmp_path / "out1", tmp_path / "out2"
    exe = [sys.executable, os.path.join(ROOT, "examples", "run_ba.py")]
    r = subprocess.run(exe + ["--demo", str(out1), "--views-hz", "50", "--window-size", "0.5", "--max-iter", "3"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    lo, hi = open(out1 / "views" / "tone.txt").read().split()
    n_frames = len(open(out1 / "views" / "times.txt").read().splitlines())
    r = subprocess.run(exe + ["--demo", str(out2), "--frames", str(out1 / "views"), "--refine-frames", "1", "--frames-huber", "8", "--init-map", "frames", "--frames-log", "0",
                              "--frames-lo", lo, "--frames-hi", hi, "--frames-skip-zero", "--max-iter", "3"], capture_output=True, text=True, timeout=600)
    print(r.stdout[-3000:])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "refine-frames round 1" in r.stdout and "frame mosaic:" in r.stdout
    rows = [l.split() for l in open(out2 / "frames_aligned.txt").read().splitlines() if l and not l.startswith("#")]
    assert len(rows) == n_frames and all(len(x) == 8 for x in rows)
    status = {int(x[5]) for x in rows}
    assert status <= {1, 2, 3, 4} and status & {1, 2}
    qn = np.array([[float(v) for v in x[1:5]] for x in rows])
    assert np.abs(np.linalg.norm(qn, axis=1) - 1.0).max() < 1e-9
    assert (out2 / "refined_traj.txt").exists() and (out2 / "frame_mosaic.pgm").exists()
    # --refine-frames refuses without --frames, and along a trajectory that carries the timing only
    r = subprocess.run(exe + ["--demo", str(tmp_path / "out3"), "--refine-frames", "1"], capture_output=True, text=True, timeout=600)
    assert r.returncode != 0 and "--frames" in r.stderr
    r = subprocess.run(exe + ["--demo", str(tmp_path / "out3"), "--frames", str(out1 / "views"), "--refine-frames", "1", "--init-poses", "identity", "--window-size", "0.5"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode != 0 and "given poses" in r.stderr
