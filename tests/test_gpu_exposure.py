"""Per-frame exposure on the MI355X (include/emba_hip.h: emba_frames_exposure_eval, emba_frames_exposure_align, emba_mosaic_frames_exposure)
against the numpy forms of the same rule (emba_amd.io: exposure_terms, exposure_sums, exposure_step, exposure_bytes, mosaic_votes).  The seam is pm_out: fed
the device's pm, numpy gives the counts as equal integers and the residuals bit for bit; the 21 sums are held to the suite's standing bound for
Jacobian-derived quantities, 1e-5 relative to sum |terms| of each sum with a floor of 1e-12 of the array's scale.  Then what is shared with
emba_frames_align_eval and emba_frames_align bit for bit, determinism, the recovery of known distortions within twice numpy's recorded deviations
(tests/exposure_cases.py), the first step against io.exposure_step, the constant-byte frame, the gain bounds, the mosaic of compensated bytes as integers,
the chunk edge, every refusal, what the calls leave alone, and examples/run_ba.py --frames-exposure."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import exposure_cases as XC
import view_cases as VC
from emba_amd import _lib
from emba_amd import io as eio
from emba_amd import so3, synth
from emba_amd.legm import LinearTrajectory

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_INVALID_ARG, ERR_STATE = 1, 5
SUM_REL, SUM_FLOOR = 1e-5, 1e-12      # README: Jacobian-derived quantities
SHARED = list(eio.EXPOSURE_SHARED)
_dp, _u8p, _i32p, _u64p, _i64p = (C.POINTER(t) for t in (C.c_double, C.c_uint8, C.c_int32, C.c_uint64, C.c_int64))
PAIR_IDS = lambda p: f"sensor{p[0][0]}x{p[0][1]}-pano{p[1][1]}x{p[1][0]}"


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


def traj_of(kind):
    return LinearTrajectory(np.ascontiguousarray(VC.knots_of(kind)), VC.T0_NS, VC.DT_NS)


def numpy_eval(frames, q, gain, bias, pm, lut, plane, valid, lo, hi, skip_zero, huber_k):
    """io.exposure_terms / exposure_sums of every frame from the device's pm: (sums [F, 21], counts [F, 4], scale [F, 21], resid [F, S])."""
    out = [[], [], [], []]
    for f in range(len(q)):
        t = eio.exposure_terms(frames[f], pm[f], lut, q[f], plane, gain[f], bias[f], valid, lo, hi, skip_zero, huber_k)
        s, n, scale = eio.exposure_sums(t, with_scale=True)
        for o, v in zip(out, (s, n, scale, t["r"])):
            o.append(v)
    return [np.array(o) for o in out]


def sums_distance(got, want, scale):
    """The worst |got - want| over its allowance SUM_REL * sum |terms| + SUM_FLOOR * max |want|: at most 1 where the bound holds."""
    allow = SUM_REL * scale + SUM_FLOOR * max(float(np.abs(want).max()), 1e-300)
    return float((np.abs(got - want) / allow).max())


@pytest.mark.parametrize("kind", XC.KINDS)
@pytest.mark.parametrize("pair", XC.KEPT, ids=PAIR_IDS)
def test_every_evaluation_against_the_numpy_forms(gpu, pair, kind):
    sensor, pano = pair
    sw_, sh_ = sensor
    F = XC.F
    m = make_legm(sensor, pano)
    m.set_option("poison", 1)      # a cell that is read before it is written shows
    c = XC.case(sensor, pano, kind)
    k = 0.05
    fr = c["distorted"].copy()
    fr.reshape(-1)[::11] = 0       # pixels for skip_zero to skip inside the panorama
    fr3 = fr.reshape(F, sh_, sw_)
    gain, bias = c["gain"] * np.array([1.0, 0.9, 1.1]), c["bias"] + np.array([0.0, 0.05, -0.05])
    worst, seen = 0.0, np.zeros(4, np.int64)
    for valid in (None, c["valid"]):
        for skip_zero in (False, True):
            for huber_k in (0.0, k):
                what = f"{sensor} on {pano}, {kind}, mask = {valid is not None}, skip_zero = {skip_zero}, huber_k = {huber_k}"
                g = m.exposure_eval(fr3, c["q_start"], gain, bias, c["I"], valid, lo=c["lo"], hi=c["hi"], skip_zero=skip_zero, huber_k=huber_k, want_pm=True,
                                    want_resid=True)
                sums, counts, scale, resid = numpy_eval(fr, c["q_start"], gain, bias, g["pm"], c["lut"], c["I"], valid, c["lo"], c["hi"], skip_zero, huber_k)
                assert np.array_equal(g["counts"], counts), what
                assert (g["counts"].sum(axis=1) == sw_ * sh_).all(), what
                assert np.array_equal(bits(g["resid"]), bits(resid)), what
                d = sums_distance(g["sums"], sums, scale)
                worst = max(worst, d)
                assert d <= 1.0, (what, d)
                seen += counts.sum(axis=0)
                # gain 1, bias 0: the ten sums shared with emba_frames_align_eval and its residuals are its own, bit for bit
                e1 = m.exposure_eval(fr3, c["q_start"], 1.0, 0.0, c["I"], valid, lo=c["lo"], hi=c["hi"], skip_zero=skip_zero, huber_k=huber_k, want_resid=True)
                al = m.align_frames_eval(fr3, c["q_start"], c["I"], valid, lo=c["lo"], hi=c["hi"], skip_zero=skip_zero, huber_k=huber_k, want_resid=True)
                assert np.array_equal(bits(e1["sums"][:, SHARED]), bits(al["sums"])) and np.array_equal(e1["counts"], al["counts"]), what
                assert np.array_equal(bits(e1["resid"]), bits(al["resid"])), what
    # use_mosaic: the mosaic of the rendered frames at the true rotations is the plane, its covered cells the mask, in byte units
    m.mosaic_frames(c["frames"].reshape(F, sh_, sw_), c["ts"], traj_of(kind), skip_zero=True)
    mo = m.mosaic()
    gb, bb = np.array([1.1, 1.25, 1.45]), np.array([-12.0, -40.0, -70.0])
    for huber_k in (0.0, 4.0):
        g = m.exposure_eval(fr3, c["q_start"], gb, bb, use_mosaic=True, skip_zero=True, huber_k=huber_k, want_pm=True, want_resid=True)
        sums, counts, scale, resid = numpy_eval(fr, c["q_start"], gb, bb, g["pm"], c["lut"], mo["mean"], mo["covered"], 0.0, 255.0, True, huber_k)
        assert np.array_equal(g["counts"], counts) and np.array_equal(bits(g["resid"]), bits(resid)), (kind, "use_mosaic", huber_k)
        d = sums_distance(g["sums"], sums, scale)
        worst = max(worst, d)
        assert d <= 1.0, (kind, "use_mosaic", huber_k, d)
    after = m.mosaic()
    assert np.array_equal(after["sum_w"], mo["sum_w"]) and np.array_equal(after["sum_v"], mo["sum_v"])
    print(f"{sensor} on {pano}, {kind}: worst |sums_device - sums_numpy| = {worst * SUM_REL:.3e} of sum |terms| (allowed {SUM_REL:.0e})")
    assert seen[0] > 0 and seen[2] > 0 and seen[3] > 0 and (kind != "pitch" or seen[1] > 0)
    m.close()


def test_the_sums_are_deterministic(gpu):
    """The same call twice, and once more after an unrelated stage ran in between: bit-equal sums (64 x 48: twelve workgroups per frame).  A frame's sums do
    not depend on the frames around it."""
    sensor, pano = (64, 48), (48, 24)
    n = 65
    c = XC.case(sensor, pano, "pitch", n)
    m = make_legm(sensor, pano)
    fr = c["distorted"].reshape(n, 48, 64)
    gain, bias = np.linspace(0.8, 1.5, n), np.linspace(-0.2, 0.2, n)
    call = lambda: m.exposure_eval(fr, c["q_start"], gain, bias, c["I"], c["valid"], lo=c["lo"], hi=c["hi"], skip_zero=True, huber_k=0.05)
    a, b = call(), call()
    m.mosaic_frames_exposure(fr, c["ts"], traj_of("pitch"), gain, bias, skip_zero=True)
    m.render_views(c["ts"], VC.knots_of("yaw_pi"), VC.T0_NS, VC.DT_NS, plane=c["I"])
    m.align_frames_eval(fr, c["q_start"], c["I"], lo=c["lo"], hi=c["hi"])
    d = call()
    assert np.abs(a["sums"]).min(axis=0).max() > 0
    for other in (b, d):
        assert np.array_equal(bits(a["sums"]), bits(other["sums"])) and np.array_equal(a["counts"], other["counts"])
    one = m.exposure_eval(fr[17:18], c["q_start"][17:18], gain[17:18], bias[17:18], c["I"], c["valid"], lo=c["lo"], hi=c["hi"], skip_zero=True, huber_k=0.05)
    assert np.array_equal(bits(one["sums"][0]), bits(a["sums"][17])) and np.array_equal(one["counts"][0], a["counts"][17])
    m.close()


@pytest.mark.parametrize("pair", [((20, 13), (48, 24)), ((64, 48), (32, 16))], ids=PAIR_IDS)
def test_nothing_estimated_is_emba_frames_align(gpu, pair):
    """estimate = 0 at gain 1 and bias 0: the q_out, status and iterations of emba_frames_align, bit for bit (and its sums, counts, cost0 and n0)."""
    sensor, pano = pair
    m = make_legm(sensor, pano)
    m.set_option("poison", 1)
    for kind in XC.KINDS:
        c = XC.case(sensor, pano, kind)
        for frames, valid, huber_k in ((c["frames"], None, 0.0), (c["distorted"], c["valid"], 0.05)):
            fr = frames.reshape(XC.F, sensor[1], sensor[0])
            s = dict(XC.SETTINGS, huber_k=huber_k)
            a = m.align_frames(fr, c["q_start"], c["I"], valid, lo=c["lo"], hi=c["hi"], skip_zero=True, **s)
            e = m.align_frames_exposure(fr, c["q_start"], 1.0, 0.0, 0, c["I"], valid, lo=c["lo"], hi=c["hi"], skip_zero=True, **XC.BOUNDS, **s)
            assert np.array_equal(bits(a["q"]), bits(e["q"])) and np.array_equal(a["status"], e["status"]) and np.array_equal(a["iters"], e["iters"]), kind
            assert np.array_equal(bits(a["sums"]), bits(e["sums"][:, SHARED])) and np.array_equal(a["counts"], e["counts"]), kind
            assert np.array_equal(bits(a["cost0"]), bits(e["cost0"])) and np.array_equal(a["n0"], e["n0"]), kind
            assert (e["gain"] == 1.0).all() and (e["bias"] == 0.0).all() and (e["iters"] > 0).any()
    m.close()


@pytest.mark.parametrize("pair", XC.KEPT, ids=PAIR_IDS)
def test_recovery_against_the_true_plane(gpu, pair):
    """From PERTURB off, gain 1, bias 0, estimate = 3, against the plane the frames were rendered from: no frame ends degenerate, no frame's mean cost
    rises, and the angle, the gain and the bias end within 2 E_NP + tol_rot, 2 DA_NP and 2 DB_NP of the truth — twice what numpy's own loop leaves
    (tests/exposure_cases.py): an accept / reject near a tie may fall the other way under a pm that differs in its last bits."""
    sensor, pano = pair
    m = make_legm(sensor, pano)
    be, ba, bb = 2.0 * XC.E_NP[pair] + XC.SETTINGS["tol_rot"], 2.0 * XC.DA_NP[pair], 2.0 * XC.DB_NP[pair]
    for kind in XC.KINDS:
        c = XC.case(sensor, pano, kind)
        fr = c["distorted"].reshape(XC.F, sensor[1], sensor[0])
        r = m.align_frames_exposure(fr, c["q_start"], 1.0, 0.0, 3, c["I"], lo=c["lo"], hi=c["hi"], skip_zero=True, **XC.BOUNDS, **XC.SETTINGS)
        err = eio.rotation_angle_between(c["q_true"], r["q"])
        da, db = np.abs(r["gain"] - c["gain"]), np.abs(r["bias"] - c["bias"])
        print(f"{sensor} on {pano}, {kind}: angle {err.max():.4e} rad (bound {be:.4e}), |a - a*| {da.max():.4e} (bound {ba:.4e}), |b - b*| {db.max():.4e} "
              f"(bound {bb:.4e}), status {r['status'].tolist()}, iters {r['iters'].tolist()}")
        assert set(r["status"].tolist()) <= {eio.ALIGN_CONVERGED, eio.ALIGN_STALLED}, (kind, r["status"])
        assert (r["sums"][:, 20] / r["counts"][:, 0] <= r["cost0"] / r["n0"]).all(), kind
        assert err.max() <= be and da.max() <= ba and db.max() <= bb, (kind, err, da, db)
        # the sums and counts are the evaluation's at (q, a, b), bit for bit
        e = m.exposure_eval(fr, r["q"], r["gain"], r["bias"], c["I"], lo=c["lo"], hi=c["hi"], skip_zero=True)
        assert np.array_equal(bits(r["sums"]), bits(e["sums"])) and np.array_equal(r["counts"], e["counts"]), kind
    m.close()


def test_the_first_step_is_exposure_step_of_the_first_sums(gpu):
    sensor, pano = (20, 13), (48, 24)
    m = make_legm(sensor, pano)
    moved = 0
    for kind in XC.KINDS:
        c = XC.case(sensor, pano, kind)
        fr = c["distorted"].reshape(XC.F, 13, 20)
        kw = dict(lo=c["lo"], hi=c["hi"], skip_zero=True)
        g0, b0 = np.array([1.0, 1.2, 1.4]), np.array([0.0, -0.1, -0.2])
        start = m.exposure_eval(fr, c["q_start"], g0, b0, c["I"], **kw)
        r0 = m.align_frames_exposure(fr, c["q_start"], g0, b0, 3, c["I"], **kw, **XC.BOUNDS, **dict(XC.SETTINGS, max_iters=0))
        assert np.array_equal(bits(r0["q"]), bits(c["q_start"])) and (r0["status"] == eio.ALIGN_ITERATIONS).all() and (r0["iters"] == 0).all()
        assert np.array_equal(bits(r0["sums"]), bits(start["sums"])) and np.array_equal(bits(r0["cost0"]), bits(start["sums"][:, 20]))
        assert np.array_equal(bits(r0["gain"]), bits(g0)) and np.array_equal(bits(r0["bias"]), bits(b0)) and np.array_equal(r0["n0"], start["counts"][:, 0])
        for estimate in (0, 1, 2, 3):
            r1 = m.align_frames_exposure(fr, c["q_start"], g0, b0, estimate, c["I"], **kw, **XC.BOUNDS, **dict(XC.SETTINGS, max_iters=1))
            assert (r1["iters"] == 1).all() and np.array_equal(bits(r1["cost0"]), bits(start["sums"][:, 20]))
            for f in range(XC.F):
                if not estimate & eio.EXPOSURE_GAIN:
                    assert r1["gain"][f] == g0[f]
                if not estimate & eio.EXPOSURE_BIAS:
                    assert r1["bias"][f] == b0[f]
                if np.array_equal(r1["q"][f], c["q_start"][f]):      # the trial was rejected: nothing moved
                    assert r1["gain"][f] == g0[f] and r1["bias"][f] == b0[f]
                    continue
                moved += 1
                x = eio.exposure_step(start["sums"][f], XC.SETTINGS["lambda0"], estimate)
                got = np.concatenate([so3.log(so3.mul(r1["q"][f], so3.inverse(c["q_start"][f]))), [r1["gain"][f] - g0[f], r1["bias"][f] - b0[f]]])
                assert np.all(np.abs(got - x) <= 1e-9 * np.abs(x).max() + 1e-7 * np.abs(x)), (kind, estimate, f, got, x)
    assert moved >= 12
    m.close()


def test_the_constant_byte_frame_and_the_gain_bounds(gpu):
    sensor, pano = (20, 13), (48, 24)
    c = XC.case(sensor, pano, "identity")
    m = make_legm(sensor, pano)
    fr = c["distorted"].reshape(XC.F, 13, 20).copy()
    fr[1] = 93      # one constant byte: gain and bias are collinear
    kw = dict(lo=c["lo"], hi=c["hi"], skip_zero=True)
    g0, b0 = np.array([1.0, 1.3, 1.0]), np.array([0.0, -0.1, 0.0])
    r = m.align_frames_exposure(fr, c["q_start"], g0, b0, 3, c["I"], **kw, **XC.BOUNDS, **XC.SETTINGS)
    assert r["status"][1] == eio.ALIGN_DEGENERATE and r["iters"][1] == 0 and np.array_equal(bits(r["q"][1]), bits(c["q_start"][1]))
    assert r["gain"][1] == 1.3 and r["bias"][1] == -0.1 and r["counts"][1, 0] > 100
    assert r["status"][0] != eio.ALIGN_DEGENERATE and r["status"][2] != eio.ALIGN_DEGENERATE      # the frames next to it are not touched by that
    for estimate in (0, 1, 2):
        r = m.align_frames_exposure(fr, c["q_start"], g0, b0, estimate, c["I"], **kw, **XC.BOUNDS, **XC.SETTINGS)
        assert r["status"][1] != eio.ALIGN_DEGENERATE, estimate
    # a trial past gain_max is rejected: frames 1 and 2 (a* = 1.25, 1.45) reach past 1.2 when they are free, and stay inside when they are not
    fr = c["distorted"].reshape(XC.F, 13, 20)
    free = m.align_frames_exposure(fr, c["q_start"], 1.0, 0.0, 3, c["I"], **kw, **XC.BOUNDS, **XC.SETTINGS)
    held = m.align_frames_exposure(fr, c["q_start"], 1.0, 0.0, 3, c["I"], **kw, gain_min=0.5, gain_max=1.2, **XC.SETTINGS)
    assert (free["gain"][1:] > 1.2).all() and (held["gain"] <= 1.2).all() and (held["gain"] >= 0.5).all() and (held["gain"][1:] > 1.0).all()
    assert abs(held["gain"][0] - free["gain"][0]) < 1e-3      # the frame whose gain lies inside is not touched by the bound
    # a gain that is not estimated keeps its input value, outside the bounds or not
    r = m.align_frames_exposure(fr, c["q_start"], 3.0, 0.0, eio.EXPOSURE_BIAS, c["I"], **kw, gain_min=0.5, gain_max=1.2, **dict(XC.SETTINGS, max_iters=5))
    assert (r["gain"] == 3.0).all() and (r["iters"] > 0).all()
    m.close()


@pytest.mark.parametrize("pair", [((7, 5), (32, 16)), ((20, 13), (48, 24)), ((64, 48), (48, 24))], ids=PAIR_IDS)
def test_the_mosaic_of_compensated_bytes(gpu, pair):
    sensor, pano = pair
    S = sensor[0] * sensor[1]
    m = make_legm(sensor, pano)
    m.set_option("poison", 1)
    gain, bias = np.array([a for a, _ in XC.DISTORTION]), np.array([b for _, b in XC.DISTORTION])
    for kind in XC.KINDS:
        c = XC.case(sensor, pano, kind)
        fr = c["distorted"].reshape(XC.F, sensor[1], sensor[0])
        tr = traj_of(kind)
        for skip_zero in (False, True):
            g = m.mosaic_frames_exposure(fr, c["ts"], tr, gain, bias, skip_zero=skip_zero, want_pm=True)
            mo = m.mosaic()
            # the raw byte decides what is skipped; the compensated byte is what is voted
            comp, pm = eio.exposure_bytes(c["distorted"], gain, bias).reshape(-1), g["pm"].reshape(-1, 2)
            keep = (c["distorted"].reshape(-1) != 0) if skip_zero else np.ones(comp.size, bool)
            sw, sv, dropped, _ = eio.mosaic_votes(comp[keep], pm[keep], pano[0], pano[1])
            assert g["skipped"] == int((~keep).sum()) and g["dropped"] == dropped, (kind, skip_zero)
            assert np.array_equal(mo["sum_w"], sw) and np.array_equal(mo["sum_v"], sv), (kind, skip_zero)
        # gain 1, bias 0: emba_mosaic_frames' sums
        m.mosaic_frames(fr, c["ts"], tr, skip_zero=True)
        plain = m.mosaic()
        m.mosaic_frames_exposure(fr, c["ts"], tr, 1.0, 0.0, skip_zero=True)
        same = m.mosaic()
        assert np.array_equal(plain["sum_w"], same["sum_w"]) and np.array_equal(plain["sum_v"], same["sum_v"]) and plain["sum_v"].sum() > 0
        # accumulate across a plain call and a compensated call: the sum of the two
        m.mosaic_frames_exposure(fr, c["ts"], tr, gain, bias, skip_zero=True)
        only = m.mosaic()
        m.mosaic_frames(fr, c["ts"], tr, skip_zero=True)
        m.mosaic_frames_exposure(fr, c["ts"], tr, gain, bias, skip_zero=True, accumulate=True)
        both = m.mosaic()
        assert np.array_equal(both["sum_w"], plain["sum_w"] + only["sum_w"]) and np.array_equal(both["sum_v"], plain["sum_v"] + only["sum_v"])
        m.mosaic_frames(fr, c["ts"], tr, skip_zero=True, accumulate=True)
        more = m.mosaic()
        assert np.array_equal(more["sum_v"], 2 * plain["sum_v"] + only["sum_v"])
    # the 2^36 bound: a call that would reach it is refused before anything is read, and the sums stay
    before = m.mosaic()
    F_big = (1 << 36) // S + 1
    small = np.zeros(S, np.uint8)
    one_t, one_g, one_b = np.array([VC.T0_NS], np.int64), np.ones(1), np.zeros(1)
    knots = np.ascontiguousarray(VC.knots_of("identity"))
    call = lambda F_, acc: m._L.emba_mosaic_frames_exposure(m._ctx, ptr(small, _u8p), ptr(one_t, _i64p), F_, ptr(one_g, _dp), ptr(one_b, _dp), ptr(knots, _dp), VC.K,
                                                            VC.T0_NS, VC.DT_NS, 1, acc, None, None, None)
    assert call(F_big, 0) == ERR_INVALID_ARG and call(F_big - 1, 1) == ERR_INVALID_ARG      # (F_big - 1 frames alone would fit; on top of the votes that are there they do not)
    after = m.mosaic()
    assert np.array_equal(before["sum_w"], after["sum_w"]) and np.array_equal(before["sum_v"], after["sum_v"])
    m.close()


def test_chunk_edge(gpu):
    """F = 65 535 + 3 frames of the 7 x 5 sensor, evaluated once: two chunks.  The frames on both sides of the cut give the counts and sums of the same frames
    in a small call, bit for bit: a frame's result does not depend on the chunk it is in."""
    sensor, pano = (7, 5), (32, 16)
    F = 65535 + 3
    c = XC.case(sensor, pano, "yaw_pi")
    m = make_legm(sensor, pano)
    m.set_option("poison", 1)
    rng = np.random.default_rng(65538)
    frames = rng.integers(0, 256, (F, 5, 7)).astype(np.uint8)
    q = rng.standard_normal((F, 4))
    q /= np.linalg.norm(q, axis=1)[:, None]
    gain, bias = rng.uniform(0.5, 2.0, F), rng.uniform(-0.3, 0.3, F)
    kw = dict(valid=c["valid"], lo=c["lo"], hi=c["hi"], skip_zero=True, huber_k=0.1)
    big = m.exposure_eval(frames, q, gain, bias, c["I"], **kw)
    edge = slice(65535 - 4, 65535 + 3)
    small = m.exposure_eval(frames[edge], q[edge], gain[edge], bias[edge], c["I"], **kw)
    assert np.array_equal(bits(big["sums"][edge]), bits(small["sums"])) and np.array_equal(big["counts"][edge], small["counts"])
    first = m.exposure_eval(frames[:2], q[:2], gain[:2], bias[:2], c["I"], **kw)
    assert np.array_equal(bits(big["sums"][:2]), bits(first["sums"])) and np.array_equal(big["counts"][:2], first["counts"])
    assert (big["counts"].sum(axis=1) == 35).all() and big["counts"][:, 0].sum() > F and np.abs(small["sums"]).max() > 0
    m.close()


def test_every_refusal_and_what_the_calls_leave_alone(gpu, scene):
    """Every refusal leaves the outputs and the mosaic as they were; the step path's ep and the resident map are unchanged after all three calls."""
    w = scene
    S = 64 * 48
    m = make_legm((64, 48), (512, 256), lut=w.lut)
    m.set_events(w.events)
    m.upload_map(w.Gx, w.Gy)
    first = m.step(w.traj, w.thres_valid_pixel, w.alpha)
    ep0 = m.get_ep()
    map0 = m.downloadMap()
    L = m._L
    F = 2
    t_end = w.traj.t0_ns + w.traj.dt_ns * (w.K - 1) - 1
    ts = np.array([w.traj.t0_ns, t_end], np.int64)
    frames = np.random.default_rng(3).integers(0, 256, (F, 48, 64)).astype(np.uint8)
    q = np.array([w.traj.evaluate(int(t)) for t in ts])
    knots = np.ascontiguousarray(w.traj.knots_xyzw, dtype=np.float64).reshape(-1, 4)
    plane = np.random.default_rng(4).random((256, 512)) * 255.0
    m.mosaic_frames(frames, ts, w.traj)
    mos0 = m.mosaic()
    gain, bias = np.array([1.1, 0.9]), np.array([2.0, -3.0])
    out = dict(sums=np.full((F, 21), 4.25), counts=np.full((F, 4), 77, np.uint64), pm=np.full((F, S, 2), -1.5), resid=np.full((F, S), 2.5), q=np.full((F, 4), 3.5),
               gain=np.full(F, 6.5), bias=np.full(F, 7.5), status=np.full(F, 9, np.int32), iters=np.full(F, 8, np.int32), cost0=np.full(F, 1.5),
               n0=np.full(F, 55, np.uint64), dropped=np.full(1, 31, np.uint64), skipped=np.full(1, 32, np.uint64))
    fills = dict(sums=4.25, counts=77, pm=-1.5, resid=2.5, q=3.5, gain=6.5, bias=7.5, status=9, iters=8, cost0=1.5, n0=55, dropped=31, skipped=32)
    good = dict(eio.ALIGN_DEFAULTS, max_iters=3)

    def untouched():
        return all((out[k] == v).all() for k, v in fills.items())

    def call_eval(fr=frames, F_=F, q_=q, g_=gain, b_=bias, pl=plane, use_mosaic=0, min_weight=256, fill=0.0, lo=0.0, hi=255.0, huber_k=0.0):
        return L.emba_frames_exposure_eval(m._ctx, ptr(fr, _u8p), F_, ptr(q_, _dp), ptr(g_, _dp), ptr(b_, _dp), ptr(pl, _dp), None, use_mosaic, min_weight, fill, lo, hi,
                                           1, huber_k, ptr(out["sums"], _dp), ptr(out["counts"], _u64p), ptr(out["pm"], _dp), ptr(out["resid"], _dp))

    def call_loop(fr=frames, F_=F, q_=q, g_=gain, b_=bias, pl=plane, use_mosaic=0, min_weight=256, fill=0.0, lo=0.0, hi=255.0, estimate=3, gain_min=0.25, gain_max=4.0,
                  null_settings=False, **kw):
        s = dict(good, **kw)
        cs = _lib.EmbaExposureSettings(_lib.EmbaAlignSettings(int(s["max_iters"]), int(s["min_pixels"]), s["lambda0"], s["lambda_up"], s["lambda_down"], s["lambda_min"],
                                                              s["lambda_max"], s["tol_rot"], s["huber_k"]), gain_min, gain_max)
        return L.emba_frames_exposure_align(m._ctx, ptr(fr, _u8p), F_, ptr(q_, _dp), ptr(g_, _dp), ptr(b_, _dp), estimate, ptr(pl, _dp), None, use_mosaic, min_weight,
                                            fill, lo, hi, 1, None if null_settings else C.addressof(cs), ptr(out["q"], _dp), ptr(out["gain"], _dp), ptr(out["bias"], _dp),
                                            ptr(out["sums"], _dp), ptr(out["counts"], _u64p), ptr(out["status"], _i32p), ptr(out["iters"], _i32p), ptr(out["cost0"], _dp),
                                            ptr(out["n0"], _u64p))

    def call_vote(fr=frames, t_=ts, F_=F, g_=gain, b_=bias, kn=knots, K_=None, dt=None, accumulate=1):
        return L.emba_mosaic_frames_exposure(m._ctx, ptr(fr, _u8p), ptr(t_, _i64p), F_, ptr(g_, _dp), ptr(b_, _dp), ptr(kn, _dp), knots.shape[0] if K_ is None else K_,
                                             int(w.traj.t0_ns), int(w.traj.dt_ns) if dt is None else dt, 0, accumulate, ptr(out["dropped"], _u64p),
                                             ptr(out["skipped"], _u64p), ptr(out["pm"], _dp))

    def unchanged(st, want):
        mo = m.mosaic()
        return st == want and untouched() and np.array_equal(mo["sum_w"], mos0["sum_w"]) and np.array_equal(mo["sum_v"], mos0["sum_v"])

    nan, inf = float("nan"), float("inf")
    bad_gb = []
    for v in (nan, inf, -inf):
        bad_gb.append(dict(g_=np.array([1.1, v])))
        bad_gb.append(dict(b_=np.array([v, 0.0])))
    bad_gb += [dict(g_=np.array([0.0, 1.0])), dict(g_=np.array([1.0, -2.0])), dict(g_=None), dict(b_=None)]
    bad_q = q.copy()
    bad_q[1, 2] = nan
    for call in (call_eval, call_loop, call_vote):
        for kw in bad_gb:
            assert unchanged(call(**kw), ERR_INVALID_ARG), (call.__name__, kw)
        assert unchanged(call(fr=None), ERR_INVALID_ARG)
    for call in (call_eval, call_loop):      # what emba_frames_align_eval / emba_frames_align refuse
        assert unchanged(call(q_=None), ERR_INVALID_ARG) and unchanged(call(q_=bad_q), ERR_INVALID_ARG) and unchanged(call(F_=1 << 31), ERR_INVALID_ARG)
        for lo, hi in ((nan, 1.0), (0.0, inf), (1.0, 1.0)):
            assert unchanged(call(lo=lo, hi=hi), ERR_INVALID_ARG), (lo, hi)
        assert unchanged(call(pl=None), ERR_INVALID_ARG) and unchanged(call(pl=None, use_mosaic=1, min_weight=0), ERR_INVALID_ARG)
        assert unchanged(call(pl=None, use_mosaic=1, fill=nan), ERR_INVALID_ARG)
    assert unchanged(call_eval(huber_k=nan), ERR_INVALID_ARG) and unchanged(call_loop(huber_k=nan), ERR_INVALID_ARG)
    assert unchanged(call_loop(null_settings=True), ERR_INVALID_ARG)
    for kw in (dict(estimate=-1), dict(estimate=4), dict(gain_min=0.0), dict(gain_min=-1.0), dict(gain_min=1.5), dict(gain_max=0.9), dict(gain_min=nan), dict(gain_max=nan),
               dict(gain_max=inf), dict(max_iters=-1), dict(lambda_up=1.0), dict(lambda0=0.0), dict(min_pixels=2), dict(tol_rot=-1.0), dict(lambda_max=nan)):
        assert unchanged(call_loop(**kw), ERR_INVALID_ARG), kw
    # what emba_mosaic_frames refuses
    assert unchanged(call_vote(t_=None), ERR_INVALID_ARG) and unchanged(call_vote(kn=None), ERR_INVALID_ARG) and unchanged(call_vote(K_=1), ERR_INVALID_ARG)
    assert unchanged(call_vote(dt=0), ERR_INVALID_ARG) and unchanged(call_vote(F_=1 << 31), ERR_INVALID_ARG)
    late = ts.copy()
    late[1] = t_end + 2 * int(w.traj.dt_ns)
    st = call_vote(t_=late)
    assert st not in (0, ERR_INVALID_ARG) and unchanged(st, st)      # EMBA_ERR_TIME_RANGE: decided before anything is voted or zeroed
    # use_mosaic with nothing accumulated is a matter of state
    m2 = make_legm((64, 48), (512, 256), lut=w.lut)
    st2 = m2._L.emba_frames_exposure_eval(m2._ctx, ptr(frames, _u8p), F, ptr(q, _dp), ptr(gain, _dp), ptr(bias, _dp), None, None, 1, 256, 0.0, 0.0, 255.0, 1, 0.0,
                                          ptr(out["sums"], _dp), None, None, None)
    assert st2 == ERR_STATE and untouched()
    m2.close()
    # F = 0: nothing launched, nothing written
    assert unchanged(call_eval(F_=0, fr=None, q_=None, g_=None, b_=None), 0) and unchanged(call_loop(F_=0, fr=None, q_=None, g_=None, b_=None), 0)
    # the calls themselves still go: against a plane, against the mosaic, and the vote on top of the mosaic
    assert call_eval() == 0 and call_loop() == 0 and call_eval(pl=None, use_mosaic=1) == 0 and call_loop(pl=None, use_mosaic=1) == 0 and not untouched()
    assert (out["counts"].sum(axis=1) == S).all() and set(out["status"].tolist()) <= {1, 2, 3, 4}
    mo = m.mosaic()
    assert np.array_equal(mo["sum_w"], mos0["sum_w"]) and np.array_equal(mo["sum_v"], mos0["sum_v"])      # (evaluating and aligning do not vote)
    assert call_vote() == 0
    mo = m.mosaic()
    assert int(mo["sum_w"].sum()) > int(mos0["sum_w"].sum()) and (mo["sum_w"] >= mos0["sum_w"]).all() and not np.array_equal(mo["sum_v"], mos0["sum_v"])
    # ... and the step path and the resident map have not seen any of it
    again = m.step(w.traj, w.thres_valid_pixel, w.alpha)
    map1 = m.downloadMap()
    assert again == first and np.array_equal(bits(m.get_ep()), bits(ep0))
    assert np.array_equal(bits(map0[0]), bits(map1[0])) and np.array_equal(bits(map0[1]), bits(map1[1]))
    m.close()


def test_run_ba_estimates_the_exposure_of_distorted_views(gpu, tmp_path):
    """examples/run_ba.py --demo with --views-hz writes frames; they are distorted frame by frame with a known exposure a*_f (v <- rint(a*_f v), 0 stays 0) and a
    second run takes them as --frames with --refine-frames 2 --frames-exposure gain-bias --init-map frames.  It runs to the end, writes the two extra columns,
    and the recovered gains a_f undo the exposures up to the common tone (a_f a*_f is one constant where they do): the standard deviation of a_f a*_f over the frames is lower than that of a*_f."""
    out1, out2, dist = tmp_path / "out1", tmp_path / "out2", tmp_path / "distorted"
    exe = [sys.executable, os.path.join(ROOT, "examples", "run_ba.py")]
    r = subprocess.run(exe + ["--demo", str(out1), "--views-hz", "50", "--window-size", "0.5", "--max-iter", "3"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    lo, hi = open(out1 / "views" / "tone.txt").read().split()
    lines = [l for l in open(out1 / "views" / "times.txt").read().splitlines() if l.strip()]
    os.makedirs(dist)
    a_star = 1.0 - 0.25 * (0.5 + 0.5 * np.sin(1.7 * np.arange(len(lines))))      # 0.75 ... 1: the bytes are compressed, none saturates
    for k, line in enumerate(lines):
        i = int(line.split()[0])
        img = eio.load_pgm(str(out1 / "views" / ("frame_%06d.pgm" % i)))
        eio.save_pgm(str(dist / ("frame_%06d.pgm" % i)), np.where(img != 0, np.clip(np.rint(img * a_star[k]), 1, 255), 0).astype(np.uint8))
    with open(dist / "times.txt", "w") as fh:
        fh.write("\n".join(lines) + "\n")
    r = subprocess.run(exe + ["--demo", str(out2), "--frames", str(dist), "--refine-frames", "2", "--frames-exposure", "gain-bias", "--init-map", "frames", "--frames-log", "0",
                              "--frames-lo", lo, "--frames-hi", hi, "--frames-skip-zero", "--max-iter", "3"], capture_output=True, text=True, timeout=600)
    print(r.stdout[-3000:])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "refine-frames round 2" in r.stdout and "frame mosaic:" in r.stdout
    rows = [l.split() for l in open(out2 / "frames_aligned.txt").read().splitlines() if l and not l.startswith("#")]
    assert len(rows) == len(lines) and all(len(x) == 10 for x in rows)
    gains = np.array([float(x[8]) for x in rows])
    assert np.isfinite(gains).all() and (gains > 0).all()
    print(f"std of a*_f: {a_star.std():.5f}; std of a_f a*_f: {(gains * a_star / np.mean(gains * a_star)).std():.5f} (normalised to mean 1: "
          f"{(a_star / a_star.mean()).std():.5f} before)")
    assert (gains * a_star).std() < a_star.std()
    assert (out2 / "refined_traj.txt").exists() and (out2 / "frame_mosaic.pgm").exists()
    # the flag without --refine-frames is refused with a message
    r = subprocess.run(exe + ["--demo", str(tmp_path / "out3"), "--frames", str(dist), "--frames-exposure", "bias"], capture_output=True, text=True, timeout=600)
    assert r.returncode != 0 and "--refine-frames" in r.stderr
