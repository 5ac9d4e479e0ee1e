"""The numpy forms of the frame tracker with exposure (emba_amd.io: track_exposure_terms, track_votes_exposure, track_frames_exposure) on a CPU:
against a scalar loop that follows include/emba_hip.h's words on 7 x 5 / 32 x 16, estimate = 0 against io.track_frames in every output, the condition on the
bytes of tests/track_exposure_cases.py, the recorded recovery figures, and plain tracking on the same distorted frames ending worse by the recorded figures."""
import math
import struct

import numpy as np
import pytest

import track_cases as TC
import track_exposure_cases as XC
import view_cases as VC
from emba_amd import io as eio
from emba_amd import so3

SENSOR, PANO = (7, 5), (32, 16)


def bits(x):
    return struct.pack("<d", float(x))


def small_scene():
    """Three frames of 7 x 5 on 32 x 16 near the equator, two of them voted (the third lost), with non-trivial exposures, and the level sums they leave."""
    rng = np.random.default_rng(11)
    lut = VC.lut_of(SENSOR)
    S = SENSOR[0] * SENSOR[1]
    q = np.array([so3.exp(np.array([0.02 * f, 0.15 * f - 0.1, 0.01])) for f in range(3)])
    frames = rng.integers(1, 256, size=(3, S)).astype(np.uint8)
    frames[:, ::6] = 0
    pm = np.array([eio.align_warp(lut, q[f], *PANO)[1] for f in range(3)])
    status = np.array([eio.TRACK_ANCHOR, eio.TRACK_LOST, eio.TRACK_TRACKED])
    gain, bias = np.array([1.0, 3.0, 1.2]), np.array([0.0, 50.0, -7.5])
    return lut, q, frames, pm, status, gain, bias


def test_votes_against_a_scalar_loop():
    lut, q, frames, pm, status, gain, bias = small_scene()
    W, H = PANO
    levels = (2, 1)      # level 0 is voted although the schedule does not name it
    for skip_zero in (False, True):
        got = eio.track_votes_exposure(frames, pm, status, gain, bias, W, H, levels, skip_zero)
        assert sorted(got["planes"]) == [0, 1, 2]
        dropped = skipped = 0
        for l in (2, 1, 0):
            Wl, Hl = W >> l, H >> l
            sw, sv = np.zeros((Hl, Wl), np.uint64), np.zeros((Hl, Wl), np.uint64)
            for f in (0, 2):      # the lost frame casts no vote
                for s in range(frames.shape[1]):
                    raw = int(frames[f, s])
                    if skip_zero and raw == 0:
                        skipped += l == 0
                        continue
                    v = min(max(int(np.rint(gain[f] * raw + bias[f])), 0), 255)
                    x, y = pm[f, s, 0] / (1 << l), pm[f, s, 1] / (1 << l)
                    ix, iy = math.floor(x), math.floor(y)
                    wx, wy = int((x - ix) * 16.0), int((y - iy) * 16.0)
                    for dx, dy, w in ((0, 0, (16 - wx) * (16 - wy)), (1, 0, wx * (16 - wy)), (0, 1, (16 - wx) * wy), (1, 1, wx * wy)):
                        if not w:
                            continue
                        if not 0 <= iy + dy < Hl:
                            dropped += 1
                            continue
                        sw[iy + dy, (ix + dx) % Wl] += np.uint64(w)
                        sv[iy + dy, (ix + dx) % Wl] += np.uint64(w * v)
            assert np.array_equal(got["planes"][l][0], sw) and np.array_equal(got["planes"][l][1], sv), (l, skip_zero)
        assert got["dropped"] == dropped and got["skipped"] == skipped
    # unit exposures: track_votes itself
    one = eio.track_votes_exposure(frames, pm, status, np.ones(3), np.zeros(3), W, H, levels, True)
    ref = eio.track_votes(frames, pm, status, W, H, levels, True)
    assert one["dropped"] == ref["dropped"] and one["skipped"] == ref["skipped"]
    assert all(np.array_equal(one["planes"][l][k], ref["planes"][l][k]) for l in (0, 1, 2) for k in (0, 1))


def test_terms_against_a_scalar_loop():
    lut, q, frames, pm, status, gain, bias = small_scene()
    W, H = PANO
    planes = eio.track_votes_exposure(frames, pm, status, gain, bias, W, H, (1,), True)["planes"]
    frame = frames[1]
    seen = set()
    # near where the frames voted, and pitched towards either pole, where the cell leaves the plane
    for qe in (so3.mul(so3.exp(np.array([0.01, -0.03, 0.02])), q[1]), so3.mul(so3.exp(np.array([1.45, 0.0, 0.0])), q[1]),
               so3.mul(so3.exp(np.array([-1.45, 0.0, 0.0])), q[1])):
        for l, min_weight in ((0, 64), (1, 256)):
            sw, sv = planes[l]
            Hl, Wl = sw.shape
            pm_l = eio.track_level_pm(eio.align_warp(lut, qe, W, H)[1], l)
            J23 = eio.align_warp(lut, qe, Wl, Hl)[2]
            for skip_zero in (False, True):
                for huber_k in (0.0, 6.0):
                    a, b = 1.3, -11.25
                    t = eio.track_exposure_terms(frame, pm_l, lut, qe, sw, sv, a, b, min_weight, skip_zero, huber_k)
                    for s in range(frame.size):
                        x, y = pm_l[s]
                        ix, iy = math.floor(x), math.floor(y)
                        v = int(frame[s])
                        if not (iy >= 0 and iy + 1 <= Hl - 1):
                            cls = eio.ALIGN_OUTSIDE
                        else:
                            c0 = ix % Wl
                            c1 = 0 if c0 + 1 == Wl else c0 + 1
                            cells = ((iy, c0), (iy, c1), (iy + 1, c0), (iy + 1, c1))
                            if any(int(sw[c]) < min_weight for c in cells):
                                cls = eio.ALIGN_MASKED
                            elif skip_zero and v == 0:
                                cls = eio.ALIGN_SKIPPED
                            else:
                                cls = eio.ALIGN_USED
                        seen.add(cls)
                        assert t["cls"][s] == cls, (l, s)
                        if cls != eio.ALIGN_USED:
                            assert t["r"][s] == 0.0 and t["w"][s] == 0.0 and t["I0"][s] == 0.0
                            continue
                        p00, p01, p10, p11 = (float(sv[c]) / float(sw[c]) for c in cells)
                        ax, ay = x - ix, y - iy
                        val = (1.0 - ay) * ((1.0 - ax) * p00 + ax * p01) + ay * ((1.0 - ax) * p10 + ax * p11)
                        gx = (1.0 - ay) * (p01 - p00) + ay * (p11 - p10)
                        gy = (1.0 - ax) * (p10 - p00) + ax * (p11 - p01)
                        scaled = a * float(v)
                        r = val - (scaled + b)
                        assert bits(t["r"][s]) == bits(r) and t["I0"][s] == float(v), (l, s)
                        w = 1.0 if not huber_k > 0.0 or abs(r) <= huber_k else huber_k / abs(r)
                        assert bits(t["w"][s]) == bits(w)
                        g = gx * J23[s, 0] + gy * J23[s, 1]
                        assert np.array_equal(t["g"][s], g)
                    # a = 1, b = 0: track_terms' members, bit for bit
                    one = eio.track_exposure_terms(frame, pm_l, lut, qe, sw, sv, 1.0, 0.0, min_weight, skip_zero, huber_k)
                    ref = eio.track_terms(frame, pm_l, lut, qe, sw, sv, min_weight, skip_zero, huber_k)
                    assert all(np.array_equal(one[k], ref[k]) for k in ("cls", "r", "w", "rho", "g"))
    assert seen == {eio.ALIGN_USED, eio.ALIGN_OUTSIDE, eio.ALIGN_MASKED, eio.ALIGN_SKIPPED}


def test_estimate_zero_is_the_plain_tracker():
    key = ((20, 13), (128, 64), "large")
    c = XC.case(*key)
    for batch in (1, 3):
        args = XC.track_args(*key, batch=batch)
        e = eio.track_frames_exposure(c["distorted"], c["ts"], c["lut"], 128, 64, estimate=0, **XC.BOUNDS, **args)
        p = eio.track_frames(c["distorted"], c["ts"], c["lut"], 128, 64, **args)
        for k in ("q", "status", "iters", "cost", "overlap", "counts"):
            assert np.array_equal(e[k], p[k]), (batch, k)
        assert np.array_equal(e["pm"], p["pm"], equal_nan=True)
        assert (e["gain"] == 1.0).all() and (e["bias"] == 0.0).all()
        assert all(np.array_equal(e["planes"][l][i], p["planes"][l][i]) for l in p["planes"] for i in (0, 1))


def test_the_distortion_keeps_every_used_byte_inside():
    """No used byte of a distorted frame reaches 0 or 255, and a* v' + b* gives the rendered byte back within half a step of the distorted byte."""
    assert (XC.A_STAR[1:] > 1.0).all() and XC.A_STAR[0] == 1.0 and XC.B_STAR[0] == 0.0
    assert (XC.B_STAR[1:] <= 1.0 - XC.A_STAR[1:]).all() and (XC.B_STAR[1:] >= 255.0 - 254.0 * XC.A_STAR[1:]).all()
    for key in XC.CASES:
        c = XC.case(*key)
        assert np.array_equal(c["distorted"][0], c["frames"][0])      # the anchor is left as it is
        for f in range(1, XC.F):
            raw, d = c["frames"][f], c["distorted"][f]
            assert np.array_equal(d == 0, raw == 0)
            used = d[raw != 0].astype(np.float64)
            assert used.min() >= 1 and used.max() <= 254, (key, f)
            assert np.abs(XC.A_STAR[f] * used + XC.B_STAR[f] - raw[raw != 0]).max() <= 0.5 * XC.A_STAR[f] + 1e-9


@pytest.mark.parametrize("key", XC.CASES, ids=lambda k: f"{k[0][0]}x{k[0][1]}-{k[2]}")
def test_recovery_figures(key):
    """numpy alone tracks every frame with no level ending degenerate, reproduces the recorded figures, and plain tracking on the same frames ends worse by the
    recorded figure: beyond the bound the device's exposure tracker is held to."""
    c, r = XC.case(*key), XC.track_numpy(*key)
    assert key in XC.RECOVERY
    assert r["status"].tolist() == [eio.TRACK_ANCHOR] + [eio.TRACK_TRACKED] * (XC.F - 1) and r["levels_degenerate"] == []
    assert r["gain"][0] == 1.0 and r["bias"][0] == 0.0
    e, da, db = XC.worst_angle(*key, r["q"]), np.abs(r["gain"] - c["gain"]).max(), np.abs(r["bias"] - c["bias"]).max()
    print(key, f"E {e:.4e} DA {da:.4e} DB {db:.4e} iters {r['iters'].sum(axis=0).tolist()}")
    assert e == pytest.approx(XC.E_NP[key], rel=1e-3) and da == pytest.approx(XC.DA_NP[key], rel=1e-3) and db == pytest.approx(XC.DB_NP[key], rel=1e-3)
    assert tuple(int(x) for x in r["iters"].sum(axis=0)) == XC.ITERS_NP[key]
    p = XC.track_numpy_plain(*key)
    ep = XC.worst_angle(*key, p["q"])
    print(key, f"plain E {ep:.4e}")
    assert ep == pytest.approx(XC.E_PLAIN[key], rel=1e-3)
    assert ep > XC.angle_bound(key) and ep > 5.0 * e
    # the compensated mosaic is what the next frame is aligned to: the recovered exposures follow the ramp
    assert (np.diff(r["gain"]) > 0.0).all() and (np.diff(r["bias"]) < 0.0).all()
