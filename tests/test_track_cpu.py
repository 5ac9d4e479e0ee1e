"""The numpy forms of the frame tracker (emba_amd.io: track_level_pm, track_votes, track_terms, track_predict, track_frames) on a CPU:
track_terms against a scalar python loop, the level votes against mosaic_votes of the scaled pm, the prediction, the numpy tracker on every case of
tests/track_cases.py with its recorded E_NP, the schedule (0,) against the coarse-to-fine schedule, and the symbols with ABI 2."""
import os

import numpy as np
import pytest

import track_cases as TC
from emba_amd import _lib
from emba_amd import io as eio
from emba_amd import so3

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def scalar_terms(frame, pm_l, J23_l, sum_w, sum_v, min_weight, skip_zero, huber_k):
    """track_pixel (track_rule.h) pixel by pixel in plain python."""
    H, W = sum_w.shape
    out = []
    for s in range(frame.size):
        x, y, v = float(pm_l[s, 0]), float(pm_l[s, 1]), int(frame[s])
        ix, iy = int(np.floor(x)), int(np.floor(y))
        if iy < 0 or iy + 1 > H - 1:
            out.append((eio.ALIGN_OUTSIDE, 0.0, 0.0, 0.0, (0.0, 0.0, 0.0)))
            continue
        ax, ay, c0 = x - np.floor(x), y - np.floor(y), ix % W
        c1 = 0 if c0 + 1 == W else c0 + 1
        cells = ((iy, c0), (iy, c1), (iy + 1, c0), (iy + 1, c1))
        if any(int(sum_w[c]) < min_weight for c in cells):
            out.append((eio.ALIGN_MASKED, 0.0, 0.0, 0.0, (0.0, 0.0, 0.0)))
            continue
        if skip_zero and v == 0:
            out.append((eio.ALIGN_SKIPPED, 0.0, 0.0, 0.0, (0.0, 0.0, 0.0)))
            continue
        p00, p01, p10, p11 = (float(sum_v[c]) / float(sum_w[c]) for c in cells)
        val = (1.0 - ay) * ((1.0 - ax) * p00 + ax * p01) + ay * ((1.0 - ax) * p10 + ax * p11)
        gx = (1.0 - ay) * (p01 - p00) + ay * (p11 - p10)
        gy = (1.0 - ax) * (p10 - p00) + ax * (p11 - p01)
        r = val - float(v)
        a = abs(r)
        w, rho = (1.0, r * r) if not huber_k > 0.0 or a <= huber_k else (huber_k / a, 2.0 * huber_k * a - huber_k * huber_k)
        out.append((eio.ALIGN_USED, r, w, rho, tuple(gx * J23_l[s, 0, j] + gy * J23_l[s, 1, j] for j in range(3))))
    return out


@pytest.mark.parametrize("sensor,pano", [((20, 13), (32, 16)), ((64, 48), (32, 16)), ((20, 13), (128, 64))])
def test_track_terms_against_a_scalar_loop(sensor, pano):
    c = TC.case(sensor, pano, "small")
    W, H = pano
    status = np.array([eio.TRACK_ANCHOR] + [eio.TRACK_TRACKED] * 5 + [eio.TRACK_LOST] * (TC.F - 6))
    pm = np.array([eio.align_warp(c["lut"], q, W, H)[1] for q in c["q_true"]])
    fr = c["frames"].copy()
    fr.reshape(-1)[::11] = 0      # bytes for skip_zero to skip inside the panorama
    votes = eio.track_votes(fr, pm, status, W, H, TC.SCHEDULE[pano], skip_zero=True)
    seen = set()
    q = so3.mul(so3.exp(np.array([0.01, 0.02, -0.01])), c["q_true"][6])
    _, pm6, J23 = eio.align_warp(c["lut"], q, W, H)
    for l in TC.SCHEDULE[pano]:
        Wl, Hl, scale = eio.track_level_shape(W, H, l)
        sw, sv = votes["planes"][l]
        assert sw.shape == (Hl, Wl)
        for mw in (256, 32):
            for skip_zero in (False, True):
                for hk in (0.0, 3.0):
                    t = eio.track_terms(fr[6], pm6 * scale, c["lut"], q, sw, sv, mw, skip_zero, hk)
                    ref = scalar_terms(fr[6], pm6 * scale, J23 * scale, sw, sv, mw, skip_zero, hk)
                    assert [x[0] for x in ref] == t["cls"].tolist()
                    assert np.array_equal(np.array([x[1] for x in ref]), t["r"])      # the same bits
                    assert np.array_equal(np.array([x[2] for x in ref]), t["w"]) and np.array_equal(np.array([x[3] for x in ref]), t["rho"])
                    g = np.array([x[4] for x in ref])
                    assert np.abs(g - t["g"]).max() <= 1e-9 * max(np.abs(g).max(), 1e-300)      # (J23 on the level's grid against J23 * 2^-l)
                    seen |= set(t["cls"].tolist())
    assert {eio.ALIGN_USED, eio.ALIGN_MASKED, eio.ALIGN_SKIPPED} <= seen


@pytest.mark.parametrize("pano", TC.PANOS, ids=lambda p: f"pano{p[1]}x{p[0]}")
def test_level_votes_are_mosaic_votes_of_the_scaled_pm(pano):
    sensor = (20, 13)
    c = TC.case(sensor, pano, "large")
    W, H = pano
    pm = np.array([eio.align_warp(c["lut"], q, W, H)[1] for q in c["q_true"]])
    status = np.full(TC.F, eio.TRACK_TRACKED)
    status[0], status[4], status[7] = eio.TRACK_ANCHOR, eio.TRACK_LOST, eio.TRACK_LOST
    keep = status != eio.TRACK_LOST
    for levels in (TC.SCHEDULE[pano], TC.SCHEDULE[pano][:-1], (1, 1)):
        v = eio.track_votes(c["frames"], pm, status, W, H, levels, skip_zero=True)
        assert sorted(v["planes"]) == sorted(set(levels) | {0})      # level 0 is always voted
        dropped = 0
        for l, (sw, sv) in v["planes"].items():
            Wl, Hl, scale = eio.track_level_shape(W, H, l)
            assert np.array_equal(eio.track_level_pm(pm, l), pm * scale)
            rw, rv, d, skipped = eio.mosaic_votes(c["frames"][keep], (pm[keep] * scale).reshape(-1, 2), Wl, Hl, True)
            assert np.array_equal(sw, rw) and np.array_equal(sv, rv) and skipped == v["skipped"]
            whole = 256 * (int(keep.sum()) * sensor[0] * sensor[1] - skipped)      # every pixel votes 256 units, what is dropped aside
            assert int(sw.sum()) == whole if d == 0 else whole - 256 * d < int(sw.sum()) < whole
            dropped += d
        assert dropped == v["dropped"]
    assert eio.track_level_shape(32, 16, 3) == (4, 2, 0.125)
    for bad in (4, 5, 8, -1):      # one row left; 16 not divisible by 32; out of range
        with pytest.raises(ValueError):
            eio.track_level_shape(32, 16, bad)


def test_track_predict():
    axis = np.array([0.6, 0.0, 0.8])
    qa, qb = so3.exp(0.1 * axis), so3.exp(0.3 * axis)
    assert np.array_equal(eio.track_predict(None, None, qb, 20, 30), qb) and np.array_equal(eio.track_predict(qa, 10, qb, 20, 30, predict=False), qb)
    for t, want in ((30, 0.5), (25, 0.4), (50, 0.9)):      # equal gaps, half a gap, a lost frame or two in between
        assert eio.rotation_angle_between(eio.track_predict(qa, 10, qb, 20, t), so3.exp(want * axis))[0] < 1e-12
    assert eio.rotation_angle_between(eio.track_predict(qa, 10, -qb, 20, 30), so3.exp(0.5 * axis))[0] < 1e-12


@pytest.mark.parametrize("key", list(TC.TRACKING), ids=lambda k: f"{k[0][0]}x{k[0][1]}-on-{k[1][0]}x{k[1][1]}-{k[2]}")
def test_the_numpy_tracker_on_the_cases(key):
    """Every frame tracked, the overlap above MIN_OVERLAP, the worst angle to the truth within the recorded E_NP; and (0,) against the schedule."""
    r = TC.track_numpy(*key)
    e = TC.worst_angle(*key, r["q"])
    print(f"{key}: numpy's worst angle to the truth {e:.4e} rad (E_NP {TC.E_NP[key]:.4e}), overlap >= {r['overlap'][1:].min():.3f}, iters {r['iters'].sum(axis=0).tolist()}")
    assert r["status"].tolist() == [eio.TRACK_ANCHOR] + [eio.TRACK_TRACKED] * (TC.F - 1)
    assert (r["overlap"][1:] >= TC.MIN_OVERLAP).all() and not np.isnan(r["pm"]).any()
    assert e <= TC.E_NP[key] * (1.0 + 1e-3)
    sw, sv = r["planes"][0]
    v = eio.track_votes(TC.case(*key)["frames"], r["pm"], r["status"], key[1][0], key[1][1], TC.SCHEDULE[key[1]], skip_zero=True)
    for l in r["planes"]:
        assert np.array_equal(r["planes"][l][0], v["planes"][l][0]) and np.array_equal(r["planes"][l][1], v["planes"][l][1])
    assert tuple(r["iters"].sum(axis=0).tolist()) == TC.ITERS_NP[key]
    assert (np.diff(TC.ITERS_NP[key]) < 0).all()      # every level starts where the coarser one ended: fewer trials from level to level
    back = TC.track_numpy(*key, levels=TC.SCHEDULE[key[1]][::-1])["iters"].sum(axis=0)[::-1]      # the reversed schedule, per level
    print(f"{key}: trials per level {TC.ITERS_NP[key]}, under the reversed schedule {back.tolist()}")
    assert np.abs(back - np.array(TC.ITERS_NP[key])).max() > TC.ITERS_SLACK      # ... so the trials tell the schedules apart
    if key[2] == "large":
        e0 = TC.worst_angle(*key, TC.track_numpy(*key, levels=(0,))["q"])
        print(f"{key}: the schedule (0,) alone ends at {e0:.4e} rad")
        assert (e0 > 2.0 * TC.E_NP[key] + TC.F * TC.SETTINGS["tol_rot"]) == (key in TC.COARSE_BEATS_FINE)


def test_a_black_frame_is_lost_in_numpy():
    key = ((64, 48), (128, 64), "small")
    c = TC.case(*key)
    fr = c["frames"].copy()
    fr[5] = 0
    r = eio.track_frames(fr, c["ts"], c["lut"], 128, 64, q0=TC.Q_START, levels=(1, 0), skip_zero=True, min_overlap=TC.MIN_OVERLAP, **TC.SETTINGS)
    assert r["status"][5] == eio.TRACK_LOST and (np.delete(r["status"], 5)[1:] == eio.TRACK_TRACKED).all() and np.isnan(r["pm"][5]).all()
    assert np.array_equal(r["q"][5], eio.track_predict(r["q"][3], c["ts"][3], r["q"][4], c["ts"][4], c["ts"][5]))      # q_out of a lost frame is its prediction


def test_the_abi_still_reports_2_and_has_the_three_symbols(hip_lib):
    header = open(os.path.join(ROOT, "include", "emba_hip.h")).read()
    for name in ("emba_frames_track", "emba_track_eval", "emba_track_level_get"):
        assert name in _lib.SIGNATURES and f"emba_status {name}(" in header and hasattr(hip_lib, name)
    assert "#define EMBA_ABI_VERSION 2" in header and hip_lib.emba_abi_version() == 2
    blob = open(os.path.join(ROOT, "emba_amd", "libemba_hip.so"), "rb").read()
    for kernel in (b"emba_frames_track_eval_kernel", b"emba_frames_track_vote_kernel", b"emba_frames_track_frame_kernel"):
        assert kernel in blob, kernel
    assert [eio.TRACK_ANCHOR, eio.TRACK_TRACKED, eio.TRACK_LOST] == [int(header.split(f"#define EMBA_TRACK_{n} ")[1].split()[0]) for n in ("ANCHOR", "TRACKED", "LOST")]
    assert len(_lib.EmbaTrackSettings._fields_) == 8 and _lib.EmbaTrackSettings.align.offset % 8 == 0
