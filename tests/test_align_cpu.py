"""The numpy forms of the frame alignment (emba_amd.io: align_sample, align_terms, align_sums, align_step, align_frames) without a GPU:
align_terms against a scalar python loop, the analytic row g against a central finite difference of the sample in delta, the loop recovering perturbed
rotations on every convergence case of tests/align_cases.py with the final angles recorded there, and the C ABI's two new entry points."""
import math
import os

import numpy as np
import pytest

import align_cases as AC
from emba_amd import _lib
from emba_amd import io as eio
from emba_amd import so3

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def scalar_terms(frame, pm, J23, P, valid, lo, hi, skip_zero, k):
    """align_pixel (align_rule.h) pixel by pixel in python floats."""
    H, W = P.shape
    out = []
    for s in range(frame.size):
        x, y, v = float(pm[s, 0]), float(pm[s, 1]), int(frame[s])
        if not (abs(x) < 2147483648.0 and abs(y) < 2147483648.0):
            out.append((eio.ALIGN_OUTSIDE, 0.0, 0.0, 0.0, (0.0, 0.0, 0.0)))
            continue
        ix, iy = math.floor(x), math.floor(y)
        if iy < 0 or iy + 1 > H - 1:
            out.append((eio.ALIGN_OUTSIDE, 0.0, 0.0, 0.0, (0.0, 0.0, 0.0)))
            continue
        ax, ay = x - ix, y - iy
        c0 = ix % W
        c1 = 0 if c0 + 1 == W else c0 + 1
        if valid is not None and not (valid[iy, c0] and valid[iy, c1] and valid[iy + 1, c0] and valid[iy + 1, c1]):
            out.append((eio.ALIGN_MASKED, 0.0, 0.0, 0.0, (0.0, 0.0, 0.0)))
            continue
        if skip_zero and v == 0:
            out.append((eio.ALIGN_SKIPPED, 0.0, 0.0, 0.0, (0.0, 0.0, 0.0)))
            continue
        p00, p01, p10, p11 = float(P[iy, c0]), float(P[iy, c1]), float(P[iy + 1, c0]), float(P[iy + 1, c1])
        val = (1.0 - ay) * ((1.0 - ax) * p00 + ax * p01) + ay * ((1.0 - ax) * p10 + ax * p11)
        gx = (1.0 - ay) * (p01 - p00) + ay * (p11 - p10)
        gy = (1.0 - ax) * (p10 - p00) + ax * (p11 - p01)
        r = val - (lo + v * (hi - lo) / 255.0)
        if k > 0.0 and abs(r) > k:
            w, rho = k / abs(r), 2.0 * k * abs(r) - k * k
        else:
            w, rho = 1.0, r * r
        out.append((eio.ALIGN_USED, r, w, rho, tuple(gx * float(J23[s, 0, j]) + gy * float(J23[s, 1, j]) for j in range(3))))
    return out


@pytest.mark.parametrize("sensor,pano,kind", [((7, 5), (32, 16), "pitch"), ((20, 13), (48, 24), "yaw_pi"), ((20, 13), (32, 16), "pitch")])
def test_align_terms_against_a_scalar_loop(sensor, pano, kind):
    c = AC.case(sensor, pano, kind, 3)
    H, W = c["I"].shape
    k = AC.huber_split(c)
    seen = set()
    for f in range(3):
        q = c["q_start"][f]
        _, pm, J23 = eio.align_warp(c["lut"], q, W, H)
        for valid in (None, c["valid"]):
            for skip_zero in (False, True):
                for hk in (0.0, k):
                    t = eio.align_terms(c["frames"][f], pm, c["lut"], q, c["I"], valid, c["lo"], c["hi"], skip_zero, hk)
                    ref = scalar_terms(c["frames"][f], pm, J23, c["I"], valid, c["lo"], c["hi"], skip_zero, hk)
                    assert t["cls"].tolist() == [r[0] for r in ref]
                    assert t["r"].tolist() == [r[1] for r in ref] and t["w"].tolist() == [r[2] for r in ref] and t["rho"].tolist() == [r[3] for r in ref]
                    assert np.array_equal(t["g"], np.array([r[4] for r in ref]))
                    sums, counts, scale = eio.align_sums(t, with_scale=True)
                    assert counts.sum() == c["frames"][f].size and counts.tolist() == [sum(r[0] == cl for r in ref) for cl in range(4)]
                    want = [math.fsum(r[2] * r[4][a] * r[4][b] for r in ref) for a, b in ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))]
                    want += [math.fsum(r[2] * r[4][a] * r[1] for r in ref) for a in range(3)] + [math.fsum(r[3] for r in ref)]
                    assert np.all(np.abs(sums - np.array(want)) <= 1e-14 * scale + 1e-300)
                    seen |= set(t["cls"].tolist())
                    if hk > 0:
                        used = t["cls"] == eio.ALIGN_USED
                        assert (t["w"][used] < 1.0).any() and (t["w"][used] == 1.0).any()      # the k splits the residuals
    assert seen >= {eio.ALIGN_USED, eio.ALIGN_MASKED} and (kind != "pitch" or eio.ALIGN_OUTSIDE in seen)


@pytest.mark.parametrize("kind", AC.KINDS)
def test_the_row_g_is_the_derivative_of_the_sample(kind):
    """g = gx J23[0,:] + gy J23[1,:] against (val(exp(h e_k) q) - val(exp(-h e_k) q)) / 2h over the pixels whose cell the step does not leave: the sample is
    bilinear inside a cell, so what is left is the projection's curvature, O(h^2), and rounding, O(eps / h)."""
    sensor, pano = (20, 13), (128, 64)
    c = AC.case(sensor, pano, kind, 3)
    H, W = c["I"].shape
    h, checked = 1e-6, 0
    for f in range(3):
        q = c["q_start"][f]
        _, pm, _ = eio.align_warp(c["lut"], q, W, H)
        t = eio.align_terms(c["frames"][f], pm, c["lut"], q, c["I"], None, c["lo"], c["hi"])
        for k in range(3):
            d = np.zeros(3)
            d[k] = h
            pp = eio.align_warp(c["lut"], so3.mul(so3.exp(d), q), W, H)[1]
            pn = eio.align_warp(c["lut"], so3.mul(so3.exp(-d), q), W, H)[1]
            same = (np.floor(pp) == np.floor(pm)).all(axis=1) & (np.floor(pn) == np.floor(pm)).all(axis=1) & (t["cls"] == eio.ALIGN_USED)
            fd = (eio.align_sample(c["I"], pp)[0] - eio.align_sample(c["I"], pn)[0]) / (2.0 * h)
            assert same.sum() > 100
            assert np.abs(fd - t["g"][:, k])[same].max() <= 1e-7 * max(1.0, np.abs(t["g"]).max())
            checked += int(same.sum())
    assert checked > 1000


def test_align_step_solves_and_refuses():
    rng = np.random.default_rng(11)
    A = rng.standard_normal((5, 3))
    Hm = A.T @ A
    x = np.array([0.3, -0.2, 0.1])
    for lam in (0.0, 1e-3, 2.0):
        b = -(Hm + lam * np.diag(np.diag(Hm))) @ x
        assert np.abs(eio.align_step(Hm, b, lam) - x).max() < 1e-12
        assert np.array_equal(eio.align_step(Hm, b, lam), eio.align_step(Hm[np.triu_indices(3)], b, lam))
    v = np.array([1.0, 2.0, 3.0])
    assert eio.align_step(np.outer(v, v), v, 0.0) is None and eio.align_step(np.outer(v, v), v, 1e-3) is not None
    assert eio.align_step(np.zeros((3, 3)), v, 1.0) is None and eio.align_step(np.full((3, 3), np.nan), v, 1.0) is None
    with pytest.raises(ValueError):
        eio.align_settings(min_pixels=2)
    with pytest.raises(ValueError):
        eio.align_settings(lambda_up=1.0)
    with pytest.raises(ValueError):
        eio.align_settings(step=3)


@pytest.mark.parametrize("pano", AC.PANOS, ids=lambda p: f"pano{p[1]}x{p[0]}")
@pytest.mark.parametrize("sensor", AC.SENSORS, ids=lambda s: f"sensor{s[0]}x{s[1]}")
def test_the_numpy_loop_recovers_the_perturbed_rotations(sensor, pano):
    """From AC.PERTURB rad off, every frame of every kind ends converged or stalled, its mean cost lower than at the start, and its angle to the truth
    within the pair's recorded E_NP — the figure the device is measured against (tests/test_gpu_align.py)."""
    worst = 0.0
    for kind in AC.KINDS:
        c = AC.case(sensor, pano, kind, AC.CONVERGENCE_F)
        start = eio.rotation_angle_between(c["q_true"], c["q_start"])
        assert np.abs(start - AC.PERTURB).max() < 1e-9
        r = eio.align_frames(c["frames"], c["q_start"], c["lut"], c["I"], None, c["lo"], c["hi"], skip_zero=True, **AC.SETTINGS)
        assert set(r["status"].tolist()) <= {eio.ALIGN_CONVERGED, eio.ALIGN_STALLED}, (kind, r["status"])
        assert (r["counts"][:, 0] >= AC.SETTINGS["min_pixels"]).all()
        assert (r["sums"][:, 9] / r["counts"][:, 0] <= r["cost0"] / r["n0"]).all()
        worst = max(worst, float(eio.rotation_angle_between(c["q_true"], r["q"]).max()))
    print(f"{sensor} on {pano}: numpy's worst final angle {worst:.4e} rad (E_NP {AC.E_NP[(sensor, pano)]:.4e})")
    assert worst <= AC.E_NP[(sensor, pano)] * (1 + 1e-3) and worst < AC.PERTURB / 10


def test_the_numpy_loop_through_the_mosaic():
    import mosaic_cases as MC
    sensor, pano = AC.MOSAIC_PAIR
    W, H = pano
    worst = 0.0
    for kind in AC.KINDS:
        c, m = AC.case(sensor, pano, kind, AC.CONVERGENCE_F), MC.case(sensor, pano, kind, AC.CONVERGENCE_F)
        sw, sv, _, _ = eio.mosaic_votes(c["frames"], m["pm"], W, H, True)
        mean, cov = eio.mosaic_mean(sw, sv, 256, 0.0)
        r = eio.align_frames(c["frames"], c["q_start"], c["lut"], mean, cov, 0.0, 255.0, skip_zero=True, **AC.SETTINGS)
        assert set(r["status"].tolist()) <= {eio.ALIGN_CONVERGED, eio.ALIGN_STALLED}
        worst = max(worst, float(eio.rotation_angle_between(c["q_true"], r["q"]).max()))
    print(f"through the mosaic: numpy's worst final angle {worst:.4e} rad")
    assert worst <= AC.E_NP_MOSAIC * (1 + 1e-3) and worst < AC.PERTURB / 5


def test_statuses_in_numpy():
    c = AC.case((20, 13), (48, 24), "yaw_pi", 3)
    r = eio.align_frames(c["frames"], c["q_start"], c["lut"], c["I"], np.zeros(c["I"].shape, bool), c["lo"], c["hi"], **AC.SETTINGS)
    assert (r["status"] == eio.ALIGN_DEGENERATE).all() and np.array_equal(r["q"], c["q_start"]) and (r["counts"][:, 0] == 0).all() and (r["iters"] == 0).all()
    r = eio.align_frames(c["frames"], c["q_start"], c["lut"], c["I"], None, c["lo"], c["hi"], **dict(AC.SETTINGS, max_iters=2))
    assert (r["status"] == eio.ALIGN_ITERATIONS).all() and (r["iters"] == 2).all()
    r = eio.align_frames(c["frames"], c["q_start"], c["lut"], c["I"], None, c["lo"], c["hi"], **dict(AC.SETTINGS, max_iters=0))
    assert (r["status"] == eio.ALIGN_ITERATIONS).all() and np.array_equal(r["q"], c["q_start"]) and np.array_equal(r["cost0"], r["sums"][:, 9])


def test_the_abi_still_reports_2_and_has_the_two_symbols(hip_lib):
    header = open(os.path.join(ROOT, "include", "emba_hip.h")).read()
    for name in ("emba_frames_align_eval", "emba_frames_align"):
        assert name in _lib.SIGNATURES and f"emba_status {name}(" in header
    assert "#define EMBA_ABI_VERSION 2" in header and hip_lib.emba_abi_version() == 2
    assert hasattr(hip_lib, "emba_frames_align_eval") and hasattr(hip_lib, "emba_frames_align")
    blob = open(os.path.join(ROOT, "emba_amd", "libemba_hip.so"), "rb").read()
    for kernel in (b"emba_frames_align_eval_kernel", b"emba_frames_align_reduce_kernel", b"emba_frames_align_step_kernel"):
        assert kernel in blob, kernel
    assert [eio.ALIGN_CONVERGED, eio.ALIGN_STALLED, eio.ALIGN_ITERATIONS, eio.ALIGN_DEGENERATE] == [
        int(header.split(f"#define EMBA_ALIGN_{n} ")[1].split()[0]) for n in ("CONVERGED", "STALLED", "ITERATIONS", "DEGENERATE")]
    assert len(_lib.EmbaAlignSettings._fields_) == 9
