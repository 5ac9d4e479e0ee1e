"""The numpy forms of the coarse-to-fine pair alignment (emba_amd.io.pair_level_* / pair_exposure_* / pair_align_levels) on a CPU: the rules of
a level, the two identities against io.pair_align and io.pair_terms, the exposure's Jacobian against differences, and the figures tests/pair_level_cases.py
records for the basin and for the exposure."""
import numpy as np
import pytest

import pair_cases as PC
import pair_level_cases as LC
from emba_amd import io as eio
from emba_amd import so3


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def test_the_rules_of_a_level():
    assert eio.pair_level_size((64, 48), 3) == (8, 6) and eio.pair_level_size((20, 13), 1) == (10, 6) and eio.pair_level_size((20, 13), 2) == (5, 3)
    assert eio.pair_level_size((8, 8), 2) == (2, 2)
    for sensor, level in (((20, 13), 3), ((8, 8), 3), ((64, 48), 8), ((64, 48), -1)):
        with pytest.raises(ValueError):
            eio.pair_level_size(sensor, level)
    assert eio.pair_check_levels([2, 0, 1, 1], (64, 48)) == (2, 0, 1, 1)
    for lv in ((), (0,) * 9, (0, 8), (0, 5)):
        with pytest.raises(ValueError):
            eio.pair_check_levels(lv, (64, 48))
    # bytes: the rounding tie goes up; a zero in the box; the left-over row and columns take no part
    fr = np.array([[1, 2, 1, 1, 9], [2, 1, 2, 1, 9], [0, 200, 255, 255, 9], [200, 200, 255, 255, 9], [7, 7, 7, 7, 9]], np.uint8)
    assert eio.pair_level_bytes(fr, 1).tolist() == [[2, 1], [150, 255]] and eio.pair_level_bytes(fr, 1, skip_zero=True).tolist() == [[2, 1], [0, 255]]
    assert np.array_equal(eio.pair_level_bytes(fr, 0), fr)
    rng = np.random.default_rng(5)
    big = rng.integers(0, 256, (3, 13, 20)).astype(np.uint8)
    big[big % 7 == 0] = 0
    for skip in (False, True):
        got = eio.pair_level_bytes(big, 2, skip)
        assert got.shape == (3, 3, 5)
        for f in range(3):
            for Y in range(3):
                for X in range(5):
                    box = big[f, 4 * Y:4 * Y + 4, 4 * X:4 * X + 4].astype(np.int64)
                    assert got[f, Y, X] == (0 if skip and (box == 0).any() else (box.sum() + 8) // 16)
        assert not skip or ((got > 0) == ~(big[:, :12, :20].reshape(3, 3, 4, 5, 4) == 0).any(axis=(2, 4))).all()
    # camera: level 0 bit for bit; a point's u_l
    cal = eio.pair_calib(33.3, 31.7, 30.9, 23.1, PC.LENS_D)
    c0 = eio.pair_level_calib(cal, 0)
    assert all(np.array_equal(bits(c0[k]), bits(cal[k])) for k in ("fu", "fv", "cu", "cv")) and c0["D"] is cal["D"]
    lut = PC.lens_lut()
    for l in (1, 2, 3):
        uv, uvl = eio.pair_project(lut, [0.01, -0.02, 0.03, 1.0], cal)[1], eio.pair_project(lut, [0.01, -0.02, 0.03, 1.0], eio.pair_level_calib(cal, l))[1]
        assert np.abs(uvl - (uv - ((1 << l) - 1) / 2.0) / (1 << l)).max() < 1e-12
    # table: behind the pinhole the analytic centre; level 0 the table itself
    plut = PC.case(False)["lut"]
    assert np.array_equal(bits(eio.pair_level_lut(plut, PC.SENSOR, 0)), bits(plut))
    for l in (1, 3):
        wl, hl = eio.pair_level_size(PC.SENSOR, l)
        X, Y = np.meshgrid(np.arange(wl), np.arange(hl))
        n, half = float(1 << l), ((1 << l) - 1) / 2.0
        want = np.stack([(X * n + half - PC.PINHOLE["cu"]) / PC.PINHOLE["fu"], (Y * n + half - PC.PINHOLE["cv"]) / PC.PINHOLE["fv"], np.ones_like(X, float)], axis=-1)
        assert np.abs(eio.pair_level_lut(plut, PC.SENSOR, l) - want.reshape(-1, 3)).max() < 1e-15
    assert [eio.pair_level_min_pixels(16, l) for l in (0, 1, 2)] == [16, 8, 8] and eio.pair_level_min_pixels(1000, 2) == 62 and eio.pair_level_min_pixels(5, 3) == 5


def test_the_two_identities():
    """The schedule (0) with estimate = 0 is io.pair_align; the terms at level 0 are io.pair_terms' and the ten shared sums io.pair_sums'."""
    c = PC.case(True)
    pairs = list(PC.ALIGN_PAIRS)
    Q0 = np.array([PC.start_off(PC.true_pair(c, *p), PC.START_CELLS * PC.CELL) for p in pairs])
    a = eio.pair_align(c["frames"], pairs, Q0, c["lut"], c["calib"], PC.SENSOR, gain=[0.9, 1.1], bias=[3.0, -4.0], skip_zero=True, **dict(PC.SETTINGS, huber_k=9.0))
    b = eio.pair_align_levels(c["frames"], pairs, Q0, c["lut"], c["calib"], PC.SENSOR, levels=(0,), estimate=0, gain=[0.9, 1.1], bias=[3.0, -4.0], skip_zero=True,
                              **dict(PC.SETTINGS, huber_k=9.0))
    for k in ("q", "cost0", "info"):
        assert np.array_equal(bits(a[k]), bits(b[k])), k
    for k in ("counts", "status", "iters", "n0"):
        assert np.array_equal(a[k], b[k]), k
    assert np.array_equal(bits(a["sums"]), bits(b["sums"][:, list(eio.EXPOSURE_SHARED)])) and (a["iters"] > 0).all()
    fr = c["frames"].reshape(PC.F, PC.SH, PC.SW)
    fb, tl, cl = eio.pair_level_bytes(fr, 0, True), eio.pair_level_lut(c["lut"], PC.SENSOR, 0), eio.pair_level_calib(c["calib"], 0)
    uv = eio.pair_project(c["lut"], Q0[0], c["calib"])[1]
    assert np.array_equal(bits(eio.pair_project(tl, Q0[0], cl)[1]), bits(uv))
    t10 = eio.pair_terms(fr[3].reshape(-1), fr[10], uv, c["lut"], Q0[0], c["calib"], 0.9, 3.0, True, 9.0)
    t21 = eio.pair_exposure_terms(fb[3].reshape(-1), fb[10], uv, tl, Q0[0], cl, 0.9, 3.0, True, 9.0)
    for k in t10:
        assert np.array_equal(bits(t10[k]), bits(t21[k])) if t10[k].dtype == np.float64 else np.array_equal(t10[k], t21[k]), k
    s10, n10 = eio.pair_sums(t10)
    s21, n21 = eio.pair_exposure_sums(t21)
    assert np.array_equal(n10, n21) and np.array_equal(bits(s10), bits(s21[list(eio.EXPOSURE_SHARED)]))


def test_the_exposure_jacobian_against_differences():
    """d r / d a = -v and d r / d b = -1 on every used pixel of a level, by central differences of pair_exposure_terms' r; b = sum w J r accordingly."""
    c = LC.case()
    fr = c["frames"].reshape(LC.F, LC.SH, LC.SW)
    l = 1
    fb, tl, cl = eio.pair_level_bytes(fr, l, True), eio.pair_level_lut(c["lut"], LC.SENSOR, l), eio.pair_level_calib(c["calib"], l)
    Q = LC.start(1.0)
    uv = eio.pair_project(tl, Q, cl)[1]
    i, j = LC.PAIR
    T = lambda a, b: eio.pair_exposure_terms(fb[i].reshape(-1), fb[j], uv, tl, Q, cl, a, b, True, 0.0)      # noqa: E731
    t = T(0.9, 3.0)
    used = t["cls"] == eio.ALIGN_USED
    h = 1e-3
    da = (T(0.9 + h, 3.0)["r"] - T(0.9 - h, 3.0)["r"]) / (2 * h)
    db = (T(0.9, 3.0 + h)["r"] - T(0.9, 3.0 - h)["r"]) / (2 * h)
    assert used.sum() > 500 and np.abs(da[used] + t["I0"][used]).max() < 1e-8 and np.abs(db[used] + 1.0).max() < 1e-9
    assert np.array_equal(t["I0"][used], fb[i].reshape(-1)[used].astype(np.float64)) and not t["I0"][~used].any()
    s, n = eio.pair_exposure_sums(t)
    assert s[eio.EXPOSURE_RHS + 3] == pytest.approx(-(t["w"] * t["I0"] * t["r"]).sum(), rel=1e-12) and s[eio.EXPOSURE_RHS + 4] == pytest.approx(-(t["w"] * t["r"])[used].sum(), rel=1e-12)
    # the rotation's rows against differences of r in delta, at the level
    g = np.zeros((used.size, 3))
    for k in range(3):
        d = np.zeros(3)
        d[k] = 1e-6
        rp = eio.pair_exposure_terms(fb[i].reshape(-1), fb[j], eio.pair_project(tl, so3.mul(so3.exp(d), Q), cl)[1], tl, Q, cl, 0.9, 3.0, True, 0.0)
        rm = eio.pair_exposure_terms(fb[i].reshape(-1), fb[j], eio.pair_project(tl, so3.mul(so3.exp(-d), Q), cl)[1], tl, Q, cl, 0.9, 3.0, True, 0.0)
        both = used & (rp["cls"] == eio.ALIGN_USED) & (rm["cls"] == eio.ALIGN_USED)
        g[:, k] = np.where(both, (rp["r"] - rm["r"]) / 2e-6, np.nan)
    ok = np.isfinite(g).all(axis=1)
    close = np.abs(g[ok] - t["g"][ok]).max(axis=1) <= 1e-3 * (1.0 + np.abs(t["g"][ok]).max(axis=1))      # (a pixel whose cell changes between the two sides differs)
    assert ok.sum() > 500 and close.mean() > 0.97


def test_the_recorded_basin():
    e = LC.end_angle(LC.align_numpy((0,), 1.0)["q"][0])
    assert e == pytest.approx(LC.END_NP, rel=1e-3)
    b0, home0 = LC.basin((0,))
    bs, homes = LC.basin(LC.SCHEDULE)
    print(f"level 0 alone: {b0} cells {home0}; {LC.SCHEDULE}: {bs} cells {homes}")
    assert b0 == LC.BASIN_0 and bs == LC.BASIN_S and LC.BASIN_0 < LC.WIDE_CELLS <= LC.BASIN_S
    if LC.WIDENS:      # numpy shows the widening: the schedule ends at level 0's own end point from a start level 0 alone does not come home from
        alone, sched = LC.align_numpy((0,), LC.WIDE_CELLS), LC.align_numpy(LC.SCHEDULE, LC.WIDE_CELLS)
        assert LC.end_angle(alone["q"][0]) > LC.angle_bound() >= LC.end_angle(sched["q"][0])
        d = float(eio.rotation_angle_between(LC.align_numpy((0,), 1.0)["q"], sched["q"])[0])
        assert d <= LC.SETTINGS["tol_rot"] and d == pytest.approx(LC.SAME_END_NP, rel=0.05)
        assert (sched["level_status"] != 0).all() and sched["iters"][0] == sched["level_iters"].sum() and sched["status"][0] == sched["level_status"][0, -1]


def test_the_recorded_exposure_case():
    fr = LC.exposure_frames()
    assert fr[LC.PAIR[1]].max() < 255 and np.array_equal(fr[LC.PAIR[1]] == 0, LC.case()["frames"][LC.PAIR[1]] == 0)      # no byte saturates; "no data" stays
    r0, r3 = LC.align_numpy(LC.SCHEDULE, LC.EXPOSURE_CELLS, 0, True), LC.align_numpy(LC.SCHEDULE, LC.EXPOSURE_CELLS, 3, True)
    print(f"estimate 0: {LC.end_angle(r0['q'][0]):.4e} rad; estimate 3: {LC.end_angle(r3['q'][0]):.4e} rad, a {r3['gain'][0]:.6f} b {r3['bias'][0]:.4f}")
    assert LC.end_angle(r0["q"][0]) == pytest.approx(LC.EXPOSURE_END[0], rel=1e-3) and LC.end_angle(r3["q"][0]) == pytest.approx(LC.EXPOSURE_END[3], rel=1e-3)
    assert r3["gain"][0] == pytest.approx(LC.EXPOSURE_AB[0], abs=1e-6) and r3["bias"][0] == pytest.approx(LC.EXPOSURE_AB[1], abs=1e-4)
    assert r0["gain"][0] == 1.0 and r0["bias"][0] == 0.0
    if LC.EXPOSURE_IMPROVES:
        assert LC.end_angle(r3["q"][0]) <= LC.angle_bound() < LC.end_angle(r0["q"][0])
        assert abs(r3["gain"][0] - LC.GAIN_J) < 0.01 and abs(r3["bias"][0] - LC.BIAS_J) < 0.5
    # the spread that bounds the device: a permuted summation in plain fp64, and the last accepted step
    c = LC.case()
    y = eio.pair_align_levels(fr, [LC.PAIR], [LC.start(LC.EXPOSURE_CELLS)], c["lut"], c["calib"], LC.SENSOR, levels=LC.SCHEDULE, estimate=3, skip_zero=True,
                              order=LC.permuted, **LC.SETTINGS)
    assert abs(y["gain"][0] - r3["gain"][0]) <= max(LC.AB_SPREAD_NP[0], 1e-15) and abs(y["bias"][0] - r3["bias"][0]) <= max(LC.AB_SPREAD_NP[1], 1e-13)
    assert np.array_equal(y["level_iters"], r3["level_iters"])
    assert abs(r3["last_x"][0, 3]) <= LC.AB_LAST_STEP[0] and abs(r3["last_x"][0, 4]) <= LC.AB_LAST_STEP[1]
    # a pair that ends degenerate at its first level: one constant byte, gain and bias both estimated
    flat = fr.copy()
    flat[LC.PAIR[0]] = 90
    d = eio.pair_align_levels(flat, [LC.PAIR], [LC.start(1.0)], c["lut"], c["calib"], LC.SENSOR, levels=LC.SCHEDULE, estimate=3, gain=1.2, bias=3.0, skip_zero=True,
                              **LC.SETTINGS)
    assert d["status"][0] == eio.ALIGN_DEGENERATE and d["level_status"][0].tolist() == [eio.ALIGN_DEGENERATE, 0, 0] and d["iters"][0] == 0
    assert np.array_equal(bits(d["q"][0]), bits(LC.start(1.0))) and d["gain"][0] == 1.2 and d["bias"][0] == 3.0
