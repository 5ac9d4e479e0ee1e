"""The mosaic of intensity frames without a GPU: the numpy forms of emba_mosaic_frames, emba_mosaic_get and emba_mosaic_map (emba_amd.io:
mosaic_votes, mosaic_mean, mosaic_log, gradient_from_plane) against what they state, the new symbols of libemba_hip.so, and the loop
plane -> frames -> mosaic -> gradient map closed in numpy alone."""
import inspect
import math
import os

import numpy as np
import pytest

import mosaic_cases as MC
from emba_amd import io as eio

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_new_symbols_resolve(hip_lib):
    from emba_amd import LEGM, _lib
    for name in ("emba_mosaic_frames", "emba_mosaic_get", "emba_mosaic_map", "emba_mosaic_clear"):
        assert hasattr(hip_lib, name) and name in _lib.SIGNATURES, name
    assert hip_lib.emba_abi_version() == 2
    blob = open(os.path.join(ROOT, "emba_amd", "libemba_hip.so"), "rb").read()
    for kernel in (b"emba_mosaic_vote_kernel", b"emba_mosaic_mean_kernel", b"emba_mosaic_log_kernel", b"emba_mosaic_map_kernel"):
        assert kernel in blob, kernel
    p = inspect.signature(LEGM.mosaic_frames).parameters
    assert list(p)[1:] == ["frames", "frame_t_ns", "traj", "skip_zero", "accumulate", "want_pm"]
    assert (p["skip_zero"].default, p["accumulate"].default, p["want_pm"].default) == (False, False, False)
    p = inspect.signature(LEGM.mosaic).parameters
    assert list(p)[1:] == ["min_weight", "fill"] and (p["min_weight"].default, p["fill"].default) == (256, 0.0)
    p = inspect.signature(LEGM.mosaic_map).parameters
    assert list(p)[1:] == ["min_weight", "lo", "hi", "eps", "take_log", "resident"]
    assert (p["min_weight"].default, p["lo"].default, p["hi"].default, p["eps"].default, p["take_log"].default, p["resident"].default) == (256, 0.0, 1.0, 1 / 255, True, False)
    assert list(inspect.signature(LEGM.mosaic_clear).parameters) == ["self"]


def loop_votes(frames, pm, W, H, skip_zero):
    """The rule of emba_mosaic_frames as include/emba_hip.h states it: one pixel and one vote at a time, in python ints."""
    sum_w, sum_v = [0] * (W * H), [0] * (W * H)
    dropped = skipped = 0
    for v, (x, y) in zip(frames.reshape(-1).tolist(), pm.reshape(-1, 2).tolist()):
        if skip_zero and v == 0:
            skipped += 1
            continue
        if not (abs(x) < 2147483648.0 and abs(y) < 2147483648.0):
            continue
        ix, iy = math.floor(x), math.floor(y)
        wx, wy = int((x - ix) * 16.0), int((y - iy) * 16.0)
        for col, row, w in ((ix, iy, (16 - wx) * (16 - wy)), (ix + 1, iy, wx * (16 - wy)), (ix, iy + 1, (16 - wx) * wy), (ix + 1, iy + 1, wx * wy)):
            if w == 0:
                continue
            if not 0 <= row < H:
                dropped += 1
                continue
            c = row * W + col % W
            sum_w[c] += w
            sum_v[c] += w * v
    return sum_w, sum_v, dropped, skipped


@pytest.mark.parametrize("pano", MC.PANOS, ids=lambda p: f"pano{p[1]}x{p[0]}")
@pytest.mark.parametrize("sensor", MC.SENSORS, ids=lambda s: f"sensor{s[0]}x{s[1]}")
def test_votes_against_a_scalar_loop(sensor, pano):
    W, H = pano
    seen_dropped = seen_skipped = seen_seam = 0
    for kind in MC.KINDS:
        for F in MC.FRAMES:
            c = MC.case(sensor, pano, kind, F)
            for skip_zero in (False, True):
                sw, sv, dropped, skipped = eio.mosaic_votes(c["frames"], c["pm"], W, H, skip_zero)
                lw, lv, ld, ls = loop_votes(c["frames"], c["pm"], W, H, skip_zero)
                what = (sensor, pano, kind, F, skip_zero)
                assert sw.dtype == np.uint64 and sv.dtype == np.uint64 and sw.shape == (H, W) and sv.shape == (H, W), what
                assert sw.reshape(-1).tolist() == lw and sv.reshape(-1).tolist() == lv and (dropped, skipped) == (ld, ls), what
                # every vote is somewhere: 256 per voting pixel, on the panorama or dropped
                assert int(sw.sum()) <= 256 * (c["frames"].size - skipped) and (dropped > 0 or int(sw.sum()) == 256 * (c["frames"].size - skipped)), what
                seen_dropped += dropped
                seen_skipped += skipped
            if kind == "yaw_pi":
                seen_seam += int(sw[:, 0].sum() > 0 and sw[:, W - 1].sum() > 0)
    assert seen_dropped > 0 and seen_skipped > 0 and seen_seam > 0      # the pitched views drop rows, their outside pixels are zeros; yaw_pi wraps


def test_accumulate_over_two_halves_is_one_call():
    sensor, pano = (20, 13), (48, 24)
    c = MC.case(sensor, pano, "pitch", 65)
    whole = eio.mosaic_votes(c["frames"], c["pm"], *pano, skip_zero=True)
    a = eio.mosaic_votes(c["frames"][:23], c["pm"][:23], *pano, skip_zero=True)
    b = eio.mosaic_votes(c["frames"][23:], c["pm"][23:], *pano, skip_zero=True)
    assert np.array_equal(a[0] + b[0], whole[0]) and np.array_equal(a[1] + b[1], whole[1]) and a[2] + b[2] == whole[2] and a[3] + b[3] == whole[3]


def test_skip_zero_removes_exactly_the_zero_bytes():
    sensor, pano = (16, 12), (32, 16)
    c = MC.case(sensor, pano, "pitch", 3)
    fr = c["frames"]
    assert (fr == 0).any() and (fr != 0).any()
    plain = eio.mosaic_votes(fr, c["pm"], *pano, skip_zero=False)
    skip = eio.mosaic_votes(fr, c["pm"], *pano, skip_zero=True)
    assert skip[3] == int((fr == 0).sum()) and plain[3] == 0
    assert np.array_equal(skip[1], plain[1])                       # a zero byte adds nothing to sum_v either way
    only_zero = eio.mosaic_votes(np.where(fr == 0, 1, 0).astype(np.uint8), c["pm"], *pano, skip_zero=True)      # the votes of exactly the zero pixels
    assert np.array_equal(plain[0] - skip[0], only_zero[0]) and plain[2] - skip[2] == only_zero[2]
    # the sums of the non-zero pixels alone
    keep = fr.reshape(-1) != 0
    alone = eio.mosaic_votes(fr.reshape(-1)[keep], c["pm"].reshape(-1, 2)[keep], *pano, skip_zero=False)
    assert np.array_equal(alone[0], skip[0]) and np.array_equal(alone[1], skip[1]) and alone[2] == skip[2]
    with pytest.raises(ValueError):
        eio.mosaic_votes(fr, c["pm"][:1], *pano)


def test_mean_log_and_gradient_on_a_plane_with_holes():
    """The 3 x 4 plane of tests/cpp/mosaic_rule_test.cpp, through the numpy forms: holes, the wrapped column, row 0."""
    sum_w = np.array([[256, 0, 512, 256], [255, 256, 256, 1024], [256, 256, 0, 256]], np.uint64)
    sum_v = np.array([[256 * 10, 0, 512 * 30, 256 * 255], [255 * 99, 256 * 20, 256 * 40, 1024 * 60], [0, 256 * 51, 0, 256 * 102]], np.uint64)
    mean, cov = eio.mosaic_mean(sum_w, sum_v, 256, -1.0)
    assert cov.tolist() == [[True, False, True, True], [False, True, True, True], [True, True, False, True]]
    assert mean.tolist() == [[10.0, -1.0, 30.0, 255.0], [-1.0, 20.0, 40.0, 60.0], [0.0, 51.0, -1.0, 102.0]]
    assert eio.mosaic_mean(sum_w, sum_v, 1, -1.0)[1].sum() == 10 and eio.mosaic_mean(sum_w, sum_v, 1, -1.0)[0][1, 0] == 99.0
    assert eio.mosaic_mean(np.array([3], np.uint64), np.array([1], np.uint64), 1)[0][0] == 1.0 / 3.0
    with pytest.raises(ValueError):
        eio.mosaic_mean(sum_w, sum_v, 0)
    L, cov0 = eio.mosaic_log(mean, cov, 0.0, 255.0, 0.0, take_log=False)       # lo = 0, hi = 255: I is the mean itself
    assert np.array_equal(cov0, cov) and np.array_equal(L, np.where(cov, mean, 0.0))
    Gx, Gy = eio.gradient_from_plane(L, cov0)
    assert Gx.tolist() == [[10.0 - 255.0, 0.0, 0.0, 255.0 - 30.0], [0.0, 0.0, 20.0, 20.0], [0.0 - 102.0, 51.0, 0.0, 0.0]]
    assert Gy.tolist() == [[0.0, 0.0, 0.0, 0.0], [0.0, 0.0, 10.0, 60.0 - 255.0], [0.0, 31.0, 0.0, 42.0]]
    # the logarithm: a mean of 0 with eps = 0 has no logarithm and becomes uncovered; with eps > 0 it stays
    Ll, covl = eio.mosaic_log(mean, cov, 0.0, 255.0, 0.0, take_log=True)
    assert not covl[2, 0] and covl.sum() == cov.sum() - 1 and Ll[2, 0] == 0.0 and Ll[0, 0] == pytest.approx(math.log(10.0), rel=1e-15)
    Ll, covl = eio.mosaic_log(mean, cov, 0.0, 255.0, 0.5, take_log=True)
    assert covl[2, 0] and Ll[2, 0] == pytest.approx(math.log(0.5), rel=1e-15) and Ll[0, 3] == pytest.approx(math.log(255.5), rel=1e-15)
    assert eio.mosaic_log(mean, cov, -2.0, -1.0, 0.5, take_log=True)[1].sum() == 0      # every I + eps <= 0
    assert eio.mosaic_log(np.array([51.0]), np.array([True]), 0.25, 1.75, 0.0, False)[0][0] == 0.25 + 51.0 * (1.75 - 0.25) / 255.0
    for bad in ((1.0, 1.0, 0.0), (2.0, 1.0, 0.0), (0.0, np.inf, 0.0), (0.0, 1.0, np.nan)):
        with pytest.raises(ValueError):
            eio.mosaic_log(mean, cov, *bad)


def test_gradient_is_the_field_of_the_five_point_operator():
    """The backward differences of a plane without holes are the integrable field of tests/test_poisson_wrap_cpu.py: the wrapped left neighbour, row 0 free."""
    P = MC.smooth_plane((32, 16))
    Gx, Gy = MC.backward_differences(P)
    assert np.array_equal(Gx, P - np.roll(P, 1, axis=1)) and np.array_equal(Gy[1:], P[1:] - P[:-1]) and not Gy[0].any()


def test_load_pgm_reads_what_save_pgm_writes(tmp_path):
    img = np.random.default_rng(1).integers(0, 256, (5, 7)).astype(np.uint8)
    eio.save_pgm(str(tmp_path / "a.pgm"), img)
    assert np.array_equal(eio.load_pgm(str(tmp_path / "a.pgm")), img)
    (tmp_path / "b.pgm").write_bytes(b"P5 # a comment\n2 1\n# another\n65535\n" + bytes([1, 2, 255, 254]))
    assert eio.load_pgm(str(tmp_path / "b.pgm")).tolist() == [[258, 65534]]
    (tmp_path / "c.pgm").write_bytes(b"P2\n1 1\n255\n0\n")
    with pytest.raises(ValueError):
        eio.load_pgm(str(tmp_path / "c.pgm"))


@pytest.mark.parametrize("sensor,pano", MC.E2E_SMALL + MC.E2E_LARGE, ids=lambda v: f"{v[0]}x{v[1]}")
def test_end_to_end_in_numpy(sensor, pano):
    """plane -> exp -> render_views -> view_u8 -> mosaic_votes(skip_zero) -> mosaic_mean(256) -> mosaic_log -> gradient_from_plane against the backward
    differences of the plane, over the cells where both differences of the mosaic exist: Pearson correlation >= 0.95 on every kind of trajectory and every
    F of the cases.  A condition on the inputs — how well a forward splat of that few frames shows that plane again — not on the device.
    Measured with these cases: 0.953 - 0.992 on the four small pairs, 0.973 - 0.996 on the two large ones; max |mean - I| / max I over the covered cells
    0.004 - 0.18, the largest on the pitched views of 32 x 16 (printed, not asserted: cells at the rim of a view hold one pixel's bilinear share)."""
    W, H = pano
    for kind in MC.KINDS:
        for F in MC.FRAMES:
            c = MC.case(sensor, pano, kind, F)
            sw, sv, dropped, skipped = eio.mosaic_votes(c["frames"], c["pm"], W, H, skip_zero=True)
            mean, cov = eio.mosaic_mean(sw, sv, 256, 0.0)
            L, cov = eio.mosaic_log(mean, cov, c["lo"], c["hi"], 1.0 / 255.0, True)
            both = MC.gradient_mask(cov)
            r = MC.correlation(eio.gradient_from_plane(L, cov), MC.backward_differences(c["P"]), both)
            err = float((np.abs(c["lo"] + mean * (c["hi"] - c["lo"]) / 255.0 - c["I"])[cov]).max() / c["I"].max())
            print(f"{sensor} on {pano}, {kind}, F = {F}: {int(cov.sum())} covered cells, {int(both.sum())} with both differences, correlation {r:.4f}, "
                  f"max |mean - I| / max I {err:.4f}, {skipped} skipped")
            assert both.sum() >= 30 and r >= MC.E2E_MIN_CORRELATION, (sensor, pano, kind, F, r)
