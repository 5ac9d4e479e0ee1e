"""record_data's map images on the MI355X (-m gpu): emba_normalize_robust / emba_render_map_images against the host rule
(emba_amd/io.normalize_robust and the numpy restatement in tests/record_ref.py), the recorder inside the device LM loop, and
examples/run_ba.py --record-data."""
import os
import subprocess
import sys

import numpy as np
import pytest

from emba_amd import io as eio
from record_ref import decode_png, hsv_channels, hsv_to_rgb, ranks_f32, render_np

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def legm():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from emba_amd import LEGM
    from emba_amd.synth import pinhole_bearing_lut
    m = LEGM(8, 8, pinhole_bearing_lut(8, 8, 10, 10, 4, 4), 0.2, 64, 32)
    yield m
    m.close()


def _check_normalize(m, a, pct=0.1):
    u8, (rmin, rmax) = m.normalizeRobust(a, pct, with_range=True)
    assert u8.shape == a.shape and u8.dtype == np.uint8
    assert np.array_equal(u8, eio.normalize_robust(a, pct))
    srt = np.sort(a, axis=None)
    k0, k1 = ranks_f32(a.size, pct)
    # bit for bit, except that numpy leaves the order of -0.0 and +0.0 unspecified
    for got, want in ((rmin, srt[k0]), (rmax, srt[k1])):
        assert got == want
        if want != 0.0:
            assert np.float64(got).tobytes() == np.float64(want).tobytes()


@pytest.mark.parametrize("H", [512, 1024, 2048])
def test_normalize_robust_bit_exact_at_panorama_sizes(legm, H):
    rng = np.random.default_rng(H)
    a = rng.standard_cauchy(size=(H, 2 * H)) * 1e-3
    a[rng.random(a.shape) < 0.3] = 0.0                      # unobserved pixels of a map: exact zeros, a heavy tie
    _check_normalize(legm, a)
    _check_normalize(legm, rng.normal(size=(H, 2 * H)), 0.5)


def test_normalize_robust_edge_cases(legm):
    rng = np.random.default_rng(1)
    _check_normalize(legm, rng.integers(-3, 4, size=(300, 600)).astype(np.float64))     # heavy ties: seven values
    const = np.full((64, 128), 0.25)
    _check_normalize(legm, const)                                                       # rmax == rmin: scale 1
    assert (legm.normalizeRobust(const) == 0).all()
    pm = rng.choice([-0.0, 0.0, 1.0, -1.0], size=(50, 100), p=[0.45, 0.45, 0.05, 0.05])
    _check_normalize(legm, pm)                                                          # a +-0 mix
    z = np.where(rng.random((40, 80)) < 0.5, -0.0, 0.0)
    u8, (rmin, rmax) = legm.normalizeRobust(z, 0.1, with_range=True)
    assert rmin == 0.0 and rmax == 0.0 and np.array_equal(u8, eio.normalize_robust(z))  # either zero gives the same image
    tiny = rng.normal(size=18)
    assert ranks_f32(18) == (0, 17)
    _check_normalize(legm, tiny)                                                        # n = 18: i_min = 0
    _check_normalize(legm, np.array([3.5]))
    _check_normalize(legm, np.array([np.inf, -np.inf, 1.0, -2.0, 5e-324, -5e-324, 1e308]), 30.0)


def _lm_model(w, recorder=None, max_iter=4):
    from emba_amd import LEGM
    from emba_amd.solver import BASettings, LMSettings, solve_time_window
    from test_lm_solver_cpu import perturbed
    m = LEGM(w.sensor_w, w.sensor_h, w.lut, w.C_th, w.pano_w, w.pano_h, device=0)
    r = solve_time_window(m, perturbed(w), w.events, w.Gx, w.Gy, BASettings(alpha=1.0), LMSettings(max_num_iter=max_iter), resident=True,
                          map_recorder=recorder)
    return m, r


@pytest.fixture(scope="module")
def scene():
    import torch
    assert torch.cuda.is_available()
    from emba_amd import synth
    return synth.make_scene_workload(n_steps=1000)


def test_render_matches_host_rule_after_lm_steps(scene):
    m, _ = _lm_model(scene)
    imgs = m.renderMapImages(0.1, poisson=True)
    gx, gy = m.downloadMap()
    assert np.array_equal(imgs["Gx"], eio.normalize_robust(gx, 0.1))
    assert np.array_equal(imgs["Gy"], eio.normalize_robust(gy, 0.1))
    M = m.reconstructIntensity()
    assert np.array_equal(imgs["map_poisson"], eio.normalize_robust(M, 0.1))
    # G_hsv: device and host atan2 may differ by 1 ulp -> at most one hue level on at most 1e-4 of the pixels; everything else exact
    ref = render_np(gx, gy)["G_hsv"]
    got = imgs["G_hsv"]
    assert got.shape == (m.H, m.W, 3)
    bad = np.argwhere((got != ref).any(axis=-1))
    assert len(bad) <= max(1, int(1e-4 * m.H * m.W)), len(bad)
    Hc, Vc = hsv_channels(gx, gy)
    for i, j in bad:
        alts = [hsv_to_rgb(np.array([h], np.uint8), np.array([255], np.uint8), Vc[i, j:j + 1])[0] for h in (int(Hc[i, j]) - 1, int(Hc[i, j]) + 1) if 0 <= h <= 255]
        assert any(np.array_equal(a, got[i, j]) for a in alts), (i, j, got[i, j], ref[i, j])
    # without Poisson, and single images
    again = m.renderMapImages(0.1, poisson=False)
    assert again["map_poisson"] is None
    for k in ("Gx", "Gy", "G_hsv"):
        assert np.array_equal(again[k], imgs[k])


def test_recorder_leaves_the_device_loop_unchanged(scene, tmp_path):
    from emba_amd.solver import MapRecorder
    m0, r0 = _lm_model(scene)
    rec = MapRecorder(str(tmp_path))
    m1, r1 = _lm_model(scene, rec)
    rec.close()
    # The device loop is not bit-reproducible from run to run by itself (its cost and normal-equation sums use float atomics: two plain runs
    # differ in the last bits), so the recorder's runs are held to that: the same decisions and iteration count, costs, trajectory and map to
    # 1e-12.  tests/test_record_cpu.py shows bit-identity on the (deterministic) oracle loop.
    assert [e[4] for e in r0.log] == [e[4] for e in r1.log]
    assert (r0.iterations, r0.converged, r0.reason) == (r1.iterations, r1.converged, r1.reason)
    for a, b in zip(r0.log, r1.log):
        assert a[0] == b[0] and a[1] == b[1] and a[2] == pytest.approx(b[2], rel=1e-12) and a[3] == pytest.approx(b[3], rel=1e-12)
    assert r0.cost_min == pytest.approx(r1.cost_min, rel=1e-12)
    assert np.abs(r0.traj.knots_xyzw - r1.traj.knots_xyzw).max() < 1e-12
    for a, b in zip(m0.downloadMap(), m1.downloadMap()):
        assert np.abs(a - b).max() <= 1e-12 * np.abs(a).max()
    N = r1.iterations
    assert rec.sets == N + 2 and len(rec.files) == 4 * (N + 2)
    final = m1.renderMapImages()
    for key, folder, stem in MapRecorder.OPT:
        assert np.array_equal(decode_png(str(tmp_path / folder / f"win_0000_{stem}_{N:04d}.png")), final[key])


def test_run_ba_record_data(tmp_path):
    out = tmp_path / "out"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "run_ba.py"), "--demo", str(out), "--record-data", "--max-iter", "6"],
                       capture_output=True, text=True, timeout=600)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stderr
    for f in ("refined_traj.txt", "Gx.bin", "Gy.bin", "map_poisson_opt.pgm"):      # what run_ba writes without the flag
        assert (out / f).exists()
    evo = {d: sorted(os.listdir(out / d)) for d in ("Gx_evo", "Gy_evo", "G_hsv_evo", "map_poisson_evo")}
    iters = [int(f[-8:-4]) for f in evo["Gx_evo"]]
    assert iters == list(range(len(iters))) and len(iters) >= 2
    N = iters[-1]
    for d, stem in (("Gx_evo", "Gx_evo"), ("Gy_evo", "Gy_evo"), ("G_hsv_evo", "G_hsv_evo"), ("map_poisson_evo", "map_poisson_evo")):
        assert evo[d] == [f"win_0000_{stem}_{i:04d}.png" for i in iters]
    assert sorted(os.listdir(out / "map_opt")) == sorted(f"win_0000_{s}_opt_{N:04d}.png" for s in ("Gx", "Gy", "G_hsv", "map_poisson"))
    gx, gy = eio.load_map(str(out))
    img = decode_png(str(out / "map_opt" / f"win_0000_Gx_opt_{N:04d}.png"))
    assert np.array_equal(img, eio.normalize_robust(gx, 0.1))
    assert decode_png(str(out / "map_opt" / f"win_0000_G_hsv_opt_{N:04d}.png")).shape == gx.shape + (3,)
    for d in evo:
        for f in evo[d]:
            decode_png(str(out / d / f))
