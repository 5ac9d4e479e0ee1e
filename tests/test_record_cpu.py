"""record_data's map images without a GPU: the PNG writer, the rank arithmetic of normalizeRobust, the HSV rule's numpy restatement
(tests/record_ref.py) and emba_amd.solver.MapRecorder driven by the LM loop on the CPU oracle."""
import os

import numpy as np
import pytest

from emba_amd import io as eio
from emba_amd import synth
from emba_amd.solver import BASettings, LMSettings, MapRecorder, solve_time_window
from helpers import OracleModel
from record_ref import decode_png, hsv_channels, hsv_to_rgb, ranks_f32, ranks_f64, render_np
from test_lm_solver_cpu import perturbed


@pytest.mark.parametrize("shape", [(1, 1), (5, 7), (64, 128), (33, 65, 3), (2, 3, 3)])
def test_save_png_round_trip(tmp_path, shape):
    rng = np.random.default_rng(sum(shape))
    a = rng.integers(0, 256, size=shape, dtype=np.uint8)
    p = str(tmp_path / "a.png")
    eio.save_png(p, a)
    assert np.array_equal(decode_png(p), a)
    try:
        from PIL import Image
    except ImportError:
        return
    im = Image.open(p)
    assert im.mode == ("RGB" if a.ndim == 3 else "L")
    assert np.array_equal(np.array(im), a)


def test_save_png_rejects_other_shapes(tmp_path):
    with pytest.raises(ValueError):
        eio.save_png(str(tmp_path / "x.png"), np.zeros((4, 4, 4), np.uint8))


@pytest.mark.parametrize("H", [96, 128, 256, 512, 1024, 2048, 4096])
def test_rank_arithmetic_float32_equals_double(H):
    """io.normalize_robust's float32 ranks (the device's) equal the reference's double ranks at every panorama size of the project."""
    n = H * 2 * H
    assert ranks_f32(n, 0.1) == ranks_f64(n, 0.1)


def test_rank_restatement_is_io_normalize_robust():
    rng = np.random.default_rng(3)
    a = rng.normal(size=(48, 96))
    srt = np.sort(a, axis=None)
    k0, k1 = ranks_f32(a.size)
    rmin, rmax = srt[k0], srt[k1]
    assert np.array_equal(eio.normalize_robust(a, 0.1), np.clip(np.rint(255.0 / (rmax - rmin) * (a - rmin)), 0, 255).astype(np.uint8))


def test_hsv_rule_gives_pure_colours():
    H = np.array([0, 30, 60, 90, 120, 150], np.uint8)
    rgb = hsv_to_rgb(H, np.full_like(H, 255), np.full_like(H, 255))
    expect = [(255, 0, 0), (255, 255, 0), (0, 255, 0), (0, 255, 255), (0, 0, 255), (255, 0, 255)]
    assert [tuple(int(c) for c in px) for px in rgb] == expect
    assert (hsv_to_rgb(H, np.full_like(H, 255), np.zeros_like(H)) == 0).all()        # V = 0: black
    grey = hsv_to_rgb(H, np.zeros_like(H), np.full_like(H, 128))                       # S = 0: grey
    assert (grey == 128).all()


def test_hsv_hue_follows_gradient_orientation():
    """Gradients along +x, +y, -x, -y (magnitude 2) and a zero one: hue = 0.5*angle min-max normalised to [0, 179], value = magnitude to [0, 255]."""
    gx = np.array([[2.0, 0.0, -2.0, 0.0, 0.0]])
    gy = np.array([[0.0, 2.0, 0.0, -2.0, 0.0]])
    H, V = hsv_channels(gx, gy)
    assert H.tolist() == [[0, 60, 119, 179, 0]]          # 0.5*angle = 0, 45, 90, 135, 0 -> x 179/135
    assert V.tolist() == [[255, 255, 255, 255, 0]]
    img = render_np(gx, gy)["G_hsv"][0]
    assert tuple(int(c) for c in img[0]) == (255, 0, 0)   # hue 0: red
    assert tuple(int(c) for c in img[4]) == (0, 0, 0)     # no gradient: black


class RenderingOracle(OracleModel):
    """The CPU oracle with renderMapImages restated in numpy on the map the next evaluation would use."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.rendered = []

    def renderMapImages(self, pct=0.1, poisson=True):
        gx, gy = self.downloadMap()
        self.rendered.append((gx.copy(), gy.copy()))
        return render_np(gx, gy, gx + gy if poisson else None, pct)


def _names(win, it, table):
    return [os.path.join(folder, f"{win}{stem}_{it:04d}.png") for _, folder, stem in table]


@pytest.mark.parametrize("max_iter,tol,reason", [(3, 1e-3, "max_iter"), (50, 0.9, "tolerance")])
def test_recorder_follows_lm_log(oracle_mod, tmp_path, max_iter, tol, reason):
    w = synth.make_scene_workload(n_steps=600)
    init = perturbed(w)
    ba, lm = BASettings(alpha=1.0), LMSettings(max_num_iter=max_iter, tol_fun=tol, num_times_tol_fun_sat=1 if reason == "tolerance" else 2)
    r0 = solve_time_window(OracleModel(oracle_mod, w), init, w.events, w.Gx, w.Gy, ba, lm)
    m = RenderingOracle(oracle_mod, w)
    rec = MapRecorder(str(tmp_path), writers=2)
    r1 = solve_time_window(m, init, w.events, w.Gx, w.Gy, ba, lm, map_recorder=rec)
    rec.close()
    # the loop's result is the same with and without the recorder
    assert (r0.cost_min, r0.iterations, r0.converged, r0.reason, r0.log) == (r1.cost_min, r1.iterations, r1.converged, r1.reason, r1.log)
    assert np.array_equal(r0.traj.knots_xyzw, r1.traj.knots_xyzw)
    assert r1.reason == reason
    # one evo set per loop iteration (iter 0 .. N-1), evo + opt at the end with iter N
    N = r1.iterations
    assert len(r1.log) == N
    expect = []
    for it in range(N):
        expect += _names("win_0000_", it, MapRecorder.EVO)
    expect += _names("win_0000_", N, MapRecorder.EVO) + _names("win_0000_", N, MapRecorder.OPT)
    assert sorted(os.path.relpath(p, tmp_path) for p in rec.files) == sorted(expect)
    found = sorted(os.path.relpath(os.path.join(d, f), tmp_path) for d, _, fs in os.walk(tmp_path) for f in fs)
    assert found == sorted(expect)
    assert len(m.rendered) == N + 1 and rec.sets == N + 2
    sm = rec.summary()
    assert sm["files"] == 4 * (N + 2) and sm["render_s"] > 0 and sm["encode_s"] > 0
    # the last evo set and the opt set show the final (accepted) map
    final = render_np(*m.rendered[-1], m.rendered[-1][0] + m.rendered[-1][1])
    for key, folder, stem in MapRecorder.OPT:
        assert np.array_equal(decode_png(str(tmp_path / folder / f"win_0000_{stem}_{N:04d}.png")), final[key])
    gx_last, _ = m.rendered[-1]
    assert np.array_equal(gx_last, m.downloadMap()[0])
    for key, folder, stem in MapRecorder.EVO:
        assert np.array_equal(decode_png(str(tmp_path / folder / f"win_0000_{stem}_{N:04d}.png")), final[key])
