"""One frame aligned to another, in numpy (emba_amd.io.pair_*): the identity pair on an ideal table of bearings, the pair alignment from a
start a stated angle off with and without a lens, the candidates, and the bookkeeping around them.  tests/pair_cases.py has the cases and the figures."""
import numpy as np
import pytest

import pair_cases as PC
from emba_amd import io as eio
from emba_amd import so3


def test_abi_declares_the_pair_stage(hip_lib):
    from emba_amd import _lib
    import os
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "emba_hip.h")).read()
    for name in ("emba_frames_pair_eval", "emba_frames_pair_align", "emba_rotation_graph_solve"):
        assert hasattr(hip_lib, name) and name in _lib.SIGNATURES and f"emba_status {name}(" in header


def test_identity_pair_has_no_residual_and_closed_form_counts():
    """(i, i) at Q = identity behind the ideal pinhole (focal length 32: uv is the pixel, exactly): every used pixel has r = 0 bit for bit, used is
    (sw - 1)(sh - 1), outside the last column and the last row; with skip_zero the zero bytes of the frame move pixels to masked and skipped and r stays 0."""
    c = PC.case(False)
    I4 = np.array([0.0, 0.0, 0.0, 1.0])
    uv = eio.pair_project(c["lut"], I4, c["calib"])[1]
    xs, ys = np.meshgrid(np.arange(PC.SW, dtype=np.float64), np.arange(PC.SH, dtype=np.float64))
    assert np.array_equal(uv[:, 0], xs.ravel()) and np.array_equal(uv[:, 1], ys.ravel())
    for f in (0, 5):
        fr = c["frames"][f]
        t = eio.pair_terms(fr, fr.reshape(PC.SH, PC.SW), uv, c["lut"], I4, c["calib"])
        sums, counts = eio.pair_sums(t)
        assert counts.tolist() == [(PC.SW - 1) * (PC.SH - 1), PC.SW + PC.SH - 1, 0, 0]
        assert not t["r"].any() and sums[9] == 0.0 and not sums[6:9].any() and sums[0] > 0.0
        t = eio.pair_terms(fr, fr.reshape(PC.SH, PC.SW), uv, c["lut"], I4, c["calib"], skip_zero=True)
        img = fr.reshape(PC.SH, PC.SW)
        cell_zero = (img[:-1, :-1] == 0) | (img[:-1, 1:] == 0) | (img[1:, :-1] == 0) | (img[1:, 1:] == 0)
        counts = eio.pair_sums(t)[1]
        assert counts[2] == int(cell_zero.sum()) and counts[3] == 0 and counts[0] + counts[2] == (PC.SW - 1) * (PC.SH - 1) and not t["r"].any()


def test_exposure_enters_the_residual():
    c = PC.case(False)
    Q = PC.true_pair(c, 1, 4)
    uv = eio.pair_project(c["lut"], Q, c["calib"])[1]
    a, b = 0.8, 7.0
    t0 = eio.pair_terms(c["frames"][1], c["frames"][4].reshape(PC.SH, PC.SW), uv, c["lut"], Q, c["calib"])
    t1 = eio.pair_terms(c["frames"][1], c["frames"][4].reshape(PC.SH, PC.SW), uv, c["lut"], Q, c["calib"], gain=a, bias=b)
    used = t0["cls"] == eio.ALIGN_USED
    v = c["frames"][1].astype(np.float64)
    assert np.array_equal(t0["cls"], t1["cls"]) and np.array_equal(t1["r"][used], (t0["r"] + v)[used] - (a * v + b)[used]) and np.array_equal(t0["g"], t1["g"])
    Qs, ga, bi = eio.pair_start(c["q_true"], np.linspace(1.0, 2.0, PC.F), np.linspace(0.0, 11.0, PC.F), [(1, 4), (4, 1), (3, 3)])
    assert np.allclose(Qs[0], Q, atol=1e-15) and np.allclose(so3.mul(Qs[0], Qs[1]), [0, 0, 0, 1], atol=1e-15) and np.allclose(Qs[2], [0, 0, 0, 1], atol=1e-15)
    g = np.linspace(1.0, 2.0, PC.F)
    assert ga[0] == g[1] / g[4] and bi[0] == (1.0 - 4.0) / g[4] and ga[2] == 1.0 and bi[2] == 0.0


def test_ju_is_the_derivative_of_uv_under_the_left_perturbation():
    c = PC.case(True)
    Q = PC.true_pair(c, 1, 4)
    Ju = eio.pair_project(c["lut"], Q, c["calib"])[3]
    h = 1e-6
    for k in range(3):
        d = np.zeros(3)
        d[k] = h
        up = eio.pair_project(c["lut"], so3.mul(so3.exp(d), Q), c["calib"])[1]
        dn = eio.pair_project(c["lut"], so3.mul(so3.exp(-d), Q), c["calib"])[1]
        assert np.allclose((up - dn) / (2 * h), Ju[:, :, k], rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize("lens", (False, True))
@pytest.mark.parametrize("pair", PC.ALIGN_PAIRS)
def test_pair_align_ends_where_recorded(lens, pair):
    """From one cell off the true relative rotation numpy's loop converges and ends at the recorded angle; so it does from the largest start recorded, and
    from the next start tried it does not."""
    r = PC.align_numpy(lens, pair, PC.START_CELLS)
    e = PC.end_angle(lens, pair, r["q"][0])
    print(f"lens {lens} pair {pair}: {e:.4e} rad, recorded {PC.END_NP[(lens, pair)]:.4e}; iters {r['iters'][0]}, n {r['counts'][0, 0]}")
    assert r["status"][0] == eio.ALIGN_CONVERGED and e == pytest.approx(PC.END_NP[(lens, pair)], rel=1e-3)
    assert r["cost0"][0] > 10.0 * r["sums"][0, 9] and r["n0"][0] > 0
    far = PC.align_numpy(lens, pair, PC.BASIN_NP[(lens, pair)])
    assert far["status"][0] == eio.ALIGN_CONVERGED and PC.end_angle(lens, pair, far["q"][0]) <= PC.angle_bound(lens, pair)
    lost = PC.align_numpy(lens, pair, PC.BASIN_FAILS[(lens, pair)])      # the recorded edge of the basin: the next start tried ends elsewhere
    assert PC.end_angle(lens, pair, lost["q"][0]) > PC.angle_bound(lens, pair)
    info = eio.pair_information(r["sums"], r["counts"])[0]
    s2 = r["sums"][0, 9] / (r["counts"][0, 0] - 3)
    assert np.array_equal(info, r["sums"][0, :6] / s2) and np.array_equal(info, r["info"][0])


def test_the_lens_matters():
    """The frames seen through the lens, aligned with the pinhole's projection, end further from the truth than with the lens's: D is live."""
    c = PC.case(True)
    pair = (1, 4)
    Q0 = PC.start_off(PC.true_pair(c, *pair), PC.CELL)
    wrong = eio.pair_align(c["frames"], [pair], [Q0], c["lut"], PC.PINHOLE, PC.SENSOR, skip_zero=True, **PC.SETTINGS)
    assert PC.end_angle(True, pair, wrong["q"][0]) > 5.0 * PC.END_NP[(True, pair)]


def test_playroom_fixture_is_the_zero_lens():
    K, D, w, h = PC.playroom_calibration()
    assert (w, h) == (128, 128) and K[0, 0] == K[1, 1] == 91.4014729896821 and K[0, 2] == 64.0 and not D.any()
    lut = eio.bearing_lut_from_calibration(K, D, w, h)
    cal = eio.pair_calib(K[0, 0], K[1, 1], K[0, 2], K[1, 2], D)
    uv = eio.pair_project(lut, [0, 0, 0, 1], cal)[1]
    uv0 = eio.pair_project(lut, [0, 0, 0, 1], eio.pair_calib(K[0, 0], K[1, 1], K[0, 2], K[1, 2]))[1]
    xs, ys = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    assert np.array_equal(uv, uv0) and np.abs(uv - np.stack([xs.ravel(), ys.ravel()], axis=1)).max() < 1e-12


def test_candidates():
    q, status = PC.drifted()
    pairs = eio.pair_candidates(q, status, **PC.CANDIDATES)
    assert len(pairs) == PC.N_PAIRS_NP and (pairs[:, 0] < pairs[:, 1]).all() and pairs.tolist() == [list(p) for p in sorted(set(map(tuple, pairs.tolist())))]
    near = {tuple(p) for p in pairs.tolist() if p[1] - p[0] <= 2}
    assert near == {(i, j) for i in range(PC.F) for j in range(i + 1, min(i + 3, PC.F))}
    assert (0, 11) not in {tuple(p) for p in pairs.tolist()}      # 3.85 cells of drift between two frames a cell apart: beyond max_angle = 3 cells
    only_window = eio.pair_candidates(q, status, window=1)
    assert only_window.tolist() == [[f, f + 1] for f in range(PC.F - 1)]
    st = status.copy()
    st[5] = 3      # a lost frame takes no part
    assert 5 not in eio.pair_candidates(q, st, **PC.CANDIDATES)
    ties = eio.pair_candidates(np.tile([0.0, 0.0, 0.0, 1.0], (6, 1)), [1, 2, 2, 2, 2, 2], window=0, min_gap=0, max_angle=0.1, max_per_frame=1)
    assert ties.tolist() == [[0, f] for f in range(1, 6)]      # every angle is 0: frame 0 takes frame 1, every other frame takes frame 0
    with pytest.raises(ValueError):
        eio.pair_candidates(np.zeros((eio.PAIR_MAX_CANDIDATE_FRAMES + 1, 4)), np.ones(eio.PAIR_MAX_CANDIDATE_FRAMES + 1))
