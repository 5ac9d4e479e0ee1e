"""The cases of the pair and rotation-graph tests, shared by tests/test_pair_cpu.py and tests/test_graph_cpu.py (the numpy forms) and
tests/test_gpu_pair.py (the device and the C entry against them): the out-and-back frames of tests/refit_cases.py — 64 x 48 on the 128 x 64 panorama, the
last frames see what the first saw — behind the wide pinhole of tests/view_cases.py, and behind the same pinhole with a plumb_bob lens.  Every figure below
was measured with the numpy forms (python tests/pair_cases.py prints them; the CPU tests check them); nothing comes from the device."""
import functools
import os

import numpy as np

import refit_cases as RC
import track_cases as TC
from emba_amd import io as eio
from emba_amd import so3

SENSOR, PANO = RC.SENSOR, RC.PANO
SW, SH = SENSOR
F = 12
STEP = "small"
CELL = 2.0 * np.pi / PANO[0]                                    # a level-0 cell of the panorama, rad
SETTINGS = dict(TC.SETTINGS)
# the camera of tests/view_cases.py's lut_of(SENSOR): focal length half the width (32: a power of two, so (x - cu) / fu * fu + cu is x exactly)
PINHOLE = eio.pair_calib(0.5 * SW, 0.5 * SW, 0.5 * (SW - 1), 0.5 * (SH - 1))
# a lens: the coefficients tests/test_io_formats.py uses for bearing_lut_from_calibration, 8 % of barrel distortion at the corner of this sensor
LENS_D = (-0.3, 0.1, 1e-3, -2e-3, 0.0)
LENS = eio.pair_calib(0.5 * SW, 0.5 * SW, 0.5 * (SW - 1), 0.5 * (SH - 1), LENS_D)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "DVS-playroom.yaml")


def playroom_calibration():
    """(K [3, 3], D [5], width, height) of the playroom calibration, a settings fixture (tests/golden/DVS-playroom.yaml).  Its D is all zero: the recording
    is a synthetic one.  The lens of these tests is LENS_D for that reason."""
    rows, key = {}, None
    for line in open(GOLDEN):
        s = line.strip()
        if s.endswith(":"):
            key = s[:-1]
        elif s.startswith("data:") and key:
            rows[key] = [float(v) for v in s[s.index("[") + 1:s.index("]")].split(",")]
        elif ":" in s and not s.startswith(("rows", "cols")):
            k, v = s.split(":", 1)
            rows[k.strip()] = v.strip()
    return np.array(rows["camera_matrix"]).reshape(3, 3), np.array(rows["distortion_coefficients"]), int(rows["image_width"]), int(rows["image_height"])


def lens_lut():
    K = np.array([[LENS["fu"], 0.0, LENS["cu"]], [0.0, LENS["fv"], LENS["cv"]], [0.0, 0.0, 1.0]])
    return eio.bearing_lut_from_calibration(K, LENS_D, SW, SH, iters=20)


@functools.lru_cache(maxsize=None)
def case(lens=False):
    """frames uint8 [F, S] at q_true [F, 4] along tests/refit_cases.py's out-and-back trajectory; with `lens` seen through LENS (the bearings of
    io.bearing_lut_from_calibration, 20 iterations: the undistortion is then exact to rounding).  Read-only."""
    if not lens:
        c = RC.case(STEP, F)
        return dict(frames=c["frames"], q_true=c["q_true"], ts=c["ts"], lut=c["lut"], calib=PINHOLE)
    import mosaic_cases as MC
    W, H = PANO
    inten = np.exp(MC.smooth_plane(PANO))
    lo, hi = float(inten.min()), float(inten.max())
    lut = lens_lut()
    q_true = RC.case(STEP, F)["q_true"]
    pm = np.array([eio.align_warp(lut, q, W, H)[1] for q in q_true])
    views, outside = eio.render_views(inten, pm, with_outside=True)
    frames = eio.view_u8(views, lo, hi, outside=outside)
    for a in (frames, lut):
        a.setflags(write=False)
    return dict(frames=frames, q_true=q_true, ts=RC.times(F), lut=lut, calib=LENS)


def true_pair(c, i, j):
    return so3.mul(so3.inverse(c["q_true"][j]), c["q_true"][i])


OFF_AXIS = np.array([0.3, 1.0, -0.2]) / np.linalg.norm([0.3, 1.0, -0.2])


def start_off(Q, angle):
    """Q turned by `angle` about OFF_AXIS on the left."""
    return so3.mul(so3.exp(angle * OFF_AXIS), Q)


# ---- one pair from a start a stated angle off: frames 3 and 10 (half a cell apart, on the way out and on the way back) and frames 1 and 4 (1.5 cells apart).
# Frames f and 12 - f of this trajectory are the same bytes and are left out here: their pair ends at a cost of 0.  START_CELLS: the start is one cell off.
# END_NP: the angle between numpy's pair_align result and the true relative rotation (rad): what byte rounding and the bilinear sample leave.  BASIN_NP: the
# largest start (cells) of BASIN_TRIED below the first one from which numpy no longer ends within 2 END_NP + tol_rot; BASIN_FAILS: that first failing start.
# Behind the pinhole every start up to 14 cells (0.69 rad, three quarters of the 90 degree view) ends there and 16 does not; seen through the lens 16 does
# and 20 does not.  Beyond the edge the outcome is patchy (20 and 24 cells behind the pinhole end there again, 32 never): the edge is the first failure.
ALIGN_PAIRS = ((3, 10), (1, 4))
START_CELLS = 1.0
BASIN_TRIED = (0.5, 1.0, 2.0, 3.0, 4.0, 6.0, 8.0, 10.0, 12.0, 14.0, 16.0, 20.0, 24.0, 32.0)
END_NP = {
    (False, (3, 10)): 4.6068e-04, (False, (1, 4)): 1.5153e-04,
    (True, (3, 10)): 4.1086e-04, (True, (1, 4)): 1.4253e-04,
}
BASIN_NP = {key: 16.0 if key[0] else 14.0 for key in END_NP}
BASIN_FAILS = {key: 20.0 if key[0] else 16.0 for key in END_NP}


def angle_bound(lens, pair):
    """The project's bound from tests/track_cases.py: the device may end at twice numpy's angle plus tol_rot."""
    return 2.0 * END_NP[(lens, pair)] + SETTINGS["tol_rot"]


@functools.lru_cache(maxsize=None)
def align_numpy(lens, pair, cells):
    c = case(lens)
    Q0 = start_off(true_pair(c, *pair), cells * CELL)
    return eio.pair_align(c["frames"], [pair], [Q0], c["lut"], c["calib"], SENSOR, skip_zero=True, **SETTINGS)


def end_angle(lens, pair, q):
    return float(eio.rotation_angle_between(true_pair(case(lens), *pair), q)[0])


# ---- the closing case: the out-and-back truth with a known drift added, DRIFT_CELLS cells per frame about OFF_AXIS, growing with the frame index — the shape
# of a tracker's error (tests/refit_cases.py: 0, 1.8, 2.7 ... 6 mrad), made thirty times as large: frame 11 is 11 * 0.35 = 3.85 cells (0.19 rad) off, so
# the pair (0, 11)... (2, 11) start inside the 14 cells measured above.  Candidates -> pairs -> the kept pairs -> graph with frame 0 the anchor; a pair's
# information takes io.PAIR_NOISE_FLOOR under its s^2, because frames f and 12 - f are the same bytes (s^2 = 0).  Measured with numpy: 44 candidates, all
# converged and kept; the worst angle to the truth falls from E_BEFORE_NP to E_AFTER_NP (rad), 350 times: numpy shows an improvement, so it is asserted.
DRIFT_CELLS = 0.35
CANDIDATES = dict(window=2, min_gap=2, max_angle=3.0 * CELL, max_per_frame=3)
MIN_OVERLAP = 0.3
E_BEFORE_NP = 1.8899e-01
E_AFTER_NP = 5.3559e-04
N_PAIRS_NP = 44
IMPROVES = (True,)


@functools.lru_cache(maxsize=None)
def drifted():
    c = case(False)
    q = np.array([so3.mul(so3.exp(f * DRIFT_CELLS * CELL * OFF_AXIS), c["q_true"][f]) for f in range(F)])
    status = np.array([1] + [2] * (F - 1), dtype=np.int32)
    q.setflags(write=False)
    status.setflags(write=False)
    return q, status


@functools.lru_cache(maxsize=None)
def closing_numpy():
    """candidates -> pair_align -> the kept pairs -> rotation_graph_solve, all in numpy, computed once."""
    c = case(False)
    q, status = drifted()
    pairs = eio.pair_candidates(q, status, **CANDIDATES)
    Q0, a, b = eio.pair_start(q, None, None, pairs)
    al = eio.pair_align(c["frames"], pairs, Q0, c["lut"], c["calib"], SENSOR, skip_zero=True, **SETTINGS)
    keep = closing_keep(al)
    info = eio.pair_information(al["sums"], al["counts"], floor=eio.PAIR_NOISE_FLOOR)
    g = eio.rotation_graph_solve(q, status, pairs[keep], al["q"][keep], info[keep])
    return dict(pairs=pairs, Q0=Q0, align=al, keep=keep, info=info, graph=g)


def closing_keep(al):
    ok = (al["status"] == eio.ALIGN_CONVERGED) | (al["status"] == eio.ALIGN_ITERATIONS)
    return ok & (al["counts"][:, 0] / float(SW * SH) >= MIN_OVERLAP)


def worst_angle(q):
    return float(eio.rotation_angle_between(case(False)["q_true"], q).max())


# ---- the graph alone: the closing case's kept edges.  Measured with numpy: the edge list permuted moves no frame by more than 5.6e-17 rad, and tol and
# cg_tol a hundred times tighter by nothing at all — below what the stopping rule determines: the solve ends on |delta|_inf < tol, so two correct solvers
# (numpy solves each step directly, the C entry by conjugate gradients to cg_tol) agree no closer than tol.  GRAPH_SPREAD is the larger of the two, tol; the
# C entry is held to ten times it.
GRAPH_PERMUTED_NP = 5.6e-17
GRAPH_SPREAD = max(GRAPH_PERMUTED_NP, eio.GRAPH_DEFAULTS["tol"])


def permuted(n):
    return (np.arange(n) * 7 + 3) % n if n % 7 else np.arange(n)[::-1]


if __name__ == "__main__":
    print("playroom D:", playroom_calibration()[1])
    for lens in (False, True):
        for pair in ALIGN_PAIRS:
            r = align_numpy(lens, pair, START_CELLS)
            e = end_angle(lens, pair, r["q"][0])
            basin = [cells for cells in BASIN_TRIED if end_angle(lens, pair, align_numpy(lens, pair, cells)["q"][0]) <= 2.0 * e + SETTINGS["tol_rot"]]
            print(f"lens {lens} pair {pair}: end {e:.4e} status {r['status'][0]} iters {r['iters'][0]} n {r['counts'][0, 0]} ends there from {basin}")
    r = closing_numpy()
    q, status = drifted()
    print("pairs", len(r["pairs"]), "kept", int(r["keep"].sum()), r["pairs"].tolist())
    print("status", r["align"]["status"].tolist(), "n", r["align"]["counts"][:, 0].tolist())
    print(f"before {worst_angle(q):.4e} after {worst_angle(r['graph']['q']):.4e} graph", {k: v for k, v in r["graph"].items() if k != "q"})
    keep = r["keep"]
    ed, Qe, info = r["pairs"][keep], r["align"]["q"][keep], r["info"][keep]
    p = permuted(len(ed))
    g1 = eio.rotation_graph_solve(q, status, ed[p], Qe[p], info[p])
    g2 = eio.rotation_graph_solve(q, status, ed, Qe, info, tol=1e-12, cg_tol=1e-12)
    print("spread", float(eio.rotation_angle_between(r["graph"]["q"], g1["q"]).max()), float(eio.rotation_angle_between(r["graph"]["q"], g2["q"]).max()))
