"""The cases of the appearance search, shared by tests/test_match_cpu.py (the numpy forms) and tests/test_gpu_match.py (the device against
them): tests/pair_cases.py's geometry — 64 x 48 behind the wide pinhole, F = 12 out and back on the 128 x 64 panorama — on tests/pair_level_cases.py's
rippled plane, with a drift per frame so large that io.pair_candidates, at the driver's default close_angle, proposes no pair beyond the window: what the
appearance search is for.  Every figure below was measured with the numpy forms (python tests/match_cases.py prints them; the CPU test checks them); nothing
comes from the device."""
import functools

import numpy as np

import pair_cases as PC
import pair_level_cases as LC
from emba_amd import io as eio
from emba_amd import so3

SENSOR, PANO, F, CELL = PC.SENSOR, PC.PANO, PC.F, PC.CELL
SW, SH = SENSOR
SETTINGS = dict(PC.SETTINGS)
# the driver's defaults (driver.SequenceSettings): what "rotations" searches with
WINDOW, GAP, ANGLE, PER_FRAME, MIN_OVERLAP = 1, 4, 0.2, 2, 0.3
SCHEDULE = LC.SCHEDULE               # (2, 1, 0): §27's basin of 12 cells takes a start that is a level pixel or two off
# The drift: DRIFT_CELLS panorama cells per frame about tests/pair_cases.py's OFF_AXIS, growing with the frame index, as its closing case has it — but 1.5
# cells where that has 0.35: two frames more than GAP apart then differ by 7.5 cells of drift at the least, the nearest such pair is 0.256 rad apart as
# tracked, and none is within ANGLE (at 1.2 cells one pair, (6, 11), still is).  Frame 11 is 16.5 cells (0.81 rad) off.
DRIFT_CELLS = 1.5
# the search: level 2 is 16 x 12 (a level pixel is 4 pixels, 0.125 rad at the centre of this camera), level 1 is 32 x 24
RANGE = {1: (12, 8), 2: (6, 4)}
SCORE_MIN = 0.5                      # the signed square of the correlation: r = 0.71
N_MIN = {1: 32 * 24 // 4, 2: 16 * 12 // 4}      # a quarter of the thumbnail
K = 2
TRUE_ANGLE = 3.0 * CELL              # a true loop pair: more than GAP apart and within this angle in truth


def case():
    return LC.case()


@functools.lru_cache(maxsize=None)
def drifted():
    c = case()
    q = np.array([so3.mul(so3.exp(f * DRIFT_CELLS * CELL * PC.OFF_AXIS), c["q_true"][f]) for f in range(F)])
    status = np.array([1] + [2] * (F - 1), dtype=np.int32)
    q.setflags(write=False)
    status.setflags(write=False)
    return q, status


def frames3():
    return case()["frames"].reshape(F, SH, SW)


@functools.lru_cache(maxsize=None)
def true_loops():
    """the pairs i < j more than GAP apart whose true relative rotation is below TRUE_ANGLE, sorted"""
    c = case()
    return tuple((i, j) for i in range(F) for j in range(i + GAP + 1, F)
                 if float(eio.rotation_angle_between(c["q_true"][i], c["q_true"][j])[0]) <= TRUE_ANGLE)


@functools.lru_cache(maxsize=None)
def search_numpy(level, k=K):
    rx, ry = RANGE[level]
    r = eio.match_search(frames3(), drifted()[1], level=level, rx=rx, ry=ry, min_gap=GAP, skip_zero=True, n_min=N_MIN[level], score_min=SCORE_MIN, k=k)
    for v in r.values():
        v.setflags(write=False)
    return r


def start_error(level, pair, shift):
    """the angle (rad) between match_start of a found shift and the true relative rotation of the pair"""
    cal = case()["calib"]
    Q = eio.match_start(shift[0], shift[1], level, cal["fu"], cal["fv"], cal["cu"], cal["cv"], SW, SH)
    return float(eio.rotation_angle_between(PC.true_pair(case(), *pair), Q)[0])


def closing_pairs(mode, level=2):
    """(pairs, source, Q0, match score, match shift) as driver.close_tracked_frames forms them: the window's neighbours, the angle candidates of
    "rotations" and "both", the matched pairs of "appearance" and "both" (started from match_start unless the rotations propose them too)."""
    c = case()
    q, status = drifted()
    cal = c["calib"]
    win = {tuple(p) for p in eio.pair_candidates(q, status, window=WINDOW, min_gap=GAP, max_angle=ANGLE, max_per_frame=0).tolist()}
    rot = {tuple(p) for p in eio.pair_candidates(q, status, window=WINDOW, min_gap=GAP, max_angle=ANGLE, max_per_frame=PER_FRAME).tolist()} if mode != "appearance" else set(win)
    app = {}
    if mode != "rotations":
        mp, ms, md = eio.match_pairs(search_numpy(level), with_info=True)
        app = {tuple(p): (s, d) for p, s, d in zip(mp.tolist(), ms, md)}
    pairs = np.array(sorted(win | rot | set(app)), dtype=np.int32).reshape(-1, 2)
    source = np.array([0 if tuple(p) in win else 1 if tuple(p) in rot else 2 for p in pairs.tolist()], dtype=np.int32)
    Q0 = eio.pair_start(q, None, None, pairs)[0]
    score, shift = np.full(len(pairs), eio.MATCH_UNSCORED), np.zeros((len(pairs), 2), np.int32)
    for n, p in enumerate(pairs.tolist()):
        if tuple(p) in app:
            score[n], shift[n] = app[tuple(p)]
            if source[n] == 2:
                Q0[n] = eio.match_start(shift[n, 0], shift[n, 1], level, cal["fu"], cal["fv"], cal["cu"], cal["cv"], SW, SH)
    return pairs, source, Q0, score, shift


@functools.lru_cache(maxsize=None)
def closing_numpy(mode, level=2):
    """pairs -> pair_align_levels over SCHEDULE -> the kept pairs -> rotation_graph_solve, all in numpy, computed once per mode"""
    c = case()
    q, status = drifted()
    pairs, source, Q0, score, shift = closing_pairs(mode, level)
    al = eio.pair_align_levels(c["frames"], pairs, Q0, c["lut"], c["calib"], SENSOR, levels=SCHEDULE, estimate=0, skip_zero=True, **SETTINGS)
    ok = (al["status"] == eio.ALIGN_CONVERGED) | (al["status"] == eio.ALIGN_ITERATIONS)
    keep = ok & (al["counts"][:, 0] >= MIN_OVERLAP * SW * SH) & (al["level_status"][:, -1] != 0)
    info = eio.pair_information(al["sums"][:, list(eio.EXPOSURE_SHARED)], al["counts"], floor=eio.PAIR_NOISE_FLOOR)
    g = eio.rotation_graph_solve(q, status, pairs[keep], al["q"][keep], info[keep])
    return dict(pairs=pairs, source=source, Q0=Q0, align=al, keep=keep, graph=g)


def worst_angle(q):
    return float(eio.rotation_angle_between(case()["q_true"], q).max())


# ---- what numpy measured (python tests/match_cases.py)
# (a) the finding.  ROTATION_LOOPS: the pairs beyond the window that io.pair_candidates proposes from the drifted rotations at the driver's defaults: none.
# 28 pairs are true loops (more than GAP apart, within TRUE_ANGLE in truth).  At level 1 and at level 2 alike the search hands on N_MATCHED = 17 pairs, every
# one a true loop; three of them, (1, 11), (2, 10), (3, 9), are frames f and 12 - f, the same bytes (score exactly 1 at shift (0, 0)): they show the tie rule
# and are no evidence of finding; N_DISTINCT = 14 are.  Their shifts are 0 ... 3 level pixels in x at level 1 (one in y for the pairs 2 cells and more
# apart), 0 or 1 at level 2; START_ERROR: the worst angle between match_start of a matched pair and its true relative rotation, in cells — inside §27's basin
# of 12 cells.  numpy shows that appearance finds loops where the rotations find none: it is asserted.
# (b) the closing.  Worst angle to the truth (rad): E_BEFORE as tracked; E_ROTATIONS behind close_tracked_frames' pipeline with "rotations" (the 11 window
# pairs alone: a chain, whose alignment errors add up along it); E_APPEARANCE with "appearance" at level 2 (28 pairs, 25 kept: three matched pairs end
# stalled and are dropped by the gate).  "both" is "appearance" here, since the rotations add nothing.  numpy shows the improvement, 3.6 times: its direction
# is asserted.
ROTATION_LOOPS = 0
N_TRUE_LOOPS = 28
N_MATCHED = {1: 17, 2: 17}
N_DISTINCT = {1: 14, 2: 14}
SAME_BYTES = ((1, 11), (2, 10), (3, 9))
START_ERROR = {1: 1.04, 2: 1.21}
FINDS = (True,)
E_BEFORE = 8.0994e-01
E_ROTATIONS = 1.1674e-03
E_APPEARANCE = 3.2792e-04
N_PAIRS = {"rotations": 11, "appearance": 28, "both": 28}
N_KEPT = {"rotations": 11, "appearance": 25, "both": 25}
IMPROVES = (True,)


if __name__ == "__main__":
    q, status = drifted()
    rot = eio.pair_candidates(q, status, window=WINDOW, min_gap=GAP, max_angle=ANGLE, max_per_frame=PER_FRAME)
    beyond = [tuple(p) for p in rot.tolist() if p[1] - p[0] > WINDOW]
    print("drift per frame", DRIFT_CELLS, "cells; rotation candidates beyond the window:", beyond)
    ang = eio.rotation_angle_between
    print("smallest tracked angle beyond the gap:", min(float(ang(q[i], q[j])[0]) for i in range(F) for j in range(i + GAP + 1, F)))
    print("true loops", true_loops())
    for level in (1, 2):
        r = search_numpy(level)
        mp, ms, md = eio.match_pairs(r, with_info=True)
        print(f"level {level}, range {RANGE[level]}, n_min {N_MIN[level]}: partner\n{r['partner'].T}\nscore\n{np.round(r['score'].T, 3)}")
        for p, s, d in zip(mp.tolist(), ms, md):
            t = float(ang(case()['q_true'][p[0]], case()['q_true'][p[1]])[0])
            print(f"   pair {tuple(p)} score {s:.4f} shift {tuple(d)} true angle {t / CELL:.2f} cells; start off by {start_error(level, tuple(p), d) / CELL:.2f} cells"
                  f"{' (true loop)' if tuple(p) in true_loops() else ''}")
    print(f"before: worst angle {worst_angle(q):.4e}")
    for mode in ("rotations", "appearance", "both"):
        r = closing_numpy(mode)
        print(f"{mode}: {len(r['pairs'])} pairs, sources {np.bincount(r['source'], minlength=3).tolist()}, kept {int(r['keep'].sum())}; status {r['align']['status'].tolist()}; "
              f"worst angle {worst_angle(r['graph']['q']):.4e}; graph end {r['graph']['end']}")
