"""The cases of the coarse-to-fine pair alignment, shared by tests/test_pair_level_cpu.py (the numpy forms) and tests/test_gpu_pair_level.py (the
device against them): tests/pair_cases.py's geometry — 64 x 48 behind the wide pinhole, the out-and-back trajectory on the 128 x 64 panorama — on a plane
textured finely: the smooth plane of tests/mosaic_cases.py plus a ripple FINE_CELLS panorama cells long, so that level 0 alone is caught by the ripple's side
minima a few cells from the truth while a box-reduced level sees the smooth part.  Every figure below was measured with the numpy forms (python
tests/pair_level_cases.py prints them; the CPU test checks them); nothing comes from the device."""
import functools

import numpy as np

import mosaic_cases as MC
import pair_cases as PC
import refit_cases as RC
from emba_amd import io as eio

SENSOR, PANO, F, CELL = PC.SENSOR, PC.PANO, PC.F, PC.CELL
SW, SH = SENSOR
SETTINGS = dict(PC.SETTINGS)
SCHEDULE = (2, 1, 0)
PAIR = (3, 10)                       # tests/pair_cases.py's first pair: half a cell apart, on the way out and on the way back
FINE_CELLS = 6.0                     # the ripple's wavelength in panorama cells (about 9 sensor pixels, 2.4 pixels of level 2)
FINE_AMPLITUDE = 0.35                # ... and its amplitude in log intensity, beside the smooth plane's 0.8 and 0.3


def fine_plane():
    W, H = PANO
    x, y = np.arange(W, dtype=np.float64)[None, :], np.arange(H, dtype=np.float64)[:, None]
    k = 2.0 * np.pi / FINE_CELLS
    return MC.smooth_plane(PANO) + FINE_AMPLITUDE * np.sin(k * x + 0.7 * np.sin(k * y / 1.7)) * np.cos(k * y / 1.3)


@functools.lru_cache(maxsize=None)
def case():
    """frames uint8 [F, S] of the fine plane at tests/pair_cases.py's q_true, behind its pinhole.  Read-only."""
    W, H = PANO
    c = PC.case(False)
    inten = np.exp(fine_plane())
    lo, hi = float(inten.min()), float(inten.max())
    pm = np.array([eio.align_warp(c["lut"], q, W, H)[1] for q in c["q_true"]])
    views, outside = eio.render_views(inten, pm, with_outside=True)
    frames = eio.view_u8(views, lo, hi, outside=outside)
    frames.setflags(write=False)
    return dict(frames=frames, q_true=c["q_true"], ts=RC.times(F), lut=c["lut"], calib=PC.PINHOLE)


def start(cells):
    return PC.start_off(PC.true_pair(case(), *PAIR), cells * CELL)


def end_angle(q):
    return float(eio.rotation_angle_between(PC.true_pair(case(), *PAIR), q)[0])


@functools.lru_cache(maxsize=None)
def align_numpy(levels, cells, estimate=0, exposure=False):
    c = case()
    fr = exposure_frames() if exposure else c["frames"]
    return eio.pair_align_levels(fr, [PAIR], [start(cells)], c["lut"], c["calib"], SENSOR, levels=levels, estimate=estimate, skip_zero=True, **SETTINGS)


# ---- the basin.  END_NP: the angle (rad) between numpy's end at level 0 from a start one cell off and the truth.  A start "comes home" when it ends within
# angle_bound() of the truth, derived as tests/pair_cases.py's angle_bound: twice numpy's own end plus tol_rot.  BASIN_0 / BASIN_S: the largest start (cells)
# of BASIN_TRIED below the first one that does not come home, with level 0 alone and with SCHEDULE.  WIDENS: (True,) where numpy shows that the schedule ends
# at level 0's own end point from a start level 0 alone does not come home from — WIDE_CELLS is that start; () records that it does not.
BASIN_TRIED = (0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0, 8.0, 10.0, 12.0)
# Measured: level 0 alone comes home from 3 cells and ends 0.2 rad off from 4 (in a side minimum of the ripple); SCHEDULE comes home from every start tried,
# 12 cells among them, and ends within 2.4e-9 rad of level 0's own end point each time: numpy shows the widening, so it is asserted.
END_NP = 2.9839e-04
BASIN_0 = 3.0
BASIN_S = 12.0
WIDE_CELLS = 8.0
WIDENS = (True,)
SAME_END_NP = 2.402e-09              # the schedule's end against level 0's own end point (rad)


def angle_bound():
    return 2.0 * END_NP + SETTINGS["tol_rot"]


def basin(levels):
    home = [end_angle(align_numpy(levels, cells)["q"][0]) <= angle_bound() for cells in BASIN_TRIED]
    first_fail = home.index(False) if False in home else len(home)
    return (BASIN_TRIED[first_fail - 1] if first_fail else 0.0), home


# ---- the exposure.  The same frames with frame j = PAIR[1] under a gain and a bias the pair is not told: v_j <- rint(GAIN_J v_j + BIAS_J), chosen so that no
# byte saturates (the largest byte of the frame stays below 255, the smallest non-zero one above 0; zero stays zero: "no data").  The pair's relative exposure
# is then a = GAIN_J, b = BIAS_J (r = val_j - (a v_i + b)); it starts at a = 1, b = 0, EXPOSURE_CELLS off.  EXPOSURE_END: numpy's end angle with estimate = 0
# and with estimate = 3; EXPOSURE_AB: the recovered (a, b).  EXPOSURE_IMPROVES: (True,) where numpy shows the improvement.
GAIN_J, BIAS_J = 0.8, 20.0
EXPOSURE_CELLS = 1.0
# Measured: with estimate = 0 the schedule ends 2.3e-3 rad off (levels 2 and 1 use up their iterations); with estimate = 3 it ends 2.4e-4 rad off, inside
# angle_bound(), at a = 0.7966, b = 20.26 (the truth but for the rounding of frame j's bytes): numpy shows the improvement, so it is asserted.
EXPOSURE_END = {0: 2.3357e-03, 3: 2.4271e-04}
EXPOSURE_AB = (0.796601, 20.2566)
EXPOSURE_IMPROVES = (True,)
# How closely two correct loops agree on (a, b).  AB_SPREAD_NP: numpy's own spread at the end of the schedule under a permuted order of summation (permuted():
# the pixels of a level reversed and strided, summed in plain fp64 against np.longdouble in pixel order): none at all, the loop ends at a fixed point that
# both reach.  AB_LAST_STEP: |x_a|, |x_b| of numpy's last accepted step — what the stopping rule leaves undetermined, since converged tests the rotation
# alone: a loop that takes one trial more or less (tests/test_gpu_pair.py's allowance) ends that far away.  The device is held to AB_MARGIN times the larger.
AB_SPREAD_NP = (0.0, 0.0)
AB_LAST_STEP = (5.4e-10, 5.9e-08)
AB_MARGIN = 10.0


@functools.lru_cache(maxsize=None)
def exposure_frames():
    fr = case()["frames"].copy()
    v = fr[PAIR[1]].astype(np.float64)
    out = np.rint(GAIN_J * v + BIAS_J)
    assert out[v > 0].max() < 255.0 and out[v > 0].min() > 0.0      # no byte saturates: the model stays affine
    fr[PAIR[1]] = np.where(v > 0, out, 0.0).astype(np.uint8)
    fr.setflags(write=False)
    return fr


def permuted(n):
    return np.concatenate([np.arange(n)[::-1][k::7] for k in range(7)])


def ab_bound():
    return tuple(AB_MARGIN * max(s, x) for s, x in zip(AB_SPREAD_NP, AB_LAST_STEP))


if __name__ == "__main__":
    r = align_numpy((0,), 1.0)
    e = end_angle(r["q"][0])
    print(f"END_NP = {e:.4e} (status {r['status'][0]}, iters {r['iters'][0]}, n {r['counts'][0, 0]})")
    for lv in ((0,), SCHEDULE):
        b, home = basin(lv)
        ends = [end_angle(align_numpy(lv, cells)["q"][0]) for cells in BASIN_TRIED]
        print(f"levels {lv}: basin {b} cells; home {dict(zip(BASIN_TRIED, home))}; ends {[f'{x:.2e}' for x in ends]}")
        print("   level status", [align_numpy(lv, cells)["level_status"][0].tolist() for cells in BASIN_TRIED])
    for cells in BASIN_TRIED:
        q0, qs = align_numpy((0,), 1.0)["q"][0], align_numpy(SCHEDULE, cells)["q"][0]
        print(f"   {cells}: schedule's end against level 0's own end point {float(eio.rotation_angle_between(q0, qs)[0]):.3e}")
    fr = exposure_frames()
    for est in (0, 3):
        x = align_numpy(SCHEDULE, EXPOSURE_CELLS, est, True)
        print(f"exposure, estimate {est}: end {end_angle(x['q'][0]):.4e} a {x['gain'][0]:.6f} b {x['bias'][0]:.4f} status {x['level_status'][0].tolist()} iters {x['level_iters'][0].tolist()}")
    c = case()
    kw = dict(levels=SCHEDULE, estimate=3, skip_zero=True, **SETTINGS)
    x = align_numpy(SCHEDULE, EXPOSURE_CELLS, 3, True)
    y = eio.pair_align_levels(fr, [PAIR], [start(EXPOSURE_CELLS)], c["lut"], c["calib"], SENSOR, order=permuted, **kw)
    print("last accepted step", x["last_x"][0].tolist())
    print(f"spread under a permuted summation: a {abs(x['gain'][0] - y['gain'][0]):.3e} b {abs(x['bias'][0] - y['bias'][0]):.3e} "
          f"angle {float(eio.rotation_angle_between(x['q'], y['q'])[0]):.3e} iters {x['level_iters'][0].tolist()} / {y['level_iters'][0].tolist()}")
