"""The cases of the frame-alignment tests, shared by tests/test_align_cpu.py (the numpy forms) and tests/test_gpu_align.py (the device against
them): the trajectories and frame times of tests/view_cases.py, the smooth plane of tests/mosaic_cases.py, frames made by io.render_views and io.view_u8 of
exp of that plane at the TRUE rotations, and start rotations that are the true ones turned by a fixed-seed perturbation about random axes."""
import functools

import numpy as np

import mosaic_cases as MC
import view_cases as VC
from emba_amd import io as eio
from emba_amd import so3

SENSORS = ((7, 5), (20, 13), (64, 48))      # a partial wave; 260 pixels: they cross a 256-lane workgroup; 12 workgroups per frame: the reduction across them runs
PANOS = ((32, 16), (48, 24), (128, 64))
KINDS, FRAMES = VC.KINDS, VC.FRAMES
PERTURB = 0.03                              # rad: the angle every start rotation is turned by (chosen on the CPU, tests/test_align_cpu.py)
SETTINGS = dict(max_iters=100, lambda0=1e-3, lambda_up=10.0, lambda_down=10.0, lambda_min=1e-9, lambda_max=1e6, tol_rot=1e-7, min_pixels=16, huber_k=0.0)

# The convergence cases: the (sensor, panorama) pairs on which the numpy form alone, from PERTURB, ends every frame of every kind converged or stalled and
# closer to the truth than it started, with F = CONVERGENCE_F frames: all nine (0.02, 0.03 and 0.05 rad were tried; the final angles are the same for all
# three, and at 0.03 every frame ends converged within 42 trials).  E_NP: numpy's worst final angle to the truth (rad) over the kinds and frames of the pair
# — the measured yardstick of tests/test_gpu_align.py, which allows the device 2 E_NP + tol_rot.  What is left of the angle is the bytes' quantisation, seen
# through few pixels: the 7 x 5 sensor's 35 pixels leave ten times the angle of the 64 x 48 sensor's 3072.
CONVERGENCE_F = 3
E_NP = {
    ((7, 5), (32, 16)): 1.7413e-03,
    ((7, 5), (48, 24)): 2.3507e-03,
    ((7, 5), (128, 64)): 6.1177e-04,
    ((20, 13), (32, 16)): 3.8843e-04,
    ((20, 13), (48, 24)): 3.8661e-04,
    ((20, 13), (128, 64)): 4.5361e-04,
    ((64, 48), (32, 16)): 1.2001e-04,
    ((64, 48), (48, 24)): 1.3462e-04,
    ((64, 48), (128, 64)): 1.4191e-04,
}
# ... and for the route through the mosaic: frames stitched at the true rotations, then aligned to the mosaic's mean under its covered cells from PERTURB
MOSAIC_PAIR = ((64, 48), (128, 64))
E_NP_MOSAIC = 2.6291e-03      # (the mosaic's 16ths-of-a-cell votes blur the plane: twenty times the angle of the plane itself)


def true_rotations(kind, ts):
    """The spline of VC.knots_of(kind) at the frame times: q [F, 4]."""
    knots = VC.knots_of(kind)
    return np.array([so3.spline_evaluate(knots, VC.T0_NS, VC.DT_NS, int(t)) for t in ts])


def perturbed(q_true, angle=PERTURB, seed=20):
    """Every rotation turned by `angle` about an axis of its own, drawn with a fixed seed: exp(angle axis) (x) q."""
    rng = np.random.default_rng(seed)
    axes = rng.standard_normal((len(q_true), 3))
    axes /= np.linalg.norm(axes, axis=1)[:, None]
    return np.array([so3.mul(so3.exp(angle * a), q) for a, q in zip(axes, q_true)])


def holed_mask(pano, seed=5):
    """A valid plane with holes: one block of 0 a sixth of the panorama wide around the middle row, and one cell in sixteen at random."""
    W, H = pano
    valid = np.random.default_rng(seed).random((H, W)) >= 1.0 / 16.0
    valid[H // 2 - 1:H // 2 + 2, W // 2:W // 2 + W // 6] = False
    return valid


@functools.lru_cache(maxsize=None)
def case(sensor, pano, kind, F):
    """One case, computed once: a dict of frames uint8 [F, S] rendered at q_true [F, 4], q_start [F, 4], the intensity plane I = exp(P) the frames were
    sampled from (the plane they are aligned to), its tone lo / hi, the mask `valid` and the lut.  Read-only."""
    c = MC.case(sensor, pano, kind, F)
    q_true = true_rotations(kind, c["ts"])
    q_start = perturbed(q_true)
    valid = holed_mask(pano)
    lut = VC.lut_of(sensor)
    for a in (q_true, q_start, valid, lut):
        a.setflags(write=False)
    return dict(frames=c["frames"], q_true=q_true, q_start=q_start, I=c["I"], lo=c["lo"], hi=c["hi"], valid=valid, lut=lut, ts=c["ts"])


def huber_split(c):
    """A huber_k that splits the residuals of the case at its start rotations: their median magnitude over the first frame's used pixels (0.05 where there
    are none)."""
    H, W = c["I"].shape
    pm = eio.align_warp(c["lut"], c["q_start"][0], W, H)[1]
    t = eio.align_terms(c["frames"][0], pm, c["lut"], c["q_start"][0], c["I"], None, c["lo"], c["hi"])
    r = np.abs(t["r"][t["cls"] == eio.ALIGN_USED])
    return float(np.median(r)) if r.size and np.median(r) > 0 else 0.05
