"""The cases of the frame-mosaic tests, shared by tests/test_mosaic_cpu.py (the numpy forms) and tests/test_gpu_mosaic.py (the device
against them): the sensors, panoramas, trajectories and frame times of tests/view_cases.py, which keep clear of the pole rows, and frames made by
io.render_views and io.view_u8 of exp of a smooth plane — so a mosaic of them, taken back through the logarithm, should show that plane again."""
import functools

import numpy as np

import view_cases as VC
from emba_amd import io as eio

SENSORS, PANOS, KINDS, FRAMES = VC.SENSORS, VC.PANOS, VC.KINDS, VC.FRAMES
# the end-to-end cases: (sensor, panorama) pairs on which the correlation bound of 0.95 was measured with the rule in numpy (min_weight = 256)
E2E_SMALL = tuple((s, p) for s in ((20, 13), (16, 12)) for p in ((48, 24), (32, 16)))
E2E_LARGE = (((64, 48), (128, 64)), ((64, 48), (256, 128)))      # 64 x 48 behind the 90 degree pinhole of VC.lut_of
E2E_MIN_CORRELATION = 0.95


def smooth_plane(pano):
    """The log-intensity plane 0.8 sin(4 pi x / W) cos(2 pi y / H) + 0.3 cos(6 pi x / W): periodic in x, as the panorama is."""
    W, H = pano
    x, y = np.arange(W, dtype=np.float64)[None, :], np.arange(H, dtype=np.float64)[:, None]
    return 0.8 * np.sin(4.0 * np.pi * x / W) * np.cos(2.0 * np.pi * y / H) + 0.3 * np.cos(6.0 * np.pi * x / W)


def backward_differences(P):
    """The gradient map of a plane without holes: io.gradient_from_plane with every cell covered."""
    return eio.gradient_from_plane(P, np.ones(P.shape, dtype=bool))


@functools.lru_cache(maxsize=None)
def case(sensor, pano, kind, F):
    """The frames of one case, computed once: a dict of frames uint8 [F, S], ts, knots, pm (numpy's own) [F, S, 2], the intensity plane I = exp(P) the
    frames were sampled from, and the tone lo / hi = min / max of I.  Pixels outside the panorama hold the byte 0.  Read-only."""
    W, H = pano
    P = smooth_plane(pano)
    inten = np.exp(P)
    lo, hi = float(inten.min()), float(inten.max())
    ts, knots = VC.frame_times(F), VC.knots_of(kind)
    pm = eio.view_pm(VC.lut_of(sensor), knots, VC.T0_NS, VC.DT_NS, ts, W, H)
    views, outside = eio.render_views(inten, pm, with_outside=True)
    frames = eio.view_u8(views, lo, hi, outside=outside)
    for a in (P, inten, ts, knots, pm, frames):
        a.setflags(write=False)
    return dict(frames=frames, ts=ts, knots=knots, pm=pm, P=P, I=inten, lo=lo, hi=hi, outside=int(outside.sum()))


def correlation(G, G_ref, both):
    """Pearson correlation of the gradient pairs (Gx, Gy) G and G_ref over the cells of the mask `both`, x and y components together."""
    a = np.concatenate([G[0][both], G[1][both]])
    b = np.concatenate([G_ref[0][both], G_ref[1][both]])
    return float(np.corrcoef(a, b)[0, 1])


def gradient_mask(covered):
    """The cells where a backward difference of a plane with the holes ~covered is a difference at all: the cell and its left neighbour (wrapped), the
    cell and the one above it.  Returns the mask where both differences exist."""
    cov = np.asarray(covered).astype(bool)
    up = np.zeros_like(cov)
    up[1:] = cov[:-1]
    return cov & np.roll(cov, 1, axis=1) & up
