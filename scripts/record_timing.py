"""record_data's map images (EMBA::saveEvoData / saveOptData, solver.cpp:370-479): what one set costs on the device and on the host route, and what
recording costs an LM loop.  One GPU run:
  1. LEGM.renderMapImages at 1024 x 2048 and 2048 x 4096, with and without Poisson: HIP events on the context's stream around the call (kernels +
     the images' device -> host copies) and the host clock;
  2. the host route it replaces: downloadMap + reconstructIntensity() + io.normalize_robust x 3 + the HSV image in numpy;
  3. the city shape's LM loop (10 M events, K = 97, 640 x 480 sensor, 1024 x 2048) with and without a MapRecorder (PNG level 1, 2 writer threads).
    python scripts/record_timing.py [reps] [lm_iters]
With PROF=1: only step 1 (a few calls per shape), for rocprofv3 --kernel-trace --stats."""
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from emba_amd import LEGM, io as eio                                   # noqa: E402
from emba_amd.synth import make_workload, pinhole_bearing_lut          # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
lm_iters = int(sys.argv[2]) if len(sys.argv) > 2 else 6
prof = os.environ.get("PROF") == "1"


def host_hsv(gx, gy):
    a = np.arctan2(gy, gx) * (180.0 / np.pi)
    half = 0.5 * np.where(a < 0, a + 360.0, a)
    mag = np.sqrt(gx * gx + gy * gy)
    def mm(v, s_):
        mn, mx = v.min(), v.max()
        s = s_ * (1.0 / (mx - mn)) if mx - mn > np.finfo(float).eps else 0.0
        return np.clip(np.rint(v * s + (0.0 - mn * s)), 0, 255).astype(np.uint8)
    H, V = mm(half, 179.0), mm(mag, 255.0)
    f = np.float32
    h = H.astype(f) * (f(6) / f(180)); v = V.astype(f) * (f(1) / f(255)); s = f(255) * (f(1) / f(255))
    sec = np.floor(h); h = h - sec; sec = sec.astype(np.int64) % 6
    tab = np.stack([v, v * (1 - s), v * (1 - s * h), v * (1 - s * (1 - h))])
    sd = np.array([[1, 3, 0], [1, 0, 2], [3, 0, 1], [0, 2, 1], [0, 1, 3], [2, 1, 0]])[sec]
    return np.stack([np.clip(np.rint(np.take_along_axis(tab, sd[None, ..., c], 0)[0] * f(255)), 0, 255).astype(np.uint8) for c in (2, 1, 0)], -1)


def med(xs):
    return float(np.median(xs))


for ph in (1024, 2048):
    pw = 2 * ph
    rng = np.random.default_rng(ph)
    gx = rng.standard_cauchy((ph, pw)) * 1e-2
    gy = rng.standard_cauchy((ph, pw)) * 1e-2
    gx[rng.random(gx.shape) < 0.3] = 0.0
    gy[gx == 0.0] = 0.0
    m = LEGM(8, 8, pinhole_bearing_lut(8, 8, 10, 10, 4, 4), 0.2, pw, ph)
    m.upload_map(gx, gy)
    m.sync()
    for poisson in (False, True):
        for _ in range(3):
            m.renderMapImages(0.1, poisson)
        if prof:
            continue
        ev, wall = [], []
        for _ in range(reps):
            t0 = time.perf_counter()
            m.timer_start(0)
            m.renderMapImages(0.1, poisson)
            m.timer_stop(0)
            ev.append(m.timer_ms(0))
            wall.append((time.perf_counter() - t0) * 1e3)
        print(f"{ph}x{pw} renderMapImages poisson={poisson}: {med(ev):.3f} ms (HIP events, median of {reps}), {med(wall):.3f} ms host clock", flush=True)
    if prof:
        m.close()
        continue
    t = []
    for _ in range(3):
        t0 = time.perf_counter()
        a, b = m.downloadMap()
        M = m.reconstructIntensity()
        imgs = (eio.normalize_robust(a), eio.normalize_robust(b), host_hsv(a, b), eio.normalize_robust(M))
        t.append((time.perf_counter() - t0) * 1e3)
    print(f"{ph}x{pw} host route (downloadMap + reconstructIntensity + normalize_robust x3 + numpy HSV): {med(t):.1f} ms (median of 3)", flush=True)
    dev = m.renderMapImages(0.1, True)
    print(f"   same images as the host route: Gx {np.array_equal(dev['Gx'], imgs[0])}, Gy {np.array_equal(dev['Gy'], imgs[1])}, "
          f"map_poisson {np.array_equal(dev['map_poisson'], imgs[3])}, G_hsv pixels differing {int((dev['G_hsv'] != imgs[2]).any(-1).sum())}", flush=True)
    m.close()

if not prof and lm_iters > 0:
    from emba_amd.solver import BASettings, LMSettings, MapRecorder, solve_time_window
    from test_lm_solver_cpu import perturbed
    t0 = time.perf_counter()
    w = make_workload(n_events=10_000_000, pano_h=1024, K=97, sensor=(640, 480), focal=200.0 * 640 / 240.0, yaw_rate=0.1)
    init = perturbed(w, 0.002)
    print(f"city shape: {w.events.size()} events, K = {w.K}, {w.pano_h}x{w.pano_w} (generated in {time.perf_counter() - t0:.0f} s)", flush=True)
    m = LEGM(w.sensor_w, w.sensor_h, w.lut, w.C_th, w.pano_w, w.pano_h)
    lm = LMSettings(max_num_iter=lm_iters)
    solve_time_window(m, init, w.events, w.Gx, w.Gy, BASettings(), LMSettings(max_num_iter=1), resident=True)      # warm-up: buffers, code objects
    with tempfile.TemporaryDirectory() as d:
        for label in ("plain", "record", "plain", "record"):
            rec = MapRecorder(os.path.join(d, label)) if label == "record" else None
            t0 = time.perf_counter()
            r = solve_time_window(m, init, w.events, w.Gx, w.Gy, BASettings(), lm, resident=True, map_recorder=rec)
            dt = (time.perf_counter() - t0) * 1e3
            msg = f"   LM loop {label:6s}: {r.iterations} iterations in {dt:.1f} ms ({dt / max(r.iterations, 1):.2f} ms per iteration)"
            if rec is not None:
                t1 = time.perf_counter()
                rec.close()
                sm = rec.summary()
                msg += (f"; {sm['sets']} sets, render {sm['render_s'] * 1e3:.1f} ms in the loop, encode + write {sm['encode_s'] * 1e3:.1f} ms on the writers, "
                        f"close() waited {(time.perf_counter() - t1) * 1e3:.1f} ms")
            print(msg, flush=True)
