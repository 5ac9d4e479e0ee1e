#!/usr/bin/env python3
"""Intensity frames tracked against their own growing mosaic (emba_frames_track): what a frame costs, and what a batch of one costs.

240 x 180 frames on a 1024 x 2048 panorama, F = 100 frames rendered from a smooth plane along the slow trajectory of scripts/align_timing.py (0.5 rad of yaw
over the call), tracked from the first frame's true rotation under the schedules (0,) and (3,2,1,0) with batch 1 and batch 8.  Stream time between two HIP
events: timer slot 0 brackets a whole call (uploads, every launch, the 4-byte reads that end the loops, the downloads); with emba_enable_kernel_timing on,
timer slot 7 brackets the call's first evaluation kernel — of one frame with batch 1, of eight with batch 8, at the schedule's first level.  Every figure:
the median of --reps calls after --warmup, with (min - max); the four configurations alternate inside one session.  Beside them §20's evaluation kernel
(emba_frames_align_eval against the tracked mosaic's mean) on the same 100 frames, and the number of evaluations a call made (every frame's trials plus one
first evaluation per level), which gives the stream time per evaluation.  No ratio is asserted.  Needs the GPU; writes --out (default
profiles/track_timing.txt)."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from emba_amd import LEGM                                            # noqa: E402
from emba_amd import io as eio                                       # noqa: E402
from emba_amd import so3                                             # noqa: E402
from emba_amd.legm import LinearTrajectory                           # noqa: E402
from emba_amd.synth import pinhole_bearing_lut                       # noqa: E402

SW, SH, W, H = 240, 180, 2048, 1024
K, T0, DT = 11, 10**9, 10**8
SCHEDULES = ((0,), (3, 2, 1, 0))
BATCHES = (1, 8)
# The sensor's pixels are coarser than the panorama's cells here (240 pixels across some 350 cells): a frame leaves about 120 units of weight in a level-0
# cell, so "one pixel's worth" (256) would mask level 0 altogether and lose every frame.  An eighth of a pixel's worth covers it.
MIN_WEIGHT = 32


def fmt(v, unit):
    v = sorted(v)
    return f"{v[len(v) // 2]:10.1f} {unit} ({v[0]:.1f} - {v[-1]:.1f})"


def med(v):
    return sorted(v)[len(v) // 2]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--frames", type=int, default=100)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "track_timing.txt"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("track_timing.py measures on the GPU: none is visible")
    F, S = a.frames, SW * SH
    out = [f"scripts/track_timing.py --reps {a.reps} --warmup {a.warmup} --frames {F}: median (min - max); {torch.cuda.get_device_name(0)}"]
    lut = pinhole_bearing_lut(SW, SH, 200.0, 200.0, 0.5 * (SW - 1), 0.5 * (SH - 1))
    m = LEGM(SW, SH, lut, 0.2, W, H)
    m.enable_kernel_timing(True)
    x, y = np.arange(W, dtype=np.float64)[None, :], np.arange(H, dtype=np.float64)[:, None]
    plane = 128.0 + 60.0 * np.sin(40.0 * np.pi * x / W) * np.cos(20.0 * np.pi * y / H) + 40.0 * np.cos(64.0 * np.pi * x / W + 3.0 * np.pi * y / H)
    traj = LinearTrajectory(np.array([so3.exp(np.array([0.0, 0.05 * i, 0.0])) for i in range(K)]), T0, DT)
    ts = T0 + (np.arange(F, dtype=np.int64) * ((K - 1) * DT - 1)) // max(F - 1, 1)
    frames = m.render_views(ts, traj.knots_xyzw, T0, DT, plane=plane, want_u8=True, lo=0.0, hi=255.0)["u8"]
    q_true = np.array([traj.evaluate(int(t)) for t in ts])
    out.append(f"== {SW}x{SH} frames on a {H}x{W} panorama, F = {F}, {F * -(-S // 256)} workgroups over all frames; io.ALIGN_DEFAULTS (max_iters 30, tol_rot 1e-6), "
               f"min_weight {MIN_WEIGHT}, min_overlap 0.3, prediction on")
    configs = [(lv, b) for lv in SCHEDULES for b in BATCHES]
    whole, kern, info = ({c: [] for c in configs} for _ in range(3))
    for i in range(a.warmup + a.reps):
        for c in configs:      # alternating: every configuration sees the same session
            m.timer_start(0)
            r = m.track_frames(frames, ts, q0=q_true[0], levels=c[0], batch=c[1], skip_zero=True, min_overlap=0.3, min_weight=MIN_WEIGHT)
            m.timer_stop(0)
            m.sync()
            if i >= a.warmup:
                whole[c].append(m.timer_ms(0) * 1e3)
                kern[c].append(m.timer_ms(7) * 1e3)
            info[c] = (r["tracked"], r["lost"], int(r["iters"].sum()) + (F - 1) * len(c[0]), float(eio.rotation_angle_between(q_true, r["q"]).max()), r["iters"].sum(axis=0).tolist())
    for c in configs:
        tracked, lost, evals, err, iters = info[c]
        w = med(whole[c])
        out.append(f"  levels {','.join(map(str, c[0])):8s} batch {c[1]}: whole call {fmt(whole[c], 'us')}   {w / F:9.1f} us per frame   first evaluation kernel ({c[1]} frame(s)) {fmt(kern[c], 'us')}")
        out.append(f"      {tracked} tracked, {lost} lost; {evals} frame evaluations (trials per level {iters}): {w / evals:.1f} us of stream time per frame evaluation; "
                   f"worst angle to the truth {err:.3e} rad")
    # §20's evaluation kernel on the same pixels: all F frames in one launch against the tracked mosaic's mean
    k20, w20 = [], []
    for i in range(a.warmup + a.reps):
        m.timer_start(0)
        m.align_frames_eval(frames, q_true, use_mosaic=True, min_weight=MIN_WEIGHT, skip_zero=True)
        m.timer_stop(0)
        m.sync()
        if i >= a.warmup:
            k20.append(m.timer_ms(7) * 1e3)
            w20.append(m.timer_ms(0) * 1e3)
    out.append(f"== beside them, §20 on the same pixels: emba_frames_align_eval(use_mosaic) of all {F} frames in one launch: evaluation kernel {fmt(k20, 'us')}   "
               f"whole call {fmt(w20, 'us')}   {med(k20) / F:.2f} us per frame")
    m.close()
    text = "\n".join(out) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
