#!/usr/bin/env python3
"""The frame tracker with a per-frame exposure (emba_frames_track_exposure): what the two parameters more cost a frame.

The shape of scripts/track_timing.py: 240 x 180 frames on a 1024 x 2048 panorama, F = 100 frames rendered from a smooth plane along a slow trajectory (0.5 rad
of yaw over the call), every frame behind the first put under an exposure of its own (a* rising from 1 to 1.3, b* = -100 (a* - 1) bytes:
v <- clamp(rint((v - b*) / a*))), tracked from the first frame's true rotation under the schedules (0,) and (3,2,1,0) with batch 1 and batch 8.  Three calls
alternate inside one session: emba_frames_track, emba_frames_track_exposure with estimate = 0 (the same arithmetic in the 21-sum kernels) and with
estimate = 3.  Stream time between two HIP events: timer slot 0 brackets a whole call; with emba_enable_kernel_timing on, timer slot 7 brackets the call's
first evaluation kernel.  Every figure: the median of --reps calls after --warmup, with (min - max).  No ratio is asserted.  Needs the GPU; writes --out
(default profiles/track_exposure_timing.txt)."""
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
MIN_WEIGHT = 32      # (scripts/track_timing.py: the sensor's pixels are coarser than the panorama's cells here)
CALLS = ("emba_frames_track", "exposure, estimate 0", "exposure, estimate 3")


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
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "track_exposure_timing.txt"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("track_exposure_timing.py measures on the GPU: none is visible")
    F, S = a.frames, SW * SH
    out = [f"scripts/track_exposure_timing.py --reps {a.reps} --warmup {a.warmup} --frames {F}: median (min - max); {torch.cuda.get_device_name(0)}"]
    lut = pinhole_bearing_lut(SW, SH, 200.0, 200.0, 0.5 * (SW - 1), 0.5 * (SH - 1))
    m = LEGM(SW, SH, lut, 0.2, W, H)
    m.enable_kernel_timing(True)
    x, y = np.arange(W, dtype=np.float64)[None, :], np.arange(H, dtype=np.float64)[:, None]
    plane = 128.0 + 60.0 * np.sin(40.0 * np.pi * x / W) * np.cos(20.0 * np.pi * y / H) + 40.0 * np.cos(64.0 * np.pi * x / W + 3.0 * np.pi * y / H)
    traj = LinearTrajectory(np.array([so3.exp(np.array([0.0, 0.05 * i, 0.0])) for i in range(K)]), T0, DT)
    ts = T0 + (np.arange(F, dtype=np.int64) * ((K - 1) * DT - 1)) // max(F - 1, 1)
    frames = m.render_views(ts, traj.knots_xyzw, T0, DT, plane=plane, want_u8=True, lo=0.0, hi=255.0)["u8"]
    a_star = 1.0 + 0.3 * np.arange(F) / max(F - 1, 1)
    b_star = -100.0 * (a_star - 1.0)
    v = frames.reshape(F, -1).astype(np.float64)
    dist = np.where(v != 0.0, np.clip(np.rint((v - b_star[:, None]) / a_star[:, None]), 1.0, 255.0), 0.0).astype(np.uint8).reshape(frames.shape)
    dist[0] = frames[0]
    q_true = np.array([traj.evaluate(int(t)) for t in ts])
    out.append(f"== {SW}x{SH} frames on a {H}x{W} panorama, F = {F}, every frame under its own exposure (a* 1 ... 1.3, b* 0 ... -30 bytes); io.ALIGN_DEFAULTS, "
               f"min_weight {MIN_WEIGHT}, min_overlap 0.3, prediction on")
    kw = dict(q0=q_true[0], skip_zero=True, min_overlap=0.3, min_weight=MIN_WEIGHT)
    run = {CALLS[0]: lambda lv, b: m.track_frames(dist, ts, levels=lv, batch=b, **kw),
           CALLS[1]: lambda lv, b: m.track_frames_exposure(dist, ts, levels=lv, batch=b, estimate=0, **kw),
           CALLS[2]: lambda lv, b: m.track_frames_exposure(dist, ts, levels=lv, batch=b, estimate=3, **kw)}
    configs = [(lv, b, name) for lv in SCHEDULES for b in BATCHES for name in CALLS]
    whole, kern, info = ({c: [] for c in configs} for _ in range(3))
    for i in range(a.warmup + a.reps):
        for c in configs:      # alternating: every configuration sees the same session
            m.timer_start(0)
            r = run[c[2]](c[0], c[1])
            m.timer_stop(0)
            m.sync()
            if i >= a.warmup:
                whole[c].append(m.timer_ms(0) * 1e3)
                kern[c].append(m.timer_ms(7) * 1e3)
            info[c] = (r["tracked"], r["lost"], int(r["iters"].sum()) + (F - 1) * len(c[0]), float(eio.rotation_angle_between(q_true, r["q"]).max()),
                       float(np.abs(r["gain"] - a_star).max()) if "gain" in r else None)
    for lv in SCHEDULES:
        for b in BATCHES:
            out.append(f"  levels {','.join(map(str, lv))} batch {b}:")
            for name in CALLS:
                c = (lv, b, name)
                tracked, lost, evals, err, da = info[c]
                w = med(whole[c])
                out.append(f"    {name:22s} whole call {fmt(whole[c], 'us')}   {w / F:9.1f} us per frame   first evaluation kernel ({b} frame(s)) {fmt(kern[c], 'us')}")
                out.append(f"        {tracked} tracked, {lost} lost; {evals} frame evaluations: {w / evals:.1f} us of stream time each; worst angle to the truth {err:.3e} rad"
                           + ("" if da is None else f"; worst |a - a*| {da:.3e}"))
            k10, k21 = med(kern[(lv, b, CALLS[0])]), med(kern[(lv, b, CALLS[1])])
            out.append(f"    the 21-sum evaluation kernel is {k21 / k10:.2f} times the 10-sum one here (first evaluation kernel, estimate 0 against emba_frames_track)")
    m.close()
    text = "\n".join(out) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
