#!/usr/bin/env python3
"""Tracked frames refitted against the mosaic of the other frames (emba_frames_refit): what a sweep costs.

The shape of scripts/track_timing.py: 240 x 180 frames on a 1024 x 2048 panorama, F = 100 frames rendered from a smooth plane along a slow trajectory (0.5 rad
of yaw over the call), tracked once by emba_frames_track from the first frame's true rotation under the schedules (0,) and (3,2,1,0) with batch 1 and batch 8;
the refit then runs behind that tracker's output with sweeps = 0, 1 and 2, the three alternating inside one session.  Stream time between two HIP events:
timer slot 0 brackets a whole call.  Per configuration:
  * the whole call at sweeps = 0 (the build: the frames' upload and one vote launch per batch), 1 and 2;
  * a sweep: (sweeps 2 - sweeps 0) / 2, and per frame;
  * the un-vote plus vote launches of a sweep, taken as the build's time: the same kernel over the same batches, once for each of the two (the build also
    holds the first upload of the frames, a sweep re-uploads them only where the call has more than one chunk: an upper figure);
  * the share of a sweep that is left: the evaluation loop with its per-frame bookkeeping and the 4-byte read that ends an iteration.
Every figure: the median of --reps calls after --warmup, with (min - max).  Nothing is asserted.  Needs the GPU; writes --out (default
profiles/refit_timing.txt)."""
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
SWEEPS = (0, 1, 2)


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
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "refit_timing.txt"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("refit_timing.py measures on the GPU: none is visible")
    F = a.frames
    out = [f"scripts/refit_timing.py --reps {a.reps} --warmup {a.warmup} --frames {F}: median (min - max); {torch.cuda.get_device_name(0)}"]
    lut = pinhole_bearing_lut(SW, SH, 200.0, 200.0, 0.5 * (SW - 1), 0.5 * (SH - 1))
    m = LEGM(SW, SH, lut, 0.2, W, H)
    x, y = np.arange(W, dtype=np.float64)[None, :], np.arange(H, dtype=np.float64)[:, None]
    plane = 128.0 + 60.0 * np.sin(40.0 * np.pi * x / W) * np.cos(20.0 * np.pi * y / H) + 40.0 * np.cos(64.0 * np.pi * x / W + 3.0 * np.pi * y / H)
    traj = LinearTrajectory(np.array([so3.exp(np.array([0.0, 0.05 * i, 0.0])) for i in range(K)]), T0, DT)
    ts = T0 + (np.arange(F, dtype=np.int64) * ((K - 1) * DT - 1)) // max(F - 1, 1)
    frames = m.render_views(ts, traj.knots_xyzw, T0, DT, plane=plane, want_u8=True, lo=0.0, hi=255.0)["u8"]
    q_true = np.array([traj.evaluate(int(t)) for t in ts])
    out.append(f"== {SW}x{SH} frames on a {H}x{W} panorama, F = {F}; io.ALIGN_DEFAULTS, min_weight {MIN_WEIGHT}, min_overlap 0.3; emba_frames_track, then "
               f"emba_frames_refit (estimate 0, alternate, recover) behind its output")
    kw = dict(skip_zero=True, min_overlap=0.3, min_weight=MIN_WEIGHT)
    tracked = {(lv, b): m.track_frames(frames, ts, q0=q_true[0], levels=lv, batch=b, **kw) for lv in SCHEDULES for b in BATCHES}
    configs = [(lv, b, n) for lv in SCHEDULES for b in BATCHES for n in SWEEPS]
    whole, info = {c: [] for c in configs}, {}
    for i in range(a.warmup + a.reps):
        for c in configs:      # alternating: every configuration sees the same session
            t = tracked[c[:2]]
            m.timer_start(0)
            r = m.refit_frames(frames, ts, t["q"], t["status"], levels=c[0], batch=c[1], sweeps=c[2], **kw)
            m.timer_stop(0)
            m.sync()
            if i >= a.warmup:
                whole[c].append(m.timer_ms(0) * 1e3)
            info[c] = r
    for lv in SCHEDULES:
        for b in BATCHES:
            t = tracked[(lv, b)]
            out.append(f"  levels {','.join(map(str, lv))} batch {b}: the tracker left {t['tracked']} tracked, {t['lost']} lost, worst angle to the truth "
                       f"{eio.rotation_angle_between(q_true, t['q']).max():.3e} rad")
            for n in SWEEPS:
                r = info[(lv, b, n)]
                codes = [int((r["refit"] == c).sum()) for c in (eio.REFIT_MOVED, eio.REFIT_KEPT, eio.REFIT_RECOVERED, eio.REFIT_LOST)]
                out.append(f"    sweeps {n}: whole call {fmt(whole[(lv, b, n)], 'us')}; moved / kept / recovered / lost {codes}; {int(r['iters'].sum())} trials in the last "
                           f"sweep; worst angle to the truth {eio.rotation_angle_between(q_true, r['q']).max():.3e} rad")
            build, two = med(whole[(lv, b, 0)]), med(whole[(lv, b, 2)])
            sweep = 0.5 * (two - build)
            out.append(f"    a sweep: {sweep:10.1f} us, {sweep / F:9.1f} us per frame; un-vote plus vote launches (2 x the build) {2.0 * build:10.1f} us, "
                       f"{100.0 * min(2.0 * build / sweep, 1.0) if sweep > 0 else 0.0:.1f} per cent; the evaluation loop's share "
                       f"{100.0 * max(1.0 - 2.0 * build / sweep, 0.0) if sweep > 0 else 0.0:.1f} per cent")
    m.close()
    text = "\n".join(out) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
