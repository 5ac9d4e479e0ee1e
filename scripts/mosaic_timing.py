#!/usr/bin/env python3
"""The mosaic of intensity frames (emba_mosaic_frames): what the vote kernel costs, and what its contended atomics cost it.

240 x 180 frames of random bytes on a 1024 x 2048 panorama, F = 100 and F = 1000 frames, along two trajectories over one second:
  slow   the demo's rotation, 0.5 rad of yaw over the trajectory: consecutive frames land on the same cells — high contention
  fast   6 rad of yaw with some pitch: the frames spread over most of the panorama's width
Stream time between two HIP events: with emba_enable_kernel_timing on, timer slot 7 brackets the vote kernel of a call's first chunk (at most 776 frames of
240 x 180 bytes: F = 100 is all of it, F = 1000 its first 776 frames); timer slot 0 brackets the whole call — the pose stage, the upload of the bytes, every
chunk.  Every figure: the median of --reps calls after --warmup, with (min - max); the two trajectories alternate inside one session.  Beside them the wall
time of the numpy form (io.view_pm + io.mosaic_votes) on this host at --numpy-frames frames, on both trajectories.

The vote kernel is set against two models: its bytes (1 B of frame and 24 B of bearing LUT per pixel at the plain-copy rate of profiles/r06_stream_bw.txt,
5.34 TB/s) and its atomics (eight 64-bit adds per pixel, fewer where a weight or the byte is zero).  Needs the GPU; writes --out (default
profiles/mosaic_timing.txt)."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from emba_amd import LEGM                                            # noqa: E402
from emba_amd import io as eio                                       # noqa: E402
from emba_amd import so3                                             # noqa: E402
from emba_amd.legm import LinearTrajectory                           # noqa: E402
from emba_amd.synth import pinhole_bearing_lut                       # noqa: E402

COPY_TBS = 5.34          # profiles/r06_stream_bw.txt: copy (read + write) of 1.2 GB
SW, SH, W, H = 240, 180, 2048, 1024
CHUNK_FRAMES = (32 << 20) // (SW * SH)      # view_rule.h: view_chunk_frames(S, 1)
K, T0, DT = 11, 10**9, 10**8


def fmt(v, unit):
    v = sorted(v)
    return f"{v[len(v) // 2]:9.1f} {unit} ({v[0]:.1f} - {v[-1]:.1f})"


def med(v):
    return sorted(v)[len(v) // 2]


def trajectory(kind):
    if kind == "slow":
        knots = [so3.exp(np.array([0.0, 0.05 * i, 0.0])) for i in range(K)]
    else:
        knots = [so3.mul(so3.exp(np.array([0.0, 0.6 * i, 0.0])), so3.exp(np.array([0.3 * np.sin(i), 0.0, 0.0]))) for i in range(K)]
    return LinearTrajectory(np.array(knots), T0, DT)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--frames", type=int, nargs="+", default=[100, 1000])
    ap.add_argument("--numpy-frames", type=int, default=100, help="the numpy form is timed at this many frames (0: not at all)")
    ap.add_argument("--numpy-reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "mosaic_timing.txt"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("mosaic_timing.py measures on the GPU: none is visible")
    out = [f"scripts/mosaic_timing.py --reps {a.reps} --warmup {a.warmup} --frames {' '.join(map(str, a.frames))}: median (min - max); {torch.cuda.get_device_name(0)}"]
    rng = np.random.default_rng(0)
    lut = pinhole_bearing_lut(SW, SH, 200.0, 200.0, 0.5 * (SW - 1), 0.5 * (SH - 1))
    m = LEGM(SW, SH, lut, 0.2, W, H)
    m.enable_kernel_timing(True)
    S = SW * SH
    trajs = {kind: trajectory(kind) for kind in ("slow", "fast")}
    out.append(f"== emba_mosaic_frames: {SW}x{SH} frames of random bytes on a {H}x{W} panorama; the plain form: two return-less 64-bit atomic adds per cell in HBM")
    for F in a.frames:
        frames = rng.integers(0, 256, (F, SH, SW)).astype(np.uint8)
        ts = T0 + (np.arange(F, dtype=np.int64) * ((K - 1) * DT - 1)) // max(F - 1, 1)
        first = min(CHUNK_FRAMES, F)
        kern, whole, cells = {k: [] for k in trajs}, {k: [] for k in trajs}, {}
        for i in range(a.warmup + a.reps):
            for kind, traj in trajs.items():      # alternating: both trajectories see the same session
                m.timer_start(0)
                m.mosaic_frames(frames, ts, traj)
                m.timer_stop(0)
                m.sync()
                if i >= a.warmup:
                    kern[kind].append(m.timer_ms(7) * 1e3)
                    whole[kind].append(m.timer_ms(0) * 1e3)
                if i == 0:
                    cells[kind] = m.mosaic(min_weight=1)["n_covered"]
        byte_us = first * S * 25 / (COPY_TBS * 1e12) * 1e6
        out.append(f"  F = {F} ({-(-F // CHUNK_FRAMES)} chunk(s) of at most {CHUNK_FRAMES} frames); byte model of the first chunk ({first} frames, 25 B per pixel at {COPY_TBS} TB/s) {byte_us:.1f} us")
        for kind in trajs:
            k = med(kern[kind])
            adds = 8.0 * first * S
            out.append(f"    {kind:4s}: vote kernel of the first chunk {fmt(kern[kind], 'us')}   whole call {fmt(whole[kind], 'us')}   {cells[kind]} cells touched by the {F} frames")
            out.append(f"          {k * 1e3 / (first * S):.3f} ns per pixel, {adds / (k * 1e3):.1f} 64-bit atomic adds per ns at eight per pixel; {k / byte_us:.1f} x the byte model")
        out.append(f"    slow / fast, vote kernel: {med(kern['slow']) / med(kern['fast']):.2f} x — what the contention of consecutive frames on the same cells costs")
    if a.numpy_frames:      # the numpy form beside them: wall time on this host, one warm-up and --numpy-reps repeats per trajectory, alternating
        F = a.numpy_frames
        frames = rng.integers(0, 256, (F, SH, SW)).astype(np.uint8)
        ts = T0 + (np.arange(F, dtype=np.int64) * ((K - 1) * DT - 1)) // max(F - 1, 1)
        t_pm, t_votes = {k: [] for k in trajs}, {k: [] for k in trajs}
        for i in range(1 + a.numpy_reps):
            for kind, traj in trajs.items():
                t0 = time.perf_counter()
                pm = eio.view_pm(lut, traj.knots_xyzw, T0, DT, ts, W, H)
                t1 = time.perf_counter()
                eio.mosaic_votes(frames, pm, W, H)
                t2 = time.perf_counter()
                if i >= 1:
                    t_pm[kind].append(1e3 * (t1 - t0))
                    t_votes[kind].append(1e3 * (t2 - t1))
        out.append(f"== the numpy form on this host, F = {F}, wall time, median of {a.numpy_reps} after 1 warm-up (min - max)")
        for kind in trajs:
            out.append(f"    {kind:4s}: io.view_pm {fmt(t_pm[kind], 'ms')}   io.mosaic_votes {fmt(t_votes[kind], 'ms')}")
    m.close()
    text = "\n".join(out) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
