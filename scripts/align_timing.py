#!/usr/bin/env python3
"""Intensity frames aligned to a panorama plane (emba_frames_align_eval, emba_frames_align): what the evaluation kernel costs.

240 x 180 frames on a 1024 x 2048 panorama, F = 100 and F = 776 frames (one chunk), along the two trajectories of scripts/mosaic_timing.py over one second:
  slow   0.5 rad of yaw over the trajectory: consecutive frames read the same patch of the plane
  fast   6 rad of yaw with some pitch: the frames read most of the plane's width
The frames are rendered from a smooth plane at the trajectory's rotations and aligned from rotations turned by 0.01 rad.  Stream time between two HIP
events: with emba_enable_kernel_timing on, timer slot 7 brackets the evaluation kernel of a call's first launch (without the reduction of its partial sums
and the step); timer slot 0 brackets a whole call.  Every figure: the median of --reps calls after --warmup, with (min - max); the two trajectories alternate
inside one session.  Beside them the wall time of one evaluation in numpy (io.align_warp + io.align_terms + io.align_sums) on this host at --numpy-frames.

The evaluation kernel is set against its byte model: 1 B of frame and 24 B of bearing LUT per pixel at the plain-copy rate of profiles/r06_stream_bw.txt,
5.34 TB/s; the plane's patch is read from L2.  Needs the GPU; writes --out (default profiles/align_timing.txt)."""
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
    ap.add_argument("--frames", type=int, nargs="+", default=[100, 776])
    ap.add_argument("--iters", type=int, default=10, help="the loop is timed at exactly this many trials per frame (tol_rot = 0, lambda_max = inf)")
    ap.add_argument("--numpy-frames", type=int, default=100, help="the numpy form is timed at this many frames (0: not at all)")
    ap.add_argument("--numpy-reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "align_timing.txt"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("align_timing.py measures on the GPU: none is visible")
    out = [f"scripts/align_timing.py --reps {a.reps} --warmup {a.warmup} --frames {' '.join(map(str, a.frames))} --iters {a.iters}: median (min - max); "
           f"{torch.cuda.get_device_name(0)}"]
    lut = pinhole_bearing_lut(SW, SH, 200.0, 200.0, 0.5 * (SW - 1), 0.5 * (SH - 1))
    m = LEGM(SW, SH, lut, 0.2, W, H)
    m.enable_kernel_timing(True)
    S = SW * SH
    x, y = np.arange(W, dtype=np.float64)[None, :], np.arange(H, dtype=np.float64)[:, None]
    plane = 128.0 + 60.0 * np.sin(40.0 * np.pi * x / W) * np.cos(20.0 * np.pi * y / H) + 40.0 * np.cos(64.0 * np.pi * x / W + 3.0 * np.pi * y / H)
    trajs = {kind: trajectory(kind) for kind in ("slow", "fast")}
    rng = np.random.default_rng(0)
    loop_kw = dict(max_iters=a.iters, tol_rot=0.0, lambda_max=float("inf"))
    out.append(f"== {SW}x{SH} frames on a {H}x{W} panorama; the reduction: per-workgroup partial sums, added in workgroup order by a second kernel (the one form built)")
    numpy_case = {}
    for F in a.frames:
        ts = T0 + (np.arange(F, dtype=np.int64) * ((K - 1) * DT - 1)) // max(F - 1, 1)
        data = {}
        for kind, traj in trajs.items():
            v = m.render_views(ts, traj.knots_xyzw, T0, DT, plane=plane, want_u8=True, lo=0.0, hi=255.0)
            q_true = np.array([traj.evaluate(int(t)) for t in ts])
            axes = rng.standard_normal((F, 3))
            axes /= np.linalg.norm(axes, axis=1)[:, None]
            data[kind] = (v["u8"], np.array([so3.mul(so3.exp(0.01 * ax), q) for ax, q in zip(axes, q_true)]), q_true)
            if F == a.numpy_frames:
                numpy_case[kind] = data[kind]
        kern, whole, loop, err = ({k: [] for k in trajs} for _ in range(4))
        for i in range(a.warmup + a.reps):
            for kind in trajs:      # alternating: both trajectories see the same session
                fr, q0, q_true = data[kind]
                m.timer_start(0)
                m.align_frames_eval(fr, q0, plane, skip_zero=True)
                m.timer_stop(0)
                m.sync()
                if i >= a.warmup:
                    kern[kind].append(m.timer_ms(7) * 1e3)
                    whole[kind].append(m.timer_ms(0) * 1e3)
                m.timer_start(0)
                r = m.align_frames(fr, q0, plane, skip_zero=True, **loop_kw)
                m.timer_stop(0)
                m.sync()
                if i >= a.warmup:
                    loop[kind].append(m.timer_ms(0) * 1e3)
                if i == 0:
                    err[kind] = (eio.rotation_angle_between(q_true, q0).mean(), eio.rotation_angle_between(q_true, r["q"]).mean(), int(r["iters"].max()))
        byte_us = F * S * 25 / (COPY_TBS * 1e12) * 1e6
        out.append(f"  F = {F}: {F * -(-S // 256)} workgroups; byte model ({F} frames, 25 B per pixel at {COPY_TBS} TB/s) {byte_us:.1f} us")
        for kind in trajs:
            k = med(kern[kind])
            out.append(f"    {kind:4s}: evaluation kernel {fmt(kern[kind], 'us')}   whole evaluation call {fmt(whole[kind], 'us')}   loop of {err[kind][2]} trials, whole call {fmt(loop[kind], 'us')}")
            out.append(f"          {k * 1e3 / (F * S):.3f} ns per pixel; {k / byte_us:.1f} x the byte model; mean angle to the truth {err[kind][0]:.3e} -> {err[kind][1]:.3e} rad")
    if a.numpy_frames and numpy_case:      # the numpy form beside them: wall time of ONE evaluation on this host
        t_np = {k: [] for k in trajs}
        for i in range(1 + a.numpy_reps):
            for kind in trajs:
                fr, q0, _ = numpy_case[kind]
                t0 = time.perf_counter()
                for f in range(a.numpy_frames):
                    pm = eio.align_warp(lut, q0[f], W, H)[1]
                    eio.align_sums(eio.align_terms(fr[f].reshape(-1), pm, lut, q0[f], plane, None, 0.0, 255.0, True, 0.0))
                if i >= 1:
                    t_np[kind].append(1e3 * (time.perf_counter() - t0))
        out.append(f"== the numpy form on this host, one evaluation of F = {a.numpy_frames} frames, wall time, median of {a.numpy_reps} after 1 warm-up (min - max)")
        for kind in trajs:
            out.append(f"    {kind:4s}: io.align_warp + io.align_terms + io.align_sums {fmt(t_np[kind], 'ms')}")
    m.close()
    text = "\n".join(out) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
