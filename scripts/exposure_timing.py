#!/usr/bin/env python3
"""Per-frame exposure (emba_frames_exposure_eval, emba_frames_exposure_align): what the 21-sum evaluation kernel costs beside the 10-sum one.

scripts/align_timing.py's shape: 240 x 180 frames on a 1024 x 2048 panorama, F = 100 frames along its `fast` trajectory, rendered from a smooth plane at the
trajectory's rotations, every frame's bytes then put under an exposure of its own (v <- rint(a_f v + b_f), a_f in 0.8 ... 1, b_f in 0 ... 10), aligned from
rotations turned by 0.01 rad at gain 1 and bias 0.  Stream time between two HIP events: with emba_enable_kernel_timing on, timer slot 7 brackets the
evaluation kernel of a call's first launch; timer slot 0 brackets a whole call.  Every figure: the median of --reps calls after --warmup, with (min - max).
The columns are the evaluation kernel and the whole loop call under estimate = 0 and estimate = 3, beside emba_frames_align on the same pixels; the three
alternate inside one session.  No figure is asserted.  Needs the GPU; writes --out (default profiles/exposure_timing.txt)."""
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


def fmt(v, unit):
    v = sorted(v)
    return f"{v[len(v) // 2]:9.1f} {unit} ({v[0]:.1f} - {v[-1]:.1f})"


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--frames", type=int, default=100)
    ap.add_argument("--iters", type=int, default=10, help="the loops are timed at exactly this many trials per frame (tol_rot = 0, lambda_max = inf)")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "exposure_timing.txt"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("exposure_timing.py measures on the GPU: none is visible")
    F = a.frames
    out = [f"scripts/exposure_timing.py --reps {a.reps} --warmup {a.warmup} --frames {F} --iters {a.iters}: median (min - max); {torch.cuda.get_device_name(0)}"]
    lut = pinhole_bearing_lut(SW, SH, 200.0, 200.0, 0.5 * (SW - 1), 0.5 * (SH - 1))
    m = LEGM(SW, SH, lut, 0.2, W, H)
    m.enable_kernel_timing(True)
    S = SW * SH
    x, y = np.arange(W, dtype=np.float64)[None, :], np.arange(H, dtype=np.float64)[:, None]
    plane = 128.0 + 60.0 * np.sin(40.0 * np.pi * x / W) * np.cos(20.0 * np.pi * y / H) + 40.0 * np.cos(64.0 * np.pi * x / W + 3.0 * np.pi * y / H)
    traj = LinearTrajectory(np.array([so3.mul(so3.exp(np.array([0.0, 0.6 * i, 0.0])), so3.exp(np.array([0.3 * np.sin(i), 0.0, 0.0]))) for i in range(K)]), T0, DT)
    ts = T0 + (np.arange(F, dtype=np.int64) * ((K - 1) * DT - 1)) // max(F - 1, 1)
    rng = np.random.default_rng(0)
    clean = m.render_views(ts, traj.knots_xyzw, T0, DT, plane=plane, want_u8=True, lo=0.0, hi=255.0)["u8"].reshape(F, S)
    a_f, b_f = rng.uniform(0.8, 1.0, F), rng.uniform(0.0, 10.0, F)
    fr = np.where(clean != 0, np.clip(np.rint(a_f[:, None] * clean + b_f[:, None]), 1, 255), 0).astype(np.uint8).reshape(F, SH, SW)
    q_true = np.array([traj.evaluate(int(t)) for t in ts])
    axes = rng.standard_normal((F, 3))
    axes /= np.linalg.norm(axes, axis=1)[:, None]
    q0 = np.array([so3.mul(so3.exp(0.01 * ax), q) for ax, q in zip(axes, q_true)])
    loop_kw = dict(max_iters=a.iters, tol_rot=0.0, lambda_max=float("inf"))
    calls = {
        "emba_frames_align": lambda: m.align_frames(fr, q0, plane, skip_zero=True, **loop_kw),
        "exposure, estimate = 0": lambda: m.align_frames_exposure(fr, q0, 1.0, 0.0, 0, plane, skip_zero=True, **loop_kw),
        "exposure, estimate = 3": lambda: m.align_frames_exposure(fr, q0, 1.0, 0.0, 3, plane, skip_zero=True, **loop_kw),
    }
    kern, whole, info = ({k: [] for k in calls} for _ in range(3))
    for i in range(a.warmup + a.reps):
        for name, call in calls.items():      # alternating: the three see the same session
            m.timer_start(0)
            r = call()
            m.timer_stop(0)
            m.sync()
            if i >= a.warmup:
                kern[name].append(m.timer_ms(7) * 1e3)
                whole[name].append(m.timer_ms(0) * 1e3)
            if i == 0:
                info[name] = (eio.rotation_angle_between(q_true, q0).mean(), eio.rotation_angle_between(q_true, r["q"]).mean(), int(r["iters"].max()))
    out.append(f"== {SW}x{SH} frames on a {H}x{W} panorama, F = {F}: {F * -(-S // 256)} workgroups; every frame under an exposure of its own")
    for name in calls:
        out.append(f"    {name:24s}: evaluation kernel {fmt(kern[name], 'us')}   loop of {info[name][2]} trials, whole call {fmt(whole[name], 'us')}   "
                   f"mean angle to the truth {info[name][0]:.3e} -> {info[name][1]:.3e} rad")
    m.close()
    text = "\n".join(out) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
