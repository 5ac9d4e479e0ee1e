#!/usr/bin/env python3
"""The pair alignment coarse to fine, with the pair's exposure estimated (emba_frames_pair_level_eval, emba_frames_pair_align_levels), on
scripts/pair_timing.py's shape: 240 x 180 frames rendered on the device from a textured plane behind a 200-pixel pinhole, 100 frames out and back, the pairs
io.pair_candidates of the drifted rotations.  Stream time between two HIP events: median (min - max) of --reps after --warmup.  Recorded:
  * the reduce kernel, which reads every frame byte once and makes the bytes of the levels asked for (timer slot 6), for level 1 alone and for level 3 alone
    (the cascade runs up to the highest level asked for);
  * the evaluation kernel per level (timer slot 7), in level pixels per us beside the 10-sum kernel's figure on the same pairs;
  * the whole call of emba_frames_pair_align_levels for (0), (2, 1, 0) and (3, 2, 1, 0), with estimate = 0 and estimate = 3, beside emba_frames_pair_align.
Nothing measured here is asserted anywhere.  Writes --out (default profiles/pair_level_timing.txt)."""
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
FOCAL = 200.0
DRIFT_PX = 0.05


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
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "pair_level_timing.txt"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("pair_level_timing.py measures on the GPU: none is visible")
    F = a.frames
    out = [f"scripts/pair_level_timing.py --reps {a.reps} --warmup {a.warmup} --frames {F}: median (min - max); {torch.cuda.get_device_name(0)}"]
    calib = eio.pair_calib(FOCAL, FOCAL, 0.5 * (SW - 1), 0.5 * (SH - 1))
    lut = pinhole_bearing_lut(SW, SH, FOCAL, FOCAL, calib["cu"], calib["cv"])
    m = LEGM(SW, SH, lut, 0.2, W, H)
    x, y = np.arange(W, dtype=np.float64)[None, :], np.arange(H, dtype=np.float64)[:, None]
    plane = 128.0 + 60.0 * np.sin(40.0 * np.pi * x / W) * np.cos(20.0 * np.pi * y / H) + 40.0 * np.cos(64.0 * np.pi * x / W + 3.0 * np.pi * y / H)
    traj = LinearTrajectory(np.array([so3.exp(np.array([0.0, 0.05 * (i if i <= K // 2 else K - 1 - i + 0.37), 0.0])) for i in range(K)]), T0, DT)
    ts = T0 + (np.arange(F, dtype=np.int64) * ((K - 1) * DT - 1)) // max(F - 1, 1)
    frames = m.render_views(ts, traj.knots_xyzw, T0, DT, plane=plane, want_u8=True, lo=0.0, hi=255.0)["u8"]
    q_true = np.array([traj.evaluate(int(t)) for t in ts])
    axis = np.array([0.3, 1.0, -0.2]) / np.linalg.norm([0.3, 1.0, -0.2])
    q = np.array([so3.mul(so3.exp(f * DRIFT_PX / FOCAL * axis), q_true[f]) for f in range(F)])
    status = np.array([1] + [2] * (F - 1), np.int32)
    pairs = eio.pair_candidates(q, status, window=2, min_gap=4, max_angle=0.2, max_per_frame=2)
    Q0 = eio.pair_start(q, None, None, pairs)[0]
    P = len(pairs)
    out.append(f"== {SW}x{SH} frames, F = {F} out and back, {DRIFT_PX} pixels of drift per frame; {P} pairs; io.ALIGN_DEFAULTS, skip_zero")
    m.enable_kernel_timing(True)

    def timed(call):
        whole, kernel, r = [], [], None
        for i in range(a.warmup + a.reps):
            m.timer_start(0)
            r = call()
            m.timer_stop(0)
            m.sync()
            if i >= a.warmup:
                whole.append(m.timer_ms(0) * 1e3)
                kernel.append(m.timer_ms(7) * 1e3)
        return whole, kernel, r

    for l in (1, 3):
        red = []
        for i in range(a.warmup + a.reps):
            m.pair_level_eval(frames, pairs[:1], Q0[:1], calib, l, skip_zero=True)
            m.sync()
            if i >= a.warmup:
                red.append(m.timer_ms(6) * 1e3)
        out.append(f"  emba_frames_pair_reduce_kernel, {F} frames of {SW}x{SH}, up to level {l}: {fmt(red, 'us')}, {F * SW * SH / med(red):.0f} frame bytes per us")
    t10, k10, _ = timed(lambda: m.pair_eval(frames, pairs, Q0, calib, skip_zero=True))
    out.append(f"  emba_frames_pair_eval (10 sums), {P} pairs: whole call {fmt(t10, 'us')}; the evaluation kernel {fmt(k10, 'us')}, {P * SW * SH / med(k10):.0f} pixels per us")
    for l in (0, 1, 2, 3):
        Sl = (SW >> l) * (SH >> l)
        t, k, _ = timed(lambda: m.pair_level_eval(frames, pairs, Q0, calib, l, skip_zero=True))
        out.append(f"  emba_frames_pair_level_eval (21 sums), level {l} ({SW >> l} x {SH >> l}): whole call {fmt(t, 'us')}; the evaluation kernel {fmt(k, 'us')}, "
                   f"{P * Sl / med(k):.0f} level pixels per us")
    t, _, al = timed(lambda: m.pair_align(frames, pairs, Q0, calib, skip_zero=True))
    out.append(f"  emba_frames_pair_align: whole call {fmt(t, 'us')}, {med(t) / P:.1f} us per pair; {int(al['iters'].sum())} trials")
    for levels in ((0,), (2, 1, 0), (3, 2, 1, 0)):
        for estimate in (0, 3):
            t, _, al = timed(lambda: m.pair_align_levels(frames, pairs, Q0, calib, levels=levels, estimate=estimate, skip_zero=True))
            names = ", ".join(f"{int((al['status'] == k).sum())} {v}" for k, v in eio.ALIGN_STATUS_NAMES.items())
            out.append(f"  emba_frames_pair_align_levels {levels}, estimate = {estimate}: whole call {fmt(t, 'us')}, {med(t) / P:.1f} us per pair; {names}; trials per level "
                       f"{al['level_iters'].sum(axis=0).tolist()}, the slowest pair {al['level_iters'].max(axis=0).tolist()}")
    m.close()
    text = "\n".join(out) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
