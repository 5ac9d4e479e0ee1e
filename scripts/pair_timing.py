#!/usr/bin/env python3
"""One frame aligned to another, and the rotation graph over all frames (emba_frames_pair_eval, emba_frames_pair_align, emba_rotation_graph_solve;
DESIGN.md §26): what closing the loops of a tracked sequence costs.

The shape of scripts/track_timing.py: 240 x 180 frames on a 1024 x 2048 panorama, F = 100 frames rendered from a smooth plane along a slow trajectory that
goes out for half the frames and comes back, so that the way back sees the way out.  The tracked rotations are the truth with a drift of 0.05 sensor pixels
per frame added; the pairs are io.pair_candidates of them (window 2, beyond 4 frames the 2 nearest within 0.2 rad).  Stream time between two HIP events:
with emba_enable_kernel_timing on, timer slot 7 brackets the evaluation kernel
of a call's first launch; timer slot 0 brackets a whole call.  Measured:
  * emba_frames_pair_eval of all pairs: the whole call, the evaluation kernel, per pair, and the source pixels per second of the kernel;
  * emba_frames_pair_align of all pairs: the whole call, per pair and per trial of the slowest pair (the loop waits on the stream once per iteration);
  * emba_rotation_graph_solve on the kept pairs: host wall time;
  * the stitch at the new rotations (emba_frames_refit, sweeps = 0).
Every figure: the median of --reps calls after --warmup, with (min - max).  Nothing is asserted.  Needs the GPU; writes --out (default
profiles/pair_timing.txt)."""
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
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "pair_timing.txt"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("pair_timing.py measures on the GPU: none is visible")
    F, S = a.frames, SW * SH
    out = [f"scripts/pair_timing.py --reps {a.reps} --warmup {a.warmup} --frames {F}: median (min - max); {torch.cuda.get_device_name(0)}"]
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
    out.append(f"== {SW}x{SH} frames on a {H}x{W} panorama, F = {F} out and back, {DRIFT_PX} pixels of drift per frame; {P} pairs (window 2; beyond 4 frames the 2 nearest "
               f"within 0.2 rad); io.ALIGN_DEFAULTS, skip_zero")
    t_eval, k_eval, t_align, t_graph, t_stitch = [], [], [], [], []
    m.enable_kernel_timing(True)
    for i in range(a.warmup + a.reps):
        m.timer_start(0)
        m.pair_eval(frames, pairs, Q0, calib, skip_zero=True)
        m.timer_stop(0)
        m.sync()
        te, ke = m.timer_ms(0) * 1e3, m.timer_ms(7) * 1e3
        m.timer_start(0)
        al = m.pair_align(frames, pairs, Q0, calib, skip_zero=True)
        m.timer_stop(0)
        m.sync()
        ta = m.timer_ms(0) * 1e3
        kept = ((al["status"] == eio.ALIGN_CONVERGED) | (al["status"] == eio.ALIGN_ITERATIONS)) & (al["counts"][:, 0] >= 0.3 * S)
        info = eio.pair_information(al["sums"], al["counts"], floor=eio.PAIR_NOISE_FLOOR)
        t0 = time.perf_counter()
        g = LEGM.rotation_graph_solve(q, status, pairs[kept], al["q"][kept], info[kept])
        tg = (time.perf_counter() - t0) * 1e6
        m.timer_start(0)
        m.refit_frames(frames, ts, g["q"], status, levels=(0,), batch=8, sweeps=0, skip_zero=True, min_weight=32, min_overlap=0.3)
        m.timer_stop(0)
        m.sync()
        if i >= a.warmup:
            t_eval.append(te); k_eval.append(ke); t_align.append(ta); t_graph.append(tg); t_stitch.append(m.timer_ms(0) * 1e3)
    names = ", ".join(f"{int((al['status'] == k).sum())} {v}" for k, v in eio.ALIGN_STATUS_NAMES.items())
    out.append(f"  emba_frames_pair_eval, {P} pairs: whole call {fmt(t_eval, 'us')}; the evaluation kernel {fmt(k_eval, 'us')}, {med(k_eval) / P:.2f} us per pair, "
               f"{P * S / med(k_eval):.0f} source pixels per us")
    out.append(f"  emba_frames_pair_align: whole call {fmt(t_align, 'us')}, {med(t_align) / P:.1f} us per pair; {names}; {int(al['iters'].sum())} trials, the slowest pair "
               f"{int(al['iters'].max())}: {med(t_align) / (int(al['iters'].max()) + 1):.1f} us per iteration of the loop; {int(kept.sum())} pairs kept")
    out.append(f"  emba_rotation_graph_solve, {int(kept.sum())} edges over {F} frames (host): {fmt(t_graph, 'us')}; {g['iters']} steps, {g['cg_iters']} CG iterations, "
               f"{eio.GRAPH_END_NAMES[g['end']]}; cost {g['cost0']:.6g} -> {g['cost']:.6g}")
    out.append(f"  the stitch at the new rotations (emba_frames_refit, sweeps = 0, level 0, batch 8): {fmt(t_stitch, 'us')}")
    out.append(f"  worst angle to the truth: drifted {eio.rotation_angle_between(q_true, q).max():.3e} rad -> closed {eio.rotation_angle_between(q_true, g['q']).max():.3e} rad")
    m.close()
    text = "\n".join(out) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
