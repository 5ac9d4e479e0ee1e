#!/usr/bin/env python3
"""What the contrast-maximisation objective does on the simulator's recordings (CPU only, numpy form): per recording the true body rate of
every knot interval; per slice length the slices' time span, the motion in pixels at the true rate, and J(true rate) / J(0) — on the image as the rule
builds it and after 1, 2 and 4 passes of a 1-2-1 binomial blur of the image before the squares.

  python scripts/cmax_scene_check.py"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import cmax_cases as CC                          # noqa: E402
from emba_amd import io as eio, so3, synth       # noqa: E402


def blur(I, passes):
    I = I.astype(np.float64)
    for _ in range(passes):
        p = np.pad(I, 1); I = (p[:-2, 1:-1] + 2 * p[1:-1, 1:-1] + p[2:, 1:-1]) / 4
        p = np.pad(I, 1); I = (p[1:-1, :-2] + 2 * p[1:-1, 1:-1] + p[1:-1, 2:]) / 4
    return I


def report(name, w, focal, slice_lengths):
    t = np.asarray(w.events.t_ns)
    print(f"{name}: {t.size} events; true body rate per knot interval (rad/s):")
    for i in range(w.traj.size() - 1):
        r = CC.body_rate(w.traj, w.traj.t0_ns + i * w.traj.dt_ns + 1)
        print(f"    {np.round(r, 3)}  |w| = {np.linalg.norm(r):.3f}")
    for m in slice_lengths:
        span, px, ratio = [], [], {0: [], 1: [], 2: [], 4: []}
        for s in range(t.size // m):
            b, e = s * m, (s + 1) * m
            wt = CC.body_rate(w.traj, (int(t[b]) + int(t[e - 1])) // 2)
            span.append((t[e - 1] - t[b]) * 1e-6)
            px.append(np.linalg.norm(wt) * span[-1] * 1e-3 * focal)
            J, iwe = eio.cmax_objective(w.events, w.lut, w.sensor_w, w.sensor_h, [[0, 0, 0], wt], b, e)
            ratio[0].append(float(J[1]) / float(J[0]))
            for n in (1, 2, 4):
                ratio[n].append((blur(iwe[1], n) ** 2).sum() / (blur(iwe[0], n) ** 2).sum())
        print(f"  slices of {m}: {len(span)}, span {min(span):.1f}-{max(span):.1f} ms, {min(px):.2f}-{max(px):.2f} px at the true rate, J(true)/J(0) "
              + ", ".join(f"{'rule' if n == 0 else f'blur x{n}'} {min(v):.3f}-{max(v):.3f}" for n, v in ratio.items()))


def main():
    report("scene 64x48", synth.make_scene_workload(), 60.0, (777, 2000, 10000))
    wd = synth.make_scene_workload(pano_h=512, K=11, sensor=(128, 96), focal=120.0, n_steps=2000)
    report("demo 128x96", wd, 120.0, (10000,))
    k = wd.traj.knots_xyzw
    rel = [np.linalg.norm(so3.log(so3.mul(so3.inverse(k[0]), q))) for q in k]
    print(f"demo: the truth turns {np.degrees(rel[-1]):.2f} deg in all; identity poses are {np.degrees(np.mean(rel)):.2f} deg off on average (relative to the first control pose)")
    ev, lut = CC.constant_rate_events(CC.CONST_OMEGA)
    J, iwe = eio.cmax_objective(ev, lut, 64, 48, [[0, 0, 0], CC.CONST_OMEGA], 0, CC.CONST_SLICE)
    print(f"fixed scene points, constant rate: J(true)/J(0) rule {float(J[1]) / float(J[0]):.3f}, blur x2 {(blur(iwe[1], 2) ** 2).sum() / (blur(iwe[0], 2) ** 2).sum():.3f}")


if __name__ == "__main__":
    main()
