"""Device time (emba_timer_*: HIP events on the context's stream) of the two partial solves, emba_solve_map_only and emba_solve_poses_only, next to
emba_solve_normal_eq on the same equations: the BASELINE shape and config 2's shape.  Information only."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from emba_amd import LEGM                      # noqa: E402
from emba_amd.synth import make_workload       # noqa: E402

CONFIGS = (("BASELINE", 1_000_000, 1024, 21, 0.05), ("config 2", 10_000_000, 1024, 201, 0.05))
LAM, REPS = 1e-3, 7
for name, n, ph, K, dt in CONFIGS:
    w = make_workload(n_events=n, pano_h=ph, K=K, dt_knots=dt)
    m = LEGM(w.sensor_w, w.sensor_h, w.lut, w.C_th, w.pano_w, w.pano_h)
    m.set_events(w.events); m.upload_map(w.Gx, w.Gy)
    m.eval_launch(w.traj); m.eval_finish(sync=False); m.form_active(w.thres_valid_pixel, sync=False); m.form_accumulate(); m.form_finish(w.alpha)
    P = m.last_counts()[1]
    calls = (("solve_normal_eq", lambda: m.solveNormalEq(LAM, fix_first_pose=True, resident_x2=True)),
             ("solve_map_only", lambda: m.solveMapOnly(LAM, resident_x2=True)),
             ("solve_poses_only", lambda: m.solvePosesOnly(LAM, fix_first_pose=True)))
    out = []
    for what, call in calls:
        ms = []
        for _ in range(REPS):      # (the first call of each grows its scratch; the joint solve's second reuses its record lists, as a re-solve in an LM loop does)
            m.sync(); m.timer_start(0); call(); m.timer_stop(0)
            ms.append(m.timer_ms(0))
        out.append(f"{what} first {ms[0]:.3f} ms, median of the next {REPS - 1}: {np.median(ms[1:]):.3f} ms (min {min(ms[1:]):.3f})")
    print(f"{name}: N = {n}, K = {K}, P = {P}\n    " + "\n    ".join(out), flush=True)
    m.close()
