#!/usr/bin/env python3
"""The event simulator (emba_simulate_events): what a recording of about 1 M events costs on the device, phase by phase, next to the numpy
form of the same rule.

A 240 x 180 sensor in front of a 1024 x 2048 log-intensity plane (the sinusoid scene of bench.py --data scene, its amplitude set so that the count lands near
--events) along the make_scene_stream trajectory, --steps steps.  Stream time between two HIP events: timer slot 0 brackets the whole call (uploads, every
chunk, the one word read per chunk); with emba_enable_kernel_timing on, the timer slots 3 ... 7 bracket the phases of the call's FIRST chunk (97 steps at this
sensor): views, count, scan, emit, sort (the gather into the recording included).  Every figure: the median of --reps calls after --warmup, with (min - max).
Beside it io.simulate_from_plane at the same shape, wall time of one call on the CPUs the job may use: the yardstick, no ratio is asserted anywhere.
Needs the GPU; writes --out (default profiles/sim_timing.txt)."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from emba_amd import LEGM                                            # noqa: E402
from emba_amd import io as eio                                       # noqa: E402
from emba_amd import synth                                           # noqa: E402

SW, SH, W, H, FOCAL, K, C_TH = 240, 180, 2048, 1024, 200.0, 21, 0.2
CHUNK_STEPS = (32 << 20) // (SW * SH * 8)      # sim_rule.h: sim_chunk_steps
PHASES = ("views", "count", "scan", "emit", "sort")


def fmt(v, unit):
    v = sorted(v)
    return f"{v[len(v) // 2]:9.1f} {unit} ({v[0]:.1f} - {v[-1]:.1f})"


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--events", type=int, default=1_000_000)
    ap.add_argument("--no-numpy", action="store_true")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "sim_timing.txt"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("sim_timing.py measures on the GPU: none is visible")
    out = [f"scripts/sim_timing.py --reps {a.reps} --warmup {a.warmup} --steps {a.steps} --events {a.events}: median (min - max); {torch.cuda.get_device_name(0)}"]
    lut = synth.pinhole_bearing_lut(SW, SH, FOCAL, FOCAL, SW / 2.0, SH / 2.0)
    traj = synth.make_trajectory(K)
    ts = np.linspace(traj.t0_ns, traj.t0_ns + traj.dt_ns * (K - 1) - 1, a.steps + 1).astype(np.int64)
    px, py = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    unit = synth.SinusoidScene(H, n_terms=8, max_freq=(40, 20), amp=1.0, seed=3).value(px, py)
    m = LEGM(SW, SH, lut, C_TH, W, H)
    args = (ts, traj.knots_xyzw, traj.t0_ns, traj.dt_ns)
    probe = int(m.simulate_events(*args, plane=unit)[0])
    amp = a.events / max(probe, 1)      # the count is close to linear in the amplitude
    plane = amp * unit
    m.enable_kernel_timing(True)
    whole, phases, stats = [], {p: [] for p in PHASES}, None
    for i in range(a.warmup + a.reps):
        m.timer_start(0)
        stats = m.simulate_events(*args, plane=plane)
        m.timer_stop(0)
        m.sync()
        if i >= a.warmup:
            whole.append(m.timer_ms(0))
            for k, p in enumerate(PHASES):
                phases[p].append(m.timer_ms(3 + k) * 1e3)
    n = int(stats[0])
    chunks, first = -(-a.steps // CHUNK_STEPS), min(CHUNK_STEPS, a.steps)
    out.append(f"== emba_simulate_events: {SW}x{SH} sensor, {H}x{W} plane of amplitude {amp:.3f}, {a.steps} steps in {chunks} chunks of at most {CHUNK_STEPS}, C = {C_TH}")
    out.append(f"  {n} events ({int(stats[1])} positive), {int(stats[2])} (pixel, step) pairs capped, {int(stats[3])} (pixel, frame) pairs outside")
    out.append(f"  whole call           {fmt(whole, 'ms')}   {n / (sorted(whole)[len(whole) // 2] * 1e-3) * 1e-6:.1f} M events per second")
    out.append(f"  first chunk, {first} steps of {SW * SH} pixels:")
    for p in PHASES:
        out.append(f"    {p:6s} {fmt(phases[p], 'us')}")
    t0 = time.perf_counter()
    seq_n = m.sequence_from_simulation()
    m.sync()
    out.append(f"  emba_seq_from_sim: {seq_n} events into the resident sequence, {(time.perf_counter() - t0) * 1e3:.2f} ms wall (one call)")
    if not a.no_numpy:
        t0 = time.perf_counter()
        ev, st = eio.simulate_from_plane(plane, lut, traj.knots_xyzw, traj.t0_ns, traj.dt_ns, ts, (SW, SH), C_TH)
        dt = time.perf_counter() - t0
        out.append(f"== io.simulate_from_plane, the same shape: {int(st[0])} events in {dt:.2f} s wall (one call; numpy's own pm, so the count may differ by a few)")
    m.close()
    text = "\n".join(out) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
