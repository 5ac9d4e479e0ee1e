#!/usr/bin/env python3
"""The prior of the smooth contrast (emba_seq_contrast_prior_add, emba_seq_contrast_gradient_prior): what it costs.

  * one evaluation (J and gradient) with and without a prior, per level 0 ... 3, on the demo recording of examples/run_ba.py (128x96 on 512x1024) and on
    1 M uniform events at 240x180 on 1024x2048: the stream time of the whole call between two HIP events (emba_timer_start / _stop around it: the pose
    stage, the zeroing or the prior's pass over the image, the votes, the gradient, the reduction, the copies), the wall time of the call, and the vote and
    gradient kernels alone (timer slot 7), from the same session.  The prior is what the first half of the events voted; both calls evaluate the second half.
  * prior_add over the levels 3, 2, 1, 0 in one call (every event warped once) against four single-level calls: stream time, wall time, and the vote
    kernels alone (slot 7; the four calls' summed).

Every figure: the median of --reps calls after --warmup, with (min - max).  Needs the GPU; writes --out (default profiles/contrast_prior_timing.txt)."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from emba_amd import LEGM, synth                                     # noqa: E402

LEVELS = (3, 2, 1, 0)
PATHS = {0: "hbm", 1: "lds"}


def fmt(v, unit):
    v = sorted(v)
    return f"{v[len(v) // 2]:9.1f} {unit} ({v[0]:.1f} - {v[-1]:.1f})"


def measure(m, f, reps, warmup):
    """f() `warmup + reps` times: (stream time between HIP events around it, wall time, slot 7 of its last library call), microseconds."""
    m.enable_kernel_timing(True)
    ev, wall, k7 = [], [], []
    for i in range(warmup + reps):
        t = time.perf_counter()
        m.timer_start(0)
        slot7 = f()
        m.timer_stop(0)
        m.sync()
        dt = (time.perf_counter() - t) * 1e6
        if i >= warmup:
            ev.append(m.timer_ms(0) * 1e3)
            wall.append(dt)
            k7.append(slot7)
    m.enable_kernel_timing(False)
    return ev, wall, k7


def measure_shape(name, w, reps, warmup, out):
    m = LEGM(w.sensor_w, w.sensor_h, w.lut, w.C_th, w.pano_w, w.pano_h)
    n = m.set_sequence(w.events)
    half = n // 200 * 100
    out.append(f"== {name}: {n} events, sensor {w.sensor_w}x{w.sensor_h}, panorama {w.pano_h}x{w.pano_w}, K = {w.K}; prior = events [0, {half}), evaluated: [{half}, {n})")

    def one_call():
        m.contrast_prior_clear()
        m.contrast_prior_add(w.traj, 0, half, levels=LEVELS)
        return m.timer_ms(7) * 1e3

    def four_calls():
        m.contrast_prior_clear()
        t = 0.0
        for l in LEVELS:
            m.contrast_prior_add(w.traj, 0, half, levels=(l,))
            t += m.timer_ms(7) * 1e3
        return t
    for what, f in (("prior_add, levels 3,2,1,0 in one call ", one_call), ("prior_add, four single-level calls    ", four_calls)):
        ev, wall, k7 = measure(m, f, reps, warmup)
        out.append(f"  {what}: stream {fmt(ev, 'us')}   wall {fmt(wall, 'us')}   vote kernels {fmt(k7, 'us')}")
    one_call()
    for l in reversed(LEVELS):
        rows = []
        for what, kw in (("without a prior", {}), ("with the prior ", dict(prior_weight=1.0))):
            def f():
                m.contrast_gradient(w.traj, half, n, level=l, **kw)
                return m.timer_ms(7) * 1e3
            ev, wall, k7 = measure(m, f, reps, warmup)
            rows.append(sorted(ev)[len(ev) // 2])
            out.append(f"  level {l} ({w.pano_h >> l}x{w.pano_w >> l}, votes in {PATHS[m.get_option('contrast_vote_path')]}), J and gradient, {what}: "
                       f"stream {fmt(ev, 'us')}   wall {fmt(wall, 'us')}   vote + gradient kernels {fmt(k7, 'us')}")
        out.append(f"  level {l}: the prior adds {rows[1] - rows[0]:+.1f} us of stream time (median against median)")
    m.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "contrast_prior_timing.txt"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("contrast_prior_timing.py measures on the GPU: none is visible")
    out = [f"scripts/contrast_prior_timing.py --reps {a.reps} --warmup {a.warmup}: median (min - max); {torch.cuda.get_device_name(0)}"]
    measure_shape("demo", synth.make_scene_workload(pano_h=512, K=11, sensor=(128, 96), focal=120.0, n_steps=2000), a.reps, a.warmup, out)
    measure_shape("1M uniform", synth.make_workload(), a.reps, a.warmup, out)
    text = "\n".join(out) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
