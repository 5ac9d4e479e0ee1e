#!/usr/bin/env python3
"""The smooth contrast and its gradient by level (emba_seq_contrast_gradient_level): what one evaluation costs at each level, and what the
LDS vote is worth against the HBM vote where both are possible.

  * per level 0 ... --max-level, on the demo recording of examples/run_ba.py (128x96 on 512x1024) and on 1 M uniform events at 240x180 on 1024x2048: wall
    time of one J-only call and of one J-plus-gradient call of LEGM.contrast_gradient(level=l) — a host clock around calls that end in a device
    synchronise — and the vote kernel's time alone (a J-only call) and the vote and gradient kernels' time together from HIP events
    (emba_enable_kernel_timing: timer slot 7).  Level 0 is the existing entry point: §13's figures, from the same session.
  * at every level whose image fits LDS: the same with option contrast_vote = 0, the votes forced to HBM — the comparison that says whether summing the
    votes on chip pays
  * which vote kernel each call took (emba_get_option "contrast_vote_path"), and the device's J against the numpy rule on the level of its own pm / D

Every figure: the median of --reps calls after --warmup, with (min - max).  Needs the GPU; prints one JSON document (and writes it to --out)."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from emba_amd import LEGM, synth                                     # noqa: E402
from emba_amd import io as eio                                       # noqa: E402

PATHS = {0: "hbm", 1: "lds"}


def stats(v):
    v = sorted(v)
    return dict(median=v[len(v) // 2], min=v[0], max=v[-1])


def timed(f, reps, warmup):
    for _ in range(warmup):
        f()
    out = []
    for _ in range(reps):
        t = time.perf_counter()
        f()
        out.append((time.perf_counter() - t) * 1e3)
    return stats(out)


def slot7_us(m, f, reps, warmup):
    m.enable_kernel_timing(True)
    out = []
    for i in range(warmup + reps):
        f()
        if i >= warmup:
            out.append(m.timer_ms(7) * 1e3)
    m.enable_kernel_timing(False)
    return stats(out)


def measure_level(m, w, n, level, reps, warmup):
    j_only = lambda: m.contrast_gradient(w.traj, 0, n, want_grad=False, level=level)      # noqa: E731
    j_grad = lambda: m.contrast_gradient(w.traj, 0, n, level=level)                       # noqa: E731
    j_only()
    path = PATHS[m.get_option("contrast_vote_path")]
    return dict(vote=path, wall_ms_J_only=timed(j_only, reps, warmup), wall_ms_J_and_grad=timed(j_grad, reps, warmup),
                slot7_us_vote=slot7_us(m, j_only, reps, warmup), slot7_us_vote_and_grad=slot7_us(m, j_grad, reps, warmup))


def measure_shape(name, w, max_level, reps, warmup):
    m = LEGM(w.sensor_w, w.sensor_h, w.lut, w.C_th, w.pano_w, w.pano_h)
    n = m.set_sequence(w.events)
    nn = n // 100 * 100
    pol = np.asarray(w.events.polarity)[:nn]
    levels = []
    for level in range(max_level + 1):
        try:
            eio.contrast_level(np.zeros((1, 2)), None, w.pano_w, w.pano_h, level)
        except ValueError:
            break
        row = dict(level=level, grid=[w.pano_h >> level, w.pano_w >> level], **measure_level(m, w, n, level, reps, warmup))
        if row["vote"] == "lds":
            m.set_option("contrast_vote", 0)
            row["forced_hbm"] = measure_level(m, w, n, level, reps, warmup)
            m.set_option("contrast_vote", -1)
            assert row["forced_hbm"]["vote"] == "hbm"
        got = m.contrast_gradient(w.traj, 0, n, want_pm=True, want_D=True, level=level)
        pm_l, D_l, Wl, Hl = eio.contrast_level(got["pm"], got["D"], w.pano_w, w.pano_h, level)
        want = eio.contrast_gradient(pm_l, D_l, got["cp"], pol, w.K, Wl, Hl)
        row["J"], row["rel_J_vs_numpy"] = got["J"], abs(got["J"] - want["J"]) / want["J"]
        row["rel_grad_vs_numpy"] = float(np.abs(got["grad"] - want["grad"]).max() / np.abs(want["grad"]).max())
        row["image_adds"] = int(np.count_nonzero(eio.contrast_votes(pm_l, Wl, Hl)[1]))
        row["cells_touched"] = int(np.count_nonzero(want["image"]))
        assert row["rel_J_vs_numpy"] < 1e-9 and row["rel_grad_vs_numpy"] < 1e-9, "the device differs from the numpy rule on its own pm / D"
        levels.append(row)
    m.close()
    return dict(shape=name, events=n, used=nn, K=w.K, sensor=[w.sensor_w, w.sensor_h], pano=[w.pano_h, w.pano_w], levels=levels)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--max-level", type=int, default=5)
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("contrast_pyramid_timing.py measures on the GPU: none is visible")
    demo = synth.make_scene_workload(pano_h=512, K=11, sensor=(128, 96), focal=120.0, n_steps=2000)
    bench = synth.make_workload()
    doc = dict(shapes=[measure_shape("demo", demo, a.max_level, a.reps, a.warmup), measure_shape("1M uniform", bench, a.max_level, a.reps, a.warmup)])
    text = json.dumps(doc, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
