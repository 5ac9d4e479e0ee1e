#!/usr/bin/env python3
"""The smooth contrast of the panorama of warped events and its gradient (emba_seq_contrast_gradient): what one evaluation costs.

  * wall time of one J-only call and of one J-plus-gradient call of LEGM.contrast_gradient, on the demo recording of examples/run_ba.py (128x96 on
    512x1024) and on 1 M uniform events at 240x180 on 1024x2048 — a host clock around calls that end in a device synchronise
  * the vote kernel's time alone (a J-only call) and the vote and gradient kernels' time together (a J-plus-gradient call) from HIP events
    (emba_enable_kernel_timing: timer slot 7)
  * the numpy form (io.contrast_gradient on the call's own pm, D, cp) on the same host
  * beside them a MODEL, not a measurement of a parent (there is none): the bytes each kernel has to move over an 8 TB/s memory system, and its global
    atomic adds at the rate DESIGN.md §12 measured for the integer votes (23 adds per ns)

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

HBM_BYTES_PER_S = 8.0e12
ADDS_PER_NS = 23.0          # the int32 votes of emba_pano_vote_kernel at 1 M events


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


def measure_shape(name, w, reps, warmup, numpy_reps):
    m = LEGM(w.sensor_w, w.sensor_h, w.lut, w.C_th, w.pano_w, w.pano_h)
    n = m.set_sequence(w.events)
    nn = n // 100 * 100
    j_only = lambda: m.contrast_gradient(w.traj, 0, n, want_grad=False)      # noqa: E731
    j_grad = lambda: m.contrast_gradient(w.traj, 0, n)                       # noqa: E731
    wall_j, wall_g = timed(j_only, reps, warmup), timed(j_grad, reps, warmup)
    kern_j, kern_g = slot7_us(m, j_only, reps, warmup), slot7_us(m, j_grad, reps, warmup)
    got = m.contrast_gradient(w.traj, 0, n, want_image=True, want_pm=True, want_D=True)
    pol = np.asarray(w.events.polarity)[:nn]
    host = timed(lambda: eio.contrast_gradient(got["pm"], got["D"], got["cp"], pol, w.K, w.pano_w, w.pano_h), numpy_reps, 1)
    want = eio.contrast_gradient(got["pm"], got["D"], got["cp"], pol, w.K, w.pano_w, w.pano_h)
    rel = lambda a, b: float(np.abs(np.asarray(a) - np.asarray(b)).max() / np.abs(np.asarray(b)).max())      # noqa: E731
    assert rel(got["grad"], want["grad"]) < 1e-9 and rel(got["J"], want["J"]) < 1e-9, "the device differs from the numpy rule on its own pm / D"
    votes = int(np.count_nonzero(eio.contrast_votes(got["pm"], w.pano_w, w.pano_h)[1]))
    cells = min(w.pano_w * w.pano_h, 4 * nn)
    fixed = 24 * w.sensor_w * w.sensor_h + 112 * (nn // 100)                 # the bearing LUT and the pose table, once
    vote_bytes = 5 * nn + fixed + 16 * cells                                  # events; every touched cell of the zeroed fp64 image read and written once
    grad_bytes = 5 * nn + fixed + 8 * cells                                   # events; every touched cell read once
    m.close()
    return dict(shape=name, events=n, used=nn, K=w.K, sensor=[w.sensor_w, w.sensor_h], pano=[w.pano_h, w.pano_w], wall_ms_J_only=wall_j, wall_ms_J_and_grad=wall_g,
                slot7_us_vote=kern_j, slot7_us_vote_and_grad=kern_g, numpy_ms=host, numpy_reps=numpy_reps, image_adds=votes,
                model=dict(note="a model, not a measurement", vote_us_bytes_at_8TBps=vote_bytes / HBM_BYTES_PER_S * 1e6, vote_us_adds_at_23_per_ns=votes / ADDS_PER_NS * 1e-3,
                           grad_us_bytes_at_8TBps=grad_bytes / HBM_BYTES_PER_S * 1e6),
                J=got["J"], grad_max=float(np.abs(got["grad"]).max()), rel_grad_vs_numpy=rel(got["grad"], want["grad"]), rel_J_vs_numpy=rel(got["J"], want["J"]))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--numpy-reps", type=int, default=3)
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("contrast_gradient_timing.py measures on the GPU: none is visible")
    demo = synth.make_scene_workload(pano_h=512, K=11, sensor=(128, 96), focal=120.0, n_steps=2000)
    bench = synth.make_workload()
    doc = dict(shapes=[measure_shape("demo", demo, a.reps, a.warmup, a.numpy_reps), measure_shape("1M uniform", bench, a.reps, a.warmup, a.numpy_reps)])
    text = json.dumps(doc, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
