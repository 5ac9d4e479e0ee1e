#!/usr/bin/env python3
"""The panorama of warped events (emba_seq_event_panorama): what nobody had measured.

  * wall time of LEGM.event_panorama without the image download against the numpy form (io.event_panorama) on the same host, on the demo recording of
    examples/run_ba.py (128x96 on 512x1024) and on 1 M uniform events at 240x180 on 1024x2048 — a host clock around calls that end in a device synchronise
  * the vote kernel's time from HIP events at both shapes (emba_enable_kernel_timing: timer slot 7), beside the time an 8 TB/s memory system needs for the
    bytes the kernel has to move
  * J(truth) / J(identity) and J(contrast-maximisation estimate) / J(identity) over the whole of the two recordings of DESIGN.md §11

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
from emba_amd.legm import LinearTrajectory                            # noqa: E402

HBM_BYTES_PER_S = 8.0e12


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


def vote_kernel_bytes(n_used, sw, sh, W, H):
    """What the vote kernel has to move at the least: the events' x, y, polarity (5 B each), the bearing LUT and the pose table once, and every cell of
    the zeroed image that an add touches read and written once — at most the whole image, at most 4 cells per event."""
    cells = min(W * H, 4 * n_used)
    return 5 * n_used + 24 * sw * sh + 112 * (n_used // 100) + 8 * cells


def measure_shape(name, w, reps, warmup, numpy_reps):
    m = LEGM(w.sensor_w, w.sensor_h, w.lut, w.C_th, w.pano_w, w.pano_h)
    n = m.set_sequence(w.events)
    nn = n // 100 * 100
    dev = timed(lambda: m.event_panorama(w.traj, 0, n, want_image=False), reps, warmup)
    dev_img = timed(lambda: m.event_panorama(w.traj, 0, n), reps, warmup)
    m.enable_kernel_timing(True)
    kern = []
    for i in range(warmup + reps):
        m.event_panorama(w.traj, 0, n, want_image=False)
        if i >= warmup:
            kern.append(m.timer_ms(7) * 1e3)
    m.enable_kernel_timing(False)
    host = timed(lambda: eio.event_panorama(w.events, w.lut, w.sensor_w, w.sensor_h, w.pano_w, w.pano_h, w.traj), numpy_reps, 1)
    got = m.event_panorama(w.traj, 0, n, want_pm=True)
    same = eio.event_panorama(w.events, None, w.sensor_w, w.sensor_h, w.pano_w, w.pano_h, None, 0, n, pm=got["pm"])
    assert np.array_equal(same["image"], got["image"]) and same["J"] == got["J"], "the device image differs from the numpy rule on its own pm"
    b = vote_kernel_bytes(nn, w.sensor_w, w.sensor_h, w.pano_w, w.pano_h)
    m.close()
    return dict(shape=name, events=n, used=nn, sensor=[w.sensor_w, w.sensor_h], pano=[w.pano_h, w.pano_w], device_ms_no_image=dev, device_ms_with_image=dev_img,
                numpy_ms=host, numpy_reps=numpy_reps, vote_kernel_us=stats(kern), vote_kernel_bytes=b, model_us_at_8TBps=b / HBM_BYTES_PER_S * 1e6,
                atomic_adds=int(np.count_nonzero(eio.pano_votes(got["pm"], w.pano_w, w.pano_h)[1])), J=got["J"], nonzero=got["nonzero"])


def contrast_ratios(name, w, slice_events):
    """J over the whole recording at the true trajectory, at the integrated contrast-maximisation estimate and at the identity."""
    m = LEGM(w.sensor_w, w.sensor_h, w.lut, w.C_th, w.pano_w, w.pano_h)
    n = m.set_sequence(w.events)
    est = m.estimate_angular_velocity(slice_events, 8.0)
    tq = w.traj.t0_ns + w.traj.dt_ns * np.arange(w.K, dtype=np.int64)
    cm = LinearTrajectory(eio.integrate_angular_velocity(est["omega"], est["t_ref_ns"], tq)[1], w.traj.t0_ns, w.traj.dt_ns)
    ident = LinearTrajectory(np.tile([0.0, 0.0, 0.0, 1.0], (w.K, 1)), w.traj.t0_ns, w.traj.dt_ns)
    J = {k: m.event_panorama(t, 0, n, want_image=False)["J"] for k, t in (("truth", w.traj), ("cmax", cm), ("identity", ident))}
    m.close()
    return dict(recording=name, events=n, slice_events=slice_events, J=J, truth_over_identity=J["truth"] / J["identity"], cmax_over_identity=J["cmax"] / J["identity"])


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--numpy-reps", type=int, default=7)
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("event_panorama_timing.py measures on the GPU: none is visible")
    demo = synth.make_scene_workload(pano_h=512, K=11, sensor=(128, 96), focal=120.0, n_steps=2000)
    bench = synth.make_workload()
    scene = synth.make_scene_workload()
    doc = dict(shapes=[measure_shape("demo", demo, a.reps, a.warmup, a.numpy_reps), measure_shape("1M uniform", bench, a.reps, a.warmup, a.numpy_reps)],
               contrast=[contrast_ratios("scene workload", scene, 2000), contrast_ratios("demo", demo, 10000)])
    text = json.dumps(doc, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
