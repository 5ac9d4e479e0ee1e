#!/usr/bin/env python3
"""Wall time of the contrast maximisation of DESIGN.md §11 (LEGM.estimate_angular_velocity: one launch + the download of the per-slice results) on one
GPU, next to the numpy form (io.estimate_angular_velocity) on the same input and host, and whether both gave the same results.

  python scripts/cmax_timing.py [out.json]

Inputs: the demo recording of examples/run_ba.py (128x96, about 266 k events) and the 1 M-event 240x180 stream of synth.make_workload, slices of 10 000
events, omega_max 8.  Device: one warm-up call (allocations, code load), then the median, minimum and maximum of 7 calls timed with time.perf_counter
(every call ends in a host synchronisation).  numpy: one call."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from emba_amd import LEGM, io as eio, synth      # noqa: E402


def bench(name, w, m=10000, wmax=8.0, reps=7):
    legm = LEGM(w.sensor_w, w.sensor_h, w.lut, w.C_th, w.pano_w, w.pano_h, device=0)
    legm.set_sequence(w.events)
    est = legm.estimate_angular_velocity(m, wmax)
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        est = legm.estimate_angular_velocity(m, wmax)
        ts.append(time.perf_counter() - t0)
    t0 = time.perf_counter()
    ref = eio.estimate_angular_velocity(w.events, w.lut, w.sensor_w, w.sensor_h, m, wmax)
    t_np = time.perf_counter() - t0
    r = dict(name=name, events=w.events.size(), sensor=[w.sensor_w, w.sensor_h], slices=len(est["omega"]), evals=int(est["evals"].sum()),
             device_ms_median=1e3 * float(np.median(ts)), device_ms_min=1e3 * min(ts), device_ms_max=1e3 * max(ts), numpy_s=t_np,
             equal=bool(all(np.array_equal(est[k], ref[k]) for k in est)))
    print(json.dumps(r), flush=True)
    legm.close()
    return r


def main():
    out = [bench("demo", synth.make_scene_workload(pano_h=512, K=11, sensor=(128, 96), focal=120.0, n_steps=2000)),
           bench("1M 240x180", synth.make_workload())]
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
