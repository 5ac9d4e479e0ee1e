#!/usr/bin/env python3
"""Boundary EMBA_POISSON_WRAP_X of the intensity panorama (emba_reconstruct_intensity_bc): what it costs next to the reference's boundary.

Both calls on the resident map of one context, no host copies in the timed region (download=False): the stream time of the whole call between two HIP
events (emba_timer_start / _stop around it) and the wall time of the call, at 1024 x 2048 and 2048 x 4096.  The two boundaries alternate call by call, so
that both see the same clocks.  The tables (sine matrices, Thomas factors, q) are built by a first call of each, outside the timed region.  Against the
difference: the closing pass reads two planes and writes one, 24 bytes per pixel, at the plain-copy rate of profiles/r06_stream_bw.txt (5.34 TB/s).

Every figure: the median of --reps calls after --warmup, with (min - max).  Needs the GPU; writes --out (default profiles/poisson_wrap_timing.txt)."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from emba_amd import LEGM                                            # noqa: E402
from emba_amd.synth import pinhole_bearing_lut                       # noqa: E402

COPY_TBS = 5.34      # profiles/r06_stream_bw.txt: copy (read + write) of 1.2 GB


def fmt(v, unit):
    v = sorted(v)
    return f"{v[len(v) // 2]:9.1f} {unit} ({v[0]:.1f} - {v[-1]:.1f})"


def measure_shape(H, W, reps, warmup, out):
    m = LEGM(64, 48, pinhole_bearing_lut(64, 48, 60., 60., 32., 24.), 0.2, W, H)
    rng = np.random.default_rng(H)
    m.upload_map(rng.normal(size=(H, W)), rng.normal(size=(H, W)))
    for b in ("dirichlet", "wrap"):
        m.reconstructIntensity(download=False, boundary=b)      # builds the tables
    ev, wall = {"dirichlet": [], "wrap": []}, {"dirichlet": [], "wrap": []}
    for i in range(warmup + reps):
        for b in ("dirichlet", "wrap"):
            t = time.perf_counter()
            m.timer_start(0)
            m.reconstructIntensity(download=False, boundary=b)
            m.timer_stop(0)
            m.sync()
            dt = (time.perf_counter() - t) * 1e6
            if i >= warmup:
                ev[b].append(m.timer_ms(0) * 1e3)
                wall[b].append(dt)
    m.close()
    out.append(f"== {H}x{W}, resident map")
    for b in ("dirichlet", "wrap"):
        out.append(f"  boundary {b:9s}: stream {fmt(ev[b], 'us')}   wall {fmt(wall[b], 'us')}")
    med = {b: sorted(ev[b])[len(ev[b]) // 2] for b in ev}
    spread = max(ev["dirichlet"]) - min(ev["dirichlet"])
    close_us = 24.0 * H * W / (COPY_TBS * 1e12) * 1e6
    out.append(f"  wrap - dirichlet: {med['wrap'] - med['dirichlet']:+.1f} us of stream time (median against median); dirichlet's own min-max spread {spread:.1f} us; "
               f"the closing pass at the plain-copy rate ({COPY_TBS} TB/s, 24 B per pixel): {close_us:.1f} us")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "poisson_wrap_timing.txt"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("poisson_wrap_timing.py measures on the GPU: none is visible")
    out = [f"scripts/poisson_wrap_timing.py --reps {a.reps} --warmup {a.warmup}: median (min - max); {torch.cuda.get_device_name(0)}"]
    for H, W in ((1024, 2048), (2048, 4096)):
        measure_shape(H, W, a.reps, a.warmup, out)
    text = "\n".join(out) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
