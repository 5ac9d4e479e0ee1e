#!/usr/bin/env python3
"""Sensor views along the trajectory (emba_render_views, emba_seq_event_frames): what the two kernels cost.

240 x 180 views of a 1024 x 2048 panorama at F = 1000 frames, and event frames over 1 M events on the same sensor.  Stream time between two HIP events:
with emba_enable_kernel_timing on, timer slot 7 brackets the kernel of a call's first chunk (97 frames of views; every frame of the event frames, which are
asked for in one chunk); timer slot 0 brackets the whole call, uploads, chunks and copies to pageable host memory included.  Every figure: the median of
--reps calls after --warmup, with (min - max).

Each kernel is set against its byte model at the plain-copy rate of profiles/r06_stream_bw.txt (5.34 TB/s):
  view kernel          24 B of bearing LUT in, 8 B of frame (+ 1 B of 8-bit frame) out per pixel; the four gathers hit a patch of the panorama in L2
  event-frames kernel  13 B of event in (x, y 2 B each, polarity 1 B, t 8 B) and one int32 atomic add out per event — the adds also against the rate the
                       panorama's vote kernel measured for scattered int32 adds (23 adds per ns)
and the file says which of the two each kernel is nearer to.  Needs the GPU; writes --out (default profiles/view_timing.txt)."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from emba_amd import LEGM                                            # noqa: E402
from emba_amd import so3                                             # noqa: E402
from emba_amd.legm import EventPacket                                # noqa: E402
from emba_amd.synth import pinhole_bearing_lut                       # noqa: E402

COPY_TBS = 5.34          # profiles/r06_stream_bw.txt: copy (read + write) of 1.2 GB
ADDS_PER_NS = 23.0       # the vote kernel's scattered int32 adds at 1 M events
SW, SH, W, H = 240, 180, 2048, 1024
CHUNK_FRAMES = (32 << 20) // (SW * SH * 8)      # view_rule.h: view_chunk_frames


def fmt(v, unit):
    v = sorted(v)
    return f"{v[len(v) // 2]:9.1f} {unit} ({v[0]:.1f} - {v[-1]:.1f})"


def med(v):
    return sorted(v)[len(v) // 2]


def timed(m, reps, warmup, call):
    kern, whole = [], []
    for i in range(warmup + reps):
        m.timer_start(0)
        call()
        m.timer_stop(0)
        m.sync()
        if i >= warmup:
            kern.append(m.timer_ms(7) * 1e3)
            whole.append(m.timer_ms(0) * 1e3)
    return kern, whole


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--frames", type=int, default=1000)
    ap.add_argument("--events", type=int, default=1_000_000)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "view_timing.txt"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("view_timing.py measures on the GPU: none is visible")
    out = [f"scripts/view_timing.py --reps {a.reps} --warmup {a.warmup} --frames {a.frames} --events {a.events}: median (min - max); {torch.cuda.get_device_name(0)}"]
    rng = np.random.default_rng(0)
    m = LEGM(SW, SH, pinhole_bearing_lut(SW, SH, 200.0, 200.0, 0.5 * (SW - 1), 0.5 * (SH - 1)), 0.2, W, H)
    m.enable_kernel_timing(True)
    S = SW * SH

    # ---- views: a camera turning through 2 rad of yaw with a little pitch, F frames over the trajectory
    K, t0, dt = 11, 10**9, 10**8
    knots = np.array([so3.mul(so3.exp(np.array([0.0, 0.2 * i, 0.0])), so3.exp(np.array([0.1 * np.sin(i), 0.0, 0.0]))) for i in range(K)])
    ts = t0 + (np.arange(a.frames, dtype=np.int64) * ((K - 1) * dt - 1)) // max(a.frames - 1, 1)
    plane = rng.normal(size=(H, W))
    first = min(CHUNK_FRAMES, a.frames)
    out.append(f"== emba_render_views: {SW}x{SH} views of a {H}x{W} plane, F = {a.frames} ({-(-a.frames // CHUNK_FRAMES)} chunks of at most {CHUNK_FRAMES} frames)")
    for name, kw, px_bytes in (("fp64 frames", dict(), 24 + 8), ("fp64 + 8-bit frames", dict(want_u8=True, lo=-2.0, hi=2.0), 24 + 8 + 1)):
        kern, whole = timed(m, a.reps, a.warmup, lambda: m.render_views(ts, knots, t0, dt, plane=plane, **kw))
        model_us = first * S * px_bytes / (COPY_TBS * 1e12) * 1e6
        k = med(kern)
        out.append(f"  {name:20s}: view kernel of the first chunk ({first} frames) {fmt(kern, 'us')}   whole call, copies to the host included {fmt(whole, 'us')}")
        out.append(f"  {'':20s}  {k * 1e3 / (first * S):.3f} ns per pixel; byte model ({px_bytes} B per pixel at {COPY_TBS} TB/s) {model_us:.1f} us: the kernel takes {k / model_us:.2f} x that — "
                   + ("nearer to its byte model than to twice it: it streams" if k < 1.5 * model_us else
                      "nearer to its arithmetic (fp64 atan2, asin, sqrt and a division per pixel) than to its byte model"))

    # ---- event frames: uniform events over the sensor, sorted times, all frames in one chunk
    n = a.events
    ev = EventPacket(rng.integers(0, SW, n).astype(np.uint16), rng.integers(0, SH, n).astype(np.uint16), rng.integers(0, 2, n).astype(np.uint8),
                     10**9 + np.sort(rng.integers(0, 10**9, n)).astype(np.int64))
    m.set_sequence(ev)
    out.append(f"== emba_seq_event_frames: {n} events on {SW}x{SH}, every frame in one chunk")
    for F in (10, 100):
        edges = 10**9 + (np.arange(F + 1, dtype=np.int64) * 10**9) // F
        kern, whole = timed(m, a.reps, a.warmup, lambda: m.event_frames(0, n, edges))
        k = med(kern)
        byte_us, add_us = n * 13 / (COPY_TBS * 1e12) * 1e6, n / ADDS_PER_NS * 1e-3
        out.append(f"  F = {F:4d}: kernel {fmt(kern, 'us')}   whole call, copies to the host included {fmt(whole, 'us')}")
        out.append(f"            {k * 1e3 / n:.3f} ns per event; byte model (13 B per event at {COPY_TBS} TB/s) {byte_us:.2f} us; one scattered int32 add per event at "
                   f"{ADDS_PER_NS:g} per ns {add_us:.1f} us: nearer to the " + ("adds" if abs(k - add_us) < abs(k - byte_us) else "byte model"))
    m.close()
    text = "\n".join(out) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
