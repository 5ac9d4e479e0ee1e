#!/usr/bin/env python3
"""Per-window set-up time of a sliding-window run, two ways of registering the same window, in one session on one context:
  (a) emba_set_events_seq(beg, end)   a range of the sequence resident in HBM (validated and batched on the device, device radix sort)
  (b) emba_set_events(host slice)     the host slice of the same events (host validation + batch midpoints, 5 B/event over PCIe, the same sort)
Both read back from emba_last_setup_ms (wall time of the registration, which ends in a stream synchronisation).  The stream: the BASELINE workload
(1 M i.i.d. events, 240x180 sensor, 1024x2048 panorama, 1 s) cut into four half-overlapping windows of 0.4 s.  Warm-up registrations of every window first,
then `--reps` alternating pairs; median, min, max and the 10th / 90th percentiles are printed.

  python scripts/sliding_window_setup.py [--events 1000000] [--reps 20] [--out profiles/sliding_window_setup.txt]"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from emba_amd import LEGM, EventWindow, io as eio, synth      # noqa: E402


def stats(v):
    v = np.sort(np.asarray(v))
    return f"median {np.median(v):7.3f}  min {v[0]:7.3f}  p10 {np.percentile(v, 10):7.3f}  p90 {np.percentile(v, 90):7.3f}  max {v[-1]:7.3f}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--events", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out")
    a = ap.parse_args()
    w = synth.make_workload(n_events=a.events)
    m = LEGM(w.sensor_w, w.sensor_h, w.lut, w.C_th, w.pano_w, w.pano_h, device=0)
    lines = [f"# sliding-window set-up: {w.describe()}", f"# {a.warmup} warm-up + {a.reps} timed registrations per window and path, alternating; times in ms (emba_last_setup_ms)"]
    up = []
    for _ in range(a.warmup + 5):
        t0 = time.perf_counter()
        m.set_sequence(w.events, 1)
        up.append((time.perf_counter() - t0) * 1e3)
    lines.append(f"emba_seq_upload of the whole sequence ({w.events.size()} events, once per run): {stats(up[a.warmup:])}")
    MS = 1_000_000
    wins = []
    for k in range(4):
        tb, te = (100 + 200 * k) * MS, (500 + 200 * k) * MS
        beg, end = m.sequence_window(tb, te)
        assert (beg, end) == eio.event_window(w.events.t_ns, tb, te)
        wins.append((beg, end, eio.slice_events(w.events, beg, end)))
    tw = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        m.sequence_window(300 * MS, 700 * MS)
        tw.append((time.perf_counter() - t0) * 1e3)
    lines.append(f"emba_seq_window (wall, one launch + readback): {stats(tw)}")
    for k, (beg, end, sl) in enumerate(wins):
        ta, tb_ = [], []
        for r in range(a.warmup + a.reps):
            m.set_events(EventWindow(beg, end))
            x = m.setup_info()["set_events_ms"]
            m.set_events(sl)
            y = m.setup_info()["set_events_ms"]
            if r >= a.warmup:
                ta.append(x); tb_.append(y)
        lines.append(f"window {k}: events [{beg}, {end}) = {end - beg}")
        lines.append(f"    (a) emba_set_events_seq        {stats(ta)}")
        lines.append(f"    (b) emba_set_events host slice {stats(tb_)}")
        lines.append(f"    (a) / (b) of the medians       {np.median(ta) / np.median(tb_):.3f}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
