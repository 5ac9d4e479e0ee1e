#!/usr/bin/env python3
"""Wall time of the sensor-noise filters on a whole recording, two ways (240x180 sensor, all three filters on):
  (a) emba_seq_filter on the sequence already resident in HBM (LEGM.filter_sequence): sort by pixel, starts, flags, scan, gather, all on the device
  (b) what a user would do without it: io.filter_events on the host (numpy), then the survivors uploaded again (LEGM.set_sequence)
The recording: the BASELINE event stream (i.i.d. uniform pixels, 1 s) plus synth.add_sensor_noise — 40 hot pixels and 2 % background events.  The filter
replaces the resident sequence, so every repetition of (a) starts from a fresh upload, which is timed on its own and not counted.  Both ways must leave
the same sequence; the script checks that before it reports.  Times end in a host synchronisation (the calls return the statistics / the count).

  python scripts/seq_filter_timing.py [--events 1000000 10000000] [--reps 5] [--out profiles/seq_filter_timing.txt]"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from emba_amd import LEGM, io as eio, synth      # noqa: E402

MS = 1_000_000


def stats(v):
    v = np.sort(np.asarray(v))
    return f"median {np.median(v):9.3f}  min {v[0]:9.3f}  max {v[-1]:9.3f}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--events", type=int, nargs="+", default=[1_000_000, 10_000_000])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--hot-sigma", type=float, default=5.0)
    ap.add_argument("--refractory-us", type=float, default=100.0)
    ap.add_argument("--support-ms", type=float, default=5.0)
    ap.add_argument("--out")
    a = ap.parse_args()
    refr, supp = int(a.refractory_us * 1000), int(a.support_ms * MS)
    lines = [f"# sensor-noise filters on a whole recording: hot_sigma {a.hot_sigma}, refractory {a.refractory_us} us, support {a.support_ms} ms; times in ms (wall, host clock,",
             f"# every call ends in a synchronisation); 1 warm-up + {a.reps} timed device runs, 1 + {a.host_reps} host runs per size"]
    for n in a.events:
        w = synth.make_workload(n_events=int(n * 0.97), pano_h=256)
        ev, hot = synth.add_sensor_noise(w.events, (w.sensor_w, w.sensor_h), n_hot=40, hot_events_each=int(n * 0.01) // 40, n_background=int(n * 0.02), seed=1)
        m = LEGM(w.sensor_w, w.sensor_h, w.lut, w.C_th, w.pano_w, w.pano_h)
        t_up, t_dev, t_host, t_reup = [], [], [], []
        st = None
        for k in range(1 + a.reps):
            t0 = time.perf_counter()
            m.set_sequence(ev, 1)
            t1 = time.perf_counter()
            st = m.filter_sequence(a.hot_sigma, refr, supp, 1)
            t2 = time.perf_counter()
            if k:
                t_up.append((t1 - t0) * 1e3); t_dev.append((t2 - t1) * 1e3)
        dev_seq = m.sequence_events(0, m.sequence_size())
        dev_hot = m.sequence_hot_pixels()
        for k in range(1 + a.host_reps):
            t0 = time.perf_counter()
            kept, hst, hmask = eio.filter_events(ev, w.sensor_w, w.sensor_h, a.hot_sigma, refr, supp)
            t1 = time.perf_counter()
            m.set_sequence(kept, 1)
            t2 = time.perf_counter()
            if k:
                t_host.append((t1 - t0) * 1e3); t_reup.append((t2 - t1) * 1e3)
        same = all(np.array_equal(p, q) for p, q in zip((dev_seq.x, dev_seq.y, dev_seq.polarity, dev_seq.t_ns), (kept.x, kept.y, kept.polarity, kept.t_ns)))
        same = same and np.array_equal(dev_hot, hmask) and [int(v) for v in st] == [int(v) for v in hst]
        assert same, "the device and the host filter disagree"
        s = [int(v) for v in st]
        lines.append(f"{ev.size()} events ({w.sensor_w}x{w.sensor_h}): {s[1]} hot pixels ({s[2]} events; {np.isin(hot, np.flatnonzero(dev_hot)).sum()} of the {hot.size} injected), "
                     f"{s[3]} inside the refractory period, {s[4]} without support, {s[5]} kept; device == host: {same}")
        lines.append(f"  upload of the raw recording (emba_seq_upload, not counted)      {stats(t_up)}")
        lines.append(f"  (a) emba_seq_filter on the resident sequence                    {stats(t_dev)}")
        lines.append(f"  (b) io.filter_events on the host                                {stats(t_host)}")
        lines.append(f"  (b) + upload of its survivors                                   {stats(np.array(t_host) + np.array(t_reup))}")
        lines.append(f"  (b) / (a), medians: {np.median(np.array(t_host) + np.array(t_reup)) / np.median(t_dev):.1f}")
        m.close()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
