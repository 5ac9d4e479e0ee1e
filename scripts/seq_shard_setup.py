#!/usr/bin/env python3
"""Registration time of one time-sharded window, two ways, on a group whose ranks share device 0 (what a one-GPU box can run):
  (a) emba_group_set_events_seq(beg, end)   every rank registers its range of the sequence resident in ITS context, halo built on the device
  (b) emba_group_set_events(host slice)     the host sweeps the slice for the halos, every rank's events and halo cross PCIe, host validation
Wall time of the call (all ranks) and emba_last_setup_ms of every rank (wall time of that rank's registration; in (a) the ranks register side by side from
their threads, in (b) one after the other from the caller's).  The window: 1 M events of the BASELINE workload (240x180 sensor, 1024x2048 panorama) behind
100 000 events of lead, so win_beg > 0.  Also the halo passes on their own (emba_seq_halo, count only: three passes + the scan + one 4-byte read).

  python scripts/seq_shard_setup.py [--events 1000000] [--ranks 2] [--reps 20] [--out profiles/seq_shard_setup.txt]"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from emba_amd import _lib, synth      # noqa: E402


def stats(v):
    v = np.sort(np.asarray(v))
    return f"median {np.median(v):7.3f}  min {v[0]:7.3f}  p10 {np.percentile(v, 10):7.3f}  p90 {np.percentile(v, 90):7.3f}  max {v[-1]:7.3f}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--events", type=int, default=1_000_000)
    ap.add_argument("--lead", type=int, default=100_000)
    ap.add_argument("--ranks", type=int, default=2)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out")
    a = ap.parse_args()
    L = _lib.load()
    n = a.events + a.lead
    w = synth.make_workload(n_events=n)
    ev = w.events
    x, y, pol, t = (np.ascontiguousarray(v, d) for v, d in ((ev.x, np.uint16), (ev.y, np.uint16), (ev.polarity, np.uint8), (ev.t_ns, np.int64)))
    P = lambda v, ty: v.ctypes.data_as(ty)
    lut = np.ascontiguousarray(w.lut, dtype=np.float64)
    cfg = _lib.EmbaCfg(w.sensor_w, w.sensor_h, w.pano_w, w.pano_h, P(lut, _lib._dp), float(w.C_th), 100, 10.0, 0, None)
    g = C.c_void_p()
    devs = (C.c_int32 * a.ranks)(*([0] * a.ranks))
    assert L.emba_group_create(C.byref(cfg), devs, a.ranks, C.byref(g)) == 0, L.emba_group_last_error(None)
    lines = [f"# time-sharded window set-up: {a.events} events of {w.describe()} behind {a.lead} events of lead, {a.ranks} ranks on device 0",
             f"# {a.warmup} warm-up + {a.reps} timed registrations per path, alternating; times in ms; measured on ONE device (ranks share it)"]
    try:
        t0 = time.perf_counter()
        assert L.emba_group_seq_upload(g, P(x, _lib._u16p), P(y, _lib._u16p), P(pol, _lib._u8p), P(t, _lib._i64p), n, 1, None) == 0, L.emba_group_last_error(g)
        lines.append(f"emba_group_seq_upload of {n} events to every rank's context (once per run, first call): {(time.perf_counter() - t0) * 1e3:.3f}")
        beg, end = a.lead, n
        sl = tuple(v[beg:end] for v in (x, y, pol, t))

        def rank_ms():
            out = []
            for r in range(a.ranks):
                ms = C.c_double(0)
                assert L.emba_last_setup_ms(L.emba_group_ctx(g, r), C.byref(ms), None, None, None, None) == 0
                out.append(ms.value)
            return out

        wall = {"resident": [], "host": []}
        per_rank = {"resident": [], "host": []}
        for k in range(a.warmup + a.reps):
            for path in ("resident", "host"):
                t0 = time.perf_counter()
                if path == "resident":
                    st = L.emba_group_set_events_seq(g, beg, end)
                else:
                    st = L.emba_group_set_events(g, P(sl[0], _lib._u16p), P(sl[1], _lib._u16p), P(sl[2], _lib._u8p), P(sl[3], _lib._i64p), end - beg)
                dt = (time.perf_counter() - t0) * 1e3
                assert st == 0, L.emba_group_last_error(g)
                if k >= a.warmup:
                    wall[path].append(dt); per_rank[path].append(rank_ms())
        for path, name in (("resident", "(a) emba_group_set_events_seq"), ("host", "(b) emba_group_set_events on the slice")):
            lines.append(f"{name}: wall, all ranks   {stats(wall[path])}")
            pr = np.array(per_rank[path])
            for r in range(a.ranks):
                lines.append(f"{name}: emba_last_setup_ms rank {r}   {stats(pr[:, r])}")
        lines.append(f"wall (b) / (a), medians: {np.median(wall['host']) / np.median(wall['resident']):.2f}")
        # the halo passes alone, per rank (rank r begins at lo_r): count only, so three passes + scan + the 4-byte read, no download
        nb = (end - beg) // 100
        b = 0
        for r in range(a.ranks):
            lo = beg + 100 * b
            b += nb // a.ranks + (1 if r < nb % a.ranks else 0)
            th, cnt = [], C.c_size_t(0)
            for k in range(a.warmup + a.reps):
                t0 = time.perf_counter()
                assert L.emba_seq_halo(L.emba_group_ctx(g, r), beg, lo, None, None, None, 0, C.byref(cnt)) == 0
                if k >= a.warmup:
                    th.append((time.perf_counter() - t0) * 1e3)
            lines.append(f"halo of rank {r} alone ({lo - beg} events in front, {cnt.value} entries): wall {stats(th)}")
    finally:
        L.emba_group_destroy(g)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
