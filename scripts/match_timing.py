#!/usr/bin/env python3
"""Loop-closure pairs found by appearance (emba_frames_match_eval, emba_frames_match_search), on scripts/pair_timing.py's shape: 240 x 180
frames rendered on the device from a textured plane behind a 200-pixel pinhole, 100 frames out and back.  Stream time between two HIP events: median
(min - max) of --reps after --warmup.  Recorded, per level (2: 60 x 45, 3: 30 x 22):
  * the evaluation kernel over all F (F - 1) / 2 pairs of a search (timer slot 7), in overlap pixels per us;
  * the select kernel (timer slot 6);
  * the whole call of emba_frames_match_search (upload, thumbnails, evaluation, select, download);
  * beside it what the host pays today: io.pair_candidates of the tracked rotations, and numpy's io.match_search of the same frames (wall time).
Nothing measured here is asserted anywhere.  Writes --out (default profiles/match_timing.txt)."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from emba_amd import LEGM                                            # noqa: E402
from emba_amd import io as eio                                       # noqa: E402
from emba_amd import so3                                             # noqa: E402
from emba_amd.legm import LinearTrajectory                           # noqa: E402
from emba_amd.synth import pinhole_bearing_lut                       # noqa: E402

SW, SH, W, H = 240, 180, 2048, 1024
K, T0, DT = 11, 10**9, 10**8
FOCAL = 200.0
DRIFT_PX = 0.05
RANGE = {2: (8, 6), 3: (4, 3)}      # 32 pixels and 24 pixels at full resolution, at either level
GAP, PER_FRAME, SCORE_MIN = 4, 2, 0.5


def fmt(v, unit):
    v = sorted(v)
    return f"{v[len(v) // 2]:10.1f} {unit} ({v[0]:.1f} - {v[-1]:.1f})"


def med(v):
    return sorted(v)[len(v) // 2]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--frames", type=int, default=100)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "match_timing.txt"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("match_timing.py measures on the GPU: none is visible")
    F = a.frames
    out = [f"scripts/match_timing.py --reps {a.reps} --warmup {a.warmup} --frames {F}: median (min - max); {torch.cuda.get_device_name(0)}"]
    calib = eio.pair_calib(FOCAL, FOCAL, 0.5 * (SW - 1), 0.5 * (SH - 1))
    lut = pinhole_bearing_lut(SW, SH, FOCAL, FOCAL, calib["cu"], calib["cv"])
    m = LEGM(SW, SH, lut, 0.2, W, H)
    x, y = np.arange(W, dtype=np.float64)[None, :], np.arange(H, dtype=np.float64)[:, None]
    plane = 128.0 + 60.0 * np.sin(40.0 * np.pi * x / W) * np.cos(20.0 * np.pi * y / H) + 40.0 * np.cos(64.0 * np.pi * x / W + 3.0 * np.pi * y / H)
    traj = LinearTrajectory(np.array([so3.exp(np.array([0.0, 0.05 * (i if i <= K // 2 else K - 1 - i + 0.37), 0.0])) for i in range(K)]), T0, DT)
    ts = T0 + (np.arange(F, dtype=np.int64) * ((K - 1) * DT - 1)) // max(F - 1, 1)
    frames = m.render_views(ts, traj.knots_xyzw, T0, DT, plane=plane, want_u8=True, lo=0.0, hi=255.0)["u8"]
    q_true = np.array([traj.evaluate(int(t)) for t in ts])
    axis = np.array([0.3, 1.0, -0.2]) / np.linalg.norm([0.3, 1.0, -0.2])
    q = np.array([so3.mul(so3.exp(f * DRIFT_PX / FOCAL * axis), q_true[f]) for f in range(F)])
    status = np.array([1] + [2] * (F - 1), np.int32)
    pairs = F * (F - 1) // 2
    out.append(f"== {SW}x{SH} frames, F = {F} out and back: {pairs} pairs in the table; min_gap {GAP}, k = {PER_FRAME}, score_min {SCORE_MIN}, skip_zero, n_min a quarter of the thumbnail")
    m.enable_kernel_timing(True)
    for level in (2, 3):
        w, h = SW >> level, SH >> level
        rx, ry = RANGE[level]
        kw = dict(level=level, rx=rx, ry=ry, min_gap=GAP, skip_zero=True, n_min=w * h // 4, score_min=SCORE_MIN, k=PER_FRAME)
        whole, ev, sel, r = [], [], [], None
        for i in range(a.warmup + a.reps):
            m.timer_start(0)
            r = m.match_search(frames, status, **kw)
            m.timer_stop(0)
            m.sync()
            if i >= a.warmup:
                whole.append(m.timer_ms(0) * 1e3)
                ev.append(m.timer_ms(7) * 1e3)
                sel.append(m.timer_ms(6) * 1e3)
        shifts = (2 * rx + 1) * (2 * ry + 1)
        cand = sum(max(F - i - GAP - 1, 0) for i in range(F))
        overlap = sum((w - abs(dx)) * (h - abs(dy)) for dx in range(-rx, rx + 1) for dy in range(-ry, ry + 1))
        found = eio.match_pairs(r)
        out.append(f"  level {level} ({w} x {h}), range ({rx}, {ry}) = {shifts} shifts, {cand} candidate pairs: emba_frames_match_eval_kernel (byte form) {fmt(ev, 'us')}, "
                   f"{cand * overlap / med(ev):.0f} overlap pixels per us; emba_frames_match_select_kernel {fmt(sel, 'us')}; whole emba_frames_match_search {fmt(whole, 'us')}; "
                   f"{len(found)} pairs handed on")
        t0 = time.perf_counter()
        n = eio.match_search(frames, status, **kw)
        t_np = (time.perf_counter() - t0) * 1e6
        same = all(np.array_equal(n[k], r[k]) for k in ("partner", "shift", "n")) and np.array_equal(n["score"].view(np.uint64), r["score"].view(np.uint64))
        out.append(f"     numpy io.match_search on the host (fp64 matrix products per shift): {t_np:10.1f} us, once; the same result: {same}")
    cand = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        p = eio.pair_candidates(q, status, window=2, min_gap=GAP, max_angle=0.2, max_per_frame=PER_FRAME)
        cand.append((time.perf_counter() - t0) * 1e6)
    out.append(f"  io.pair_candidates of the tracked rotations on the host (what the search costs today): {fmt(cand, 'us')}; {len(p)} pairs")
    m.close()
    text = "\n".join(out) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
