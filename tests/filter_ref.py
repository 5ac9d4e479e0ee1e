"""An independent restatement of the sensor-noise filters (include/emba_hip.h: emba_seq_filter) in plain python loops — nothing here imports
emba_amd.  A time surface (sensor pixel -> timestamp of its latest event so far) is walked event by event; the hot-pixel rule comes from integer sums;
survivors and sampling are the counting loop of emba.cpp:281-304.  What tests/test_filter_cpu.py compares emba_amd.io.filter_events with, and
tests/test_gpu_filter.py the device form."""
import math

import numpy as np


def hot_pixels(x, y, sw, sh, hot_sigma):
    """[S] booleans: pixel p = y * sw + x is hot iff float(c[p]) > mean + hot_sigma * sqrt(var) over the pixels with events (python floats: every
    operation rounded on its own)."""
    c = [0] * (sw * sh)
    for k in range(len(x)):
        c[int(y[k]) * sw + int(x[k])] += 1
    m = s1 = s2 = 0
    for v in c:
        if v > 0:
            m += 1
            s1 += v
            s2 += v * v
    if hot_sigma <= 0 or m == 0:
        return [False] * (sw * sh)
    mean = float(s1) / float(m)
    var = float(s2) / float(m) - mean * mean
    if var < 0.0:
        var = 0.0
    thr = mean + hot_sigma * math.sqrt(var)
    return [float(v) > thr for v in c]


def filter_loops(x, y, pol, t, sw, sh, hot_sigma=0.0, refractory_ns=0, support_ns=0, sampling_rate=1):
    """Returns ((x, y, pol, t) of the events kept, stats[6] as python ints, hot mask uint8[S])."""
    if hot_sigma != hot_sigma:
        raise ValueError("hot_sigma is NaN")
    n = len(t)
    hot = hot_pixels(x, y, sw, sh, hot_sigma)
    last = {}                           # the time surface
    n_hot = n_ref = n_sup = 0
    survivors = []
    for k in range(n):
        xk, yk, tk = int(x[k]), int(y[k]), int(t[k])
        p = yk * sw + xk
        f_hot = hot[p]
        f_ref = refractory_ns > 0 and p in last and tk - last[p] < refractory_ns
        f_sup = False
        if support_ns > 0:
            f_sup = True
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    qx, qy = xk + dx, yk + dy
                    if (dx == 0 and dy == 0) or qx < 0 or qx >= sw or qy < 0 or qy >= sh:
                        continue
                    q = qy * sw + qx
                    if not hot[q] and q in last and tk - last[q] <= support_ns:
                        f_sup = False
        last[p] = tk                    # whether or not the event survives
        n_hot += f_hot
        n_ref += f_ref
        n_sup += f_sup
        if not (f_hot or f_ref or f_sup):
            survivors.append(k)
    keep = survivors
    if sampling_rate >= 2:              # emba.cpp:281-304 over the survivors
        keep = []
        sampling_count = 1
        for k in survivors:
            if sampling_count == sampling_rate:
                keep.append(k)
                sampling_count = 1
            else:
                sampling_count += 1
    idx = np.array(keep, dtype=np.int64)
    stats = [n, sum(hot), n_hot, n_ref, n_sup, len(keep)]
    return (np.asarray(x)[idx], np.asarray(y)[idx], np.asarray(pol)[idx], np.asarray(t)[idx]), stats, np.array(hot, dtype=np.uint8)
