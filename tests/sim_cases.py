"""The cases of the event-simulator tests, shared by tests/test_sim_cpu.py (the numpy form; that numpy's own pm of every case keeps clear
of the pole rows) and tests/test_gpu_sim.py (the device against the numpy form): the sensors, panoramas and trajectories of tests/view_cases.py, planes whose
change across the field of view is several thresholds, and step times from the first knot to the last time the numpy spline accepts."""
import numpy as np

import view_cases as VC

C_ON, C_OFF = 0.11, 0.07          # c_on != c_off
STEPS = (1, 3, 65)
STEEP = 20.0                      # the steep plane: twenty times the amplitude, for the cap at 1 and 2
CHUNK_BYTES = 32 << 20            # the cap of a chunk of fp64 samples (include/emba_hip.h: emba_simulate_events)
LONG_DT_NS = 2_000_000_000        # knots 2 s apart: the three segments span 6 s > 2^32 ns, so a chunk's sort takes two passes


def step_times(F, dt_ns=VC.DT_NS):
    """F + 1 step times from the first knot to the last accepted time."""
    t_last = VC.T0_NS + (VC.K - 1) * dt_ns - 1
    t = VC.T0_NS + (np.arange(F + 1, dtype=np.int64) * (t_last - VC.T0_NS)) // F
    assert t[0] == VC.T0_NS and t[-1] == t_last and (np.diff(t) > 0).all()
    return t


def plane_of(pano, amp=1.0):
    return amp * VC.plane_of(pano)


def chunk_edge_steps(S):
    """An F that crosses the chunk edge by three steps on a sensor of S pixels: the chunk is as many steps of S fp64 samples as the cap in bytes holds."""
    return CHUNK_BYTES // (S * 8) + 3


def gpu_cases():
    """(sensor, pano, kind, dt_ns, step times) of every simulation tests/test_gpu_sim.py runs on the view cases."""
    out = []
    for sensor in VC.SENSORS:
        for pano in VC.PANOS:
            for kind in VC.KINDS:
                for F in STEPS:
                    out.append((sensor, pano, kind, VC.DT_NS, step_times(F)))
    out.append((VC.SENSORS[1], VC.PANOS[0], "yaw_pi", LONG_DT_NS, step_times(3, LONG_DT_NS)))
    out.append((VC.SENSORS[2], VC.PANOS[0], "pitch", VC.DT_NS, step_times(chunk_edge_steps(VC.SENSORS[2][0] * VC.SENSORS[2][1]))))
    return out


def scalar_simulation(views, outside, step_t, sw, c_on, c_off, max_per_step):
    """The rule of emba_simulate_events, one pixel and one event at a time in python floats and ints.  Returns (x, y, pol, t) lists in the output order and
    the four stats."""
    F, S = len(step_t) - 1, len(views[0])
    events, n_cap, n_out = [], 0, 0
    for s in range(S):
        armed, ref = False, 0.0
        for f in range(F + 1):
            if outside[f][s]:
                n_out += 1
                armed = False
                continue
            cur = float(views[f][s])
            if not armed:
                ref, armed = cur, True
                continue
            prev, d, k = float(views[f - 1][s]), int(step_t[f]) - int(step_t[f - 1]), 0
            while True:
                sgn, C = (1.0, c_on) if cur - ref > 0.0 else (-1.0, c_off)
                if not abs(cur - ref) >= C:
                    break
                if k == max_per_step:
                    n_cap += 1
                    break
                ref = ref + sgn * C
                num, den = ref - prev, cur - prev
                if den == 0.0:
                    frac = float("nan") if (num == 0.0 or num != num) else (float("inf") if (num > 0.0) == (np.copysign(1.0, den) > 0.0) else float("-inf"))
                else:
                    frac = num / den
                if not frac >= 0.0:
                    frac = 0.0
                elif frac > 1.0:
                    frac = 1.0
                off = min(int(frac * float(d)), d - 1)
                events.append((int(step_t[f - 1]) + off, s, f, k, 1 if sgn > 0.0 else 0))
                k += 1
    events.sort(key=lambda e: (e[0], e[1], e[2], e[3]))      # ascending t, then pixel, then emission (a later step has later times: f never decides)
    x, y, pol, t = [e[1] % sw for e in events], [e[1] // sw for e in events], [e[4] for e in events], [e[0] for e in events]
    return (x, y, pol, t), (len(events), sum(pol), n_cap, n_out)
