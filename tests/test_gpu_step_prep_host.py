"""The steady step with its segment records formed on the HOST (option step_prep = 2) against the launch in front of the warp kernel (step_prep = 0) (-m gpu).

On clean accumulator lines and fresh texels the host computes the K - 1 records {p0, delta, r1, k, r2} with the launch's own chain (seg_record_rule.h) and the
pixel-order warp kernel takes them by value in its arguments; its workgroup 0 leaves them in device memory.  The host's atan / sin / cos are the C library's,
the launch's the device library's: the records agree to the last bits, not always in them, so ep and the equations are held to helpers.assert_close and only
the integer results — count map, active set, the counts — must be identical.

Shapes: a 24 x 16 sensor on a 128 x 64 panorama, 4 k events = 64 one-wave workgroups (every XCD); K = 3 (two records), 21 (the benchmark's), seg_by_value + 1
(the last whose records fit the arguments) and seg_by_value + 2 (the first that keeps the launch: identical in every bit to step_prep = 0).

The records in device memory are read back after every step (emba_dump_segments: a plain copy of d_seg) and compared word by word, all 12 words of all K - 1
records, populated segment or not: p0 identical, delta, r1, k and r2 within the CPU test's measured bounds (tests/test_seg_record_rule_cpu.py: WORD_TOL — 4 x the
distance of the device's own records from the oracle, per quantity: 8.9e-16, 4.4e-16, 8.9e-16, 3.1e-15); where both took the launch, identical.  The dump's warp kernel
re-evaluates every event from those records: pm and D are compared too.  test_the_launch_still_forms_the_fixture_records ties that measurement to the device.
"""
import copy

import numpy as np
import pytest

from helpers import assert_close, oracle_run, small_workload
from test_gpu_parity import compare_normal_eq
from test_seg_record_rule_cpu import DEVICE, GOLD, WORD_TOL

pytestmark = pytest.mark.gpu

W_PANO = 128


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from emba_amd import build
    build.build_hip()
    return True


@pytest.fixture
def contexts():
    from emba_amd import LEGM
    made = []

    def make(w, **opts):
        m = LEGM(w.sensor_w, w.sensor_h, w.lut, w.C_th, w.pano_w, w.pano_h, device=0)
        made.append(m)
        for k, v in opts.items():
            m.set_option(k, v)
        m.set_events(w.events)
        m.upload_map(w.Gx, w.Gy)
        return m

    yield make
    for m in made:
        m.close()


_WORKLOADS = {}


def workload(K):
    if K not in _WORKLOADS:      # (made once per K and left unchanged)
        _WORKLOADS[K] = small_workload(n_events=4000, pano_h=64, K=K, sensor=(24, 16), focal=20.0, dt_knots=0.25 / (K - 1))
        assert _WORKLOADS[K].pano_w == W_PANO
    return _WORKLOADS[K]


def moved(traj, which, eps):
    """A copy of the trajectory with control pose `which` (None: all of them) rotated a little."""
    t = copy.deepcopy(traj)
    k = t.knots_xyzw.copy()
    rows = slice(None) if which is None else slice(which, which + 1)
    k[rows, 0] += eps
    k[rows] /= np.linalg.norm(k[rows], axis=1, keepdims=True)
    t.knots_xyzw = k
    return t


def step(m, w, traj, dump=False):
    n_inl, P = m.step(traj, w.thres_valid_pixel, w.alpha)
    ne = m._finish(w.alpha, False)
    _, ep, nem = m.eval_finish(want_ep=True, want_map=True)
    r = dict(n_inl=n_inl, P=P, ne=ne, ep=ep, nem=nem, on_host=m.get_option("prep_on_host"), in_warp=m.get_option("prep_in_warp"), packed=m.get_option("texels_packed"))
    r["seg"] = m.dump_segments()
    assert r["seg"].shape == (m.K - 1, 12)
    if dump:
        r["dump"] = m.dump_state(fields=("pm", "D"))
    return r


def close(a, b, what, bitwise=False):
    """step_prep = 2 (a) against step_prep = 0 (b): integers identical, sums within the suite's bounds; bitwise: both took the launch."""
    assert a["n_inl"] == b["n_inl"] and a["P"] == b["P"], what
    assert a["n_inl"] > 0, what
    assert np.array_equal(a["nem"], b["nem"]), what + ": count map"
    assert np.array_equal(a["ne"]["active"], b["ne"]["active"]), what + ": active set"
    if bitwise:
        assert np.array_equal(a["ep"], b["ep"]), what + ": ep differs in some bit"
    else:
        assert_close(a["ep"], b["ep"], f"ep {what}")
    for k in ("A11", "b1", "A22", "b2"):
        assert_close(a["ne"][k], b["ne"][k], f"{k} {what}")
    d = np.abs(a["seg"] - b["seg"]).max(axis=0)
    print(f"{what}: max |d_seg(step_prep 2) - d_seg(step_prep 0)| per word = {d} (bounds {WORD_TOL})")
    if bitwise:
        assert np.array_equal(a["seg"], b["seg"]), f"{what}: both took the launch, d_seg differs in some bit"
    else:
        assert (d <= WORD_TOL).all(), f"{what}: d_seg words {np.nonzero(d > WORD_TOL)[0]} differ by {d} (bounds {WORD_TOL})"
    if "dump" in a and "dump" in b:
        if bitwise:
            assert np.array_equal(a["dump"]["pm"], b["dump"]["pm"]), what + ": pm differs in some bit"
        else:
            assert_close(a["dump"]["pm"], b["dump"]["pm"], f"pm {what}")
        assert_close(a["dump"]["D"], b["dump"]["D"], f"D {what}", elementwise=False)


def both_forms(m, w, traj, dump=False):
    """The same poses on the same context under step_prep = 0, then 2."""
    m.set_option("step_prep", 0)
    r0 = step(m, w, traj, dump)
    assert r0["on_host"] == 0
    m.set_option("step_prep", 2)
    r2 = step(m, w, traj, dump)
    return r0, r2


def seg_by_value(contexts):
    m = contexts(workload(3))
    n = m.get_option("seg_by_value")
    assert n >= 20, "the benchmark's K = 21 must travel by value"
    return n


@pytest.mark.parametrize("K", [3, 21, "last", "past"])
def test_host_records_against_the_launch(gpu, contexts, K):
    """A step with stale texels (the launch, whatever the option), a second one (it packs the first one's rectangle), then steady steps at three knot sets under both
    forms on the same context.  K = seg_by_value + 2 keeps the launch under step_prep = 2 and is identical to step_prep = 0 in every bit."""
    n = seg_by_value(contexts)
    K = {"last": n + 1, "past": n + 2}.get(K, K)
    fits = K - 1 <= n
    w = workload(K)
    m = contexts(w, step_prep=2)
    for i in range(2):
        r = step(m, w, w.traj)
        assert r["on_host"] == 0 and r["in_warp"] == 0 and r["packed"] == (1 if i < 2 else 0), f"step {i}: stale texels keep the launch"
    for i, t in enumerate([w.traj, moved(w.traj, K // 2, 2e-3), moved(w.traj, None, -3e-3)]):
        r0, r2 = both_forms(m, w, t, dump=True)
        assert r2["on_host"] == (1 if fits else 0) and r2["packed"] == 0, f"step {i} K {K}"
        close(r2, r0, f"step {i} K {K}", bitwise=not fits)


def test_trial_rejection_between_two_steps(gpu, contexts):
    """step, a trial evaluation that is rejected, step: the trial (clean lines: host records) leaves its sums in the accumulator lines, so the step behind it
    keeps the launch (clearing blocks) and the one after that is steady again — the same under both options."""
    w = workload(21)
    t1, t2, t3 = w.traj, moved(w.traj, 7, 2e-3), moved(w.traj, None, -2e-3)
    out = {}
    for prep in (0, 2):
        m = contexts(w, step_prep=prep)
        step(m, w, t1); step(m, w, t1)
        a = step(m, w, t1)
        m.eval_launch(t2)
        trial_on_host = m.get_option("prep_on_host")
        m.rejectTrial()
        b = step(m, w, t3)
        c = step(m, w, t3)
        out[prep] = (a, b, c)
        assert a["on_host"] == (1 if prep else 0) and trial_on_host == (1 if prep else 0)
        assert b["on_host"] == 0, "the rejected trial's sums are cleared by the launch in front"
        assert c["on_host"] == (1 if prep else 0)
    for i in range(3):
        close(out[2][i], out[0][i], f"around a rejected trial, step {i}", bitwise=(i == 1))


def test_the_launch_still_forms_the_fixture_records(gpu, contexts):
    """tests/golden/seg_records_device_gfx950.npz — what the CPU test's bounds are measured from — is what the launch in front of the warp kernel (step_prep = 0)
    forms for the golden control poses (every angle branch), in every bit; and the host's records for the same poses (step_prep = 2, steady steps) stand in device
    memory within the bounds of them, word by word."""
    knots, fixture = np.load(GOLD)["knots"], np.load(DEVICE)["seg"]
    K = knots.shape[1]
    w = workload(K)
    m = contexts(w, step_prep=0)
    on_host = 0
    for c in range(0, knots.shape[0]):
        t = copy.deepcopy(w.traj)
        t.knots_xyzw = np.ascontiguousarray(knots[c])
        m.set_option("step_prep", 0)
        m.eval_launch(t); m.eval_finish()
        assert m.get_option("prep_on_host") == 0
        assert np.array_equal(m.dump_segments(), fixture[c]), f"golden case {c}: the launch's records are not the fixture's"
        if c % 8 == 0:      # (a step leaves clean lines behind it: the next evaluation is a steady one)
            m.set_option("step_prep", 2)
            for _ in range(3):      # (clearing blocks, then perhaps stale texels, then steady)
                m.step(t, w.thres_valid_pixel, w.alpha)
            on_host += m.get_option("prep_on_host")
            d = np.abs(m.dump_segments() - fixture[c]).max(axis=0)
            assert (d <= WORD_TOL).all(), f"golden case {c}: the records in d_seg differ by {d} (bounds {WORD_TOL})"
    print("golden cases whose third step took the host's records:", on_host)
    assert on_host > 0, "no steady step on the golden poses took the host's records"


def test_host_records_against_the_oracle(gpu, contexts, oracle_mod):
    w = workload(21)
    o = oracle_run(oracle_mod, w)
    m = contexts(w, step_prep=2)
    for i in range(4):
        r = step(m, w, w.traj)
        assert r["on_host"] == (1 if i >= 2 else 0)
        assert r["n_inl"] == o["ep"].size and r["P"] == o["ne"]["P"]
        assert np.array_equal(r["nem"], o["num_ev_map"])
        assert_close(r["ep"], o["ep"], "ep")
        compare_normal_eq(r["ne"], o["ne"])
