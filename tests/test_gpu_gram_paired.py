"""The pair-aligned form of the Gram launch against the CPU oracle (-m gpu), beside the multi-key form it replaces in pixel order (option gram_multikey).

Small windows at the sizes where the plan of step_rule.h (gram_pair_cuts) can go wrong; on each, with both forms: formNormalEq and formNormalEqIRLS (Huber)
on one evaluation (the Gram launch without the gather), resident steps with the gather inside the Gram launch and as a launch of its own, on one record set
and on two alternating ones, and a Huber step.  A11, b1, A22, b2, the active set (compare_normal_eq), ep and the count map (check_step) are compared
at the bounds tests/helpers.py applies everywhere (assert_close), and emba_get_option "gram_paired" tells that the intended form ran.  The oracle's
result does not depend on the form: it is computed once per window.

A11 | b1 are still added to the pack by global fp64 atomics, one set per workgroup and pair: their last bits depend on the order in which the workgroups
arrive, under both forms, so no bit-equality between two runs is asserted here.
"""
import numpy as np
import pytest

from helpers import assert_close, oracle_run, small_workload
from test_gpu_parity import compare_normal_eq
from test_gpu_variants import check_step, step_sequence

pytestmark = pytest.mark.gpu


def _first_segment_only():
    """K = 3 (two segments; pairs (0,0), (1,0), (1,1)) with every event inside the first segment: two of the three pairs hold no slot."""
    from emba_amd.legm import EventPacket
    w = small_workload(n_events=12000, K=3, thres_valid_pixel=2)
    n = w.events.size() // 2 // 100 * 100
    e = w.events
    w.events = EventPacket(e.x[:n].copy(), e.y[:n].copy(), e.polarity[:n].copy(), e.t_ns[:n].copy())
    return w


def _no_candidates():
    """Every event on a pixel of its own: no measurement, no record slot, no Gram launch."""
    from emba_amd.legm import EventPacket
    w = small_workload(n_events=2000)
    n = w.events.size()
    i = np.arange(n)
    w.events = EventPacket((i % w.sensor_w).astype(np.uint16), (i // w.sensor_w).astype(np.uint16), w.events.polarity, w.events.t_ns)
    return w


WINDOWS = {
    "k2": lambda: small_workload(n_events=5000, K=2, thres_valid_pixel=2),                   # one pair: one run
    "k3-empty-pairs": _first_segment_only,
    "k21-short-pairs": lambda: small_workload(n_events=4000, K=21, thres_valid_pixel=2),     # ~1.3 events per pixel: dozens of pairs, most shorter than the smallest share (64 slots); more pairs than gram_plan's blocks
    "k3-long-pairs": lambda: small_workload(n_events=60000, K=3),                            # ~57 k slots in three pairs, shares of 64 ... 88 slots: every pair spans hundreds of shares and several workgroups
    "no-candidates": _no_candidates,
}

PROPERTIES = {
    "k2": lambda w, o: w.K == 2,
    "k3-empty-pairs": lambda w, o: w.K == 3 and w.events.t_ns[-1] < w.traj.t0_ns + w.traj.dt_ns,
    "k21-short-pairs": lambda w, o: w.K == 21 and w.events.size() // (w.sensor_w * w.sensor_h) < 2,
    "k3-long-pairs": lambda w, o: w.K == 3 and o["ep"].size > 30000,
    "no-candidates": lambda w, o: o["ep"].size == 0 and o["ne"]["P"] == 0,
}


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from emba_amd import build
    build.build_hip()
    return True


@pytest.fixture(scope="module")
def ref(oracle_mod):
    """ref(name) -> (workload, oracle result, Huber equations): one oracle pass per window and module.  Callers must not modify what they get."""
    cache = {}

    def get(name):
        if name not in cache:
            w = WINDOWS[name]()
            o = oracle_run(oracle_mod, w)
            assert PROPERTIES[name](w, o), f"{name}: the window no longer has the property it was chosen for"
            ne = o["oracle"].form_normal_eq(o["ep"], w.K, o["num_ev_map"], w.thres_valid_pixel, 1, 0.1, False)
            cache[name] = (w, o, o["oracle"].apply_l2(ne, w.alpha, w.Gx, w.Gy))
        return cache[name]

    return get


@pytest.fixture
def contexts():
    from emba_amd import LEGM
    made = []

    def make(w, **opts):
        m = LEGM(w.sensor_w, w.sensor_h, w.lut, w.C_th, w.pano_w, w.pano_h, device=0)
        made.append(m)
        for k, v in opts.items():
            m.set_option(k, v)
        return m

    yield make
    for m in made:
        m.close()


@pytest.mark.parametrize("multikey", [0, 1], ids=["paired", "multikey"])
@pytest.mark.parametrize("name", [n for n in WINDOWS if n != "no-candidates"])
def test_gram_forms_on_windows_that_stress_the_plan(gpu, ref, contexts, name, multikey):
    w, o, ne_huber = ref(name)
    # the deferred gather inside the Gram launch on one record set; the gather as a launch of its own on two alternating sets
    for opts in (dict(step_gather=2, step_one_set=1), dict(step_gather=1, step_one_set=0)):
        m = contexts(w, order=1, gram_multikey=multikey, **opts)
        nem = np.zeros((w.pano_h, w.pano_w), dtype=np.int32)
        ep = m.evaluateDataError(w.traj, w.Gx, w.Gy, w.events, True, nem)
        assert np.array_equal(nem, o["num_ev_map"])
        assert_close(ep, o["ep"], "ep")
        m.formNormalEqIRLS(None, w.K, None, w.thres_valid_pixel, "huber", 0.1)
        compare_normal_eq(m.applyL2Reg(w.alpha), ne_huber)
        assert m.get_option("gram_paired") == 1 - multikey
        m.formNormalEq(None, w.K, None, w.thres_valid_pixel)
        compare_normal_eq(m.applyL2Reg(w.alpha), o["ne"])
        step_sequence(m, w, o)
        assert m.get_option("gram_paired") == 1 - multikey
        n_inl, P = m.step(w.traj, w.thres_valid_pixel, w.alpha, "huber", 0.1)
        assert n_inl == o["ep"].size and P == o["ne"]["P"]
        compare_normal_eq(m._finish(w.alpha, False), ne_huber)
        assert m.get_option("gram_paired") == 1 - multikey


@pytest.mark.parametrize("multikey", [0, 1], ids=["paired", "multikey"])
def test_window_without_candidates(gpu, ref, contexts, multikey):
    """No record slot: no run of slots is found, no Gram launch is made, and the equations are the oracle's (empty active set, A11 = 0, b1 = 0)."""
    w, o, _ = ref("no-candidates")
    m = contexts(w, order=1, gram_multikey=multikey)
    nem = np.zeros((w.pano_h, w.pano_w), dtype=np.int32)
    ep = m.evaluateDataError(w.traj, w.Gx, w.Gy, w.events, True, nem)
    assert ep.size == 0 and not nem.any()
    m.formNormalEq(None, w.K, None, w.thres_valid_pixel)
    compare_normal_eq(m.applyL2Reg(w.alpha), o["ne"])
    check_step(m, w, o, "step")
    assert m.get_option("gram_paired") == 0
