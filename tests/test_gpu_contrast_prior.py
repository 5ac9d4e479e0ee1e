"""The prior of the smooth contrast on the MI355X (include/emba_hip.h: emba_seq_contrast_prior_add / _set / _get / _clear, emba_seq_contrast_gradient_prior;
DESIGN.md §15) against the numpy form of the same rule — the votes of io.contrast_gradient on io.contrast_level of a call's own pm, and
io.contrast_gradient(prior = prior_weight * P).  The priors and the images are sums of fp64 atomic adds whose order is not fixed: they are compared under
the suite's bounds (helpers.assert_close), never by bits — except where a call must leave a prior alone, which is by bits.  All on the constant-rate
recording (about 3 000 events, 64x48 on 256x512): level 1 votes in HBM, levels 2, 3 and 4 in LDS."""
import ctypes as C

import numpy as np
import pytest

import cmax_cases as CC
from emba_amd import io as eio
from emba_amd import so3
from emba_amd.legm import EventWindow, LinearTrajectory
from helpers import assert_close
from test_contrast_prior_cpu import DELTA, PRIOR_LEVELS, SPLIT, abs_errors, level_votes, yawed
from test_gpu_contrast_pyramid import half_rate, untouched
from test_panorama_cpu import constant_rate_trajectory

pytestmark = pytest.mark.gpu
ERR_INVALID_ARG, ERR_TIME_RANGE, ERR_STATE = 1, 4, 5
W, H = 512, 256
HBM, LDS = 0, 1
dp, u64p = C.POINTER(C.c_double), C.POINTER(C.c_uint64)


def fresh(pano=(W, H)):
    from emba_amd import LEGM
    ev, lut = CC.constant_rate_events(CC.CONST_OMEGA)
    m = LEGM(64, 48, lut, 0.2, pano[0], pano[1], device=0)
    return m, ev, m.set_sequence(ev)


@pytest.fixture(scope="module")
def dev():
    """One context for the module, the constant-rate recording resident on it: (model, events, events in the sequence)."""
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from emba_amd import build
    build.build_hip()
    m, ev, n = fresh()
    yield m, ev, n
    m.close()


@pytest.fixture(scope="module")
def dense():
    """A random dense prior per level, negative cells included."""
    rng = np.random.default_rng(11)
    return {l: rng.normal(scale=2.0, size=(H >> l, W >> l)) for l in (0, 1, 2, 3)}


def raw_prior_eval(m, traj, beg, end, level, weight, cells, signed=0):
    """emba_seq_contrast_gradient_prior with every output given and pre-filled: (status, outputs)."""
    knots = np.ascontiguousarray(traj.knots_xyzw)
    nn = max(end - beg, 0) // 100 * 100
    out = dict(J=np.full(1, 7.5), grad=np.full(3 * knots.shape[0], 7.5), image=np.full(cells, 7.5), dropped=np.full(1, 75, np.uint64), pm=np.full((nn, 2), 7.5),
               D=np.full((nn, 2, 6), 7.5), cp=np.full(nn, 75, np.int32))
    st = m._L.emba_seq_contrast_gradient_prior(m._ctx, beg, end, knots.ctypes.data_as(dp), knots.shape[0], traj.t0_ns, traj.dt_ns, signed, level, weight,
                                               out["J"].ctypes.data_as(dp), out["grad"].ctypes.data_as(dp), out["image"].ctypes.data_as(dp),
                                               out["dropped"].ctypes.data_as(u64p), out["pm"].ctypes.data_as(dp), out["D"].ctypes.data_as(dp),
                                               out["cp"].ctypes.data_as(C.POINTER(C.c_int32)))
    return st, out


def raw_prior_add(m, traj, beg, end, mask):
    """emba_seq_contrast_prior_add with n_added and dropped pre-filled: (status, n_added, dropped [9])."""
    knots = np.ascontiguousarray(traj.knots_xyzw)
    added, dropped = C.c_size_t(77), np.full(9, 75, np.uint64)
    st = m._L.emba_seq_contrast_prior_add(m._ctx, beg, end, knots.ctypes.data_as(dp), knots.shape[0], traj.t0_ns, traj.dt_ns, 0, mask, C.byref(added),
                                          dropped.ctypes.data_as(u64p))
    return st, added.value, dropped


def check_eval(m, ev, traj, beg, end, signed, level, weight, P, what):
    """Everything a call against the prior P returned against the numpy rule on the call's own pm, D and cp; then the J-only call.  Returns (the call's
    dict, the vote kernel it took)."""
    got = m.contrast_gradient(traj, beg, end, signed=signed, want_image=True, want_pm=True, want_D=True, level=level, prior_weight=weight)
    path = m.get_option("contrast_vote_path")
    nn, K = (end - beg) // 100 * 100, traj.size()
    pm_l, D_l, Wl, Hl = eio.contrast_level(got["pm"], got["D"], W, H, level)
    want = eio.contrast_gradient(pm_l, D_l, got["cp"], np.asarray(ev.polarity)[beg:beg + nn], K, Wl, Hl, signed, prior=weight * P)
    assert_close(got["image"], want["image"], what + " image")
    assert_close(got["grad"], want["grad"], what + " grad")
    assert_close(np.array([got["J"]]), np.array([want["J"]]), what + " J")
    assert got["dropped"] == want["dropped"]
    lean = m.contrast_gradient(traj, beg, end, signed=signed, want_grad=False, level=level, prior_weight=weight)
    assert lean["grad"] is None and lean["image"] is None
    assert_close(np.array([lean["J"]]), np.array([got["J"]]), what + " J alone")
    assert lean["dropped"] == got["dropped"] and m.get_option("contrast_vote_path") == path
    return got, path


@pytest.mark.parametrize("signed", [False, True])
def test_prior_add_parity(dev, signed):
    """One call over the levels 0 ... 4 and the whole recording: every level's prior is the numpy votes of the pm a contrast_gradient call reports for that
    range, added == the events used, the dropped votes per level are numpy's.  Two adds, [0, 1300) then [1300, 2377), give the sum of their votes."""
    m, ev, n = dev
    traj, pol = half_rate(), np.asarray(ev.polarity)
    nn = n // 100 * 100
    m.contrast_prior_clear()
    assert all(m.contrast_prior_get(l) is None for l in range(8))
    pm = m.contrast_gradient(traj, 0, n, want_grad=False, want_pm=True)["pm"]
    r = m.contrast_prior_add(traj, 0, n, levels=(0, 1, 2, 3, 4), signed=signed)
    assert r["added"] == nn == pm.shape[0] and sorted(r["dropped"]) == [0, 1, 2, 3, 4]
    for l in range(5):
        want, dropped = level_votes(pm, pol[:nn], l, signed)
        got = m.contrast_prior_get(l)
        assert got.shape == (H >> l, W >> l) and (got < 0).any() == signed
        assert_close(got, want, f"prior of level {l}")
        assert r["dropped"][l] == dropped
    assert m.contrast_prior_get(5) is None
    m.contrast_prior_clear()
    sums = {l: 0.0 for l in (0, 3)}
    for beg, end in ((0, 1300), (1300, 2377)):
        pm = m.contrast_gradient(traj, beg, end, want_grad=False, want_pm=True)["pm"]
        used = (end - beg) // 100 * 100
        assert m.contrast_prior_add(traj, beg, end, levels=(3, 0), signed=signed)["added"] == used
        for l in sums:
            sums[l] = sums[l] + level_votes(pm, pol[beg:beg + used], l, signed)[0]
    for l in sums:
        assert_close(m.contrast_prior_get(l), sums[l], f"two adds, level {l}")
    m.contrast_prior_clear()


def test_evaluation_parity(dev, dense):
    """Against an uploaded dense prior: image, J, gradient and dropped at level 1 (votes in HBM), 2 and 3 (votes in LDS), weights 1 and 0.25; again with
    the votes forced to HBM; weight 0 agrees with the call without a prior."""
    m, ev, n = dev
    traj = half_rate()
    m.contrast_prior_clear()
    for l in (1, 2, 3):
        m.contrast_prior_set(l, dense[l])
        assert np.array_equal(m.contrast_prior_get(l), dense[l])
    try:
        for forced, paths in ((-1, {1: HBM, 2: LDS, 3: LDS}), (0, {1: HBM, 2: HBM, 3: HBM})):
            m.set_option("contrast_vote", forced)
            for l in (1, 2, 3):
                for weight in (1.0, 0.25):
                    got, path = check_eval(m, ev, traj, 0, n, True, l, weight, dense[l], f"level {l}, weight {weight}, contrast_vote {forced}")
                    assert path == paths[l] and got["J"] > 0 and np.abs(got["grad"]).max() > 0
    finally:
        m.set_option("contrast_vote", -1)
    for l in (1, 3):
        a = m.contrast_gradient(traj, 0, n, want_image=True, level=l, prior_weight=0.0)
        b = m.contrast_gradient(traj, 0, n, want_image=True, level=l)
        assert_close(a["image"], b["image"], f"level {l}, weight 0 image")
        assert_close(a["grad"], b["grad"], f"level {l}, weight 0 grad")
        assert_close(np.array([a["J"]]), np.array([b["J"]]), f"level {l}, weight 0 J")
        assert a["dropped"] == b["dropped"]
    for l in (1, 2, 3):
        assert np.array_equal(m.contrast_prior_get(l), dense[l])      # a call never changes a prior
    m.contrast_prior_clear()


def test_empty_range(dev, dense):
    m, ev, n = dev
    m.contrast_prior_clear()
    for l, weight in ((2, 0.25), (1, 1.0)):
        m.contrast_prior_set(l, dense[l])
        st, out = raw_prior_eval(m, half_rate(), 500, 599, l, weight, dense[l].size)
        assert st == 0 and not out["grad"].any() and out["dropped"][0] == 0
        assert_close(out["J"], np.array([weight * weight * (dense[l] ** 2).sum()]), f"level {l} J of the prior alone")
        assert np.array_equal(out["image"].reshape(dense[l].shape), weight * dense[l])
    m.contrast_prior_clear()


def test_refusals_leave_everything_untouched(dev, dense):
    from emba_amd import EmbaError
    m, ev, n = dev
    traj = half_rate()
    m.contrast_prior_clear()
    m.contrast_prior_set(2, dense[2])
    st, out = raw_prior_eval(m, traj, 0, n, 3, 1.0, dense[3].size)      # no prior at level 3
    assert st == ERR_STATE and untouched(out) and "no prior" in m._L.emba_last_error(m._ctx).decode()
    for weight in (-1.0, float("nan"), float("inf")):
        st, out = raw_prior_eval(m, traj, 0, n, 2, weight, dense[2].size)
        assert st == ERR_INVALID_ARG and untouched(out), weight
    for level in (8, 9, -1):
        st, out = raw_prior_eval(m, traj, 0, n, level, 1.0, H * W)
        assert st == ERR_INVALID_ARG and untouched(out), level
    for mask in (0, 1 << 9, 1 | (1 << 31), 1 << 8):      # no level; bits that are none; level 8 leaves one row of 256
        st, added, dropped = raw_prior_add(m, traj, 0, n, mask)
        assert st == ERR_INVALID_ARG and added == 77 and (dropped == 75).all(), mask
    st, added, dropped = raw_prior_add(m, traj, 5, 4, 1)
    assert st == ERR_INVALID_ARG and added == 77 and (dropped == 75).all()
    assert m.contrast_prior_get(0) is None and np.array_equal(m.contrast_prior_get(2), dense[2])
    with pytest.raises(EmbaError) as ei:
        m.contrast_gradient(traj, 0, n, level=1, prior_weight=1.0)
    assert ei.value.status == ERR_STATE
    # a panorama no level above 2 divides
    odd, _, _ = fresh((516, 260))
    assert raw_prior_add(odd, traj, 0, n, 1 << 3)[0] == ERR_INVALID_ARG and "divisible" in odd._L.emba_last_error(odd._ctx).decode()
    assert raw_prior_add(odd, traj, 0, n, 0b1100)[0] == ERR_INVALID_ARG and odd.contrast_prior_get(2) is None
    st, out = raw_prior_eval(odd, traj, 0, n, 3, 1.0, 260 * 516)
    assert st == ERR_INVALID_ARG and untouched(out)
    with pytest.raises(EmbaError):
        odd.contrast_prior_set(3, np.zeros((260 >> 3, 516 >> 3)))
    st, added, dropped = raw_prior_add(odd, traj, 0, n, 0b101)      # 129 x 65 cells at level 2: an odd number of them
    assert st == 0 and added == n // 100 * 100 and dropped[1] == 0
    r = odd.contrast_gradient(traj, 0, n, want_image=True, level=2, prior_weight=1.0)
    assert_close(r["image"], 2.0 * odd.contrast_prior_get(2), "the window against its own votes, 129 x 65 cells")
    odd.close()
    # a trajectory that ends before the events: EMBA_ERR_TIME_RANGE, and every prior bit for bit as it was
    m.contrast_prior_add(traj, 0, n, levels=(0, 1, 3, 4))
    before = {l: m.contrast_prior_get(l) for l in range(6)}
    assert before[5] is None and all(before[l] is not None for l in range(5))
    early = LinearTrajectory(traj.knots_xyzw[:2].copy(), 800_000_000, 50_000_000)
    st, added, dropped = raw_prior_add(m, early, 0, n, 0b111111)
    assert st == ERR_TIME_RANGE and added == 77 and (dropped == 75).all()
    for l in range(5):
        assert np.array_equal(m.contrast_prior_get(l), before[l]), l
    assert m.contrast_prior_get(5) is None
    st, out = raw_prior_eval(m, early, 0, n, 2, 1.0, dense[2].size)
    assert st == ERR_TIME_RANGE and untouched(out)
    m.contrast_prior_clear()


def test_what_is_left_alone(dev, dense):
    """With priors present the calls without prior_weight return what they returned before there were any; the registered window, the last evaluation and
    the integer panorama stay; evaluations leave the prior bit for bit; a new sequence, a filter and emba_seq_free leave no prior."""
    from emba_amd import EmbaError
    m, ev, n = dev
    traj, other = half_rate(), constant_rate_trajectory(CC.CONST_OMEGA)
    m.contrast_prior_clear()
    kw = dict(signed=True, want_image=True, want_pm=True, want_D=True)
    before = {l: m.contrast_gradient(traj, 300, 2000, level=l, **kw) for l in (0, 1, 3)}
    Z = np.zeros((H, W))
    m.set_events(EventWindow(0, n))
    ep = m.evaluateDataError(traj, Z, Z)
    counts, evc = m.last_counts(), m.event_counts()
    pano = m.event_panorama(traj, 300, 2000, signed=True, want_pm=True)
    m.contrast_prior_add(other, 0, 1500, levels=(0, 1, 2, 3))
    held = {l: m.contrast_prior_get(l) for l in (0, 1, 2, 3)}
    for l in (1, 3):
        assert m.contrast_gradient(other, 300, 2000, level=l, prior_weight=0.5, **kw)["J"] > 0
    for l, b in before.items():
        a = m.contrast_gradient(traj, 300, 2000, level=l, **kw)
        assert np.array_equal(a["pm"], b["pm"]) and np.array_equal(a["D"], b["D"]) and np.array_equal(a["cp"], b["cp"]) and a["dropped"] == b["dropped"]
        assert_close(a["image"], b["image"], f"level {l} image, priors present")
        assert_close(a["grad"], b["grad"], f"level {l} grad, priors present")
        assert_close(np.array([a["J"]]), np.array([b["J"]]), f"level {l} J, priors present")
    assert m.last_counts() == counts and m.event_counts() == evc and m.n_events == n
    assert np.array_equal(m.evaluateDataError(traj, None, None), ep)
    again = m.event_panorama(traj, 300, 2000, signed=True, want_pm=True)
    assert np.array_equal(again["image"], pano["image"]) and np.array_equal(again["pm"], pano["pm"]) and all(again[k] == pano[k] for k in ("J", "sum", "nonzero", "dropped"))
    for l, p in held.items():
        assert np.array_equal(m.contrast_prior_get(l), p), l
    m.contrast_prior_clear()
    # the sequence calls
    f, ev2, n2 = fresh()
    f.contrast_prior_set(1, dense[1])
    f.contrast_prior_add(traj, 0, n2, levels=(3,))
    assert f.contrast_prior_get(1) is not None and f.contrast_prior_get(3) is not None
    f.set_sequence(CC.constant_rate_events(CC.CONST_OMEGA / 2)[0])
    assert f.contrast_prior_get(1) is None and f.contrast_prior_get(3) is None
    f.contrast_prior_set(1, dense[1])
    f.filter_sequence(refractory_ns=1000)
    assert f.contrast_prior_get(1) is None
    f.contrast_prior_set(1, dense[1])
    f.free_sequence()
    with pytest.raises(EmbaError) as ei:
        f.contrast_prior_get(1)
    assert ei.value.status == ERR_STATE
    f.set_sequence(ev2)
    assert f.contrast_prior_get(1) is None
    f.close()


def test_poisoned_workspace(dense):
    """Option poison on a fresh context: every new allocation reads as 0xFF bytes (NaN).  prior_add is the first contrast call the context sees, then an
    evaluation at a level that votes in LDS and at one that votes in HBM: finite, and numpy's."""
    from emba_amd import LEGM
    ev, lut = CC.constant_rate_events(CC.CONST_OMEGA)
    m = LEGM(64, 48, lut, 0.2, W, H, device=0)
    m.set_option("poison", 1)
    n = m.set_sequence(ev)
    traj = half_rate()
    r = m.contrast_prior_add(constant_rate_trajectory(CC.CONST_OMEGA), 0, 1500, levels=(3, 1))
    assert r["added"] == 1500 and r["dropped"] == {1: 0, 3: 0}
    for l, took in ((3, LDS), (1, HBM)):
        P = m.contrast_prior_get(l)
        assert np.isfinite(P).all() and abs(P.sum() - 1500) < 1e-6
        got, path = check_eval(m, ev, traj, 1500, n, False, l, 0.5, P, f"poisoned, level {l}")
        assert path == took and np.isfinite(got["image"]).all() and np.isfinite(got["grad"]).all() and np.isfinite(got["J"])
    st, out = raw_prior_eval(m, traj, 500, 599, 3, 1.0, (H >> 3) * (W >> 3))      # the empty range on the used workspace
    assert st == 0 and np.array_equal(out["image"].reshape(H >> 3, W >> 3), m.contrast_prior_get(3))
    m.close()


def test_seam_and_pole(dev):
    """prior_add at level 3 (64 x 32 cells) under the half turn — columns W_l - 1 and 0 both hit, nothing lost — and under the poses pitched to the lower
    pole: the votes of row H_l are dropped, their count numpy's."""
    m, ev, n = dev
    base = half_rate()
    nn, Wl = n // 100 * 100, W >> 3
    seam = LinearTrajectory(np.array([so3.mul(so3.exp(np.array([0.0, np.pi, 0.0])), q) for q in base.knots_xyzw]), base.t0_ns, base.dt_ns)
    pole = LinearTrajectory(np.array([so3.exp([-np.pi / 2 + 0.1, 0.02 * i, 0.0]) for i in range(4)]), base.t0_ns, base.dt_ns)
    for what, traj in (("seam", seam), ("pole", pole)):
        m.contrast_prior_clear()
        pm = m.contrast_gradient(traj, 0, n, want_grad=False, want_pm=True)["pm"]
        r = m.contrast_prior_add(traj, 0, n, levels=(3, 0))
        got = m.contrast_prior_get(3)
        for l in (3, 0):
            want, dropped = level_votes(pm, None, l)
            assert_close(m.contrast_prior_get(l), want, f"{what}, level {l}")
            assert r["dropped"][l] == dropped
        if what == "seam":
            assert got[:, 0].any() and got[:, Wl - 1].any() and not got[:, Wl // 2].any() and r["dropped"][3] == 0 and abs(got.sum() - nn) < 1e-6
        else:
            print(f"pole: dropped {r['dropped']}")
            assert r["dropped"][3] > 0 and got.sum() < nn - 1e-6
    m.contrast_prior_clear()


def test_what_the_prior_adds_on_the_device(dev):
    """The CPU demonstration (test_contrast_prior_cpu.test_what_the_prior_adds) through prior_add and refine_contrast_levels(prior_weight=1): the true poses
    turned by a common yaw of DELTA, refined on the second half of the events against the votes of the first half along the truth — the errors of knots
    2 and 3 end below half of DELTA.  Without the prior they are printed."""
    m, ev, n = dev
    truth = constant_rate_trajectory(CC.CONST_OMEGA)
    start = yawed(truth, DELTA)
    m.contrast_prior_clear()
    without, J0, J1, evals = eio.refine_contrast_levels(m, start, SPLIT, 3000, PRIOR_LEVELS, pano_w=W, fix_first_pose=False, max_iter=60)
    print(f"device, without a prior: errors -> {np.round(abs_errors(without, truth), 5).tolist()} rad, level-0 J {J0:.1f} -> {J1:.1f}, {evals} evaluations")
    assert m.contrast_prior_add(truth, 0, SPLIT, levels=PRIOR_LEVELS)["added"] == SPLIT
    traj, J0, J1, evals = eio.refine_contrast_levels(m, start, SPLIT, 3000, PRIOR_LEVELS, pano_w=W, fix_first_pose=False, max_iter=60, prior_weight=1.0)
    err = abs_errors(traj, truth)
    print(f"device, with the prior: errors {DELTA:.5f} -> {np.round(err, 5).tolist()} rad, level-0 J {J0:.1f} -> {J1:.1f}, {evals} evaluations")
    assert J1 >= J0 and err[2] < 0.5 * DELTA and err[3] < 0.5 * DELTA, err
    m.contrast_prior_clear()


def test_the_driver_retires_events_into_the_prior():
    """run_sequence(refine_contrast, contrast_prior) over three overlapping windows: the first window has no prior; before every later one the events in
    front of it — whole batches, contiguous from the first window's begin — are in the priors of every level of the schedule; J never falls."""
    from emba_amd.driver import SequenceSettings, run_sequence
    from emba_amd.solver import BASettings, LMSettings
    m, ev, n = fresh()
    pose_t = 1.0 + 0.005 * np.arange(-2, 34)
    pose_q = np.array([so3.exp(CC.CONST_OMEGA / 2 * (t - 1.0)) for t in pose_t])
    seq = SequenceSettings(time_window_size=0.1, sliding_window_stride=0.025, dt_knots=0.025, t_start=1.0, t_end=1.15, median_blur=False, init_map="events",
                           refine_contrast=True, contrast_iters=10, contrast_levels=(2, 0), contrast_prior=True, contrast_prior_weight=0.5)
    res = run_sequence(m, ev, pose_t, pose_q, None, None, seq, BASettings(alpha=0.0), LMSettings(max_num_iter=2))
    assert len(res.windows) == 3 and res.windows[0].prior_events == 0
    first = res.windows[0].beg
    for wr in res.windows:
        print(f"window {wr.index}: events [{wr.beg}, {wr.end}), {wr.prior_events} retired before it, J {wr.refine_J_before:.3f} -> {wr.refine_J_after:.3f} in {wr.refine_evals} evaluations")
        assert wr.prior_events % 100 == 0 and 0 <= wr.beg - (first + wr.prior_events) < 100      # contiguous, up to the window's begin less the sub-batch rest
        assert wr.refine_J_after >= wr.refine_J_before > 0
    assert res.windows[1].prior_events > 0 and res.windows[2].prior_events > res.windows[1].prior_events
    total = res.windows[2].prior_events
    for l in (2, 0):
        P = m.contrast_prior_get(l)
        assert P is not None and abs(P.sum() - total) < 1e-6      # one vote per retired event, nothing dropped
    assert m.contrast_prior_get(1) is None
    off = SequenceSettings(time_window_size=0.1, sliding_window_stride=0.025, dt_knots=0.025, t_start=1.0, t_end=1.15, median_blur=False, init_map="events",
                           refine_contrast=True, contrast_iters=10, contrast_levels=(2, 0))
    res = run_sequence(m, ev, pose_t, pose_q, None, None, off, BASettings(alpha=0.0), LMSettings(max_num_iter=2))
    assert all(wr.prior_events is None for wr in res.windows) and m.contrast_prior_get(0) is None
    m.close()
