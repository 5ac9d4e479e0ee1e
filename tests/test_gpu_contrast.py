"""The smooth contrast of the panorama of warped events and its gradient on the MI355X (include/emba_hip.h: emba_seq_contrast_gradient) against the numpy
form of the same rule (emba_amd.io.contrast_gradient) applied to the call's own pm_out / d_out / cp_out, and against the oracle's dump.  The image and the
gradient are sums of fp64 atomic adds whose order is not fixed: everything is compared under the suite's bounds (helpers.assert_close: 1e-9 norm-wise, 1e-5
per element with the 1e-12 floor), never by bits.  Then the smallest shapes at which the kernels take another path, the statuses, what a call leaves alone,
the ascent over the device's gradient and the driver."""
import ctypes as C

import numpy as np
import pytest

import cmax_cases as CC
from emba_amd import io as eio
from emba_amd import so3, synth
from emba_amd.driver import SequenceSettings, run_sequence
from emba_amd.legm import EventPacket, EventWindow, LinearTrajectory
from emba_amd.sharded import batch_mid_ns
from emba_amd.solver import BASettings, LMSettings
from helpers import assert_close, assert_close_elementwise
from test_contrast_cpu import check_ascent, knot_errors
from test_panorama_cpu import constant_rate_trajectory

pytestmark = pytest.mark.gpu
ERR_INVALID_ARG, ERR_TIME_RANGE, ERR_STATE = 1, 4, 5
W, H = 512, 256
TABLE_CPS = 64      # kContrastTableCps (contrast_rule.h): control poses a workgroup's LDS table holds


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from emba_amd import build
    build.build_hip()
    return True


@pytest.fixture(scope="module")
def scene():
    return synth.make_scene_workload()          # 64x48 on 256x512, K = 6: 38 965 events


@pytest.fixture(scope="module")
def const_rec():
    return CC.constant_rate_events(CC.CONST_OMEGA)      # about 3000 events, 64x48


def oracle_dump(oracle_mod, ev, lut, traj):
    """pm, D, cp of the used events by the oracle (zero maps: only the dump matters)."""
    nn = ev.size() // 100 * 100
    o = oracle_mod.OracleLEGM(64, 48, W, H, lut, 0.2)
    Z = np.zeros((H, W))
    d = o.evaluate_data_error(traj.knots_xyzw, traj.t0_ns, traj.dt_ns, Z, Z, ev.x, ev.y, ev.polarity, ev.t_ns, dump=True)[2]
    return d["pm"][:nn], d["D"][:nn], d["cp_idx"][:nn]


def make_legm(lut, sensor=(64, 48)):
    from emba_amd import LEGM
    return LEGM(sensor[0], sensor[1], lut, 0.2, W, H, device=0)


def turned(traj, w):
    return LinearTrajectory(np.array([so3.mul(so3.exp(np.asarray(w, dtype=np.float64)), q) for q in traj.knots_xyzw]), traj.t0_ns, traj.dt_ns)


def uniform_events(n, step_ns, seed=5):
    rng = np.random.default_rng(seed)
    lut = synth.pinhole_bearing_lut(64, 48, 60.0, 60.0, 32.0, 24.0)
    return EventPacket(rng.integers(0, 64, n).astype(np.uint16), rng.integers(0, 48, n).astype(np.uint16), rng.integers(0, 2, n).astype(np.uint8),
                       10**9 + step_ns * np.arange(n, dtype=np.int64)), lut


def expected_cp(ev, traj, beg, nn):
    t = np.asarray(ev.t_ns, dtype=np.int64)
    mids = np.array([batch_mid_ns(t[beg + 100 * b], t[beg + 100 * b + 99]) for b in range(nn // 100)], dtype=np.int64)
    return np.repeat((mids - traj.t0_ns) // traj.dt_ns, 100).astype(np.int32)


def check_exact(m, ev, traj, beg, end, signed, what):
    """Everything the call returned against the numpy rule applied to the call's own pm, D and cp; the control-pose indices against the batches' midpoints."""
    got = m.contrast_gradient(traj, beg, end, signed=signed, want_image=True, want_pm=True, want_D=True)
    nn = (end - beg) // 100 * 100
    K = traj.size()
    assert got["pm"].shape == (nn, 2) and got["D"].shape == (nn, 2, 6) and got["cp"].shape == (nn,) and got["grad"].shape == (3 * K,)
    assert np.array_equal(got["cp"], expected_cp(ev, traj, beg, nn))
    want = eio.contrast_gradient(got["pm"], got["D"], got["cp"], np.asarray(ev.polarity)[beg:beg + nn], K, W, H, signed)
    assert_close(got["image"], want["image"], what + " image")
    assert_close(got["grad"], want["grad"], what + " grad")
    assert_close(np.array([got["J"]]), np.array([want["J"]]), what + " J")
    assert got["dropped"] == want["dropped"]
    lean = m.contrast_gradient(traj, beg, end, signed=signed, want_grad=False)      # grad_out = NULL: the gradient pass is not launched, the same J
    assert lean["grad"] is None and lean["image"] is None and lean["pm"] is None and lean["D"] is None
    assert_close(np.array([lean["J"]]), np.array([got["J"]]), what + " J alone")
    assert lean["dropped"] == got["dropped"]
    return got, want


@pytest.mark.parametrize("signed", [False, True])
def test_exact_rule(gpu, scene, const_rec, signed):
    m = make_legm(scene.lut)
    n = m.set_sequence(scene.events)
    got, _ = check_exact(m, scene.events, scene.traj, 0, n, signed, "scene")
    assert got["dropped"] == 0 and got["J"] > 0 and np.abs(got["grad"]).max() > 0 and np.isfinite(got["grad"]).all()
    assert (got["image"] < 0).any() == signed
    if not signed:
        assert abs(got["image"].sum() - got["pm"].shape[0]) < 1e-6      # one vote per event
    m.close()
    ev, lut = const_rec
    m = make_legm(lut)
    n = m.set_sequence(ev)
    got, _ = check_exact(m, ev, constant_rate_trajectory(CC.CONST_OMEGA / 2), 0, n, signed, "constant rate")
    assert got["J"] > 0
    m.close()


def test_against_the_oracle(gpu, scene, const_rec, oracle_mod):
    """pm_out, d_out, cp_out against the oracle's dump, and J and grad against the numpy rule on the oracle's pm / D.  The gradient is discontinuous where a
    pm crosses a cell edge: on these recordings the oracle's pm come no nearer to one than 5.5e-6 px (scene) and 1.2e-5 px (constant rate at half the rate),
    measured on the CPU and asserted below, against 5.7e-14 px between the device's pm and the oracle's — no event is excluded."""
    ev2, lut2 = const_rec
    for ev, lut, traj, what in ((scene.events, scene.lut, scene.traj, "scene"), (ev2, lut2, constant_rate_trajectory(CC.CONST_OMEGA / 2), "constant rate")):
        pm_o, D_o, cp_o = oracle_dump(oracle_mod, ev, lut, traj)
        assert np.abs(pm_o - np.rint(pm_o)).min() > 1e-9
        m = make_legm(lut)
        n = m.set_sequence(ev)
        got = m.contrast_gradient(traj, 0, n, want_pm=True, want_D=True)
        assert np.array_equal(got["cp"], cp_o)
        e = assert_close_elementwise(got["pm"], pm_o, "contrast_pm against the oracle's pm")
        assert_close(got["D"], D_o, "contrast_D against the oracle's dpm_ddrot_cp")
        want = eio.contrast_gradient(pm_o, D_o, cp_o, ev.polarity[:pm_o.shape[0]], traj.size(), W, H)
        assert_close(got["grad"], want["grad"], what + " grad against the rule on the oracle's pm / D")
        assert_close(np.array([got["J"]]), np.array([want["J"]]), what + " J against the rule on the oracle's pm")
        print(f"{what}: pm worst element {e:.3e}, J device {got['J']!r} oracle {want['J']!r}")
        m.close()


def test_smallest_ranges(gpu, scene):
    """Exactly 100 events (one batch, one workgroup partly empty), a range that starts inside the sequence off the batch grid, K = 2."""
    ev = scene.events
    m = make_legm(scene.lut)
    n = m.set_sequence(ev)
    got, _ = check_exact(m, ev, scene.traj, 0, 100, False, "100 events")
    assert got["pm"].shape == (100, 2) and abs(got["image"].sum() - 100.0) < 1e-9
    one, _ = check_exact(m, ev, scene.traj, 0, 199, True, "199 events")
    assert one["pm"].shape == (100, 2) and np.array_equal(one["pm"], got["pm"])      # the tail behind the last whole batch is ignored
    got, _ = check_exact(m, ev, scene.traj, 337, 2850, False, "a range inside")
    assert got["pm"].shape == (2500, 2)
    pano = m.event_panorama(scene.traj, 337, 2850, want_pm=True)
    assert np.array_equal(pano["pm"], got["pm"])                                       # the batches and pm of emba_seq_event_panorama, bit for bit
    two = LinearTrajectory(scene.traj.knots_xyzw[[0, 5]].copy(), scene.traj.t0_ns, 5 * scene.traj.dt_ns)
    got, _ = check_exact(m, ev, two, 0, n, False, "K = 2")
    assert got["grad"].shape == (6,) and (got["cp"] == 0).all() and np.abs(got["grad"][:3]).max() > 0 and np.abs(got["grad"][3:]).max() > 0
    m.close()


def test_span_paths_of_the_gradient_kernel(gpu):
    """300 events, 1 us apart, over K = 200 control poses.  dt = 2.5 us: the three batches of the first workgroup lie 40 control poses apart, more than the
    LDS table holds — the fallback, every lane adding to g in HBM.  dt = 60 us: the batches lie 2 apart, the table holds them, and the batch boundary at
    event 100 falls inside the second wave — the mixed-cp wave path next to the shuffle path of the first wave."""
    ev, lut = uniform_events(300, 1000)
    knots = np.array([so3.exp([0.001 * i, 0.002 * i, -0.0005 * i]) for i in range(200)])
    m = make_legm(lut)
    m.set_sequence(ev)
    for dt, fallback in ((2500, True), (60_000, False)):
        traj = LinearTrajectory(knots, 10**9, dt)
        for signed in (False, True):
            got, _ = check_exact(m, ev, traj, 0, 300, signed, f"dt {dt}")
        cp = got["cp"]
        assert (cp[255] - cp[0] + 2 > TABLE_CPS) == fallback and cp[64] != cp[127]
        touched = np.nonzero(got["grad"].reshape(-1, 3).any(axis=1))[0]
        assert set(touched) == set(np.unique(cp)) | set(np.unique(cp) + 1)
    m.close()


def test_contention_on_one_patch(gpu):
    """20 000 events at one sensor pixel under one pose: every add of the vote launch goes to the same four cells, every add of the gradient to one pair of
    control poses."""
    n = 20_000
    lut = synth.pinhole_bearing_lut(64, 48, 60.0, 60.0, 32.0, 24.0)
    ev = EventPacket(np.full(n, 40, np.uint16), np.full(n, 13, np.uint16), (np.arange(n) % 2).astype(np.uint8), 10**9 + 1000 * np.arange(n, dtype=np.int64))
    traj = LinearTrajectory(np.tile(so3.exp([0.03, 0.4, -0.02]), (3, 1)), 10**9, 100_000_000)
    m = make_legm(lut)
    m.set_sequence(ev)
    got, _ = check_exact(m, ev, traj, 0, n, False, "one patch")
    assert (got["pm"] == got["pm"][0]).all() and np.count_nonzero(got["image"]) <= 4 and abs(got["image"].sum() - n) < 1e-6
    signed = m.contrast_gradient(traj, 0, n, signed=True)      # as many events of either polarity: what is left is the rounding of the adds' order
    assert abs(signed["J"]) < 1e-12 * got["J"] and np.abs(signed["grad"]).max() < 1e-9 * np.abs(got["grad"]).max()
    m.close()


def test_wrap_across_column_zero(gpu, scene):
    m = make_legm(scene.lut)
    n = m.set_sequence(scene.events)
    got, _ = check_exact(m, scene.events, turned(scene.traj, [0.0, np.pi, 0.0]), 0, n, False, "wrap")
    img = got["image"]
    assert img[:, 0].any() and img[:, W - 1].any() and not img[:, W // 2].any()
    assert (got["pm"][:, 0] < 1.0).any() and (got["pm"][:, 0] >= W - 1.0).any() and got["dropped"] == 0
    assert abs(img.sum() - got["pm"].shape[0]) < 1e-6      # nothing is lost at the seam
    m.close()


def test_dropped_rows_at_the_pole(gpu):
    """Uniform events under poses pitched to the poles, as tests/test_gpu_panorama.py builds them: at the lower pole the row below the last has no cell."""
    n = 20_000
    ev, lut = uniform_events(n, 5000)
    m = make_legm(lut)
    m.set_sequence(ev)
    for pitch, lower in ((-np.pi / 2 + 0.1, True), (np.pi / 2 - 0.1, False)):
        traj = LinearTrajectory(np.array([so3.exp([pitch, 0.02 * i, 0.0]) for i in range(4)]), 10**9, 50_000_000)
        got, _ = check_exact(m, ev, traj, 0, n, False, f"pitch {pitch:.2f}")
        print("pitch", pitch, "dropped", got["dropped"], "pm_y", got["pm"][:, 1].min(), got["pm"][:, 1].max())
        assert (got["dropped"] > 0 and got["image"].sum() < n - 1e-6) if lower else (got["dropped"] == 0 and abs(got["image"].sum() - n) < 1e-6)
    m.close()


def raw_call(m, traj, beg, end, K=None, dt=None, t0=None):
    """The C ABI with every output given and pre-filled: (status, outputs)."""
    knots = np.ascontiguousarray(traj.knots_xyzw)
    K = knots.shape[0] if K is None else K
    nn = max(end - beg, 0) // 100 * 100
    out = dict(J=np.full(1, 7.5), grad=np.full(3 * max(K, 1), 7.5), image=np.full((H, W), 7.5), dropped=np.full(1, 75, np.uint64), pm=np.full((nn, 2), 7.5),
               D=np.full((nn, 2, 6), 7.5), cp=np.full(nn, 75, np.int32))
    dp = C.POINTER(C.c_double)
    st = m._L.emba_seq_contrast_gradient(m._ctx, beg, end, knots.ctypes.data_as(dp), K, traj.t0_ns if t0 is None else t0, traj.dt_ns if dt is None else dt, 0,
                                         out["J"].ctypes.data_as(dp), out["grad"].ctypes.data_as(dp), out["image"].ctypes.data_as(dp),
                                         out["dropped"].ctypes.data_as(C.POINTER(C.c_uint64)), out["pm"].ctypes.data_as(dp), out["D"].ctypes.data_as(dp),
                                         out["cp"].ctypes.data_as(C.POINTER(C.c_int32)))
    return st, out


def untouched(out):
    return all((v == (75 if v.dtype.kind in "iu" else 7.5)).all() for v in out.values())


def test_statuses_and_what_a_call_leaves_alone(gpu, scene):
    from emba_amd import EmbaError
    ev, traj = scene.events, scene.traj
    m = make_legm(scene.lut)
    st, out = raw_call(m, traj, 0, 0)                                   # no sequence
    assert st == ERR_STATE and untouched(out)
    n = m.set_sequence(ev)
    for kw in (dict(beg=5, end=4), dict(beg=0, end=n + 1), dict(beg=0, end=n, K=1), dict(beg=0, end=n, dt=0), dict(beg=0, end=n, dt=-5)):
        st, out = raw_call(m, traj, **kw)
        assert st == ERR_INVALID_ARG and untouched(out), kw
    st, out = raw_call(m, traj, 0, n, K=3)                             # the last batches lie behind the last knot of a spline of three
    assert st == ERR_TIME_RANGE and untouched(out)
    st, out = raw_call(m, traj, 0, 1000, t0=traj.t0_ns + 10**9)        # every batch in front of a spline that begins later
    assert st == ERR_TIME_RANGE and untouched(out)
    with pytest.raises(EmbaError) as ei:
        m.contrast_gradient(LinearTrajectory(traj.knots_xyzw[:3], traj.t0_ns, traj.dt_ns), 0, n)
    assert ei.value.status == ERR_TIME_RANGE
    ok = m.contrast_gradient(LinearTrajectory(traj.knots_xyzw[:3], traj.t0_ns, traj.dt_ns), 0, 2000)      # the same three knots span the first events
    assert ok["J"] > 0 and ok["grad"].shape == (9,)
    for beg, end in ((77, 77), (500, 599), (n, n)):                    # an empty range, less than a batch: J = 0, grad = 0, a zero image
        st, out = raw_call(m, traj, beg, end)
        assert st == 0 and out["J"][0] == 0 and not out["grad"].any() and not out["image"].any() and out["dropped"][0] == 0
    # with every output NULL nothing happens (the arguments are still checked)
    knots = np.ascontiguousarray(traj.knots_xyzw)
    kp = knots.ctypes.data_as(C.POINTER(C.c_double))
    assert m._L.emba_seq_contrast_gradient(m._ctx, 0, n, kp, 6, traj.t0_ns, traj.dt_ns, 0, None, None, None, None, None, None, None) == 0
    assert m._L.emba_seq_contrast_gradient(m._ctx, 0, n, kp, 1, traj.t0_ns, traj.dt_ns, 0, None, None, None, None, None, None, None) == ERR_INVALID_ARG
    # the registered window, its ep, the last evaluation and the integer panorama's results are left alone
    m.set_events(EventWindow(0, n))
    ep = m.evaluateDataError(traj, scene.Gx, scene.Gy)
    counts, evc = m.last_counts(), m.event_counts()
    pano = m.event_panorama(traj, 300, 20000, signed=True, want_pm=True)
    a = m.contrast_gradient(turned(traj, [0.0, 1.0, 0.0]), 300, 20000, signed=True, want_image=True, want_pm=True, want_D=True)
    assert a["J"] > 0
    assert m.last_counts() == counts and m.event_counts() == evc and m.n_events == n
    assert np.array_equal(m.evaluateDataError(traj, None, None), ep)      # the window is still registered, the map still resident
    again = m.event_panorama(traj, 300, 20000, signed=True, want_pm=True)
    assert np.array_equal(again["image"], pano["image"]) and np.array_equal(again["pm"], pano["pm"]) and all(again[k] == pano[k] for k in ("J", "sum", "nonzero", "dropped"))
    m.free_sequence()
    st, out = raw_call(m, traj, 0, 0)
    assert st == ERR_STATE and untouched(out)
    m.close()


def test_poisoned_workspace(gpu, scene):
    """Option poison on a fresh context: every new allocation reads as 0xFF bytes (NaN), so a cell, slot, counter or gradient component that is read before
    it is written shows; a second call on the now used workspace gives the same results."""
    m = make_legm(scene.lut)
    m.set_option("poison", 1)
    n = m.set_sequence(scene.events)
    for signed in (False, True):
        first, _ = check_exact(m, scene.events, scene.traj, 0, n, signed, "poisoned")
        second, _ = check_exact(m, scene.events, scene.traj, 0, n, signed, "poisoned, second call")
        assert np.array_equal(first["pm"], second["pm"]) and np.array_equal(first["D"], second["D"])
        assert_close(second["grad"], first["grad"], "second call grad")
        assert_close(second["image"], first["image"], "second call image")
    short, _ = check_exact(m, scene.events, scene.traj, 0, 1000, False, "a shorter range on the used workspace")
    assert abs(short["image"].sum() - 1000.0) < 1e-9
    m.close()


@pytest.mark.parametrize("poison", [0, 1])
def test_panorama_and_contrast_share_the_pose_stage(gpu, scene, poison):
    """The batch times, the pose table and the control poses of the panorama and of the contrast gradient are one buffer set of the context, rebuilt by
    every call: a contrast call with another K on a longer range that is not nested in the panorama's leaves nothing behind that a second panorama call
    could read — it answers what the first answered, bit for bit — and what the first panorama call left does not reach the contrast call, whose pm is
    a fresh context's.  With option poison: new memory reads as NaN, so a pose record or knot read before this call wrote it would show."""
    ev, t6 = scene.events, scene.traj
    t8 = turned(LinearTrajectory(np.concatenate([t6.knots_xyzw, t6.knots_xyzw[-1:], t6.knots_xyzw[-1:]]), t6.t0_ns, t6.dt_ns), [0.01, -0.02, 0.03])
    assert t6.size() == 6 and t8.size() == 8
    A, B = (1000, 6000), (3000, 12000)
    m = make_legm(scene.lut)
    m.set_option("poison", poison)
    m.set_sequence(ev)
    first = m.event_panorama(t6, *A, want_image=True, want_pm=True)
    between = m.contrast_gradient(t8, *B, want_pm=True)
    third = m.event_panorama(t6, *A, want_image=True, want_pm=True)
    m.close()
    assert first["J"] > 0 and first["pm"].shape == (5000, 2) and np.isfinite(first["pm"]).all()
    for key in ("image", "pm", "J", "sum", "nonzero", "dropped"):
        assert np.array_equal(third[key], first[key]), key
    fresh = make_legm(scene.lut)
    fresh.set_sequence(ev)
    alone = fresh.contrast_gradient(t8, *B, want_pm=True)
    fresh.close()
    assert between["pm"].shape == (9000, 2) and np.array_equal(between["pm"], alone["pm"]) and between["dropped"] == alone["dropped"]
    assert_close(np.array([between["J"]]), np.array([alone["J"]]), "J after a panorama call")
    assert_close(between["grad"], alone["grad"], "grad after a panorama call")


@pytest.fixture(scope="module")
def device_ascent(gpu, const_rec):
    """io.refine_contrast over LEGM.contrast_gradient from the half-rate trajectory of the constant-rate recording: run once, shared."""
    ev, lut = const_rec
    start = constant_rate_trajectory(CC.CONST_OMEGA / 2)
    m = make_legm(lut)
    n = m.set_sequence(ev)

    def dev_JG(t):
        r = m.contrast_gradient(t, 0, n)
        return r["J"], r["grad"]
    dev_J = lambda t: m.contrast_gradient(t, 0, n, want_grad=False)["J"]      # noqa: E731
    traj, hist, evals = eio.refine_contrast(dev_JG, dev_J, start, fix_first_pose=True, max_iter=60, pano_w=W)
    J_true = dev_J(constant_rate_trajectory(CC.CONST_OMEGA))
    m.close()
    return start, traj, hist, evals, J_true


def test_ascent_on_the_device(device_ascent):
    """The ascent over the device's J and gradient meets the CPU test's assertions: J rises strictly, ends above J at the true trajectory, every knot error
    relative to the first knot falls below half its initial value."""
    start, traj, hist, evals, J_true = device_ascent
    truth = constant_rate_trajectory(CC.CONST_OMEGA)
    err0, err1 = knot_errors(start, truth), knot_errors(traj, truth)
    print(f"device: J {hist[0]:.3f} -> {hist[-1]:.3f} (truth {J_true:.3f}) in {len(hist) - 1} accepted steps, {evals} evaluations; "
          f"knot errors {np.round(err0, 4).tolist()} -> {np.round(err1, 4).tolist()} rad")
    check_ascent(hist, J_true, err0, err1, True)


def test_ascent_on_the_device_ends_where_the_numpy_loop_ends(device_ascent, const_rec, oracle_mod):
    """The device loop's final J within 1e-6 relative of the same loop over the numpy rule on the oracle's pm / D — where the order of the fp64 sums does not
    decide the loop's outcome; where it does, the CPU test's bounds only.

    Whether it does is measured here, on the CPU, and not assumed: the numpy loop is run twice on the same pm / D / cp, once with the events summed in
    time order and once in reverse.  Nothing else differs, and J at the start differs by one unit in the last place (8863.537627178168 against ...166).
    Measured: the two numpy loops end at 28077.861 (60 accepted steps, 186 evaluations) and 28081.300 (60 steps, 194 evaluations), 1.2e-4 relative apart
    (a random order: 28081.587, 53 steps, 175 evaluations).  The ascent multiplies a difference of the control poses by about ten per accepted step — a step
    of fixed length a along d / max|d| moves a perturbation dx by about a |Hessian| dx / |g|, far above 1 on an objective whose features are a pixel wide
    — until comparisons of the line search and of the stopping rule come out differently.  Three device runs, which differ from each other only in the
    order of their atomic adds, ended at 28081.138 (60 steps, 189 evaluations), 28080.995 and 28080.395 (47 steps, 155 evaluations).  So on this recording
    the summation order decides, the 1e-6 cannot be met by any implementation that is not bit-equal to the numpy loop, and what is asserted instead is the CPU test's bounds and that the device loop ends no
    further from the numpy loop than ten times the numpy loop's own spread between its two orders (the reference's own error, as the suite's measured
    bounds are set).  Should a change of the loop make it insensitive to the order (a spread within 1e-6), the 1e-6 bound is asserted
    (DESIGN.md §13)."""
    ev, lut = const_rec
    nn = ev.size() // 100 * 100
    start, traj, hist, evals, J_true = device_ascent
    truth = constant_rate_trajectory(CC.CONST_OMEGA)

    def numpy_loop(order):
        def np_JG(t):
            pm, D, cp = oracle_dump(oracle_mod, ev, lut, t)
            r = eio.contrast_gradient(pm[order], D[order], cp[order], ev.polarity[:nn][order], t.size(), W, H)
            return r["J"], r["grad"]
        return eio.refine_contrast(np_JG, lambda t: np_JG(t)[0], start, fix_first_pose=True, max_iter=60, pano_w=W)
    _, hist_f, evals_f = numpy_loop(np.arange(nn))
    _, hist_r, evals_r = numpy_loop(np.arange(nn)[::-1])
    J_np = hist_f[-1]
    spread, off = abs(hist_r[-1] - J_np) / J_np, abs(hist[-1] - J_np) / J_np
    print(f"device: J {hist[-1]!r} in {len(hist) - 1} accepted steps, {evals} evaluations; numpy, events summed in time order: J {J_np!r} in {len(hist_f) - 1} steps, "
          f"{evals_f} evaluations; in reverse order: J {hist_r[-1]!r} in {len(hist_r) - 1} steps, {evals_r} evaluations; the numpy loop's own spread {spread:.3e}, "
          f"device against numpy {off:.3e}")
    if spread <= 1e-6:
        assert off <= 1e-6
    else:
        print("the order of the fp64 sums decides the loop's outcome on this recording: the CPU test's bounds and ten times the numpy loop's own spread are asserted")
        check_ascent(hist, J_true, knot_errors(start, truth), knot_errors(traj, truth), True)
        assert off <= 10.0 * spread


def test_the_driver_refines_each_window(gpu, const_rec):
    """run_sequence(refine_contrast = True) over two windows of the constant-rate recording, raw poses at half the true rate, no map to start from: every
    window records a J after the refinement at least as large as before, and hands the refined control poses to the solve."""
    ev, lut = const_rec
    m = make_legm(lut)
    pose_t = 1.0 + 0.005 * np.arange(-2, 34)
    pose_q = np.array([so3.exp(CC.CONST_OMEGA / 2 * (t - 1.0)) for t in pose_t])
    seq = SequenceSettings(time_window_size=0.1, sliding_window_stride=0.05, dt_knots=0.05, t_start=1.0, t_end=1.15, median_blur=False, init_map="events",
                           refine_contrast=True, contrast_iters=10)
    res = run_sequence(m, ev, pose_t, pose_q, None, None, seq, BASettings(alpha=0.0), LMSettings(max_num_iter=2))
    assert len(res.windows) == 2
    for wr in res.windows:
        print(f"window {wr.index}: J {wr.refine_J_before:.3f} -> {wr.refine_J_after:.3f} in {wr.refine_evals} evaluations")
        assert wr.refine_J_after >= wr.refine_J_before > 0 and wr.refine_evals >= 1
        again = m.contrast_gradient(wr.traj_init, wr.beg, wr.end, want_grad=False)["J"]
        assert abs(again - wr.refine_J_after) <= 1e-9 * again      # traj_init is the refined segment
    assert res.windows[0].refine_J_after > res.windows[0].refine_J_before
    off = SequenceSettings(time_window_size=0.1, sliding_window_stride=0.05, dt_knots=0.05, t_start=1.0, t_end=1.15, median_blur=False, init_map="events")
    res = run_sequence(m, ev, pose_t, pose_q, None, None, off, BASettings(alpha=0.0), LMSettings(max_num_iter=2))
    assert all(wr.refine_J_before is None and wr.refine_J_after is None and wr.refine_evals is None for wr in res.windows)
    m.close()
