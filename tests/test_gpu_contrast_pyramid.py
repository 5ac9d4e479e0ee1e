"""The smooth contrast and its gradient on a coarser grid on the MI355X (include/emba_hip.h: emba_seq_contrast_gradient_level) against the
numpy form of the same rule — emba_amd.io.contrast_gradient on io.contrast_level of the call's own pm_out / d_out / cp_out.  The image and the gradient are
sums of fp64 atomic adds (in LDS and in HBM) whose order is not fixed: everything is compared under the suite's bounds (helpers.assert_close: 1e-9
norm-wise, 1e-5 per element with the 1e-12 floor), never by bits.  All on the constant-rate recording (about 3 000 events, 64x48 on 256x512): the image has
32 768 cells at level 1 (votes in HBM), 8 192 at level 2 — kContrastLdsCells exactly — 2 048 at level 3 and 512 at level 4 (votes in LDS)."""
import ctypes as C

import numpy as np
import pytest

import cmax_cases as CC
from emba_amd import io as eio
from emba_amd import so3
from emba_amd.legm import EventWindow, LinearTrajectory
from helpers import assert_close
from test_contrast_cpu import knot_errors
from test_panorama_cpu import constant_rate_trajectory

pytestmark = pytest.mark.gpu
ERR_INVALID_ARG = 1
W, H = 512, 256
HBM, LDS = 0, 1
LDS_CELLS = 8192      # kContrastLdsCells (contrast_rule.h)


@pytest.fixture(scope="module")
def dev():
    """One context for the module, the constant-rate recording resident on it: (model, events, events in the sequence)."""
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from emba_amd import LEGM, build
    build.build_hip()
    ev, lut = CC.constant_rate_events(CC.CONST_OMEGA)
    m = LEGM(64, 48, lut, 0.2, W, H, device=0)
    n = m.set_sequence(ev)
    yield m, ev, n
    m.close()


def half_rate():
    return constant_rate_trajectory(CC.CONST_OMEGA / 2)


def check_level(m, ev, traj, beg, end, signed, level, what):
    """Everything a level call returned against the numpy rule on the level of the call's own pm, D and cp; then the J-only call.  Returns (the call's
    dict, numpy's, the vote kernel the call took)."""
    got = m.contrast_gradient(traj, beg, end, signed=signed, want_image=True, want_pm=True, want_D=True, level=level)
    path = m.get_option("contrast_vote_path")
    nn = (end - beg) // 100 * 100
    K = traj.size()
    assert got["pm"].shape == (nn, 2) and got["D"].shape == (nn, 2, 6) and got["cp"].shape == (nn,) and got["grad"].shape == (3 * K,)
    pm_l, D_l, Wl, Hl = eio.contrast_level(got["pm"], got["D"], W, H, level)
    assert got["image"].shape == (Hl, Wl)
    want = eio.contrast_gradient(pm_l, D_l, got["cp"], np.asarray(ev.polarity)[beg:beg + nn], K, Wl, Hl, signed)
    assert_close(got["image"], want["image"], what + " image")
    assert_close(got["grad"], want["grad"], what + " grad")
    assert_close(np.array([got["J"]]), np.array([want["J"]]), what + " J")
    assert got["dropped"] == want["dropped"]
    lean = m.contrast_gradient(traj, beg, end, signed=signed, want_grad=False, level=level)      # no gradient pass: the same J
    assert lean["grad"] is None and lean["image"] is None and lean["pm"] is None and lean["D"] is None
    assert_close(np.array([lean["J"]]), np.array([got["J"]]), what + " J alone")
    assert lean["dropped"] == got["dropped"] and m.get_option("contrast_vote_path") == path
    return got, want, path


def raw_level_call(m, traj, beg, end, level, cells, signed=0, lean=False):
    """emba_seq_contrast_gradient_level with every output given and pre-filled (lean: J and dropped only): (status, outputs)."""
    knots = np.ascontiguousarray(traj.knots_xyzw)
    nn = max(end - beg, 0) // 100 * 100
    out = dict(J=np.full(1, 7.5), grad=np.full(3 * knots.shape[0], 7.5), image=np.full(cells, 7.5), dropped=np.full(1, 75, np.uint64), pm=np.full((nn, 2), 7.5),
               D=np.full((nn, 2, 6), 7.5), cp=np.full(nn, 75, np.int32))
    dp = C.POINTER(C.c_double)
    ptr = lambda k, t=dp: None if (lean and k not in ("J", "dropped")) else out[k].ctypes.data_as(t)      # noqa: E731
    st = m._L.emba_seq_contrast_gradient_level(m._ctx, beg, end, knots.ctypes.data_as(dp), knots.shape[0], traj.t0_ns, traj.dt_ns, signed, level, ptr("J"), ptr("grad"),
                                               ptr("image"), ptr("dropped", C.POINTER(C.c_uint64)), ptr("pm"), ptr("D"), ptr("cp", C.POINTER(C.c_int32)))
    return st, out


def untouched(out):
    return all((v == (75 if v.dtype.kind in "iu" else 7.5)).all() for v in out.values())


@pytest.mark.parametrize("signed", [False, True])
def test_parity_by_level(dev, signed):
    """Levels 0 ... 4 against numpy, both vote kernels exercised: level 1 (32 768 cells) votes in HBM, level 2 (8 192 = the LDS budget exactly), 3 and 4 in
    LDS.  Level 0 through the new entry point equals the existing entry point."""
    m, ev, n = dev
    traj = half_rate()
    paths = {}
    for level in (1, 2, 3, 4):
        got, want, paths[level] = check_level(m, ev, traj, 0, n, signed, level, f"level {level}")
        assert got["J"] > 0 and np.abs(got["grad"]).max() > 0 and (got["image"] < 0).any() == signed
        if not signed:
            assert got["dropped"] == 0 and abs(got["image"].sum() - got["pm"].shape[0]) < 1e-6      # one vote per event
    assert (W >> 2) * (H >> 2) == LDS_CELLS
    assert paths == {1: HBM, 2: LDS, 3: LDS, 4: LDS}, paths
    # level 0: LEGM.contrast_gradient(level=0) is the existing entry point; the new one by the C ABI
    old = m.contrast_gradient(traj, 0, n, signed=signed, want_image=True, want_pm=True, want_D=True)
    assert m.get_option("contrast_vote_path") == HBM
    st, new = raw_level_call(m, traj, 0, n, 0, H * W, signed=int(signed))
    assert st == 0 and m.get_option("contrast_vote_path") == HBM
    assert np.array_equal(new["pm"], old["pm"]) and np.array_equal(new["D"], old["D"]) and np.array_equal(new["cp"], old["cp"])
    assert_close(new["image"].reshape(H, W), old["image"], "level 0 image, new entry point against the existing one")
    assert_close(new["grad"], old["grad"], "level 0 grad")
    assert_close(new["J"], np.array([old["J"]]), "level 0 J")
    assert int(new["dropped"][0]) == old["dropped"]
    # pm_out / d_out of a level call are the unscaled ones of the existing entry point, bit for bit
    lv = m.contrast_gradient(traj, 0, n, signed=signed, want_pm=True, want_D=True, level=3)
    assert np.array_equal(lv["pm"], old["pm"]) and np.array_equal(lv["D"], old["D"]) and np.array_equal(lv["cp"], old["cp"])


def test_forced_vote_kernel(dev):
    """Option contrast_vote: 0 sends a level whose image fits LDS through the HBM vote, 1 changes nothing where the image does not fit; the results are
    those of numpy either way."""
    m, ev, n = dev
    traj = half_rate()
    try:
        m.set_option("contrast_vote", 0)
        for level in (2, 3):
            assert check_level(m, ev, traj, 0, n, True, level, f"level {level}, votes forced to HBM")[2] == HBM
        m.set_option("contrast_vote", 1)
        assert check_level(m, ev, traj, 0, n, False, 1, "level 1, LDS asked for")[2] == HBM
        assert check_level(m, ev, traj, 0, n, False, 2, "level 2, LDS asked for")[2] == LDS
    finally:
        m.set_option("contrast_vote", -1)
    assert m.get_option("contrast_vote") == -1


@pytest.mark.parametrize("beg,end", [(0, 100), (37, 1390), (1100, 2377), (0, None)])
def test_partition_independence(dev, beg, end):
    """The LDS vote under shares of every kind: 100 events — fewer than workgroups, so one workgroup votes and all the others must add nothing; ranges
    whose length is no multiple of the workgroup size (1 300 and 1 200 used events: one full round of the lanes and a partial one), off the batch grid;
    the full range."""
    m, ev, n = dev
    end = n if end is None else end
    for level in (2, 4):
        got, _, path = check_level(m, ev, half_rate(), beg, end, False, level, f"[{beg}, {end}) level {level}")
        assert path == LDS and got["pm"].shape[0] == (end - beg) // 100 * 100
        assert abs(got["image"].sum() - got["pm"].shape[0]) < 1e-6 and got["dropped"] == 0


def test_wrap_and_pole_at_a_coarse_level(dev):
    """At level 3 (64 x 32 cells): under a half turn about the vertical the events straddle the column seam — cells at column W_l - 1 and at column 0, and
    nothing lost; under poses pitched to the lower pole (as tests/test_gpu_panorama.py builds them) row H_l has no cell — its votes are dropped, and the
    count equals numpy's exactly."""
    m, ev, n = dev
    base = half_rate()
    seam = LinearTrajectory(np.array([so3.mul(so3.exp(np.array([0.0, np.pi, 0.0])), q) for q in base.knots_xyzw]), base.t0_ns, base.dt_ns)
    got, want, path = check_level(m, ev, seam, 0, n, False, 3, "seam")
    Wl, Hl = W >> 3, H >> 3
    pm_l = got["pm"] / 8
    assert path == LDS and got["image"][:, 0].any() and got["image"][:, Wl - 1].any() and not got["image"][:, Wl // 2].any()
    assert (pm_l[:, 0] >= Wl - 1).any() and (pm_l[:, 0] < 1.0).any() and got["dropped"] == 0 and abs(got["image"].sum() - pm_l.shape[0]) < 1e-6
    pole = LinearTrajectory(np.array([so3.exp([-np.pi / 2 + 0.1, 0.02 * i, 0.0]) for i in range(4)]), base.t0_ns, base.dt_ns)
    try:
        for forced, took in ((-1, LDS), (0, HBM)):      # the same level through either vote kernel
            m.set_option("contrast_vote", forced)
            got, want, path = check_level(m, ev, pole, 0, n, False, 3, f"pole, contrast_vote {forced}")
            print(f"contrast_vote {forced}: dropped {got['dropped']}, pm_l y up to {got['pm'][:, 1].max() / 8:.3f} of {Hl}")
            assert path == took and got["dropped"] == want["dropped"] > 0 and got["image"].sum() < got["pm"].shape[0] - 1e-6
            assert (got["pm"][:, 1] / 8 >= Hl - 1).any()
    finally:
        m.set_option("contrast_vote", -1)


def test_refused_levels_and_what_a_call_leaves_alone(dev):
    from emba_amd import LEGM, EmbaError
    m, ev, n = dev
    traj = half_rate()
    # level 8 leaves one row of 256; 9 and -1 are no levels: refused by name, every output untouched
    for level in (8, 9, -1, 1 << 20):
        st, out = raw_level_call(m, traj, 0, n, level, H * W)
        assert st == ERR_INVALID_ARG and untouched(out), level
    with pytest.raises(EmbaError) as ei:
        m.contrast_gradient(traj, 0, n, level=8)
    assert ei.value.status == ERR_INVALID_ARG and "level 8" in str(ei.value)
    st, out = raw_level_call(m, traj, 0, n, 7, 2 * 4)      # two rows: the coarsest level of this panorama
    assert st == 0 and out["J"][0] > 0
    # a panorama no level above 2 divides
    lut = CC.constant_rate_events(CC.CONST_OMEGA)[1]
    odd = LEGM(64, 48, lut, 0.2, 516, 260, device=0)
    odd.set_sequence(ev)
    st, out = raw_level_call(odd, traj, 0, n, 3, 260 * 516)
    assert st == ERR_INVALID_ARG and untouched(out) and "divisible" in odd._L.emba_last_error(odd._ctx).decode()
    st, out = raw_level_call(odd, traj, 0, n, 2, 65 * 129)
    assert st == 0 and out["J"][0] > 0
    odd.close()
    # the other arguments as the existing entry point's: a range that is none, an empty one
    st, out = raw_level_call(m, traj, 5, 4, 2, LDS_CELLS)
    assert st == ERR_INVALID_ARG and untouched(out)
    st, out = raw_level_call(m, traj, 500, 599, 2, LDS_CELLS)
    assert st == 0 and out["J"][0] == 0 and not out["grad"].any() and not out["image"].any() and out["dropped"][0] == 0
    # J alone (no grad_out, d_out, cp_out: no gradient pass) gives the same J, on either vote kernel
    for level in (1, 3):
        st, full = raw_level_call(m, traj, 0, n, level, (H >> level) * (W >> level))
        st2, lean = raw_level_call(m, traj, 0, n, level, (H >> level) * (W >> level), lean=True)
        assert st == st2 == 0 and (lean["grad"] == 7.5).all() and (lean["D"] == 7.5).all() and (lean["cp"] == 75).all() and (lean["image"] == 7.5).all()
        assert_close(lean["J"], full["J"], f"level {level} J alone")
        assert lean["dropped"][0] == full["dropped"][0]
    # the registered window, the last evaluation and the integer panorama are left alone
    Z = np.zeros((H, W))
    m.set_events(EventWindow(0, n))
    ep = m.evaluateDataError(traj, Z, Z)
    counts, evc = m.last_counts(), m.event_counts()
    pano = m.event_panorama(traj, 300, 2000, signed=True, want_pm=True)
    for level in (1, 3):
        a = m.contrast_gradient(constant_rate_trajectory(CC.CONST_OMEGA), 300, 2000, signed=True, want_image=True, want_pm=True, want_D=True, level=level)
        assert a["J"] > 0
    assert m.last_counts() == counts and m.event_counts() == evc and m.n_events == n
    assert np.array_equal(m.evaluateDataError(traj, None, None), ep)
    again = m.event_panorama(traj, 300, 2000, signed=True, want_pm=True)
    assert np.array_equal(again["image"], pano["image"]) and np.array_equal(again["pm"], pano["pm"]) and all(again[k] == pano[k] for k in ("J", "sum", "nonzero", "dropped"))


def test_poisoned_workspace():
    """Option poison on a fresh context: every new allocation reads as 0xFF bytes (NaN), so a cell, slot or counter read before it is written shows — first
    call at a level that votes in LDS, then one that votes in HBM, then a smaller level on the now used workspace."""
    from emba_amd import LEGM
    ev, lut = CC.constant_rate_events(CC.CONST_OMEGA)
    m = LEGM(64, 48, lut, 0.2, W, H, device=0)
    m.set_option("poison", 1)
    n = m.set_sequence(ev)
    for level, path in ((3, LDS), (1, HBM), (4, LDS), (2, LDS)):
        for signed in (False, True):
            assert check_level(m, ev, half_rate(), 0, n, signed, level, f"poisoned, level {level}")[2] == path
    m.close()


def test_the_pyramid_on_the_device(dev):
    """io.refine_contrast_pyramid over LEGM.contrast_gradient(level=l) from the identity, levels (3, 2, 1, 0): the CPU test's assertions — a level-0 J above
    J at the true trajectory, every knot error relative to the first knot below half its start, the first pose held bit for bit.  (Not: closeness to the
    numpy loop's end, which the order of the fp64 sums decides — DESIGN.md §13.)"""
    m, ev, n = dev
    truth, start = constant_rate_trajectory(CC.CONST_OMEGA), constant_rate_trajectory(np.zeros(3))
    J_true = m.contrast_gradient(truth, 0, n, want_grad=False)["J"]
    traj, J0, J1, evals = eio.refine_contrast_levels(m, start, 0, n, (3, 2, 1, 0), pano_w=W, fix_first_pose=True, max_iter=60)
    err0, err1 = knot_errors(start, truth), knot_errors(traj, truth)
    print(f"device, from the identity, levels (3, 2, 1, 0): level-0 J {J0:.3f} -> {J1:.3f} (truth {J_true:.3f}) in {evals} evaluations; "
          f"knot errors {np.round(err0, 4).tolist()} -> {np.round(err1, 4).tolist()} rad")
    assert J1 > J_true > J0
    assert all(e1 < 0.5 * e0 for e0, e1 in zip(err0, err1)), (err0, err1)
    assert np.array_equal(traj.knots_xyzw[0], start.knots_xyzw[0])
