"""GPU tests (-m gpu) of the two partial solves, through the C ABI: emba_solve_map_only (mapping with known poses: x2_i = (A22_i + lambda diag A22_i)^-1 b2_i
per active pixel) and emba_solve_poses_only ((A11 + lambda diag A11) x1 = b1), their group forms, the state they leave, and the LM loop with
BASettings.refine = "map" / "poses" against the same loop on the oracle.  References: tests/partial_ref.py (numpy)."""
import ctypes as C

import numpy as np
import pytest

import partial_ref as PR
from helpers import assert_close_elementwise, small_workload

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from emba_amd import build
    build.build_hip()
    return True


def make_legm(w):
    from emba_amd import LEGM
    return LEGM(w.sensor_w, w.sensor_h, w.lut, w.C_th, w.pano_w, w.pano_h, device=0)


LAMBDAS = (1e-3, 10.0)


def small():        # K = 6: n = 18, the single-launch Cholesky
    return small_workload()


def panel():        # K = 30: n = 90, two 64-column panels with a ragged second one — the smallest shape that enters the panel path
    return small_workload(n_events=40000, pano_h=128, K=30, sensor=(32, 24), focal=30.0, dt_knots=0.01, thres_valid_pixel=3)


def formed(w, thres=None, alpha=None, poison=0):
    """a context with eval + form + L2 done -> (LEGM, the DEVICE's downloaded A11, b1, A22, b2)"""
    m = make_legm(w)
    if poison:
        m.set_option("poison", 1)
    nem = np.zeros((w.pano_h, w.pano_w), dtype=np.int32)
    m.evaluateDataError(w.traj, w.Gx, w.Gy, w.events, True, nem)
    m.formNormalEq(None, w.K, nem, w.thres_valid_pixel if thres is None else thres)
    ne = m.applyL2Reg(w.alpha if alpha is None else alpha)
    return m, ne


@pytest.mark.parametrize("make", [small, panel], ids=["K6_single_launch", "K30_panels"])
def test_one_shot_parity(gpu, make):
    w = make()
    m, ne = formed(w)
    assert ne["P"] > 256                                     # (more than one block of the map-only kernel)
    for lam in LAMBDAS:
        rx2, bad = PR.solve_map_only(ne, lam)
        assert bad == 0
        x1, x2 = m.solveMapOnly(lam)
        assert x1.shape == (3 * w.K,) and not x1.any()
        assert_close_elementwise(x2, rx2, f"x2_map_only lambda {lam:g}")
        assert m.last_solve_info() == 0
        for fix in (0, 1):
            x1, none = m.solvePosesOnly(lam, fix_first_pose=bool(fix))
            assert none is None
            assert_close_elementwise(x1, PR.solve_poses_only(ne, lam, bool(fix)), f"x1_poses_only lambda {lam:g} fix {fix}")
            assert not fix or not x1[:3].any()
            assert m.last_solve_info() & 5 == 0
    m.close()


def test_state_around_the_partial_solves(gpu):
    from emba_amd import EmbaError
    from emba_amd._lib import ERR_STATE
    w = small()
    m, ne = formed(w)
    lam = 1e-2
    j0 = m.solveNormalEq(lam, fix_first_pose=True)

    def same_joint(what):
        j = m.solveNormalEq(lam, fix_first_pose=True)
        # (two joint solves of the same system agree to rounding only: the product's partial tiles are combined with atomics — tests/test_gpu_parity.py)
        for a, b in zip(j, j0):
            assert np.allclose(a, b, rtol=1e-9, atol=1e-9 * np.abs(b).max()), what

    # the map-only x2 is kept on the device: updateMap(None) applies it exactly as the downloaded one
    _, x2 = m.solveMapOnly(lam)
    m.updateMap(None, 0.7)
    via_dev = m.downloadMap()
    m.rejectMap()
    m.updateMap(x2, 0.7)
    via_host = m.downloadMap()
    m.rejectMap()
    assert np.array_equal(via_dev[0], via_host[0]) and np.array_equal(via_dev[1], via_host[1])
    assert not np.array_equal(via_dev[0], w.Gx)
    same_joint("joint solve after the map-only solve")
    # the poses-only solve drops the x2 the joint solve above kept
    m.solvePosesOnly(lam, fix_first_pose=True)
    with pytest.raises(EmbaError) as ei:
        m.updateMap(None, 0.7)
    assert ei.value.status == ERR_STATE
    same_joint("joint solve after the poses-only solve")
    m.updateMap(None, 0.7)                                   # ... and the joint solve's is there again
    m.rejectMap()
    m.close()
    # before emba_form_finish both are a state error
    m = make_legm(w)
    nem = np.zeros((w.pano_h, w.pano_w), dtype=np.int32)
    m.evaluateDataError(w.traj, w.Gx, w.Gy, w.events, True, nem)
    for call in (lambda: m.solveMapOnly(lam), lambda: m.solvePosesOnly(lam, True)):
        with pytest.raises(EmbaError) as ei:
            call()
        assert ei.value.status == ERR_STATE
    # no active pixel: the map-only solve has nothing to do, and says so with EMBA_OK
    m.formNormalEq(None, w.K, nem, 10 ** 6)
    ne0 = m.applyL2Reg(w.alpha)
    assert ne0["P"] == 0
    x1, x2 = m.solveMapOnly(lam)
    assert x2.size == 0 and not x1.any()
    m.updateMap(None, 1.0); m.rejectMap()
    m.close()


def test_a_block_that_is_not_positive_definite(gpu):
    """alpha = 0 and thres_valid_pixel = 1: a pixel with a single measurement has the rank-1 block dp dp^T.  Damping lifts it unless a component of dp is
    zero — then the block is singular at every lambda (on this input the numpy reference flags 5 of 5489 blocks at lambda = 1e-3, 920 undamped)."""
    from emba_amd import EmbaError
    from emba_amd._lib import ERR_NUMERIC
    from emba_amd.solver import BASettings, LMSettings, solve_time_window
    w = small()
    m, ne = formed(w, thres=1, alpha=0.0)
    for lam in (0.0, 1e-3):
        _, bad = PR.solve_map_only(ne, lam)
        print(f"blocks the numpy reference flags at lambda = {lam:g}:", bad, "of", ne["P"])
        assert bad >= 1
        with pytest.raises(EmbaError) as ei:
            m.solveMapOnly(lam)
        assert ei.value.status == ERR_NUMERIC and m.last_solve_info() & 1
    m.solvePosesOnly(1e-3, fix_first_pose=True)              # (the pose block is not concerned, and the info word is the last solve's)
    assert m.last_solve_info() & 1 == 0
    m.close()
    # the LM loop takes every such failure as a rejected step, as it does for the joint solve: lambda x 10 until it leaves [1e-300, 1e3]
    m = make_legm(w)
    knots_in = w.traj.knots_xyzw.copy()
    r = solve_time_window(m, w.traj, w.events, np.zeros_like(w.Gx), np.zeros_like(w.Gy), BASettings(alpha=0.0, thres_valid_pixel=1, refine="map"), LMSettings(),
                          resident=True)
    assert [e[4] for e in r.log] == [False] * 7 and all(e[3] == float("inf") for e in r.log)
    assert [round(e[1]) for e in r.log] == [-3, -2, -1, 0, 1, 2, 3]
    assert not r.converged and r.reason == "lambda" and r.cost_min == r.log[0][2]
    assert np.array_equal(r.traj.knots_xyzw, knots_in)
    assert not any(p.any() for p in m.downloadMap())         # the zero map was never replaced
    m.close()


@pytest.mark.parametrize("mode", ["map", "poses"])
@pytest.mark.parametrize("resident", [False, True])
def test_lm_loop_matches_the_oracle_loop(gpu, oracle_mod, mode, resident):
    """refine = "map" from a zero map / refine = "poses" against the true map on the scene workload: device and oracle decision for decision, the costs as
    tests/test_gpu_parity.py's LM parity test compares them."""
    from emba_amd import synth
    from emba_amd.solver import BASettings, LMSettings, solve_time_window
    from test_lm_solver_cpu import perturbed
    w = synth.make_scene_workload(n_steps=1000)
    init = perturbed(w)
    Gx, Gy = (np.zeros_like(w.Gx), np.zeros_like(w.Gy)) if mode == "map" else (w.Gx, w.Gy)
    ba, lm = BASettings(alpha=0.0, refine=mode), LMSettings(max_num_iter=12)
    om = PR.PartialOracleModel(oracle_mod, w)
    ro = solve_time_window(om, init, w.events, Gx, Gy, ba, lm)
    m = make_legm(w)
    rg = solve_time_window(m, init, w.events, Gx, Gy, ba, lm, resident=resident)
    assert [e[4] for e in rg.log] == [e[4] for e in ro.log], "accept/reject sequence differs"
    assert rg.iterations == ro.iterations and rg.converged == ro.converged and rg.reason == ro.reason
    for g, o in zip(rg.log, ro.log):
        assert g[3] == pytest.approx(o[3], rel=1e-7) and g[2] == pytest.approx(o[2], rel=1e-7)
    assert rg.cost_min < rg.log[0][2]
    dGx, dGy = m.downloadMap()
    if mode == "map":
        assert np.array_equal(rg.traj.knots_xyzw, init.knots_xyzw)                          # the knots are bit-identical
        for d, o in zip((dGx, dGy), om.downloadMap()):
            assert np.abs(d - o).max() < 1e-7 * np.abs(o).max()
    else:
        assert np.array_equal(dGx, w.Gx) and np.array_equal(dGy, w.Gy)                      # the map is bit-identical
        assert np.abs(rg.traj.knots_xyzw - ro.traj.knots_xyzw).max() < 1e-7
        assert np.array_equal(rg.traj.knots_xyzw[0], init.knots_xyzw[0])
    m.close()


def test_group_forms_on_one_device(gpu):
    """emba_group_solve_map_only / _poses_only with two ranks on device 0: every rank solves its replica of the all-reduced pack, nothing is exchanged."""
    from emba_amd import _lib
    L = _lib.load()
    w = small()
    lam = 1e-2
    m, ne = formed(w)
    sx2 = m.solveMapOnly(lam)[1]
    m.updateMap(None, 0.7)
    s_map = m.downloadMap()
    m.rejectMap()
    sx1 = m.solvePosesOnly(lam, fix_first_pose=True)[0]
    m.close()
    dp = _lib._dp
    lut = np.ascontiguousarray(w.lut, dtype=np.float64)
    cfg = _lib.EmbaCfg(w.sensor_w, w.sensor_h, w.pano_w, w.pano_h, lut.ctypes.data_as(dp), float(w.C_th), 100, 10.0, 0, None)
    g = C.c_void_p()
    dev = (C.c_int32 * 2)(0, 0)
    assert L.emba_group_create(C.byref(cfg), dev, 2, C.byref(g)) == 0, L.emba_group_last_error(None)
    try:
        ev = w.events
        x = np.ascontiguousarray(ev.x, np.uint16); y = np.ascontiguousarray(ev.y, np.uint16); pol = np.ascontiguousarray(ev.polarity, np.uint8)
        t = np.ascontiguousarray(ev.t_ns, np.int64)
        assert L.emba_group_set_events(g, x.ctypes.data_as(_lib._u16p), y.ctypes.data_as(_lib._u16p), pol.ctypes.data_as(_lib._u8p), t.ctypes.data_as(_lib._i64p), x.size) == 0
        Gx = np.ascontiguousarray(w.Gx); Gy = np.ascontiguousarray(w.Gy)
        assert L.emba_group_upload_map(g, Gx.ctypes.data_as(dp), Gy.ctypes.data_as(dp)) == 0
        knots = np.ascontiguousarray(w.traj.knots_xyzw, np.float64)
        n_inl, P = C.c_size_t(0), C.c_size_t(0)
        st = L.emba_group_step(g, knots.ctypes.data_as(dp), w.K, int(w.traj.t0_ns), int(w.traj.dt_ns), w.thres_valid_pixel, 0, 0.0, w.alpha, C.byref(n_inl), C.byref(P))
        assert st == 0, L.emba_group_last_error(g)
        assert P.value == ne["P"]
        ex = C.c_int32(-1)
        x1j, x2j = np.zeros(3 * w.K), np.zeros(2 * P.value)
        assert L.emba_group_solve(g, lam, 1, x1j.ctypes.data_as(dp), x2j.ctypes.data_as(dp)) == 0, L.emba_group_last_error(g)
        assert L.emba_group_last_solve_exchanged(g, C.byref(ex)) == 0 and ex.value == 1
        gx2 = np.full(2 * P.value, np.nan)
        assert L.emba_group_solve_map_only(g, lam, gx2.ctypes.data_as(dp)) == 0, L.emba_group_last_error(g)
        assert L.emba_group_last_solve_exchanged(g, C.byref(ex)) == 0 and ex.value == 0
        assert_close_elementwise(gx2, sx2, "x2_group_map_only")
        assert L.emba_group_update_map(g, None, 0.7) == 0, L.emba_group_last_error(g)
        gGx, gGy = np.empty_like(Gx), np.empty_like(Gy)
        assert L.emba_group_download_map(g, gGx.ctypes.data_as(dp), gGy.ctypes.data_as(dp)) == 0
        assert L.emba_group_map_reject(g) == 0, L.emba_group_last_error(g)
        for d, s in zip((gGx, gGy), s_map):
            assert np.allclose(d, s, rtol=0, atol=1e-9 * np.abs(s).max())
        gx1 = np.full(3 * w.K, np.nan)
        assert L.emba_group_solve_poses_only(g, lam, 1, gx1.ctypes.data_as(dp)) == 0, L.emba_group_last_error(g)
        assert L.emba_group_last_solve_exchanged(g, C.byref(ex)) == 0 and ex.value == 0
        assert_close_elementwise(gx1, sx1, "x1_group_poses_only")
        assert L.emba_group_update_map(g, None, 0.7) != 0    # no x2 on the ranks after a poses-only solve
        # the joint group solve is what it was (its received records are still cached: no second exchange)
        y1, y2 = np.zeros(3 * w.K), np.zeros(2 * P.value)
        assert L.emba_group_solve(g, lam, 1, y1.ctypes.data_as(dp), y2.ctypes.data_as(dp)) == 0, L.emba_group_last_error(g)
        assert L.emba_group_last_solve_exchanged(g, C.byref(ex)) == 0 and ex.value == 0
        assert np.allclose(y1, x1j, rtol=1e-9, atol=1e-9 * np.abs(x1j).max()) and np.allclose(y2, x2j, rtol=1e-9, atol=1e-9 * np.abs(x2j).max())
    finally:
        L.emba_group_destroy(g)


def test_poisoned_workspace(gpu):
    """option poison: every new device allocation reads as NaN — nothing of the two solves may depend on what its workspace happens to hold"""
    w = panel()
    m, ne = formed(w, poison=1)
    lam = 1e-3
    x2 = m.solveMapOnly(lam)[1]
    assert np.isfinite(x2).all()
    assert_close_elementwise(x2, PR.solve_map_only(ne, lam)[0], "x2_map_only poisoned")
    m.updateMap(None, 1.0)
    assert all(np.isfinite(p).all() for p in m.downloadMap())
    m.rejectMap()
    x1 = m.solvePosesOnly(lam, fix_first_pose=True)[0]
    assert np.isfinite(x1).all()
    assert_close_elementwise(x1, PR.solve_poses_only(ne, lam, True), "x1_poses_only poisoned")
    m.close()
