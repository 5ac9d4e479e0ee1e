"""GPU tests (-m gpu) of the solvers at their capacity edges in the number of control poses K (tests/solve_edge_cases.py derives them from the kernels' LDS
footprints): the Schur solve on either side of the launch that needs hipFuncAttributeMaxDynamicSharedMemorySize raised (K = 303 / 304), at the last K the
U build's column staging fits a CU's LDS (758: 36 row blocks of S, 163 728 of 163 840 bytes) and at the first it must refuse (759); conjugate gradients on
either side of its raise (1365 / 1366), at its last K (3413) and at its refusal (3414).  Against the CPU oracle, whose results are computed once per K.

Tolerance of the Schur parity (measured on the CPU, tests/solve_edge_cases.py: refine_once): the oracle's solution against one step of iterative refinement of
it in np.longdouble on the dense damped system differs by at most 1.3e-14 of max |x1| and 2.7e-15 of max |x2| at K = 303, 304 and 758 (36 panels, n = 2274) alike —
5.4e-6 of the suite's bound |x - ref| <= 1e-9 max |ref| + 1e-7 |ref| in that bound's own metric.  100 x the spread (5.4e-4) stays below the suite's bound, so the
suite's bound is what is asserted; the rule (the larger of the two) is evaluated again in every run, from the reference alone."""
import ctypes as C

import numpy as np
import pytest

import partial_ref as PR
import solve_edge_cases as E
from helpers import assert_close, assert_close_elementwise, oracle_run

pytestmark = pytest.mark.gpu

RTOL, ATOL_REL = 1e-7, 1e-9      # the suite's Schur parity bound (tests/test_gpu_parity.py): np.allclose(x, ref, rtol, atol = ATOL_REL max |ref|)
CG_LAM, CG_FIX = 1e-2, True


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from emba_amd import build
    build.build_hip()
    return True


def in_suite_metric(x, ref):
    """max |x - ref| / (ATOL_REL max |ref| + RTOL |ref|): <= 1 iff np.allclose(x, ref, RTOL, ATOL_REL max |ref|)"""
    ref = np.asarray(ref)
    return float(np.max(np.abs(np.asarray(x) - ref) / (ATOL_REL * np.abs(ref).max() + RTOL * np.abs(ref))))


_CASES = {}


@pytest.fixture(scope="module")
def case(oracle_mod):
    """case(K) -> the workload, the oracle's equations and its solutions, computed at the first request and kept for the module (K = 758: two dense solves of
    10 s each on one thread).  Nothing of it is written to afterwards."""
    def get(K):
        if K in _CASES:
            return _CASES[K]
        w = E.workload(K)
        dense = K in E.SCHUR_PARITY_KS
        o = oracle_run(oracle_mod, w, dense_A12=dense)
        ne = o["ne"]
        c = dict(K=K, w=w, ne=ne, P=ne["P"], A11_diag=np.diag(ne["A11"]).copy(), schur={}, n_inliers=o["ep"].size)
        if dense:
            for lam, fix in E.SOLVES:
                x1, x2 = oracle_mod.solve_normal_eq(ne, lam, fix)
                y1, y2 = E.refine_once(ne, lam, fix, x1, x2)
                spread = (E.spread(x1, y1), E.spread(x2, y2))
                scale = max(1.0, 100.0 * in_suite_metric(x1, y1), 100.0 * in_suite_metric(x2, y2))
                res = E.damped_residual(ne, lam, fix, x1, x2)
                print(f"K = {K} lambda {lam:g} fix {fix}: oracle against its refinement {spread[0]:.2e} / {spread[1]:.2e} of max |x1| / |x2|; "
                      f"bound = {scale:g} x the suite's; oracle residual {res[0]:.2e} / {res[1]:.2e}")
                c["schur"][(lam, fix)] = dict(x1=x1, x2=x2, scale=scale, res=res)
        if K >= E.K_SCHUR_REFUSED and K != E.K_CG_REFUSED:
            thres = w.thres_valid_pixel
            c["cg10"] = o["oracle"].solve_cg_sparse(ne, o["ep"], K, o["num_ev_map"], thres, 0, 0.0, CG_LAM, CG_FIX, max_iter=10, tol=1e-30)
            if K == E.K_CG_RAISE:
                c["cg"] = o["oracle"].solve_cg_sparse(ne, o["ep"], K, o["num_ev_map"], thres, 0, 0.0, CG_LAM, CG_FIX)
        if K in (E.K_SCHUR_REFUSED, E.K_CG_REFUSED):
            c["poses_only"] = PR.solve_poses_only(ne, CG_LAM, True)
            c["map_only"] = PR.solve_map_only(ne, CG_LAM)
        if K >= E.K_CG_LAST:              # (0.84 GB of A11 each: the diagonal is what the tests compare)
            ne["A11"] = None
        del o
        _CASES[K] = c
        return c
    yield get
    _CASES.clear()


def formed(c, options=None, m=None):
    """A context (or the given one, on a fresh window) with the resident step done — evaluateDataError + formNormalEq + applyL2Reg in one call, nothing read back"""
    from emba_amd import LEGM
    w = c["w"]
    if m is None:
        m = LEGM(w.sensor_w, w.sensor_h, w.lut, w.C_th, w.pano_w, w.pano_h, device=0)
        for k, v in (options or {}).items():
            m.set_option(k, v)
    m.set_events(w.events)
    m.upload_map(w.Gx, w.Gy)
    n_inl, P = m.step(w.traj, w.thres_valid_pixel, w.alpha)
    assert n_inl == c["n_inliers"] and P == c["P"]
    return m


def compare_equations(m, c):
    """(a) the device's normal equations against the oracle's: compare_normal_eq of tests/test_gpu_parity.py; from K = 3413 (A11: 0.84 GB) A11 by its diagonal"""
    from test_gpu_parity import compare_normal_eq
    g = m._finish(c["w"].alpha, False)                     # (download only: the L2 term was applied inside the step)
    if c["ne"]["A11"] is not None:
        return compare_normal_eq(g, c["ne"])
    d = np.diag(g["A11"]).copy()
    g["A11"] = None
    o = c["ne"]
    assert g["P"] == o["P"] and np.array_equal(g["active"], o["active"])
    assert_close(d, c["A11_diag"], "A11_diag"); assert_close(g["b1"], o["b1"], "b1")
    assert_close(g["A22"], o["A22"], "A22"); assert_close(g["b2"], o["b2"], "b2")


def check_schur(m, c, lam, fix, what=""):
    """(b) + (d): one solveNormalEq against the oracle's solution within the measured bound, and the residual of the full damped system for the DEVICE's
    (x1, x2) in np.longdouble — at most 100 x the same residual of the oracle's solution, pose rows and map rows (rounding order differs between the two; a wrong
    block does not give 100 x).  Measured: pose rows 22 x the oracle's at K = 304 (8.0e-14 against 3.6e-15 of max |b1|), 36 x at K = 758 (2.2e-13 against 6.1e-15);
    map rows 10 x and 17 x."""
    r = c["schur"][(lam, fix)]
    x1, x2 = m.solveNormalEq(lam, fix_first_pose=fix)
    assert m.last_solve_info() == 0, what
    assert x1.shape == r["x1"].shape and x2.shape == r["x2"].shape
    e1, e2 = in_suite_metric(x1, r["x1"]), in_suite_metric(x2, r["x2"])
    res = E.damped_residual(c["ne"], lam, fix, x1, x2)
    print(f"K = {c['K']} {what} lambda {lam:g} fix {fix}: x1 {e1:.2e} x2 {e2:.2e} of the suite's bound (asserted: {r['scale']:g}); "
          f"residual {res[0]:.2e} / {res[1]:.2e}, the oracle's {r['res'][0]:.2e} / {r['res'][1]:.2e}")
    assert e1 <= r["scale"] and e2 <= r["scale"], what
    if fix:
        assert (x1[:3] == 0).all()
    assert res[0] <= 100 * r["res"][0] and res[1] <= 100 * r["res"][1], what
    return x1, x2


@pytest.mark.parametrize("K", sorted(E.N_EVENTS))
def test_normal_equations_at_every_K(gpu, case, K):
    """(a) What a failing solve below is NOT: the equations.  Also the first parity check of the Gram path's 16-bit pair key above K = 256."""
    c = case(K)
    m = formed(c)
    compare_equations(m, c)
    m.close()


@pytest.mark.parametrize("K", E.SCHUR_PARITY_KS)
def test_schur_solve_around_the_lds_raise_and_at_the_last_K(gpu, case, K):
    """(b), (d) K = 303: 65 448 bytes of dynamic LDS, the last launch of the U build as it is; 304: 65 664, the first that needs the attribute raised;
    758: 163 728, 112 bytes under the CU's 160 KB, 36 row blocks and panels.  Twice: the second call re-uses the cached lists."""
    c = case(K)
    m = formed(c)
    for lam, fix in E.SOLVES:
        check_schur(m, c, lam, fix)
    m.close()


@pytest.mark.parametrize("opts", [dict(), dict(syrk_lists=1), dict(syrk_lists=2), dict(syrk_lists=2, syrk_item_cap=8), dict(syrk_dense=1), dict(solve_perm=0), dict(solve_perm=1)],
                         ids=["auto", "lists", "items", "items_overflow", "dense", "perm_off", "perm_on"])
def test_every_form_of_the_product_at_the_last_K(gpu, case, opts):
    """(c) K = 758: what solve_perm_size_ok and items_form decide by themselves, then every form of S -= U U^T and both column orders forced — bits 32 ... 35 of
    the slice masks, 16-row groups up to 142, 666 block pairs — against the one oracle solution."""
    c = case(E.K_SCHUR_LAST)
    m = formed(c, opts)
    lam, fix = E.SOLVES[0]
    check_schur(m, c, lam, fix, str(opts))
    m.close()


def test_schur_solve_refuses_the_first_K_beyond_the_lds(gpu, case):
    """(e) K = 759: 163 944 bytes.  The refusal by name, and a context that is intact after it."""
    from emba_amd import EmbaError
    from emba_amd._lib import ERR_CAPACITY
    c = case(E.K_SCHUR_REFUSED)
    m = formed(c)
    for _ in range(2):
        with pytest.raises(EmbaError) as ei:
            m.solveNormalEq(1e-2, fix_first_pose=True)
        assert ei.value.status == ERR_CAPACITY and f"K={E.K_SCHUR_REFUSED} too large for the per-wave column staging in LDS" in str(ei.value)
    compare_equations(m, c)
    x1 = m.solvePosesOnly(CG_LAM, fix_first_pose=True)[0]              # neither partial solve builds U
    assert_close_elementwise(x1, c["poses_only"], "x1_poses_only after the refusal")
    x2 = m.solveMapOnly(CG_LAM)[1]
    assert c["map_only"][1] == 0
    assert_close_elementwise(x2, c["map_only"][0], "x2_map_only after the refusal")
    check_cg10(m, c)                                                   # 36 432 bytes of LDS: conjugate gradients take this K
    # a fresh window of K = 304 on the same context
    c304 = case(E.K_SCHUR_RAISE)
    formed(c304, m=m)
    check_schur(m, c304, *E.SOLVES[0], what="after K = 759")
    m.close()


def check_cg10(m, c):
    """ten iterations on both sides: the same iterate to rounding (the bound of test_cg_solve_parity)"""
    o1, o2, oit, _ = c["cg10"]
    x1, x2, it, _ = m.solveNormalEqCG(CG_LAM, fix_first_pose=CG_FIX, max_iter=10, tol=1e-30)
    assert it == oit == 10
    e1, e2 = np.abs(x1 - o1).max() / np.abs(o1).max(), np.abs(x2 - o2).max() / np.abs(o2).max()
    print(f"K = {c['K']}: ten CG iterations, x1 {e1:.2e} x2 {e2:.2e} of the largest (bound 1e-8)")
    assert e1 <= 1e-8 and e2 <= 1e-8
    assert (x1[:3] == 0).all()


@pytest.mark.parametrize("K", [E.K_CG_NO_RAISE, E.K_CG_RAISE, E.K_CG_LAST])
def test_cg_around_the_lds_raise_and_at_the_last_K(gpu, case, K):
    """(f) emba_cg_pixel_kernel keeps 16 x 3K bytes: 65 520 at K = 1365, 65 568 at 1366 (the raise), 163 824 at 3413 (16 bytes under the CU's LDS).  The
    equations are formed by the resident step; at 3413 running to the tolerance would take the oracle 100 s, so fixed iteration counts only."""
    c = case(K)
    m = formed(c)
    check_cg10(m, c)
    if K == E.K_CG_RAISE:           # the default stopping rule (100 iterations, 1e-6)
        o1, o2, oit, oerr = c["cg"]
        x1, x2, it, err = m.solveNormalEqCG(CG_LAM, fix_first_pose=CG_FIX)
        print(f"K = {K}: stopped after {it} iterations at {err:.2e}, the oracle after {oit} at {oerr:.2e}")
        assert abs(it - oit) <= 2 and err < 1e-6 and oerr < 1e-6
    m.close()


def test_cg_refuses_the_first_K_beyond_the_lds(gpu, case):
    """(f) K = 3414: 163 872 bytes — refused by name; the poses-only solve on that context (160 panels of the factorisation) matches its reference."""
    from emba_amd import EmbaError
    from emba_amd._lib import ERR_CAPACITY
    c = case(E.K_CG_REFUSED)
    m = formed(c)
    with pytest.raises(EmbaError) as ei:
        m.solveNormalEqCG(CG_LAM, fix_first_pose=CG_FIX, max_iter=10, tol=1e-30)
    assert ei.value.status == ERR_CAPACITY and "solveNormalEqCG" in str(ei.value) and f"K = {E.K_CG_REFUSED}" in str(ei.value)
    x1 = m.solvePosesOnly(CG_LAM, fix_first_pose=True)[0]
    assert_close_elementwise(x1, c["poses_only"], "x1_poses_only at K = 3414")
    m.close()


def test_group_solve_raises_the_lds_too(gpu, case):
    """(g) emba_solve_shard_partial goes through the same U build and raise: K = 304 through the one-device group engine, two ranks, against the single-context
    solution (two device solutions: the suite's bound)."""
    from emba_amd import _lib
    L = _lib.load()
    c = case(E.K_SCHUR_RAISE)
    w = c["w"]
    lam, fix = E.SOLVES[0]
    m = formed(c)
    sx1, sx2 = m.solveNormalEq(lam, fix_first_pose=fix)
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
        assert P.value == c["P"]
        x1, x2 = np.zeros(3 * w.K), np.zeros(2 * P.value)
        assert L.emba_group_solve(g, lam, 1 if fix else 0, x1.ctypes.data_as(dp), x2.ctypes.data_as(dp)) == 0, L.emba_group_last_error(g)
        ex = C.c_int32(-1)
        assert L.emba_group_last_solve_exchanged(g, C.byref(ex)) == 0 and ex.value == 1
        e1, e2 = in_suite_metric(x1, sx1), in_suite_metric(x2, sx2)
        print(f"group solve at K = {w.K}: x1 {e1:.2e} x2 {e2:.2e} of the suite's bound against the single context")
        assert e1 <= 1 and e2 <= 1
        r = c["schur"][(lam, fix)]
        assert in_suite_metric(x1, r["x1"]) <= r["scale"] and in_suite_metric(x2, r["x2"]) <= r["scale"]
    finally:
        L.emba_group_destroy(g)
