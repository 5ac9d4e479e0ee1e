"""Every kernel variant behind emba_set_option against the CPU oracle (-m gpu).

include/emba_hip.h: every option changes speed or the internal form only.  The tile order's four LDS tile shapes, both grids of tile origins,
the reserves, the chunking of a tile, the auto order rule at small sizes, the pixel order's pose forms and the Gram kernel's forms, the
alternating record sets, the CSR counts of the solve and the Poisson forms are each run here, on inputs chosen for the edge they reach (a
fast pan across the panorama seam, both poles, a panorama smaller than every tile, heavy collisions, K = 2, the inline-knot limit, ragged
warp groups, the BASELINE window), and compared with the oracle at the bounds of test_gpu_parity.py.  tests/option_matrix.py lists
which test runs which option value.  The oracle's result does not depend on options: it is computed once per workload.
"""
import math

import numpy as np
import pytest

import option_matrix as OM
from helpers import assert_close, oracle_run, small_workload
from test_gpu_parity import compare_event_state, compare_normal_eq

pytestmark = pytest.mark.gpu

OPTIONS = {}      # emba_set_option values every context of a test gets, before its events are set (as in test_gpu_parity.py)
LAM = 1e-2
K_INLINE = OM.parse_constants()["kInlineKnots"]
WARP_NEW = OM.parse_constants()["kWarpNew"]
TILE_ROUND = OM.tile_round()   # entries of one round of the tiled kernel's waves: kWarpNew x kTileWaves


def _pole(sign):
    from emba_amd.synth import so3_exp_xyzw
    w = small_workload(n_events=40000, pano_h=128, K=6, thres_valid_pixel=2)
    w.traj.knots_xyzw[:] = np.stack([so3_exp_xyzw([sign * (1.2 + 0.08 * i), 0.0, 0.0]) for i in range(w.K)])
    return w


def _drift_rotated():
    """The 0.3-rad yaw rotation of test_tile_order_rebins_after_trajectory_drift, applied to every control pose."""
    from emba_amd.synth import so3_exp_xyzw
    w = WORKLOADS["drift"]()
    ex, ey, ez, ew = so3_exp_xyzw(np.array([0.0, 0.3, 0.0]))
    for i in range(w.K):
        bx, by, bz, bw = w.traj.knots_xyzw[i]
        q = np.array([ew * bx + ex * bw + ey * bz - ez * by, ew * by + ey * bw + ez * bx - ex * bz,
                      ew * bz + ez * bw + ex * by - ey * bx, ew * bw - ex * bx - ey * by - ez * bz])
        w.traj.knots_xyzw[i] = q / np.linalg.norm(q)
    return w


def _baseline():
    from emba_amd.synth import make_workload
    return make_workload()


WORKLOADS = {
    "pan": lambda: small_workload(n_events=60000, pano_h=256, K=11, sensor=(48, 36), focal=40.0, yaw_rate=6.0),     # fast pan across the seam
    "north": lambda: _pole(1),
    "south": lambda: _pole(-1),
    "tiny": lambda: small_workload(n_events=30000, pano_h=20, K=5, sensor=(24, 18), focal=8.0, yaw_rate=14.0, thres_valid_pixel=2),  # 40 x 20 panorama
    "collide": lambda: small_workload(n_events=8000, pano_h=64, K=4, sensor=(16, 12), focal=12.0),
    "k2": lambda: small_workload(n_events=5000, K=2, thres_valid_pixel=2),
    "k104": lambda: small_workload(n_events=20000, K=K_INLINE, dt_knots=0.002),          # the last K whose knots travel in the kernel arguments
    "k105": lambda: small_workload(n_events=20000, K=K_INLINE + 1, dt_knots=0.002),      # the first staged through pinned memory
    "ragged-1": lambda: small_workload(n_events=WARP_NEW * 317 - 1),
    "ragged": lambda: small_workload(n_events=WARP_NEW * 317),
    "ragged+1": lambda: small_workload(n_events=WARP_NEW * 317 + 1),
    "drift": lambda: small_workload(n_events=60000, pano_h=256, K=11, sensor=(48, 36), focal=40.0),
    "drift-rotated": _drift_rotated,
    "baseline": _baseline,                                                               # what bench.py runs
}

# what each input is chosen for, asserted on the oracle's result so that a change to synth cannot make it vacuous
PROPERTIES = {
    "pan": lambda w, o: o["num_ev_map"][:, 0].any() and o["num_ev_map"][:, -1].any(),
    "north": lambda w, o: o["num_ev_map"][0].any(),
    "south": lambda w, o: o["num_ev_map"][-1].any(),
    "tiny": lambda w, o: (w.pano_w, w.pano_h) == (40, 20) and o["num_ev_map"][:, 0].any() and o["num_ev_map"][:, -1].any() and o["num_ev_map"].max() >= 100,
    "collide": lambda w, o: o["num_ev_map"].max() >= 20,
    "k2": lambda w, o: w.K == 2 and o["num_ev_map"].max() <= 5,
    "k104": lambda w, o: w.K == K_INLINE,
    "k105": lambda w, o: w.K == K_INLINE + 1,
    "ragged-1": lambda w, o: w.events.size() % WARP_NEW == WARP_NEW - 1,
    "ragged": lambda w, o: w.events.size() % WARP_NEW == 0,
    "ragged+1": lambda w, o: w.events.size() % WARP_NEW == 1,
}

TILE_INPUTS = ["pan", "north", "south", "tiny", "baseline"]
PIXEL_INPUTS = ["ragged-1", "ragged", "ragged+1", "k104", "k105", "collide", "baseline"]


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from emba_amd import build
    build.build_hip()
    return True


@pytest.fixture(scope="module")
def ref(oracle_mod):
    """ref(name) -> (workload, oracle result): one oracle pass per workload and module (evaluation with the per-event dump, normal equations,
    L2), the Huber equations and the solve computed on first use.  Callers must not modify what they get."""
    cache = {}

    def get(name):
        if name not in cache:
            w = WORKLOADS[name]()
            big = w.events.size() > 100000
            o = oracle_run(oracle_mod, w, dump=True, dense_A12=not big)
            o["big"] = big
            assert o["ne"]["P"] > 0 and o["ep"].size > 0, f"{name}: degenerate input"
            if name in PROPERTIES:
                assert PROPERTIES[name](w, o), f"{name}: the input no longer has the property it was chosen for"
            cache[name] = (w, o)
        return cache[name]

    def huber(name):
        w, o = get(name)
        if "ne_huber" not in o:
            ne = o["oracle"].form_normal_eq(o["ep"], w.K, o["num_ev_map"], w.thres_valid_pixel, 1, 0.1, False)
            o["ne_huber"] = o["oracle"].apply_l2(ne, w.alpha, w.Gx, w.Gy)
        return o["ne_huber"]

    def solve(name):
        w, o = get(name)
        if "x" not in o:
            if o["big"]:       # (the dense 3K x 2P A12 of the BASELINE window is not formed: the oracle's sparse solve from the same evaluation)
                x1, x2 = o["oracle"].solve_sparse(o["ne"], o["ep"], w.K, o["num_ev_map"], w.thres_valid_pixel, 0, 0.0, LAM, True)
            else:
                x1, x2 = oracle_mod.solve_normal_eq(o["ne"], LAM, True)
            assert np.isfinite(x1).all() and np.isfinite(x2).all(), f"{name}: the oracle does not solve this system finitely"
            o["x"] = (x1, x2)
        return o["x"]

    get.huber, get.solve = huber, solve
    return get


@pytest.fixture
def contexts():
    """make(w, **options): a fresh context with OPTIONS and the given options set before its events; all closed after the test."""
    from emba_amd import LEGM
    made = []

    def make(w, **opts):
        m = LEGM(w.sensor_w, w.sensor_h, w.lut, w.C_th, w.pano_w, w.pano_h, device=0)
        made.append(m)
        for k, v in {**OPTIONS, **opts}.items():
            m.set_option(k, v)
        return m

    yield make
    for m in made:
        m.close()


def evaluate(m, w, o, cost=("quadratic", 0.0), ne_ref=None, dump=False):
    """evaluateDataError + formNormalEq[IRLS] + applyL2Reg on m against the oracle: count map bit-exact, ep, normal equations.  dump: the
    per-event state of the evaluation is compared with the oracle's (compare_event_state) before the equations are formed."""
    nem = np.zeros((w.pano_h, w.pano_w), dtype=np.int32)
    ep = m.evaluateDataError(w.traj, w.Gx, w.Gy, w.events, True, nem)
    if dump:
        compare_event_state(m.dump_state(), o["dump"], w.events.size() // 100 * 100)
    assert np.array_equal(nem, o["num_ev_map"])
    assert ep.shape == o["ep"].shape
    assert_close(ep, o["ep"], "ep")
    if cost[0] == "quadratic":
        m.formNormalEq(ep, w.K, nem, w.thres_valid_pixel)
    else:
        m.formNormalEqIRLS(ep, w.K, nem, w.thres_valid_pixel, cost[0], cost[1])
    compare_normal_eq(m.applyL2Reg(w.alpha), o["ne"] if ne_ref is None else ne_ref)


def check_solves(m, w, name, ref, capfd):
    """solveNormalEq on the formed equations under solve_counts = 2 (the library compares the count map with the records' counts and fails
    with EMBA_ERR_STATE on a mismatch) and, on equations formed again, under 0 (counts from the records); compared as in
    test_randomised_small_configurations."""
    ox1, ox2 = ref.solve(name)
    P = ref(name)[1]["ne"]["P"]
    for counts in (2, 0):
        if counts == 0:
            m.formNormalEq(None, w.K, None, w.thres_valid_pixel)       # (a new active set: the solve's lists are built again)
            m.applyL2Reg(w.alpha)
        m.set_option("solve_counts", counts)
        capfd.readouterr()
        x1, x2 = m.solveNormalEq(LAM, fix_first_pose=True)
        err = capfd.readouterr().err
        if counts == 2:         # the comparison ran (and found nothing: a mismatch is an error above)
            assert f"[solve counts] P {P}: 0 pixels where the count map and the records disagree" in err, err
        assert np.allclose(x1, ox1, rtol=1e-6, atol=1e-8 * max(np.abs(ox1).max(), 1e-30)), f"x1, solve_counts {counts}"
        assert np.allclose(x2, ox2, rtol=1e-6, atol=1e-8 * max(np.abs(ox2).max(), 1e-30)), f"x2, solve_counts {counts}"


def check_step(m, w, o, tag):
    """One resident step (emba_step) at the workload's trajectory against the oracle."""
    n_inl, P = m.step(w.traj, w.thres_valid_pixel, w.alpha)
    assert n_inl == o["ep"].size and P == o["ne"]["P"], tag
    compare_normal_eq(m._finish(w.alpha, False), o["ne"])
    _, ep, nem = m.eval_finish(want_ep=True, want_map=True)
    assert np.array_equal(nem, o["num_ev_map"]), tag
    assert_close(ep, o["ep"], "ep " + tag)


def step_sequence(m, w, o):
    """As test_resident_step_sequences: two steps, two evaluations at other poses that nobody forms, a step."""
    import copy
    for it in range(2):
        check_step(m, w, o, f"step {it}")
    traj2 = copy.deepcopy(w.traj)
    k = traj2.knots_xyzw.copy(); k[:, 0] += 0.01; k /= np.linalg.norm(k, axis=1, keepdims=True); traj2.knots_xyzw = k
    for _ in range(2):
        m.eval_launch(traj2); m.eval_finish(sync=False)
    check_step(m, w, o, "step after unformed evaluations")


# ---- tile order (order = 2) -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", TILE_INPUTS)
@pytest.mark.parametrize("fine", [0, 1])
@pytest.mark.parametrize("shape", [0, 1, 2, 3])
def test_every_tile_instantiation(gpu, ref, contexts, capfd, shape, fine, name):
    """Each emba_warp_tiled_kernel<tw, th> instantiation on the coarse and the fine grid of tile origins (reserve 2): evaluation, normal equations,
    the solve under both CSR count forms and a resident step, against the oracle.  The geometry the library reports is the one kTileShapes
    gives for this shape, grid and reserve: the intended kernel ran."""
    w, o = ref(name)
    m = contexts(w, order=2, tile_shape=shape, tile_fine=fine, tile_reserve=2)
    evaluate(m, w, o)
    info = m.setup_info()
    assert info["tile_order"] and info["tile"] == OM.tile_geometry(shape, bool(fine), 2), info
    if name == "pan":
        assert info["entries"] > m.event_counts()[0], "no lead-in copies on the fast pan"
    check_solves(m, w, name, ref, capfd)
    check_step(m, w, o, f"shape {shape} fine {fine}")


@pytest.mark.parametrize("reserve", [0, 5])
@pytest.mark.parametrize("shape", [0, 1, 2, 3])
def test_tile_reserve_extremes(gpu, ref, contexts, shape, reserve):
    """Reserves 0 and 5 on every shape (at 5 the 96 x 12 tile has a 2-px pitch in y), on the fast pan."""
    w, o = ref("pan")
    m = contexts(w, order=2, tile_shape=shape, tile_fine=0, tile_reserve=reserve)
    evaluate(m, w, o)
    info = m.setup_info()
    assert info["tile_order"] and info["tile"] == OM.tile_geometry(shape, False, reserve), info
    check_step(m, w, o, f"shape {shape} reserve {reserve}")


@pytest.mark.parametrize("order_bin", [0, 1])
@pytest.mark.parametrize("chunk", [TILE_ROUND, 100])
def test_tile_chunking(gpu, ref, contexts, chunk, order_bin):
    """tile_chunk = one round of the workgroup's waves, and below one round (pieces are rounded up to whole rounds: some computed pieces are
    empty and skipped, a tile's last piece is ragged), with the chunks longest first and in bin order."""
    w, o = ref("pan")
    m = contexts(w, order=2, tile_chunk=chunk, chunk_order_bin=order_bin)
    evaluate(m, w, o)
    info = m.setup_info()
    assert info["tile_order"]
    assert info["entries"] > m.event_counts()[0], "no lead-in copies on the fast pan"
    assert info["chunks"] >= math.ceil(info["entries"] / TILE_ROUND), info
    check_step(m, w, o, f"chunk {chunk} bin order {order_bin}")


@pytest.mark.parametrize("shape", [0, 1, 2, 3])
def test_tile_order_after_drift_per_shape(gpu, ref, contexts, capfd, shape):
    """test_tile_order_rebins_after_trajectory_drift for every shape: bins from the first trajectory, then poses rotated by 0.3 rad — inliers outside
    their tile go to HBM one by one — must still give the oracle's results, and the solve on them too."""
    w, o = ref("drift")
    w2, o2 = ref("drift-rotated")
    m = contexts(w, order=2, tile_shape=shape)
    evaluate(m, w, o)
    assert m.setup_info()["tile_order"] and m.setup_info()["tile"]["w"] == OM.parse_tile_shapes()[shape]["tw"]
    assert m.tile_drift() == (0, 0)
    nem = np.zeros((w2.pano_h, w2.pano_w), dtype=np.int32)
    ep = m.evaluateDataError(w2.traj, None, None, None, True, nem)       # the old bins, the new poses
    assert m.tile_drift()[0] > 0
    assert np.array_equal(nem, o2["num_ev_map"])
    assert_close(ep, o2["ep"], "ep")
    m.formNormalEq(ep, w2.K, nem, w2.thres_valid_pixel)
    compare_normal_eq(m.applyL2Reg(w2.alpha), o2["ne"])
    check_solves(m, w2, "drift-rotated", ref, capfd)


@pytest.mark.parametrize("shape,fine", [(2, 0), (3, 1)])
def test_tile_order_event_state(gpu, ref, contexts, shape, fine):
    """Per-event state of a tile-order evaluation (the dump twin of the tiled kernel) against the oracle's, one coarse and one fine shape."""
    w, o = ref("pan")
    m = contexts(w, order=2, tile_shape=shape, tile_fine=fine)
    evaluate(m, w, o, dump=True)
    assert m.setup_info()["tile"] == OM.tile_geometry(shape, bool(fine), 2)


@pytest.mark.parametrize("name", ["k2", "k105"])
def test_tile_order_k_edges(gpu, ref, contexts, name):
    w, o = ref(name)
    m = contexts(w, order=2)
    evaluate(m, w, o)
    assert m.setup_info()["tile_order"]
    check_step(m, w, o, name)


def test_auto_order_rule_at_small_sizes(gpu, ref, contexts):
    """order = 0 with tile_min_events = 0: the pricing rule runs at test sizes.  Whichever order it picks, the oracle's results; the two inputs
    take both orders between them."""
    taken = {}
    for name in ("tiny", "k2"):
        w, o = ref(name)
        m = contexts(w, order=0, tile_min_events=0)
        evaluate(m, w, o)
        taken[name] = m.setup_info()["tile_order"]
        check_step(m, w, o, name)
    print("tile order taken:", taken)
    assert set(taken.values()) == {True, False}, taken


# ---- pixel order (order = 1) ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", PIXEL_INPUTS)
@pytest.mark.parametrize("segpose", [1, 2])
def test_pixel_order_segpose(gpu, ref, contexts, capfd, segpose, name):
    """segpose 1 (per-batch pose table) and 2 (per-event pose from the segment records): evaluation, normal equations, per-event state of the
    dump kernel, and the solve under both CSR count forms."""
    w, o = ref(name)
    m = contexts(w, order=1, segpose=segpose)
    evaluate(m, w, o, dump=True)
    assert not m.setup_info()["tile_order"]
    check_solves(m, w, name, ref, capfd)


GRAM_FORMS = [dict(gram_tags=0), dict(gather_waves=1), dict(gather_waves=2), dict(gather_waves=4), dict(gram_sparse=0),
              dict(gram_sparse=1, gram_sparse_chunk=1), dict(gram_sparse=1, gram_sparse_chunk=8), dict(step_gather=3)]


@pytest.mark.parametrize("name", PIXEL_INPUTS)
@pytest.mark.parametrize("opts", GRAM_FORMS, ids=lambda d: "-".join(f"{k}{v}" for k, v in d.items()))
def test_pixel_order_gram_forms(gpu, ref, contexts, opts, name):
    """The Gram kernel's and the resident step's forms: formNormalEqIRLS (Huber) and formNormalEq on one evaluation, then two resident steps, two
    unformed evaluations, a step and a Huber step.  The forms are called with the device-resident residuals (ep = None), as solver.py calls
    them: a host ep turns the tag stream off (gram_uses_tags), and with it the tag and sparse forms of the Gram kernel under test."""
    w, o = ref(name)
    m = contexts(w, order=1, **opts)
    nem = np.zeros((w.pano_h, w.pano_w), dtype=np.int32)
    ep = m.evaluateDataError(w.traj, w.Gx, w.Gy, w.events, True, nem)
    assert np.array_equal(nem, o["num_ev_map"])
    assert_close(ep, o["ep"], "ep")
    m.formNormalEqIRLS(None, w.K, None, w.thres_valid_pixel, "huber", 0.1)
    compare_normal_eq(m.applyL2Reg(w.alpha), ref.huber(name))
    m.formNormalEq(None, w.K, None, w.thres_valid_pixel)
    compare_normal_eq(m.applyL2Reg(w.alpha), o["ne"])
    step_sequence(m, w, o)
    n_inl, P = m.step(w.traj, w.thres_valid_pixel, w.alpha, "huber", 0.1)
    assert n_inl == o["ep"].size and P == o["ne"]["P"]
    compare_normal_eq(m._finish(w.alpha, False), ref.huber(name))


@pytest.mark.parametrize("name", PIXEL_INPUTS)
def test_step_alternating_record_sets(gpu, ref, contexts, name):
    """step_one_set = 0: the step alternates between the two record sets like an LM loop's evaluations; the step sequence three times, so both
    sets are used and reused."""
    w, o = ref(name)
    m = contexts(w, order=1, step_one_set=0)
    m.set_events(w.events)
    m.upload_map(w.Gx, w.Gy)
    for _ in range(3):
        step_sequence(m, w, o)


# ---- Poisson reconstruction -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("pano_h,opts", [(256, dict(poisson=2)), (1024, dict(poisson=2)), (1024, dict(gemm64=1)), (2048, dict(gemm64=1)),
                                         (1024, dict(poisson=1))], ids=lambda x: str(x) if isinstance(x, int) else "-".join(f"{k}{v}" for k, v in x.items()))
def test_poisson_forms(gpu, contexts, pano_h, opts):
    """The unfolded Fourier form at even H, the 64-wide GEMM tiles in place of the 128-wide kernel, the dense sine transforms at 1024, against
    oracle/poisson.py at the bound of test_poisson_reconstruction_matches_oracle."""
    from oracle import poisson as OP
    w = small_workload(n_events=2000, pano_h=pano_h)
    m = contexts(w, **opts)
    rng = np.random.default_rng(pano_h)
    Gx, Gy = rng.normal(size=(w.pano_h, w.pano_w)), rng.normal(size=(w.pano_h, w.pano_w))
    assert_close(m.reconstructIntensity(Gx, Gy), OP.reconstruct_from_gradient(Gx, Gy), "intensity panorama", tight=1e-10)
