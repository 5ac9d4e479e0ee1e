"""GPU test of the sharded path with the REAL engine (emba_amd.LEGM via HipEngine): two ranks as two threads on one MI355X,
each with its own context/stream and its own time shard + halo, exchanging through an in-process all-reduce stand-in.
Checks exchange 1 (count map), exchange 2 (pack), applyL2Reg-after-reduce and the residual merge against the single-context
result and the oracle.  (The RCCL collectives themselves are exercised by bench.py --gpus N on a multi-GPU node.)"""
import threading

import numpy as np
import pytest

from helpers import assert_close, oracle_run, small_workload

pytestmark = pytest.mark.gpu


class _Shared:
    def __init__(self, world):
        self.world = world
        self.barrier = threading.Barrier(world)
        self.slots = [None] * world
        self.errors = []


class _ThreadDist:
    """torch.distributed-like handle for one rank-thread."""

    def __init__(self, shared, rank, sync_fn):
        self.s, self.rank, self.sync_fn = shared, rank, sync_fn

    def get_rank(self):
        return self.rank

    def get_world_size(self):
        return self.s.world

    class _Done:
        def wait(self):
            return True

    def all_reduce(self, t, async_op=False):
        """(async_op: performed on the spot; the handle's wait() has nothing left to do — rank threads cannot overlap it)"""
        import torch
        self.sync_fn()                       # producer kernels of this rank are done
        self.s.slots[self.rank] = t
        self.s.barrier.wait()
        if self.rank == 0:
            total = self.s.slots[0].clone()
            for other in self.s.slots[1:]:
                total += other
            for sl in self.s.slots:
                sl.copy_(total)
            torch.cuda.synchronize()
        self.s.barrier.wait()
        return self._Done() if async_op else None

    def all_to_all_single(self, out, inp, out_splits, in_splits):
        """Rank r's j-th input piece goes to rank j, where it becomes the r-th output piece."""
        import torch
        self.sync_fn()
        self.s.slots[self.rank] = (out, inp, list(out_splits), list(in_splits))
        self.s.barrier.wait()
        if self.rank == 0:
            W = self.s.world
            for src in range(W):
                _, inp_s, _, ins = self.s.slots[src]
                ioff = 0
                for dst in range(W):
                    out_d, _, outs, _ = self.s.slots[dst]
                    ooff = sum(outs[:src])
                    assert outs[src] == ins[dst]
                    out_d[ooff:ooff + outs[src]].copy_(inp_s[ioff:ioff + ins[dst]])
                    ioff += ins[dst]
            torch.cuda.synchronize()
        self.s.barrier.wait()


def _rank_main(shared, rank, w, results, compressed=False, solve=None):
    try:
        import torch
        from emba_amd import LEGM
        from emba_amd.sharded import HipEngine, ShardedLEGM
        dev = torch.device("cuda", 0)
        npix = w.pano_h * w.pano_w
        m = LEGM(w.sensor_w, w.sensor_h, w.lut, w.C_th, w.pano_w, w.pano_h, device=0)
        count = torch.zeros(npix, dtype=torch.int32, device=dev)
        pack = torch.zeros(9 * w.K * w.K + 3 * w.K + 5 * npix, dtype=torch.float64, device=dev)
        torch.cuda.synchronize()
        cu8 = torch.zeros(npix, dtype=torch.uint8, device=dev) if compressed else None
        sh = ShardedLEGM(HipEngine(m, check_stream=False), _ThreadDist(shared, rank, m.sync), count, pack, w.sensor_w, cu8)
        local = sh.set_events(w.events)
        m.upload_map(w.Gx, w.Gy)
        out = None
        for _ in range(2):                    # twice: the per-pixel accumulator must be cleared between evaluations
            n_inl, out = sh.iteration(w.traj, w.thres_valid_pixel, w.alpha, download=True)
        sol = sh.solveNormalEq(*solve[:2]) if solve else None
        extra = {}
        if solve and len(solve) > 2:          # (lam, fix, lam2): a RE-SOLVE of the same equations with another lambda, then the sharded CG on them
            extra["exchanged_first"] = sh.last_solve_exchanged
            extra["resolve"] = sh.solveNormalEq(solve[2], solve[1])
            extra["exchanged_resolve"] = sh.last_solve_exchanged
            extra["cg"] = sh.solveNormalEqCG(solve[0], solve[1])
            extra["exchanged_cg"] = sh.last_solve_exchanged
            extra["cg10"] = sh.solveNormalEqCG(solve[0], solve[1], max_iter=10, tol=1e-30)
        d = m.dump_state()
        _, ep, _ = m.eval_finish(want_ep=True)
        pix = local.y.astype(np.int64) * w.sensor_w + local.x
        ep_pix = np.zeros(ep.size, dtype=np.int64)
        sel = d["inlier_idx"] >= 0
        ep_pix[d["inlier_idx"][sel]] = pix[sel]
        resident = bool(getattr(sh, "last_form_resident", False))       # (round 5: the global saturated counts then stay in the byte buffer of exchange 1)
        results[rank] = dict(ne=out, count=(cu8 if resident else count).cpu().numpy().astype(np.int32), ep=ep.copy(), ep_pix=ep_pix, n_inl=n_inl, sol=sol,
                             resident=resident, **extra)
    except Exception as e:  # noqa: BLE001
        shared.errors.append((rank, repr(e)))
        shared.barrier.abort()
        raise


@pytest.mark.parametrize("cfg,compressed,split", [(dict(n_events=20000), False, 0), (dict(n_events=30050, pano_h=256, K=11, sensor=(64, 48), focal=60.0), False, 1),
                                                  (dict(n_events=20000), True, 1), (dict(n_events=20000), True, 0),
                                                  (dict(n_events=30050, pano_h=75, K=11, sensor=(48, 36), focal=45.0), True, None)])
def test_two_rank_threads_on_one_gpu(oracle_mod, cfg, compressed, split, monkeypatch):
    # exchange 2 in one piece (what these sizes get by default) and split (A22 | b2 rows reduced while the Gram kernel runs); compressed exchange 1 WITHOUT the
    # split: the ranks form as resident steps (round 5: emba_step_form_active on the exchanged bytes — lists, gather inside the Gram launch, no clearing pass)
    monkeypatch.setattr("emba_amd.sharded.HipEngine.x2_split", split)
    import torch
    assert torch.cuda.is_available()
    from emba_amd.sharded import merge_ep
    w = small_workload(**cfg)
    world = 2
    shared, results = _Shared(world), [None] * world
    th = [threading.Thread(target=_rank_main, args=(shared, r, w, results, compressed)) for r in range(world)]
    [t.start() for t in th]
    [t.join(timeout=120) for t in th]
    assert not shared.errors, shared.errors
    o = oracle_run(oracle_mod, w)
    for r in range(world):
        assert results[r]["resident"] == (compressed and not split)
        got = results[r]["count"].reshape(w.pano_h, w.pano_w)
        if compressed:   # saturated bytes: exact below the per-rank cap, same activity everywhere
            assert np.array_equal(got >= w.thres_valid_pixel, o["num_ev_map"] >= w.thres_valid_pixel)
            assert np.array_equal(got[o["num_ev_map"] < 127], o["num_ev_map"][o["num_ev_map"] < 127])
        else:
            assert np.array_equal(got, o["num_ev_map"])       # exchange 1, bit-exact
        ne = results[r]["ne"]
        assert np.array_equal(ne["active"], o["ne"]["active"])
        for name in ("A11", "b1", "A22", "b2"):
            assert_close(ne[name], o["ne"][name], f"rank{r} {name}")
    ep = merge_ep([results[r]["ep"] for r in range(world)], [results[r]["ep_pix"] for r in range(world)])
    assert_close(ep, o["ep"], "merged ep")
    assert sum(results[r]["n_inl"] for r in range(world)) == o["ep"].size


@pytest.mark.parametrize("cfg,world,lam,fix", [
    (dict(n_events=20000), 2, 1e-3, True),
    (dict(n_events=40000, pano_h=256, K=21, sensor=(64, 48), focal=60.0, dt_knots=0.01), 3, 1e-2, False),
])
def test_sharded_schur_solve(oracle_mod, cfg, world, lam, fix):
    """f1 under sharding: every rank-thread holds a time shard (+ halo); the records are re-distributed by pixel owner, the Schur sums
    all-reduced, and every rank ends with the x1 / x2 of the single-process oracle solve (model.cpp:721-792)."""
    import torch
    assert torch.cuda.is_available()
    w = small_workload(**cfg)
    shared, results = _Shared(world), [None] * world
    th = [threading.Thread(target=_rank_main, args=(shared, r, w, results, False, (lam, fix))) for r in range(world)]
    [t.start() for t in th]
    [t.join(timeout=180) for t in th]
    assert not shared.errors, shared.errors
    o = oracle_run(oracle_mod, w, dense_A12=True)
    ox1, ox2 = oracle_mod.solve_normal_eq(o["ne"], lam, fix)
    for r in range(world):
        x1, x2 = results[r]["sol"]
        assert x1.shape == ox1.shape and x2.shape == ox2.shape
        assert np.allclose(x1, ox1, rtol=1e-7, atol=1e-9 * np.abs(ox1).max()), f"rank {r} x1"
        assert np.allclose(x2, ox2, rtol=1e-7, atol=1e-9 * np.abs(ox2).max()), f"rank {r} x2"


@pytest.mark.parametrize("cfg,world,lam,fix,lam2", [
    (dict(n_events=20000), 2, 1e-3, True, 1e-2),
    (dict(n_events=40000, pano_h=256, K=21, sensor=(64, 48), focal=60.0, dt_knots=0.01), 3, 1e-2, False, 1e-1),
])
def test_sharded_resolve_keeps_the_records_and_sharded_cg(oracle_mod, cfg, world, lam, fix, lam2):
    """Round 6.  (i) solver.cpp:340-352 solves the SAME equations again with a larger lambda after every rejected trial: the second solve
    must find the received records still on their owners (no count / pack / all-to-all: last_solve_exchanged False) and give the oracle's solution for
    the new lambda.  (ii) LEGM::solveNormalEqCG (model.cpp:794-840) over the ranks — pixels sharded by owner, one small all-reduce per application of the
    matrix — against the oracle's restatement of Eigen's loop: same stopping behaviour at the reference's settings, same iterate after ten iterations."""
    import torch
    assert torch.cuda.is_available()
    w = small_workload(**cfg)
    shared, results = _Shared(world), [None] * world
    th = [threading.Thread(target=_rank_main, args=(shared, r, w, results, False, (lam, fix, lam2))) for r in range(world)]
    [t.start() for t in th]
    [t.join(timeout=240) for t in th]
    assert not shared.errors, shared.errors
    o = oracle_run(oracle_mod, w, dense_A12=True)
    ox1, ox2 = oracle_mod.solve_normal_eq(o["ne"], lam2, fix)
    orc = o["oracle"]
    c1, c2, cit, cerr = orc.solve_cg_sparse(o["ne"], o["ep"], w.K, o["num_ev_map"], w.thres_valid_pixel, 0, 0.0, lam, fix)
    k1, k2, kit, _ = orc.solve_cg_sparse(o["ne"], o["ep"], w.K, o["num_ev_map"], w.thres_valid_pixel, 0, 0.0, lam, fix, max_iter=10, tol=1e-30)
    for r in range(world):
        R = results[r]
        assert R["exchanged_first"] is True and R["exchanged_resolve"] is False and R["exchanged_cg"] is False, (R["exchanged_first"], R["exchanged_resolve"], R["exchanged_cg"])
        x1, x2 = R["resolve"]
        assert np.allclose(x1, ox1, rtol=1e-7, atol=1e-9 * np.abs(ox1).max()), f"rank {r}: x1 of the re-solve"
        assert np.allclose(x2, ox2, rtol=1e-7, atol=1e-9 * np.abs(ox2).max()), f"rank {r}: x2 of the re-solve"
        g1, g2, git, gerr = R["cg"]
        assert abs(git - cit) <= 2 and git < 100 and gerr < 1e-6 and cerr < 1e-6, (git, cit, gerr)
        assert np.abs(g1 - c1).max() <= 1e-4 * np.abs(c1).max() and np.abs(g2 - c2).max() <= 1e-4 * np.abs(c2).max()
        h1, h2, hit, _ = R["cg10"]
        assert hit == kit == 10
        assert np.abs(h1 - k1).max() <= 1e-8 * np.abs(k1).max() and np.abs(h2 - k2).max() <= 1e-8 * np.abs(k2).max()
        if fix:
            assert (g1[:3] == 0).all()
        if r:      # every rank holds the SAME vectors (the replicated pose part must not drift)
            assert np.array_equal(R["cg"][0], results[0]["cg"][0]) and np.array_equal(R["cg"][1], results[0]["cg"][1])


def _lm_rank_main(shared, rank, w, init, ba, lm, results):
    try:
        import torch
        from emba_amd import LEGM
        from emba_amd.sharded import HipEngine, ShardedLEGM, ShardedModel
        from emba_amd.solver import solve_time_window
        dev = torch.device("cuda", 0)
        npix = w.pano_h * w.pano_w
        m = LEGM(w.sensor_w, w.sensor_h, w.lut, w.C_th, w.pano_w, w.pano_h, device=0)
        count = torch.zeros(npix, dtype=torch.int32, device=dev)
        pack = torch.zeros(9 * w.K * w.K + 3 * w.K + 5 * npix, dtype=torch.float64, device=dev)
        torch.cuda.synchronize()
        sh = ShardedLEGM(HipEngine(m, check_stream=False), _ThreadDist(shared, rank, m.sync), count, pack, w.sensor_w, None)
        model = ShardedModel(sh, m)
        r = solve_time_window(model, init, w.events, w.Gx, w.Gy, ba, lm, resident=True)
        results[rank] = dict(res=r, maps=model.downloadMap())
    except Exception as e:  # noqa: BLE001
        shared.errors.append((rank, repr(e)))
        shared.barrier.abort()
        raise


@pytest.mark.parametrize("world,ba_kw", [(2, dict(alpha=5.0)), (3, dict(use_IRLS=True, cost_type="huber", eta=0.1, alpha=1.0)), (2, dict(alpha=5.0, use_CG=True))])
def test_sharded_lm_loop_matches_oracle_loop(oracle_mod, world, ba_kw):
    """EMBA::solveTimeWindow (solver.cpp:63-353) over time shards: every rank-thread runs emba_amd.solver.solve_time_window on a
    ShardedModel (summed data cost, sharded normal equations and Schur solve, replicated map) and must take the accept / reject
    decisions of the single-process oracle loop, with the same costs, trajectory and map."""
    import torch
    assert torch.cuda.is_available()
    from emba_amd import synth
    from emba_amd.solver import BASettings, LMSettings, solve_time_window
    from helpers import OracleModel
    from test_lm_solver_cpu import perturbed
    w = synth.make_scene_workload(n_steps=1000)
    init = perturbed(w)
    ba, lm = BASettings(**ba_kw), LMSettings(max_num_iter=10)
    om = OracleModel(oracle_mod, w, use_cg=bool(ba_kw.get("use_CG")))      # (round 6: a launch file with use_CG = true on several GPUs, solver.cpp:190-202)
    ro = solve_time_window(om, init, w.events, w.Gx, w.Gy, ba, lm)
    shared, results = _Shared(world), [None] * world
    th = [threading.Thread(target=_lm_rank_main, args=(shared, r, w, init, ba, lm, results)) for r in range(world)]
    [t.start() for t in th]
    [t.join(timeout=300) for t in th]
    assert not shared.errors, shared.errors
    # (CG stops at a relative residual of 1e-6, model.cpp:823-824: every LM step's iterate is only that well defined, and so are the costs behind it)
    # (the same bounds as the C++ hosts' CG cases, tests/test_cpp_host.py: the differences compound over the loop's iterations)
    tol = 1e-2 if ba_kw.get("use_CG") else 1e-7
    for r in range(world):
        rg = results[r]["res"]
        assert [e[4] for e in rg.log] == [e[4] for e in ro.log], f"rank {r}: accept/reject sequence differs"
        assert rg.iterations == ro.iterations and rg.converged == ro.converged
        for g, o in zip(rg.log, ro.log):
            assert g[3] == pytest.approx(o[3], rel=tol) and g[2] == pytest.approx(o[2], rel=tol)
        assert np.abs(rg.traj.knots_xyzw - ro.traj.knots_xyzw).max() < (1e-3 if ba_kw.get("use_CG") else 1e-7)
        for d, o in zip(results[r]["maps"], om.downloadMap()):
            if ba_kw.get("use_CG"):      # (a pixel at the activity threshold may differ between two loops whose iterates agree to 1e-3: the map as a whole, like tests/test_cpp_host.py)
                assert np.abs(d).sum() == pytest.approx(np.abs(o).sum(), rel=5e-2)
            else:
                assert np.abs(d - o).max() < 1e-7 * np.abs(o).max()
        if r:      # the ranks themselves must agree exactly: same reduced scalars, same decisions, same replicated map
            assert np.array_equal(rg.traj.knots_xyzw, results[0]["res"].traj.knots_xyzw)


# ---- the node: 8 ranks, at the shard sizes of the SCALE run (8 x 1 M events) and of config 4 (town.launch: 8 x 5 M, K = 97, 640x480) --------
def _rank8_main(shared, rank, w, init, lam, damping, results):
    """One rank of eight on device 0: iteration (X1 as saturated bytes with cap = 255 // 8 = 31, X2), the sharded Schur solve (8-owner
    all-to-all), then ONE Levenberg-Marquardt trial through ShardedModel (updateTraj on the host, updateMap on every replica, evaluation
    of the trial point, summed cost)."""
    try:
        import torch
        from emba_amd import LEGM, io as emba_io
        from emba_amd.sharded import HipEngine, ShardedLEGM, ShardedModel
        dev = torch.device("cuda", 0)
        npix = w.pano_h * w.pano_w
        m = LEGM(w.sensor_w, w.sensor_h, w.lut, w.C_th, w.pano_w, w.pano_h, device=0)
        m.set_option("poison", 1)      # (round 6) new workspace memory reads as NaN: nothing of this protocol may depend on what an allocation happens to hold
        count = torch.zeros(npix, dtype=torch.int32, device=dev)
        pack = torch.zeros(9 * w.K * w.K + 3 * w.K + 5 * npix, dtype=torch.float64, device=dev)
        cu8 = torch.zeros(npix, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        sh = ShardedLEGM(HipEngine(m, check_stream=False), _ThreadDist(shared, rank, m.sync), count, pack, w.sensor_w, cu8)
        model = ShardedModel(sh, m)
        model.set_events(w.events)
        model.upload_map(w.Gx, w.Gy)
        n_inl, ne = sh.iteration(init, w.thres_valid_pixel, w.alpha, download=True)
        # (the trial evaluation below starts a new count map)  Round 5: where the ranks form as resident steps the GLOBAL saturated counts stay in the byte
        # buffer of exchange 1 — the int32 map keeps the rank's own counts
        count_h = (cu8 if getattr(sh, "last_form_resident", False) else count).cpu().numpy().astype(np.int32)
        cost0 = model.dataCost() + model.regCost(w.alpha)
        x1, x2 = sh.solveNormalEq(lam, True)
        traj_new = emba_io.incremental_update(init, x1, True)
        model.updateMap(x2, damping)
        model.eval_launch(traj_new)
        model.eval_finish()
        cost1 = model.dataCost() + model.regCost(w.alpha)
        results[rank] = dict(ne=ne, count=count_h, n_inl=n_inl, x1=x1, x2=x2, cost0=cost0, cost1=cost1, setup=m.setup_info())
        m.close()
    except Exception as e:  # noqa: BLE001
        shared.errors.append((rank, repr(e)))
        shared.barrier.abort()
        raise


@pytest.mark.parametrize("name,n_total,sensor,pano_h,K,yaw", [
    ("SCALE workload: 8 x 1 M events", 8_000_000, (240, 180), 1024, 21, 0.5),
    ("town.launch shape: 8 x 5 M events", 40_000_000, (640, 480), 1024, 97, 0.1),
    ("synthetic 100 M: 8 x 12.5 M events, K = 256, 2048 x 4096", 100_000_000, (240, 180), 2048, 256, 0.5),      # config 5 as a whole protocol (round 4)
])
def test_eight_ranks_at_full_shard_size(oracle_mod, name, n_total, sensor, pano_h, K, yaw):
    """world = 8 through emba_amd.sharded with the real engine (eight contexts on one MI355X, the collectives through the thread stand-in):
    count map activity, active set, normal-equation blocks, the sharded solve and one LM decision against the single-process oracle."""
    import torch
    assert torch.cuda.is_available()
    from emba_amd import io as emba_io
    from emba_amd.synth import make_workload
    from helpers import OracleModel
    from test_lm_solver_cpu import perturbed
    O = oracle_mod
    world, lam, damping = 8, 1e-3, 1.0
    w = make_workload(n_events=n_total, pano_h=pano_h, K=K, sensor=sensor, focal=200.0 * sensor[0] / 240, yaw_rate=yaw)
    init = perturbed(w, 0.002)
    shared, results = _Shared(world), [None] * world
    th = [threading.Thread(target=_rank8_main, args=(shared, r, w, init, lam, damping, results)) for r in range(world)]
    [t.start() for t in th]
    [t.join(timeout=900) for t in th]
    assert not shared.errors, shared.errors
    O.set_threads(min(O.max_threads(), 16))     # (omp mode == ref mode: tests/test_oracle_pinned.py)
    try:
        om = OracleModel(O, w, sparse=True)
        om.set_events(w.events)
        ep_o = om.evaluateDataError(init, w.Gx, w.Gy)
        cost0 = om.dataCost() + om.regCost(w.alpha)
        nem0 = om.nem.copy()
        om.formNormalEq(ep_o, w.K, None, w.thres_valid_pixel)
        om.applyL2Reg(w.alpha)
        ne_o = {k: (v.copy() if hasattr(v, "copy") else v) for k, v in om.ne.items()}
        ox1, ox2 = om.solveNormalEq(lam, True)
        om.updateMap(ox2, damping)
        om.evaluateDataError(emba_io.incremental_update(init, ox1, True), None, None)
        cost1 = om.dataCost() + om.regCost(w.alpha)
    finally:
        O.set_threads(1)
    cap = 255 // world
    assert sum(results[r]["n_inl"] for r in range(world)) == ep_o.size
    for r in range(world):
        got = results[r]["count"].reshape(w.pano_h, w.pano_w)
        assert np.array_equal(got >= w.thres_valid_pixel, nem0 >= w.thres_valid_pixel), f"{name}: rank {r} activity"      # X1: saturated bytes
        assert np.array_equal(got[nem0 < cap], nem0[nem0 < cap])                                                            # exact below the per-rank cap
        ne = results[r]["ne"]
        assert ne["P"] == ne_o["P"] and np.array_equal(ne["active"], ne_o["active"]), f"{name}: rank {r} active set"
        for k in ("A11", "b1", "A22", "b2"):
            assert_close(ne[k], ne_o[k], f"rank{r} {k}")
        assert np.allclose(results[r]["x1"], ox1, rtol=1e-6, atol=1e-8 * np.abs(ox1).max()), f"rank {r} x1"
        assert np.allclose(results[r]["x2"], ox2, rtol=1e-6, atol=1e-8 * np.abs(ox2).max()), f"rank {r} x2"
        assert results[r]["cost0"] == pytest.approx(cost0, rel=1e-9) and results[r]["cost1"] == pytest.approx(cost1, rel=1e-7)
        assert (results[r]["cost1"] < results[r]["cost0"]) == (cost1 < cost0), "LM decision differs"
    assert all(np.array_equal(results[0]["x1"], results[r]["x1"]) for r in range(1, world)), "the replicated solve must be identical on every rank"


def test_group_of_eight_on_one_device_step_rate(oracle_mod):
    """emba_group_* with eight ranks on ONE device (devices = {0 x 8}): the SCALE workload (8 x 1 M events) through the
    single-process host — rank threads issue the launches side by side, P is taken once, the exchanges go through the in-library copies —
    must give the oracle's inlier count and active set size, and a group step must stay within 2 x (measured: 1.35 x) eight single-context steps of one shard
    (the GPU work of eight ranks on one device is serial; what comes on top is the in-library exchange — 2 x 14 cross-stream event edges per
    step, which distinct devices replace by RCCL — and the two host waits of a step: P for the size of exchange 2, and its end)."""
    import ctypes as C
    import time
    import torch
    assert torch.cuda.is_available()
    from emba_amd import LEGM, _lib
    from emba_amd.sharded import shard_events
    from emba_amd.synth import make_workload
    L = _lib.load()
    world = 8
    w = make_workload(n_events=8_000_000, pano_h=1024, K=21)
    lut = np.ascontiguousarray(w.lut, dtype=np.float64)
    cfg = _lib.EmbaCfg(w.sensor_w, w.sensor_h, w.pano_w, w.pano_h, lut.ctypes.data_as(_lib._dp), float(w.C_th), 100, 10.0, 0, None)
    g = C.c_void_p()
    dev = (C.c_int32 * world)(*([0] * world))
    assert L.emba_group_create(C.byref(cfg), dev, world, C.byref(g)) == 0, L.emba_group_last_error(None)
    try:
        ev = w.events
        x = np.ascontiguousarray(ev.x, np.uint16); y = np.ascontiguousarray(ev.y, np.uint16); pol = np.ascontiguousarray(ev.polarity, np.uint8)
        t = np.ascontiguousarray(ev.t_ns, np.int64)
        assert L.emba_group_set_events(g, x.ctypes.data_as(_lib._u16p), y.ctypes.data_as(_lib._u16p), pol.ctypes.data_as(_lib._u8p), t.ctypes.data_as(_lib._i64p), x.size) == 0
        Gx = np.ascontiguousarray(w.Gx); Gy = np.ascontiguousarray(w.Gy)
        assert L.emba_group_upload_map(g, Gx.ctypes.data_as(_lib._dp), Gy.ctypes.data_as(_lib._dp)) == 0
        knots = np.ascontiguousarray(w.traj.knots_xyzw, np.float64)
        n_inl, P = C.c_size_t(0), C.c_size_t(0)

        def gstep():
            st = L.emba_group_step(g, knots.ctypes.data_as(_lib._dp), w.K, int(w.traj.t0_ns), int(w.traj.dt_ns), w.thres_valid_pixel, 0, 0.0, w.alpha, C.byref(n_inl), C.byref(P))
            assert st == 0, L.emba_group_last_error(g)
        for _ in range(5):
            gstep()
        t_group = float("inf")
        for _ in range(3):          # (best of three blocks: the eight rank threads share the box's CPU share with whatever else runs there)
            t0 = time.perf_counter()
            for _ in range(10):
                gstep()
            t_group = min(t_group, (time.perf_counter() - t0) / 10)
    finally:
        L.emba_group_destroy(g)
    # eight single-context steps of one shard (rank 3's: 1 M events + halo)
    local, halo = shard_events(w.events, w.sensor_w, 3, world)
    m = LEGM(w.sensor_w, w.sensor_h, w.lut, w.C_th, w.pano_w, w.pano_h, device=0)
    m.set_events(local, halo); m.upload_map(w.Gx, w.Gy)
    for _ in range(5):
        m.step(w.traj, w.thres_valid_pixel, w.alpha)
    t_single = float("inf")
    for _ in range(3):
        t0 = time.perf_counter()
        for _ in range(20):
            m.step(w.traj, w.thres_valid_pixel, w.alpha)
        t_single = min(t_single, (time.perf_counter() - t0) / 20)
    m.close()
    o = oracle_mod.OracleLEGM(w.sensor_w, w.sensor_h, w.pano_w, w.pano_h, w.lut, w.C_th)
    oracle_mod.set_threads(min(oracle_mod.max_threads(), 16))
    try:
        ep_o, nem_o = o.evaluate_data_error(w.traj.knots_xyzw, w.traj.t0_ns, w.traj.dt_ns, w.Gx, w.Gy, ev.x, ev.y, ev.polarity, ev.t_ns)
    finally:
        oracle_mod.set_threads(1)
    assert n_inl.value == ep_o.size and P.value == int((nem_o >= w.thres_valid_pixel).sum())
    print(f"group step {t_group * 1e6:.0f} us  vs  8 x single-context shard step {8 * t_single * 1e6:.0f} us  (ratio {t_group / (8 * t_single):.2f})")
    # measured 1.35; the bound leaves room for a loaded host — the rate is a report, the counts above are the test
    assert t_group <= 2.0 * 8 * t_single, (t_group, t_single)


@pytest.mark.gpu
def test_group_ep_is_merged_pixel_block_by_pixel_block(oracle_mod):
    """emba_group_eval / emba_group_get_ep on several ranks (round 6): every rank's residuals are placed in the ONE output vector by sensor-pixel runs
    (emba_get_inlier_pixel_starts, emba_get_ep_by_pixel) from the ranks' own threads — the result must be the oracle's ep, element for element in its order
    (model.cpp:179-186, 221, 256), and the count map the all-reduced one.  Also the two entry points on a single context: the starts are the running counts of
    emba_get_inlier_pixels, and the identity placement reproduces emba_get_ep."""
    import ctypes as C
    import torch
    assert torch.cuda.is_available()
    from emba_amd import LEGM, _lib
    from emba_amd.synth import make_workload
    L = _lib.load()
    w = make_workload(n_events=600_000, pano_h=512, K=21)
    ev = w.events
    o = oracle_mod.OracleLEGM(w.sensor_w, w.sensor_h, w.pano_w, w.pano_h, w.lut, w.C_th)
    ep_o, nem_o = o.evaluate_data_error(w.traj.knots_xyzw, w.traj.t0_ns, w.traj.dt_ns, w.Gx, w.Gy, ev.x, ev.y, ev.polarity, ev.t_ns)
    lut = np.ascontiguousarray(w.lut, dtype=np.float64)
    knots = np.ascontiguousarray(w.traj.knots_xyzw, np.float64)
    x = np.ascontiguousarray(ev.x, np.uint16); y = np.ascontiguousarray(ev.y, np.uint16); pol = np.ascontiguousarray(ev.polarity, np.uint8)
    t = np.ascontiguousarray(ev.t_ns, np.int64)
    Gx = np.ascontiguousarray(w.Gx); Gy = np.ascontiguousarray(w.Gy)
    for world in (3, 1):
        cfg = _lib.EmbaCfg(w.sensor_w, w.sensor_h, w.pano_w, w.pano_h, lut.ctypes.data_as(_lib._dp), float(w.C_th), 100, 10.0, 0, None)
        g = C.c_void_p()
        dev = (C.c_int32 * world)(*([0] * world))
        assert L.emba_group_create(C.byref(cfg), dev, world, C.byref(g)) == 0, L.emba_group_last_error(None)
        try:
            assert L.emba_group_set_events(g, x.ctypes.data_as(_lib._u16p), y.ctypes.data_as(_lib._u16p), pol.ctypes.data_as(_lib._u8p), t.ctypes.data_as(_lib._i64p), x.size) == 0
            ep = np.full(x.size, np.nan); nem = np.zeros((w.pano_h, w.pano_w), np.int32); n_inl = C.c_size_t(0)
            st = L.emba_group_eval(g, knots.ctypes.data_as(_lib._dp), w.K, int(w.traj.t0_ns), int(w.traj.dt_ns), Gx.ctypes.data_as(_lib._dp), Gy.ctypes.data_as(_lib._dp),
                                   ep.ctypes.data_as(_lib._dp), C.byref(n_inl), nem.ctypes.data_as(_lib._i32p))
            assert st == 0, L.emba_group_last_error(g)
            assert n_inl.value == ep_o.size and np.array_equal(nem, nem_o)
            assert_close(ep[: n_inl.value], ep_o, f"group ep, {world} ranks")
            assert np.isnan(ep[n_inl.value:]).all()
            # ... and fetched again on its own (the adapter's order: count first, then the vector it returns)
            ep2 = np.full(n_inl.value, np.nan); n2 = C.c_size_t(0)
            assert L.emba_group_get_ep(g, ep2.ctypes.data_as(_lib._dp), ep2.size, C.byref(n2)) == 0, L.emba_group_last_error(g)
            assert n2.value == n_inl.value and np.array_equal(ep2, ep[: n_inl.value])
        finally:
            L.emba_group_destroy(g)
    m = LEGM(w.sensor_w, w.sensor_h, w.lut, w.C_th, w.pano_w, w.pano_h, device=0)
    try:
        m.set_events(w.events); m.upload_map(w.Gx, w.Gy)
        m.eval_launch(w.traj); n, ep, _ = m.eval_finish(want_ep=True)
        S = w.sensor_w * w.sensor_h
        px = np.zeros(n, np.uint32); starts = np.zeros(S + 1, np.uint32)
        assert L.emba_get_inlier_pixels(m._ctx, px.ctypes.data_as(_lib._u32p)) == 0
        assert L.emba_get_inlier_pixel_starts(m._ctx, starts.ctypes.data_as(_lib._u32p)) == 0
        assert np.array_equal(starts, np.concatenate([[0], np.cumsum(np.bincount(px, minlength=S))]).astype(np.uint32))
        out = np.full(n, np.nan); dst = starts[:S].astype(np.uint64)
        assert L.emba_get_ep_by_pixel(m._ctx, out.ctypes.data_as(_lib._dp), dst.ctypes.data_as(C.POINTER(C.c_uint64))) == 0
        assert np.array_equal(out, ep)
        # a new evaluation of the same point: the placement finds the kept starts stale and takes them again by itself
        m.eval_launch(w.traj); m.eval_finish(sync=False)
        out2 = np.full(n, np.nan)
        assert L.emba_get_ep_by_pixel(m._ctx, out2.ctypes.data_as(_lib._dp), dst.ctypes.data_as(C.POINTER(C.c_uint64))) == 0
        assert np.array_equal(out2, ep)
    finally:
        m.close()


@pytest.mark.gpu
def test_ep_by_pixel_takes_no_pixel_starts_across_a_rejected_trial(oracle_mod):
    """emba_get_ep_by_pixel places the residuals with the pixel starts the context kept from emba_get_inlier_pixel_starts.  That table belongs to
    ONE evaluation: a rejected trial ends the evaluation (EMBA_ERR_STATE until the next one), and the next evaluation takes its own starts even when
    nobody fetched them first.  The two trajectories are chosen so that a table kept across the rejection would go unnoticed by every size check:
    the same number of inliers (13793, on plateaus of the yaw rate four search steps of 2e-4 wide), but other runs per sensor pixel — asserted
    below on the oracle."""
    import ctypes as C
    from emba_amd import LEGM, _lib
    from emba_amd.synth import make_trajectory
    L = _lib.load()
    w = small_workload(n_events=20000)
    ev = w.events
    S = w.sensor_w * w.sensor_h
    traj_a, traj_b = make_trajectory(w.K, 0.05, 0.1, 1.9976), make_trajectory(w.K, 0.05, 0.1, -1.9838)
    o = oracle_mod.OracleLEGM(w.sensor_w, w.sensor_h, w.pano_w, w.pano_h, w.lut, w.C_th)
    pix = ev.y.astype(np.int64) * w.sensor_w + ev.x

    def oracle_starts(traj):
        r = o.evaluate_data_error(traj.knots_xyzw, traj.t0_ns, traj.dt_ns, w.Gx, w.Gy, ev.x, ev.y, ev.polarity, ev.t_ns, dump=True)
        return np.concatenate([[0], np.cumsum(np.bincount(pix[r[2]["inlier_idx"] >= 0], minlength=S))]).astype(np.uint32)

    starts_a_o, starts_b_o = oracle_starts(traj_a), oracle_starts(traj_b)
    assert starts_a_o[S] == starts_b_o[S] > 0 and np.count_nonzero(starts_a_o != starts_b_o) > S // 2     # same size, other runs

    def fetch_starts():
        s = np.zeros(S + 1, np.uint32)
        assert L.emba_get_inlier_pixel_starts(m._ctx, s.ctypes.data_as(_lib._u32p)) == 0
        return s

    m = LEGM(w.sensor_w, w.sensor_h, w.lut, w.C_th, w.pano_w, w.pano_h, device=0)
    try:
        m.set_events(ev); m.upload_map(w.Gx, w.Gy)
        m.eval_launch(traj_a); m.eval_finish(sync=False)
        assert np.array_equal(fetch_starts(), starts_a_o)              # 1. the table of A is kept
        m.form_active(w.thres_valid_pixel); m.form_accumulate(); m.form_finish(w.alpha)      # 2.
        m.eval_launch(traj_b); m.eval_finish(sync=False)               # 3. a trial
        m.rejectTrial()                                                # 4.
        # the runs of B, pixel by pixel in REVERSE order: a placement that is not the identity
        runs = np.diff(starts_b_o.astype(np.int64))
        dst = np.ascontiguousarray((np.cumsum(runs[::-1])[::-1] - runs).astype(np.uint64))
        out = np.full(int(starts_b_o[S]), np.nan)
        by_pixel = lambda: L.emba_get_ep_by_pixel(m._ctx, out.ctypes.data_as(_lib._dp), dst.ctypes.data_as(C.POINTER(C.c_uint64)))
        assert by_pixel() == _lib.ERR_STATE
        assert np.isnan(out).all()
        m.eval_launch(traj_b); m.eval_finish(sync=False)               # 5. B again, and the placement without fetching the starts first
        assert by_pixel() == 0, L.emba_last_error(m._ctx)
        starts_b = fetch_starts()
        assert np.array_equal(starts_b, starts_b_o)
        ep = m.get_ep()
        want = np.full(ep.size, np.nan)
        for q in np.flatnonzero(runs):
            want[int(dst[q]): int(dst[q]) + runs[q]] = ep[starts_b[q]: starts_b[q + 1]]
        assert not np.isnan(want).any() and np.array_equal(out, want)
    finally:
        m.close()


def test_cg_session_ends_when_a_solve_takes_the_scratch():
    """A CG session (emba_cg_shard_*) keeps its vectors and record lists in the context's solve scratch.  A solve on the same context between
    emba_cg_shard_begin and the next step takes that scratch (the session's vectors could be re-allocated under it): the session has
    ended, and its next step fails with EMBA_ERR_STATE before it launches anything.  One rank on one context, called as _sharded_solve_cg does."""
    import torch
    from emba_amd import LEGM
    from emba_amd._lib import ERR_STATE, EmbaError
    w = small_workload(n_events=20000)
    m = LEGM(w.sensor_w, w.sensor_h, w.lut, w.C_th, w.pano_w, w.pano_h, device=0)
    m.set_events(w.events)
    nem = np.zeros((w.pano_h, w.pano_w), dtype=np.int32)
    ep = m.evaluateDataError(w.traj, w.Gx, w.Gy, None, True, nem)
    m.formNormalEq(ep, w.K, nem, w.thres_valid_pixel)
    m.applyL2Reg(w.alpha)
    lam = 1e-3
    m.solveNormalEq(lam)                  # (sizes the scratch: the solve below regrows nothing)
    dev = torch.device("cuda", 0)
    n_recv = int(m.solve_shard_count(1).sum())      # one rank: the records it sends to itself are the records it receives
    recv = torch.zeros(max(n_recv, 1) * 16, dtype=torch.float64, device=dev)
    red = torch.zeros(m.cg_shard_size(), dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    m.solve_shard_pack(1, recv.data_ptr())
    m.cg_shard_begin(0, 1, recv.data_ptr(), n_recv, lam, False, red.data_ptr())
    m.sync()
    m.solveNormalEq(lam)
    with pytest.raises(EmbaError) as err:
        m.cg_shard_apply(red.data_ptr())
    assert err.value.status == ERR_STATE
    m.close()
