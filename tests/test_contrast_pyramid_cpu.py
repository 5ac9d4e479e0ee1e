"""Coarse-to-fine refinement of the poses on the smooth contrast, without a GPU: the level additions of the HIP-free rule header
(emba_amd/csrc/contrast_rule.h through tests/cpp/contrast_level_rule_test.cpp, also under the address and undefined-behaviour sanitizers), the new symbol of
libemba_hip.so, the numpy form of a level (io.contrast_level) against central differences of J_l, the pyramid (io.refine_contrast_pyramid) from starts that
level 0 alone cannot leave, its argument errors, the driver under the default schedule and under a two-level one, and the sharded hosts."""
import os
import subprocess

import numpy as np
import pytest

import cmax_cases as CC
from emba_amd import io as eio
from emba_amd import so3
from emba_amd.legm import LinearTrajectory
from test_contrast_cpu import FD_SEEDS, knot_errors
from test_panorama_cpu import constant_rate_trajectory

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 512, 256
LEVELS = (3, 2, 1, 0)

# |central difference of J_l (h = 1e-6) - g_l . d| / |g_l . d| along the unit directions FD_SEEDS (those of test_contrast_cpu.py) at the half-rate
# trajectory, the worst of the five seeds per level as the numpy form itself shows it on the oracle's pm / D / cp of the constant-rate recording, measured on
# the CPU (level 1: 8.7e-6, 9.0e-10, 6.5e-11, 5.17e-5, 3.1e-9; level 2: 1.3e-11, 2.4e-11, 5.95e-10, 2.9e-10, 2.6e-10; level 3: 2.2e-10, 3.9e-10, 8.8e-10,
# 1.86e-9, 1.8e-11).  J_l is piecewise smooth like J: a direction that moves a pm_l across a cell edge inside +-h sees the kink (seeds 100 and 103 at level
# 1); the cells of a coarser level are fewer, so fewer events sit near an edge, and at levels 2 and 3 what is left is the difference quotient's rounding.
# The asserted bound is ten times the worst measured, per level; a wrong scale factor of D_l (2, 4 or 8) is a mismatch of order one.
FD_WORST_MEASURED = {1: 5.1668071043e-05, 2: 5.9456e-10, 3: 1.8563e-09}


def test_level_rule_on_the_cpu(tmp_path):
    """contrast_rule.h's level additions (plain C++17, no HIP): tests/cpp/contrast_level_rule_test.cpp checks the grid of a level, the refusals, the scaled
    vote (level 0: the bits of contrast_vote), the plan of the vote kernel at kContrastLdsCells cells exactly and one more, and the shares of the
    persistent workgroups.  Built twice: plain, and as a stand-alone program under -fsanitize=address,undefined.  The votes it prints are compared here
    with io.contrast_votes on io.contrast_level."""
    src = os.path.join(ROOT, "tests", "cpp", "contrast_level_rule_test.cpp")
    outs = []
    for name, extra in (("contrast_level_rule_test", []), ("contrast_level_rule_test_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])):
        exe = str(tmp_path / name)
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-ffp-contract=off"] + extra + [src, "-o", exe])
        r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
        print(r.stdout[-3000:], r.stderr)
        lines = r.stdout.strip().splitlines()
        assert r.returncode == 0 and lines[-1] == "OK contrast_level_rule", r.stdout[-3000:] + r.stderr
        outs.append(lines)
    assert outs[0] == outs[1]
    votes = [l for l in outs[0] if l.startswith("LVOTE ")]
    assert len(votes) == 6
    for l in votes:
        head, cells, w, dwx, dwy = l[6:].split("|")
        px, py, pw, ph, lev = head.split()
        pm_l, _, Wl, Hl = eio.contrast_level([[float(px), float(py)]], None, int(pw), int(ph), int(lev))
        assert (Wl, Hl) == (int(pw) >> int(lev), int(ph) >> int(lev))
        got = eio.contrast_votes(pm_l, Wl, Hl)
        assert got[0][0].tolist() == [int(v) for v in cells.split()], l
        for g, want in zip(got[1:], (w, dwx, dwy)):
            assert g[0].tolist() == [float(v) for v in want.split()], l


def test_contrast_level_in_numpy():
    pm = np.array([[508.0, 100.0], [3.25, 7.5]])
    D = np.arange(24.0).reshape(2, 2, 6)
    pm0, D0, W0, H0 = eio.contrast_level(pm, D, W, H, 0)
    assert np.array_equal(pm0, pm) and np.array_equal(D0, D) and (W0, H0) == (W, H)
    pm3, D3, W3, H3 = eio.contrast_level(pm, D, W, H, 3)
    assert np.array_equal(pm3, pm / 8) and np.array_equal(D3, D / 8) and (W3, H3) == (64, 32)
    assert eio.contrast_level(pm, None, W, H, 2)[1] is None
    assert eio.contrast_level(pm, D, W, H, 7)[2:] == (4, 2)
    for bad in (-1, 8, 9):                          # 8: one row left of 256
        with pytest.raises(ValueError):
            eio.contrast_level(pm, D, W, H, bad)
    with pytest.raises(ValueError, match="divisible"):
        eio.contrast_level(pm, D, 514, 256, 2)
    with pytest.raises(ValueError, match="divisible"):
        eio.contrast_level(pm, D, 512, 258, 2)
    assert eio.contrast_level(pm, D, 1 << 20, 1 << 19, eio.CONTRAST_MAX_LEVEL)[2:] == (1 << 12, 1 << 11)


def test_new_symbol_resolves(hip_lib):
    assert hasattr(hip_lib, "emba_seq_contrast_gradient_level")
    import inspect
    from emba_amd import LEGM
    from emba_amd.sharded import HipEngine, ShardedLEGM, ShardedModel
    for k in (LEGM, HipEngine, ShardedLEGM, ShardedModel):
        assert inspect.signature(k.contrast_gradient).parameters["level"].default == 0, k
    blob = open(os.path.join(ROOT, "emba_amd", "libemba_hip.so"), "rb").read()
    assert b"emba_contrast_vote_lds_kernel" in blob


@pytest.fixture(scope="module")
def recording(oracle_mod):
    """The constant-rate recording and, per level, J_l and its gradient by the numpy rule on the oracle's warp (pm, D, cp of the used events): the level is
    formed by io.contrast_level, nothing else."""
    ev, lut = CC.constant_rate_events(CC.CONST_OMEGA)
    nn = ev.size() // 100 * 100
    o = oracle_mod.OracleLEGM(64, 48, W, H, lut, 0.2)
    Z = np.zeros((H, W))

    def J_and_grad_at(level):
        def f(traj):
            d = o.evaluate_data_error(traj.knots_xyzw, traj.t0_ns, traj.dt_ns, Z, Z, ev.x, ev.y, ev.polarity, ev.t_ns, dump=True)[2]
            pm_l, D_l, Wl, Hl = eio.contrast_level(d["pm"][:nn], d["D"][:nn], W, H, level)
            r = eio.contrast_gradient(pm_l, D_l, d["cp_idx"][:nn], ev.polarity[:nn], traj.size(), Wl, Hl)
            return r["J"], r["grad"]
        return f
    return J_and_grad_at, (lambda level: (lambda traj: J_and_grad_at(level)(traj)[0]))


@pytest.mark.parametrize("level", [1, 2, 3])
def test_gradient_against_central_differences_per_level(recording, level):
    J_and_grad_at, J_only_at = recording
    JG, J_only = J_and_grad_at(level), J_only_at(level)
    t0 = constant_rate_trajectory(CC.CONST_OMEGA / 2)
    J, g = JG(t0)
    assert g.shape == (12,) and J > 0
    h, worst = 1e-6, 0.0
    for seed in FD_SEEDS:
        d = np.random.default_rng(seed).normal(size=12)
        d /= np.linalg.norm(d)
        fd = (J_only(eio.incremental_update(t0, h * d, False)) - J_only(eio.incremental_update(t0, -h * d, False))) / (2 * h)
        mis = abs(fd - g @ d) / abs(g @ d)
        print(f"level {level} seed {seed}: central difference {fd:.6f}  g . d {g @ d:.6f}  relative mismatch {mis:.3e}")
        worst = max(worst, mis)
    print(f"level {level}: worst {worst:.4e}, measured {FD_WORST_MEASURED[level]:.4e}, bound {10.0 * FD_WORST_MEASURED[level]:.4e}")
    assert worst <= 10.0 * FD_WORST_MEASURED[level]


def identity_trajectory():
    return constant_rate_trajectory(np.zeros(3))


def test_the_pyramid_does_what_level_0_cannot(recording):
    """From the identity and from 1.8 times the true rate, the schedule (3, 2, 1, 0) ends with a level-0 J above J at the true trajectory and every knot
    error relative to the first knot below half its start, the first pose held bit for bit — where level 0 alone, from the identity, stalls far below
    J at the truth (measured: 17 227.6 against 27 770.1).  That last line is what makes the first ones mean something: should a change of
    refine_contrast make level 0 converge from the identity, it fails and wants a look.  Nothing is asserted from minus half the rate: every schedule
    tried fails there."""
    J_and_grad_at, J_only_at = recording
    truth = constant_rate_trajectory(CC.CONST_OMEGA)
    J_true = J_only_at(0)(truth)
    for what, start in (("the identity", identity_trajectory()), ("1.8 x the rate", constant_rate_trajectory(1.8 * CC.CONST_OMEGA))):
        traj, hists, evals = eio.refine_contrast_pyramid(J_and_grad_at, J_only_at, start, LEVELS, pano_w=W, fix_first_pose=True, max_iter=60)
        err0, err1 = knot_errors(start, truth), knot_errors(traj, truth)
        print(f"from {what}, levels {LEVELS}: level-0 J {hists[0][0]:.1f} -> {hists[0][-1]:.1f} (truth {J_true:.1f}), {evals} evaluations; "
              f"knot errors {np.round(err0, 4).tolist()} -> {np.round(err1, 4).tolist()} rad")
        assert list(hists) == list(LEVELS) and evals >= sum(len(h) for h in hists.values())
        for h in hists.values():
            assert all(b > a for a, b in zip(h, h[1:]))      # within a level J rises strictly
        assert hists[0][-1] > J_true
        assert all(e1 < 0.5 * e0 for e0, e1 in zip(err0, err1)), (err0, err1)
        assert np.array_equal(traj.knots_xyzw[0], start.knots_xyzw[0])
    start = identity_trajectory()
    traj, hists, evals = eio.refine_contrast_pyramid(J_and_grad_at, J_only_at, start, (0,), pano_w=W, fix_first_pose=True, max_iter=60)
    print(f"from the identity, level 0 alone: J {hists[0][0]:.1f} -> {hists[0][-1]:.1f} (truth {J_true:.1f}), {evals} evaluations; "
          f"knot errors -> {np.round(knot_errors(traj, truth), 4).tolist()} rad")
    assert hists[0][-1] < J_true
    # (0,) is refine_contrast itself, call for call
    t1, h1, n1 = eio.refine_contrast(J_and_grad_at(0), J_only_at(0), start, fix_first_pose=True, max_iter=60, pano_w=W)
    assert np.array_equal(t1.knots_xyzw, traj.knots_xyzw) and h1 == hists[0] and n1 == evals


def test_pyramid_arguments():
    t = identity_trajectory()
    flat = lambda level: (lambda tr: (1.0, np.zeros(12)))      # noqa: E731
    flat_J = lambda level: (lambda tr: 1.0)                    # noqa: E731
    with pytest.raises(TypeError):
        eio.refine_contrast_pyramid(flat, flat_J, t, (1, 0))                # no panorama width
    with pytest.raises(ValueError, match="end at level 0"):
        eio.refine_contrast_pyramid(flat, flat_J, t, (3, 2, 1), pano_w=W)
    with pytest.raises(ValueError, match="end at level 0"):
        eio.refine_contrast_pyramid(flat, flat_J, t, (), pano_w=W)
    with pytest.raises(ValueError, match="strictly decreasing"):
        eio.refine_contrast_pyramid(flat, flat_J, t, (2, 2, 0), pano_w=W)
    with pytest.raises(ValueError, match="strictly decreasing"):
        eio.refine_contrast_pyramid(flat, flat_J, t, (1, 2, 0), pano_w=W)
    with pytest.raises(ValueError, match="strictly decreasing"):
        eio.refine_contrast_pyramid(flat, flat_J, t, (0, 0), pano_w=W)
    with pytest.raises(ValueError, match="not divisible"):
        eio.refine_contrast_pyramid(flat, flat_J, t, (3, 0), pano_w=516)    # 516 = 4 x 129
    with pytest.raises(ValueError, match="levels are"):
        eio.refine_contrast_pyramid(flat, flat_J, t, (9, 0), pano_w=1 << 12)
    # a flat contrast: every level hands the trajectory on as it got it, one evaluation each; the first step is in the level's own cells
    widths = []
    real = eio.refine_contrast

    def spy(JG, J_only, traj, **kw):
        widths.append(kw["pano_w"])
        return real(JG, J_only, traj, **kw)
    eio.refine_contrast = spy
    try:
        traj, hists, evals = eio.refine_contrast_pyramid(flat, flat_J, t, (2, 1, 0), pano_w=W, max_iter=5)
    finally:
        eio.refine_contrast = real
    assert traj is t and hists == {2: [1.0], 1: [1.0], 0: [1.0]} and evals == 3 and widths == [W >> 2, W >> 1, W]
    from emba_amd.driver import SequenceSettings
    s = SequenceSettings(time_window_size=0.15, sliding_window_stride=0.1)
    assert s.contrast_levels == (0,)
    assert SequenceSettings(0.15, 0.1, contrast_levels=[3, 2, 1, 0]).contrast_levels == (3, 2, 1, 0)
    for bad in ((1,), (0, 1), (2, 2, 0), ()):
        with pytest.raises(ValueError):
            SequenceSettings(0.15, 0.1, contrast_levels=bad)


class LevelModel:
    """A stand-in for LEGM with the sequence resident: a smooth bump around `target` for every control pose, the same at every level, and a record of the
    calls."""
    W, H = W, H
    target = so3.exp(np.array([0.02, -0.05, 0.01]))

    def __init__(self):
        self.calls = []

    def bind_exchange(self, count, pack):
        pass

    def _answer(self, traj, want_grad):
        w = np.array([so3.log(so3.mul(self.target, so3.inverse(q))) for q in traj.knots_xyzw])
        e = np.exp(-50.0 * (w * w).sum(axis=1))
        return dict(J=float(e.sum()), grad=(100.0 * w * e[:, None]).reshape(-1) if want_grad else None)

    def contrast_gradient(self, traj, beg=0, end=None, signed=False, want_grad=True, want_image=False, want_pm=False, want_D=False, level=0):
        self.calls.append((beg, end, want_grad, level))
        return self._answer(traj, want_grad)


# What refine_window_poses(model, start, 10, 990, True, 20) and ShardedLEGM.refine_contrast(start, 10, 990, W, True, 20) asked this stand-in, and what both
# returned, at the commit before the level-free branches went (recorded there, with no level argument in any call).  G: J and gradient, J: J alone.
PARENT_CALLS = "GJGJGJJJGJJJJJJGJJJGJJJJG"
PARENT_KNOTS = [[0.0, 0.0, 0.0, 1.0],
                [0.010007971225612203, -0.02501992806403051, 0.005003985612806102, 0.9996243313563377],
                [0.010007971225612203, -0.02501992806403051, 0.005003985612806102, 0.9996243313563377]]
PARENT_J = (2.5821239292751734, 2.860707721143072)


def test_the_default_schedule_makes_the_calls_it_made():
    """Under contrast_levels = (0,) driver.refine_window_poses and ShardedLEGM.refine_contrast ask the model what they asked before (0,) ran through
    io.refine_contrast_levels — the same ranges and want_grad in the same order, now at level 0 — and return the same tuple: the recorded one, and bit
    for bit what io.refine_contrast over contrast_gradient gives here.  With two levels: the level-0 J before, then level 1, then level 0; evaluations
    over both."""
    from types import SimpleNamespace
    from emba_amd.driver import SequenceSettings, refine_window_poses
    from emba_amd.sharded import ShardedLEGM
    start = LinearTrajectory(np.tile([0.0, 0.0, 0.0, 1.0], (3, 1)), 0, 50_000_000)
    ref = LevelModel()
    t_ref, hist, n_ref = eio.refine_contrast(lambda t: (lambda r: (r["J"], r["grad"]))(ref.contrast_gradient(t, 10, 990)),
                                             lambda t: ref.contrast_gradient(t, 10, 990, want_grad=False)["J"], start, fix_first_pose=True, max_iter=20, pano_w=W)
    one_rank = SimpleNamespace(get_rank=lambda: 0, get_world_size=lambda: 1)
    for run in (lambda m: refine_window_poses(m, start, 10, 990, True, 20, SequenceSettings(0.15, 0.1).contrast_levels),
                lambda m: refine_window_poses(m, start, 10, 990, True, 20),      # (the argument's default)
                lambda m: ShardedLEGM(m, one_rank, None, None, 64).refine_contrast(start, 10, 990, W, True, 20, (0,))):
        m = LevelModel()
        traj, J0, J1, evals = run(m)
        assert m.calls == [(10, 990, ch == "G", 0) for ch in PARENT_CALLS] and evals == len(PARENT_CALLS) == n_ref
        assert np.array_equal(traj.knots_xyzw, t_ref.knots_xyzw) and (J0, J1) == (hist[0], hist[-1]) and (traj.t0_ns, traj.dt_ns) == (0, 50_000_000)
        assert np.allclose(traj.knots_xyzw, PARENT_KNOTS, rtol=0, atol=1e-13) and (J0, J1) == pytest.approx(PARENT_J, rel=1e-13)
    m = LevelModel()
    traj2, K0, K1, evals2 = refine_window_poses(m, start, 10, 990, True, 20, (1, 0))
    levels = [c[3] for c in m.calls]
    assert len(m.calls) == evals2 and m.calls[0] == (10, 990, False, 0) and levels[1] == 1
    first0 = levels.index(0, 1)
    assert set(levels[1:first0]) == {1} and set(levels[first0:]) == {0} and first0 > 2
    assert K0 == hist[0] and K1 > K0 and np.array_equal(traj2.knots_xyzw[0], start.knots_xyzw[0])


def test_every_rank_gets_rank_0s_pyramid():
    """Two stand-in ranks whose contexts answer one unit in the last place apart: after a two-level pyramid through driver.refine_window_poses every rank
    holds rank 0's trajectory, J and evaluation count bit for bit, rank 1's context was never asked, and the level reached the engine."""
    import threading
    from types import SimpleNamespace
    from emba_amd.driver import refine_window_poses
    from emba_amd.sharded import ShardedLEGM, ShardedModel

    class Engine(LevelModel):
        def __init__(self, rank):
            super().__init__()
            self.scale = 1.0 + rank * 2.0 ** -52

        def bind_exchange(self, count, pack):
            pass

        def _answer(self, traj, want_grad):
            r = super()._answer(traj, want_grad)
            return dict(J=self.scale * r["J"], grad=None if r["grad"] is None else self.scale * r["grad"])

    class Dist:
        def __init__(self, rank, shared):
            self.rank, self.shared = rank, shared

        def get_rank(self):
            return self.rank

        def get_world_size(self):
            return 2

        def all_reduce(self, t):
            sh = self.shared
            with sh.lock:
                sh.acc = t.clone() if sh.acc is None else sh.acc + t
                sh.reduces += 1
            sh.barrier.wait()
            t.copy_(sh.acc)
            if sh.barrier.wait() == 0:
                sh.acc = None
            sh.barrier.wait()
    start = LinearTrajectory(np.tile([0.0, 0.0, 0.0, 1.0], (3, 1)), 0, 50_000_000)
    alone = eio.refine_contrast_levels(Engine(0), start, 0, 1000, (1, 0), pano_w=W, max_iter=20)
    shared = SimpleNamespace(lock=threading.Lock(), barrier=threading.Barrier(2), acc=None, reduces=0)
    engines, results = [Engine(0), Engine(1)], [None, None]

    def rank_main(r):
        host = ShardedModel(ShardedLEGM(engines[r], Dist(r, shared), None, None, 64), SimpleNamespace(H=H, W=W))
        results[r] = refine_window_poses(host, start, 0, 1000, True, 20, (1, 0))
    threads = [threading.Thread(target=rank_main, args=(r,)) for r in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=60)
    assert all(r is not None for r in results)
    (t0, a0, b0, n0), (t1, a1, b1, n1) = results
    assert np.array_equal(t0.knots_xyzw, t1.knots_xyzw) and (a0, b0, n0) == (a1, b1, n1)
    assert np.array_equal(t0.knots_xyzw, alone[0].knots_xyzw) and (a0, b0, n0) == alone[1:]
    assert b0 > a0 and engines[1].calls == [] and {c[3] for c in engines[0].calls} == {0, 1} and shared.reduces == 2      # one all-reduce per rank


def test_sharded_hosts_forward_the_level():
    """ShardedModel -> ShardedLEGM -> HipEngine -> the rank's model: a level arrives as it was given, level 0 like any other."""
    from types import SimpleNamespace
    from emba_amd.sharded import HipEngine, ShardedLEGM, ShardedModel
    calls = []

    class Device:
        def bind_exchange(self, count, pack):
            pass

        def contrast_gradient(self, *a, **kw):
            calls.append((a, kw))
            return dict(J=7.0)
    dist = SimpleNamespace(get_rank=lambda: 0, get_world_size=lambda: 2)
    host = ShardedModel(ShardedLEGM(Device(), dist, None, None, 64), SimpleNamespace(H=4, W=8))
    assert host.contrast_gradient("traj", 3, 900, True, False, True, True, True, level=2) == dict(J=7.0)
    assert calls[-1] == (("traj", 3, 900, True, False, True, True, True), dict(level=2))
    host.contrast_gradient("traj", 3, 900)
    assert calls[-1] == (("traj", 3, 900, False, True, False, False, False), dict(level=0))
    eng = HipEngine.__new__(HipEngine)
    eng.m = Device()
    eng.contrast_gradient("traj", 1, 2, level=3)
    assert calls[-1] == (("traj", 1, 2, False, True, False, False, False), dict(level=3))
