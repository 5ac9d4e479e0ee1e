"""The smooth contrast of the panorama of warped events and its gradient without a GPU: the HIP-free rule header (emba_amd/csrc/contrast_rule.h through
tests/cpp/contrast_rule_test.cpp, also under the address and undefined-behaviour sanitizers), the new symbol of libemba_hip.so, the numpy form of the rule
(emba_amd.io: contrast_votes, contrast_gradient) against a plain loop and against central differences of J, and the conjugate-gradient ascent
(io.refine_contrast) on a recording whose motion is known, with pm / D / cp from the oracle's dump.  The values: DESIGN.md §13."""
import os
import subprocess

import numpy as np
import pytest

import cmax_cases as CC
from emba_amd import io as eio
from emba_amd import so3
from emba_amd.legm import LinearTrajectory
from test_panorama_cpu import constant_rate_trajectory

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 512, 256

# |central difference of J (h = 1e-6) - g . d| / |g . d| along the unit directions FD_SEEDS at the half-rate trajectory, the worst of the five as the numpy
# form itself shows it on the oracle's pm / D / cp of the constant-rate recording (measured on the CPU: 1.1e-4, 7.6e-10, 1.5e-11, 4.07e-3, 8.2e-10).  J is
# only piecewise smooth: a direction that moves a pm across a cell edge inside +-h sees the kink (seed 103 here), the others agree to the difference
# quotient's rounding.  The asserted bound is ten times the worst: the margin covers a seed landing nearer an edge; a wrong sign, a wrong control pose or a
# missing factor is a mismatch of order one.
FD_SEEDS = (100, 101, 102, 103, 104)
FD_WORST_MEASURED = 4.0743862914e-3
FD_BOUND = 10.0 * FD_WORST_MEASURED


def test_contrast_rule_on_the_cpu(tmp_path):
    """emba_amd/csrc/contrast_rule.h (plain C++17, no HIP): tests/cpp/contrast_rule_test.cpp checks contrast_vote — weights that sum to 1, derivatives that
    sum to 0 and equal a difference quotient, the wrap at column 0, the pole rows, an exact integer, NaN / inf — contrast_event_grad, the argument checks
    without the integer image's limit, and the span plan of the gradient kernel.  Built twice: plain, and as a stand-alone program under
    -fsanitize=address,undefined.  The votes it prints are compared here with io.contrast_votes."""
    src = os.path.join(ROOT, "tests", "cpp", "contrast_rule_test.cpp")
    outs = []
    for name, extra in (("contrast_rule_test", []), ("contrast_rule_test_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])):
        exe = str(tmp_path / name)
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-ffp-contract=off"] + extra + [src, "-o", exe])
        r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
        print(r.stdout[-3000:], r.stderr)
        lines = r.stdout.strip().splitlines()
        assert r.returncode == 0 and lines[-1] == "OK contrast_rule", r.stdout[-3000:] + r.stderr
        outs.append(lines)
    assert outs[0] == outs[1]
    votes = [l for l in outs[0] if l.startswith("VOTE ")]
    assert len(votes) == 8
    for l in votes:
        head, cells, w, dwx, dwy = l[5:].split("|")
        px, py, pw, ph = head.split()
        got = eio.contrast_votes([[float(px), float(py)]], int(pw), int(ph))
        assert got[0][0].tolist() == [int(v) for v in cells.split()], l
        for g, want in zip(got[1:], (w, dwx, dwy)):
            assert g[0].tolist() == [float(v) for v in want.split()], l
    cell, w, dwx, dwy = eio.contrast_votes([[np.nan, 1.0], [1.0, np.inf], [2.0 ** 31, 0.0], [5.0, 5.0]], W, H)
    assert (cell[:3] == -1).all() and not w[:3].any() and not dwx[:3].any() and not dwy[:3].any() and w[3].tolist() == [1.0, 0.0, 0.0, 0.0]


def test_new_symbol_resolves(hip_lib):
    assert hasattr(hip_lib, "emba_seq_contrast_gradient")
    from emba_amd import LEGM
    from emba_amd.sharded import HipEngine, ShardedLEGM, ShardedModel
    assert all(callable(getattr(k, "contrast_gradient")) for k in (LEGM, HipEngine, ShardedLEGM, ShardedModel))
    blob = open(os.path.join(ROOT, "emba_amd", "libemba_hip.so"), "rb").read()
    for k in (b"emba_contrast_vote_kernel", b"emba_contrast_grad_kernel", b"emba_contrast_reduce_kernel", b"emba_contrast_reduce_final_kernel"):
        assert k in blob, k


def plain_loop(pm, D, cp, pol, K, signed):
    """The stated formula, one event and one cell at a time: (image [H, W], J, grad [3 K], dropped votes)."""
    img = np.zeros((H, W))
    dropped = 0
    patches = []
    for (px, py), p in zip(pm.tolist(), pol.tolist()):
        patch = []
        if np.isfinite(px) and np.isfinite(py):
            ix, iy = int(np.floor(px)), int(np.floor(py))
            ax, ay = px - ix, py - iy
            s = -1.0 if (signed and p == 0) else 1.0
            for cx, cy, w, dx, dy in ((ix, iy, (1 - ax) * (1 - ay), -(1 - ay), -(1 - ax)), (ix + 1, iy, ax * (1 - ay), 1 - ay, -ax),
                                      (ix, iy + 1, (1 - ax) * ay, -ay, 1 - ax), (ix + 1, iy + 1, ax * ay, ay, ax)):
                if 0 <= cy < H:
                    img[cy][cx % W] += s * w
                    patch.append((cy, cx % W, dx, dy))
                elif w != 0:
                    dropped += 1
        patches.append(patch)
    g = np.zeros(3 * K)
    for k, patch in enumerate(patches):
        s = -1.0 if (signed and pol[k] == 0) else 1.0
        gx = sum(img[cy][cx] * dx for cy, cx, dx, dy in patch)
        gy = sum(img[cy][cx] * dy for cy, cx, dx, dy in patch)
        for j in range(6):
            g[3 * cp[k] + j] += 2.0 * s * (gx * D[k, 0, j] + gy * D[k, 1, j])
    return img, float((img * img).sum()), g, dropped


@pytest.mark.parametrize("signed", [False, True])
def test_numpy_form_equals_the_plain_loop(signed):
    """300 random events over the panorama and a margin around it: pm on the wrap column, on the pole row, on exact integers, several in the same cells and
    two that are not finite; random D, control poses 0 ... K - 2."""
    n, K = 300, 5
    rng = np.random.default_rng(31)
    pm = np.stack([rng.uniform(-3.0, W + 3.0, n), rng.uniform(-3.0, H + 3.0, n)], axis=1)
    pm[:8] = [[0.0, 0.0], [W - 0.5, 10.0], [-0.25, 10.5], [W, H], [77.0, -1.0], [77.5, H - 0.5], [np.nan, 3.0], [3.0, np.inf]]
    pm[8:30] = np.floor(pm[8:30])                                   # exact integers
    pm[30:50] = pm[10:30] + rng.uniform(0.0, 1.0, (20, 2))          # several events in the same cells
    D = rng.normal(size=(n, 2, 6))
    cp = rng.integers(0, K - 1, n).astype(np.int32)
    pol = rng.integers(0, 2, n).astype(np.uint8)
    got = eio.contrast_gradient(pm, D, cp, pol, K, W, H, signed)
    img, J, g, dropped = plain_loop(pm, D, cp, pol, K, signed)
    assert got["image"].shape == (H, W) and np.allclose(got["image"], img, rtol=1e-13, atol=1e-13)
    assert abs(got["J"] - J) <= 1e-12 * J and got["dropped"] == dropped > 0
    assert np.allclose(got["grad"], g, rtol=1e-11, atol=1e-11 * np.abs(g).max())
    assert (got["image"] < 0).any() == signed
    lean = eio.contrast_gradient(pm, None, None, pol, K, W, H, signed)
    assert lean["grad"] is None and lean["J"] == got["J"]
    # an event without a control pose in [0, K - 2] adds nothing to g
    cp2 = cp.copy(); cp2[100:110] = -1; cp2[110:120] = K - 1
    D2 = D.copy(); D2[100:120] = 0.0
    assert np.array_equal(eio.contrast_gradient(pm, D, cp2, pol, K, W, H, signed)["grad"], eio.contrast_gradient(pm, D2, np.where(cp2 < 0, 0, np.minimum(cp2, K - 2)), pol, K, W, H, signed)["grad"])


@pytest.fixture(scope="module")
def recording(oracle_mod):
    """The constant-rate recording and the oracle's warp of it along a trajectory: pm, D, cp of the used events (zero maps: only the dump matters)."""
    ev, lut = CC.constant_rate_events(CC.CONST_OMEGA)
    nn = ev.size() // 100 * 100
    o = oracle_mod.OracleLEGM(64, 48, W, H, lut, 0.2)
    Z = np.zeros((H, W))

    def warp(traj):
        d = o.evaluate_data_error(traj.knots_xyzw, traj.t0_ns, traj.dt_ns, Z, Z, ev.x, ev.y, ev.polarity, ev.t_ns, dump=True)[2]
        return d["pm"][:nn], d["D"][:nn], d["cp_idx"][:nn]

    def J_and_grad(traj):
        r = eio.contrast_gradient(*warp(traj), ev.polarity[:nn], traj.size(), W, H)
        return r["J"], r["grad"]
    return ev, lut, J_and_grad, (lambda traj: J_and_grad(traj)[0])


def knot_errors(traj, truth):
    """|log((R0^-1 Ri)_truth^-1 (R0^-1 Ri))| of every control pose behind the first: the error relative to the first knot, rad."""
    rel = lambda t, i: so3.mul(so3.inverse(t.knots_xyzw[0]), t.knots_xyzw[i])      # noqa: E731
    return [float(np.linalg.norm(so3.log(so3.mul(so3.inverse(rel(truth, i)), rel(traj, i))))) for i in range(1, traj.size())]


def check_ascent(hist, J_true, err0, err1, every_knot):
    assert len(hist) > 1 and all(b > a for a, b in zip(hist, hist[1:])), "the J history rises strictly"
    assert hist[-1] > J_true
    for i, (e0, e1) in enumerate(zip(err0, err1)):
        if every_knot or i > 0:
            assert e1 < 0.5 * e0, (i, e0, e1)


def test_gradient_against_central_differences(recording):
    ev, lut, J_and_grad, J_only = recording
    t0 = constant_rate_trajectory(CC.CONST_OMEGA / 2)
    J, g = J_and_grad(t0)
    assert g.shape == (12,) and J > 0
    h, worst = 1e-6, 0.0
    for seed in FD_SEEDS:
        d = np.random.default_rng(seed).normal(size=12)
        d /= np.linalg.norm(d)
        fd = (J_only(eio.incremental_update(t0, h * d, False)) - J_only(eio.incremental_update(t0, -h * d, False))) / (2 * h)
        mis = abs(fd - g @ d) / abs(g @ d)
        print(f"seed {seed}: central difference {fd:.6f}  g . d {g @ d:.6f}  relative mismatch {mis:.3e}")
        worst = max(worst, mis)
    print(f"worst {worst:.4e}, measured {FD_WORST_MEASURED:.4e}, bound {FD_BOUND:.4e}")
    assert worst <= FD_BOUND


@pytest.mark.parametrize("factor,every_knot", [(0.5, True), (1.3, False)])
def test_ascent_recovers_the_rate(recording, factor, every_knot):
    """refine_contrast from the trajectory at half (1.3 times) the true rate: J rises strictly, ends above J at the true trajectory, and every knot error
    relative to the first knot falls below half its initial value (from 1.3 times the rate: every knot but the first behind the fixed one)."""
    ev, lut, J_and_grad, J_only = recording
    truth = constant_rate_trajectory(CC.CONST_OMEGA)
    start = constant_rate_trajectory(CC.CONST_OMEGA * factor)
    J_true = J_only(truth)
    traj, hist, evals = eio.refine_contrast(J_and_grad, J_only, start, fix_first_pose=True, max_iter=60, pano_w=W)
    err0, err1 = knot_errors(start, truth), knot_errors(traj, truth)
    print(f"from {factor} x the rate: J {hist[0]:.1f} -> {hist[-1]:.1f} (truth {J_true:.1f}) in {len(hist) - 1} accepted steps, {evals} evaluations; "
          f"knot errors {np.round(err0, 4).tolist()} -> {np.round(err1, 4).tolist()} rad")
    assert np.array_equal(traj.knots_xyzw[0], start.knots_xyzw[0])      # the first pose was held
    check_ascent(hist, J_true, err0, err1, every_knot)


def test_ascent_with_the_sums_in_reverse_order(recording, oracle_mod):
    """The same loop with nothing but the order of the fp64 sums changed (the events handed to io.contrast_gradient in reverse): J at the start differs in
    the last place, the loop ends elsewhere — 28 081.300 against 28 077.861, 1.2e-4 relative, measured — and meets the same assertions.  The ascent is
    sensitive in where exactly it stops, not in what it achieves; nothing is asserted on the distance between the two ends."""
    ev, lut, J_and_grad, J_only = recording
    nn = ev.size() // 100 * 100
    o = oracle_mod.OracleLEGM(64, 48, W, H, lut, 0.2)
    Z = np.zeros((H, W))
    rev = np.arange(nn)[::-1]

    def JG(traj):
        d = o.evaluate_data_error(traj.knots_xyzw, traj.t0_ns, traj.dt_ns, Z, Z, ev.x, ev.y, ev.polarity, ev.t_ns, dump=True)[2]
        r = eio.contrast_gradient(d["pm"][:nn][rev], d["D"][:nn][rev], d["cp_idx"][:nn][rev], ev.polarity[:nn][rev], traj.size(), W, H)
        return r["J"], r["grad"]
    truth, start = constant_rate_trajectory(CC.CONST_OMEGA), constant_rate_trajectory(CC.CONST_OMEGA / 2)
    assert abs(JG(start)[0] - J_only(start)) <= 1e-12 * J_only(start)
    traj, hist, evals = eio.refine_contrast(JG, lambda t: JG(t)[0], start, fix_first_pose=True, max_iter=60, pano_w=W)
    err0, err1 = knot_errors(start, truth), knot_errors(traj, truth)
    print(f"sums in reverse order: J {hist[0]!r} -> {hist[-1]!r} in {len(hist) - 1} accepted steps, {evals} evaluations; knot errors -> {np.round(err1, 4).tolist()} rad")
    check_ascent(hist, J_only(truth), err0, err1, True)


def test_refine_contrast_arguments():
    t = constant_rate_trajectory(CC.CONST_OMEGA)
    with pytest.raises(TypeError):
        eio.refine_contrast(None, None, t)                  # no panorama width: no first step (a required keyword)
    # a flat contrast: no step is accepted, the trajectory comes back as it went in
    traj, hist, evals = eio.refine_contrast(lambda tr: (1.0, np.zeros(12)), lambda tr: 1.0, t, pano_w=W)
    assert traj is t and hist == [1.0] and evals == 1
    # a gradient no step along which helps: 11 trials (the step and its 10 halvings), then the loop gives up
    traj, hist, evals = eio.refine_contrast(lambda tr: (1.0, np.ones(12)), lambda tr: 1.0, t, pano_w=W)
    assert traj is t and hist == [1.0] and evals == 12


def test_the_driver_refuses_a_model_without_a_resident_sequence():
    from emba_amd.driver import SequenceSettings, refine_window_poses
    s = SequenceSettings(time_window_size=0.15, sliding_window_stride=0.1, dt_knots=0.05, t_start=1.0, t_end=1.15)
    assert s.refine_contrast is False and s.contrast_iters == 60
    with pytest.raises(ValueError, match="resident"):
        refine_window_poses(object(), constant_rate_trajectory(CC.CONST_OMEGA), 0, 100, False, 60)


def test_every_rank_gets_one_refined_trajectory():
    """Two stand-in ranks whose contexts answer J and g one unit in the last place apart (what the order of fp64 atomic adds does between devices): the
    ascent run rank by rank need not end at the same control poses; ShardedModel.refine_contrast runs it on rank 0 alone and every rank returns rank 0's
    trajectory, J and evaluation count bit for bit — and driver.refine_window_poses takes that path."""
    import threading
    from types import SimpleNamespace
    from emba_amd.driver import refine_window_poses
    from emba_amd.sharded import ShardedLEGM, ShardedModel
    target = so3.exp(np.array([0.02, -0.05, 0.01]))

    class Engine:
        """A smooth bump around `target` for every control pose, scaled by (1 + rank * 2^-52)."""

        def __init__(self, rank):
            self.scale, self.calls = 1.0 + rank * 2.0 ** -52, 0

        def bind_exchange(self, count, pack):
            pass

        def set_sequence(self, events, sampling_rate=1):
            return 0

        def contrast_gradient(self, traj, beg=0, end=None, signed=False, want_grad=True, want_image=False, want_pm=False, want_D=False, level=0):
            self.calls += 1
            w = np.array([so3.log(so3.mul(target, so3.inverse(q))) for q in traj.knots_xyzw])      # exp(x) q = target at x = w
            J = self.scale * float(np.exp(-50.0 * (w * w).sum(axis=1)).sum())
            g = self.scale * (100.0 * w * np.exp(-50.0 * (w * w).sum(axis=1))[:, None]).reshape(-1)
            return dict(J=J, grad=g if want_grad else None)

    class Dist:
        """all_reduce over two threads: both add into one tensor behind a barrier."""

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
            sh.barrier.wait()
            t.copy_(sh.acc)
            if sh.barrier.wait() == 0:
                sh.acc = None
            sh.barrier.wait()
    start = LinearTrajectory(np.tile([0.0, 0.0, 0.0, 1.0], (3, 1)), 0, 50_000_000)
    # rank by rank: the loops part ways somewhere behind the first bits
    alone = []
    for r in range(2):
        e = Engine(r)
        alone.append(eio.refine_contrast(lambda t: (lambda d: (d["J"], d["grad"]))(e.contrast_gradient(t)), lambda t: e.contrast_gradient(t, want_grad=False)["J"], start,
                                         max_iter=20, pano_w=W))
    assert alone[0][1][0] != alone[1][1][0]      # (J differs in the last place from the first evaluation on)
    shared = SimpleNamespace(lock=threading.Lock(), barrier=threading.Barrier(2), acc=None)
    engines, results = [Engine(0), Engine(1)], [None, None]

    def rank_main(r):
        host = ShardedModel(ShardedLEGM(engines[r], Dist(r, shared), None, None, 64), SimpleNamespace(H=H, W=W))
        results[r] = refine_window_poses(host, start, 0, 1000, True, 20)
    threads = [threading.Thread(target=rank_main, args=(r,)) for r in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=60)
    assert all(r is not None for r in results)
    (t0, a0, b0, n0), (t1, a1, b1, n1) = results
    assert np.array_equal(t0.knots_xyzw, t1.knots_xyzw) and (a0, b0, n0) == (a1, b1, n1) and (t0.t0_ns, t0.dt_ns) == (t1.t0_ns, t1.dt_ns) == (0, 50_000_000)
    assert np.array_equal(t0.knots_xyzw, alone[0][0].knots_xyzw) and (a0, b0, n0) == (alone[0][1][0], alone[0][1][-1], alone[0][2])      # rank 0's loop
    assert b0 > a0 and engines[0].calls > 0 and engines[1].calls == 0 and isinstance(n0, int)
    # one rank: no collective, the same result
    host = ShardedModel(ShardedLEGM(Engine(0), SimpleNamespace(get_rank=lambda: 0, get_world_size=lambda: 1), None, None, 64), SimpleNamespace(H=H, W=W))
    t_one, a_one, b_one, n_one = host.refine_contrast(start, 0, 1000, max_iter=20)
    assert np.array_equal(t_one.knots_xyzw, t0.knots_xyzw) and (a_one, b_one, n_one) == (a0, b0, n0)


def test_sharded_hosts_forward_the_gradient():
    """ShardedModel -> ShardedLEGM -> HipEngine -> the rank's model: the call and its arguments arrive unchanged."""
    from types import SimpleNamespace
    from emba_amd.sharded import HipEngine, ShardedLEGM, ShardedModel
    calls = []

    class Device:
        def bind_exchange(self, count, pack):
            pass

        def contrast_gradient(self, traj, beg=0, end=None, signed=False, want_grad=True, want_image=False, want_pm=False, want_D=False, level=0):
            calls.append((traj, beg, end, signed, want_grad, want_image, want_pm, want_D))
            return dict(J=7.0)
    dist = SimpleNamespace(get_rank=lambda: 0, get_world_size=lambda: 2)
    host = ShardedModel(ShardedLEGM(Device(), dist, None, None, 64), SimpleNamespace(H=4, W=8))
    assert host.contrast_gradient("traj", 3, 900, True, False, True, True, True) == dict(J=7.0) and calls == [("traj", 3, 900, True, False, True, True, True)]
    eng = HipEngine.__new__(HipEngine)                    # (its constructor wants a context on a GPU: the forwarding method alone)
    eng.m = Device()
    assert eng.contrast_gradient("traj", 1, 2) == dict(J=7.0) and calls[-1] == ("traj", 1, 2, False, True, False, False, False)
