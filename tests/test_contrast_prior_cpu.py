"""The prior of the smooth contrast — what earlier events already voted, as the image a window's ascent starts from — without a GPU: the
prior additions of the HIP-free rule header (emba_amd/csrc/contrast_rule.h through tests/cpp/contrast_prior_rule_test.cpp, also under the address and
undefined-behaviour sanitizers), the new symbols and kernels of libemba_hip.so and the new keywords of the Python hosts, the numpy form
(io.contrast_gradient(prior=...)) against its stated formula and against central differences of J, what the prior adds to an ascent that the window's own
contrast cannot see, and the driver's settings."""
import inspect
import os
import subprocess

import numpy as np
import pytest

import cmax_cases as CC
from emba_amd import io as eio
from emba_amd import so3
from emba_amd.legm import LinearTrajectory
from helpers import assert_close
from test_contrast_cpu import FD_BOUND as FD_BOUND_LEVEL_0
from test_contrast_cpu import FD_SEEDS
from test_contrast_pyramid_cpu import FD_WORST_MEASURED as FD_WORST_MEASURED_LEVEL
from test_panorama_cpu import constant_rate_trajectory

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 512, 256
SPLIT = 1500                    # the events [0, SPLIT) are the earlier ones, [SPLIT, 3000) the window
PRIOR_LEVELS = (2, 1, 0)
# The common yaw of the demonstration: the largest of 4, 2 and 1 level-0 pixels (2 pi / 512 rad each) at which the numpy form ends with the errors of knots
# 2 and 3 below half of it.  Measured on the CPU, errors of knots 2 and 3 against the truth, rad:
#   4 px = 0.04909: with the prior 0.00396, 0.00426; without 0.04984, 0.05026        2 px = 0.02454: with 0.00409, 0.00348; without 0.04990, 0.05023
#   1 px = 0.01227: with 0.00481, 0.00443; without 0.01428, 0.01123
DELTA_PX = 4
DELTA = DELTA_PX * 2.0 * np.pi / W


def fd_bound(level):
    """The bound of test_gradient_against_central_differences[_per_level] for that level: ten times the worst mismatch measured there without a prior."""
    return FD_BOUND_LEVEL_0 if level == 0 else 10.0 * FD_WORST_MEASURED_LEVEL[level]


def yawed(traj, delta):
    """Every control pose left-multiplied by one common yaw of delta rad (about the panorama's vertical axis)."""
    q = so3.exp(np.array([0.0, float(delta), 0.0]))
    return LinearTrajectory(np.array([so3.mul(q, k) for k in traj.knots_xyzw]), traj.t0_ns, traj.dt_ns)


def abs_errors(traj, truth):
    """|log(truth_i^-1 traj_i)| of every control pose: the error against the truth itself, rad."""
    return [float(np.linalg.norm(so3.log(so3.mul(so3.inverse(truth.knots_xyzw[i]), traj.knots_xyzw[i])))) for i in range(traj.size())]


def level_votes(pm, pol, level, signed=False):
    """The numpy votes of pm at a level: (image [H_l, W_l], dropped)."""
    pm_l, _, Wl, Hl = eio.contrast_level(pm, None, W, H, level)
    r = eio.contrast_gradient(pm_l, None, None, pol, 2, Wl, Hl, signed)
    return r["image"], r["dropped"]


def test_prior_rule_on_the_cpu(tmp_path):
    """contrast_rule.h's prior additions (plain C++17, no HIP): tests/cpp/contrast_prior_rule_test.cpp checks the level mask of
    emba_seq_contrast_prior_add, the order of its levels, the weight, the image's first cell and the rule on a small grid.  Built twice: plain, and as a
    stand-alone program under -fsanitize=address,undefined."""
    src = os.path.join(ROOT, "tests", "cpp", "contrast_prior_rule_test.cpp")
    outs = []
    for name, extra in (("contrast_prior_rule_test", []), ("contrast_prior_rule_test_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])):
        exe = str(tmp_path / name)
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-ffp-contract=off"] + extra + [src, "-o", exe])
        r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
        print(r.stdout[-3000:], r.stderr)
        assert r.returncode == 0 and r.stdout.strip().splitlines()[-1] == "OK contrast_prior_rule", r.stdout[-3000:] + r.stderr
        outs.append(r.stdout)
    assert outs[0] == outs[1]


def test_new_symbols_resolve(hip_lib):
    from emba_amd import LEGM, _lib
    from emba_amd.driver import refine_window_poses
    from emba_amd.sharded import HipEngine, ShardedLEGM, ShardedModel
    names = ("emba_seq_contrast_prior_add", "emba_seq_contrast_prior_set", "emba_seq_contrast_prior_get", "emba_seq_contrast_prior_clear",
             "emba_seq_contrast_gradient_prior")
    for name in names:
        assert hasattr(hip_lib, name) and name in _lib.SIGNATURES, name
    assert hip_lib.emba_abi_version() == 2
    blob = open(os.path.join(ROOT, "emba_amd", "libemba_hip.so"), "rb").read()
    assert b"emba_contrast_prior_vote_kernel" in blob and b"emba_contrast_prior_init_kernel" in blob
    for k in (LEGM, HipEngine, ShardedLEGM, ShardedModel):
        p = inspect.signature(k.contrast_gradient).parameters
        assert list(p)[-1] == "prior_weight" and p["prior_weight"].default is None and p["level"].default == 0, k
        p = inspect.signature(k.contrast_prior_add).parameters
        assert (p["beg"].default, p["end"].default, p["levels"].default, p["signed"].default) == (0, None, (0,), False), k
        for name in ("contrast_prior_set", "contrast_prior_get", "contrast_prior_clear"):
            assert callable(getattr(k, name)), (k, name)
    for f in (ShardedLEGM.refine_contrast, ShardedModel.refine_contrast, eio.refine_contrast_levels, refine_window_poses):
        assert inspect.signature(f).parameters["prior_weight"].default is None, f
    assert list(inspect.signature(eio.contrast_gradient).parameters)[-1] == "prior" and inspect.signature(eio.contrast_gradient).parameters["prior"].default is None


@pytest.fixture(scope="module")
def recording(oracle_mod):
    """The constant-rate recording and the oracle's warp of a range of it along a trajectory: pm, D, cp of the range's used events."""
    ev, lut = CC.constant_rate_events(CC.CONST_OMEGA)
    o = oracle_mod.OracleLEGM(64, 48, W, H, lut, 0.2)
    Z = np.zeros((H, W))

    def warp(traj, beg, end):
        nn = (end - beg) // 100 * 100
        d = o.evaluate_data_error(traj.knots_xyzw, traj.t0_ns, traj.dt_ns, Z, Z, ev.x[beg:end], ev.y[beg:end], ev.polarity[beg:end], ev.t_ns[beg:end], dump=True)[2]
        return d["pm"][:nn], d["D"][:nn], d["cp_idx"][:nn]
    return ev, warp


def test_no_prior_is_todays_result(recording):
    """io.contrast_gradient(..., prior=None), and without the argument, bit for bit: image, J, gradient, dropped — signed and not, at levels 0 and 2."""
    ev, warp = recording
    n = ev.size() // 100 * 100
    pm, D, cp = warp(constant_rate_trajectory(CC.CONST_OMEGA / 2), 0, n)
    for level in (0, 2):
        pm_l, D_l, Wl, Hl = eio.contrast_level(pm, D, W, H, level)
        for signed in (False, True):
            a = eio.contrast_gradient(pm_l, D_l, cp, ev.polarity[:n], 4, Wl, Hl, signed)
            b = eio.contrast_gradient(pm_l, D_l, cp, ev.polarity[:n], 4, Wl, Hl, signed, prior=None)
            assert np.array_equal(a["image"], b["image"]) and a["J"] == b["J"] and np.array_equal(a["grad"], b["grad"]) and a["dropped"] == b["dropped"]
    with pytest.raises(ValueError, match="prior"):
        eio.contrast_gradient(pm, D, cp, None, 4, W, H, prior=np.zeros((H, W + 1)))


@pytest.mark.parametrize("level", [0, 2])
def test_a_dense_prior_formula_and_central_differences(recording, level):
    """A random dense prior, negative cells included: the image is the prior plus the votes, J its sum of squares = the votes' own J + twice their
    correlation with the prior + the prior's, the prior itself is not written to; and the gradient agrees with central differences of that J along the
    directions FD_SEEDS under the bound of the test without a prior at that level."""
    ev, warp = recording
    n = ev.size() // 100 * 100
    t0 = constant_rate_trajectory(CC.CONST_OMEGA / 2)
    Wl, Hl = W >> level, H >> level
    P = np.random.default_rng(7).normal(scale=2.0, size=(Hl, Wl))
    keep = P.copy()
    assert (P < 0).any()

    def at(traj, prior):
        pm_l, D_l, _, _ = eio.contrast_level(*warp(traj, 0, n)[:2], W, H, level)
        return eio.contrast_gradient(pm_l, D_l, warp(traj, 0, n)[2], None, 4, Wl, Hl, prior=prior)
    own, got = at(t0, None), at(t0, 0.5 * P)
    assert np.array_equal(P, keep)
    assert_close(got["image"], 0.5 * P + own["image"], f"level {level} image = prior + votes")
    assert got["J"] == float((got["image"] ** 2).sum()) and got["dropped"] == own["dropped"]
    split = own["J"] + 2.0 * float((0.5 * P * own["image"]).sum()) + float((0.25 * P * P).sum())
    assert abs(got["J"] - split) <= 1e-12 * abs(got["J"])
    g = got["grad"]
    h, worst = 1e-6, 0.0
    for seed in FD_SEEDS:
        d = np.random.default_rng(seed).normal(size=12)
        d /= np.linalg.norm(d)
        fd = (at(eio.incremental_update(t0, h * d, False), 0.5 * P)["J"] - at(eio.incremental_update(t0, -h * d, False), 0.5 * P)["J"]) / (2 * h)
        mis = abs(fd - g @ d) / abs(g @ d)
        print(f"level {level} seed {seed}: central difference {fd:.6f}  g . d {g @ d:.6f}  relative mismatch {mis:.3e}")
        worst = max(worst, mis)
    print(f"level {level}, dense prior: worst {worst:.4e}, bound {fd_bound(level):.4e}")
    assert worst <= fd_bound(level)


def numpy_demonstration(warp, truth, start, weight):
    """The ascent of `start` on the events [SPLIT, 3000) over PRIOR_LEVELS, every pose free, against weight times the numpy votes of [0, SPLIT) along
    `truth` (weight None: on the window's own contrast)."""
    pm = warp(truth, 0, SPLIT)[0]
    prior = {l: level_votes(pm, None, l)[0] for l in PRIOR_LEVELS}

    def J_and_grad_at(l):
        def f(traj):
            pm_w, D_w, cp_w = warp(traj, SPLIT, 3000)
            pm_l, D_l, Wl, Hl = eio.contrast_level(pm_w, D_w, W, H, l)
            r = eio.contrast_gradient(pm_l, D_l, cp_w, None, traj.size(), Wl, Hl, prior=None if weight is None else weight * prior[l])
            return r["J"], r["grad"]
        return f
    return eio.refine_contrast_pyramid(J_and_grad_at, lambda l: (lambda t: J_and_grad_at(l)(t)[0]), start, PRIOR_LEVELS, pano_w=W, fix_first_pose=False, max_iter=60)


def test_what_the_prior_adds(recording):
    """The true control poses, all turned by one common yaw of DELTA (4 level-0 pixels), then refined on the second half of the events with every pose
    free.  The window's own contrast barely sees a common rotation — it moves the whole image — so without a prior the errors stay near DELTA (printed).
    Against the votes of the first half along the true trajectory the image has a place to be: the errors of knots 2 and 3, the ones the window's events
    hang on, end below half of DELTA.  Measured (numpy, rad): 0.04909 -> 0.00396, 0.00426 with the prior; 0.04984, 0.05026 without."""
    ev, warp = recording
    assert ev.size() >= 3000 and ev.t_ns[SPLIT] > 1_050_000_000      # the window's events lie behind knot 1: knots 2 and 3 carry them
    truth = constant_rate_trajectory(CC.CONST_OMEGA)
    start = yawed(truth, DELTA)
    err0 = abs_errors(start, truth)
    assert np.allclose(err0, DELTA, rtol=0, atol=1e-12)
    without, hists_wo, _ = numpy_demonstration(warp, truth, start, None)
    print(f"without a prior: errors {np.round(err0, 5).tolist()} -> {np.round(abs_errors(without, truth), 5).tolist()} rad, level-0 J {hists_wo[0][0]:.1f} -> {hists_wo[0][-1]:.1f}")
    traj, hists, evals = numpy_demonstration(warp, truth, start, 1.0)
    err1 = abs_errors(traj, truth)
    print(f"with the prior:  errors {np.round(err0, 5).tolist()} -> {np.round(err1, 5).tolist()} rad, level-0 J {hists[0][0]:.1f} -> {hists[0][-1]:.1f}, {evals} evaluations")
    assert err1[2] < 0.5 * DELTA and err1[3] < 0.5 * DELTA, err1


def test_settings_and_the_drivers_refusals():
    from emba_amd.driver import SequenceSettings, WindowResult, run_sequence
    s = SequenceSettings(time_window_size=0.15, sliding_window_stride=0.1)
    assert s.contrast_prior is False and s.contrast_prior_weight == 1.0
    assert WindowResult.__dataclass_fields__["prior_events"].default is None
    ok = SequenceSettings(0.15, 0.1, refine_contrast=True, contrast_prior=True, contrast_prior_weight=0.0)
    assert ok.contrast_prior and ok.contrast_prior_weight == 0.0
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="contrast_prior_weight"):
            SequenceSettings(0.15, 0.1, refine_contrast=True, contrast_prior=True, contrast_prior_weight=bad)
    with pytest.raises(ValueError, match="refine_contrast"):
        SequenceSettings(0.15, 0.1, contrast_prior=True)
    # the driver: a model without a resident sequence, a model that has no priors
    ev, _ = CC.constant_rate_events(CC.CONST_OMEGA)
    seq = SequenceSettings(0.1, 0.05, t_start=1.0, t_end=1.15, refine_contrast=True, contrast_prior=True)
    Z = np.zeros((H, W))
    t = np.array([1.0, 1.2])
    q = np.tile([0.0, 0.0, 0.0, 1.0], (2, 1))

    class NoSequence:
        W, H = W, H
    with pytest.raises(ValueError, match="contrast_prior needs a model with the event sequence resident"):
        run_sequence(NoSequence(), ev, t, q, Z, Z, seq, resident_sequence=False)

    class NoPriors(NoSequence):
        def set_sequence(self, events, sampling_rate=1):
            return events.size()
    with pytest.raises(ValueError, match="contrast_prior needs a model with the event sequence resident"):
        run_sequence(NoPriors(), ev, t, q, Z, Z, seq)
    seq.refine_contrast = False      # (changed behind __post_init__'s back: the driver checks again)
    with pytest.raises(ValueError, match="refine_contrast"):
        run_sequence(NoPriors(), ev, t, q, Z, Z, seq)


def test_the_hosts_forward_the_prior():
    """ShardedModel -> ShardedLEGM -> HipEngine -> the rank's model: prior_weight arrives where it is given and is not mentioned where it is not; the prior
    calls reach the rank's own context; the driver's retirement and ascent ask what they should."""
    from types import SimpleNamespace
    from emba_amd.driver import refine_window_poses, retire_events
    from emba_amd.sharded import HipEngine, ShardedLEGM, ShardedModel
    calls = []

    class Device:
        W, H = 8, 4

        def bind_exchange(self, count, pack):
            pass

        def contrast_gradient(self, *a, **kw):
            calls.append(("gradient", a, kw))
            return dict(J=7.0, grad=np.zeros(12))

        def contrast_prior_add(self, *a, **kw):
            calls.append(("add", a, kw))
            return dict(added=300, dropped={0: 0})

        def contrast_prior_set(self, *a):
            calls.append(("set", a))

        def contrast_prior_get(self, *a):
            calls.append(("get", a))
            return "image"

        def contrast_prior_clear(self):
            calls.append(("clear",))
    dist = SimpleNamespace(get_rank=lambda: 0, get_world_size=lambda: 1)
    eng = HipEngine.__new__(HipEngine)
    eng.m = Device()
    eng.contrast_gradient("traj", 1, 2, level=3, prior_weight=2.0)
    assert calls[-1] == ("gradient", ("traj", 1, 2, False, True, False, False, False), dict(level=3, prior_weight=2.0))
    eng.contrast_gradient("traj", 1, 2, level=3)
    assert calls[-1] == ("gradient", ("traj", 1, 2, False, True, False, False, False), dict(level=3))
    assert eng.contrast_prior_add("traj", 5, 905, (1,), True)["added"] == 300 and calls[-1] == ("add", ("traj", 5, 905, (1,), True), {})
    eng.contrast_prior_set(2, None)
    assert calls[-1] == ("set", (2, None)) and eng.contrast_prior_get(0) == "image" and calls[-1] == ("get", (0,))
    eng.contrast_prior_clear()
    assert calls[-1] == ("clear",)
    host = ShardedModel(ShardedLEGM(Device(), dist, None, None, 64), SimpleNamespace(H=4, W=8))
    host.contrast_gradient("traj", 3, 900, level=2, prior_weight=0.25)
    assert calls[-1] == ("gradient", ("traj", 3, 900, False, True, False, False, False), dict(level=2, prior_weight=0.25))
    host.contrast_gradient("traj", 3, 900, level=2)
    assert calls[-1] == ("gradient", ("traj", 3, 900, False, True, False, False, False), dict(level=2))
    assert host.contrast_prior_add("traj", 5, 905, levels=(2, 0), signed=True) == dict(added=300, dropped={0: 0})
    assert calls[-1] == ("add", ("traj", 5, 905, (2, 0), True), {})
    host.contrast_prior_set(1, "P")
    assert calls[-1] == ("set", (1, "P"))
    assert host.contrast_prior_get(1) == "image" and calls[-1] == ("get", (1,))
    host.contrast_prior_clear()
    assert calls[-1] == ("clear",)
    # the ascent: every evaluation of every level carries the weight, through either host
    start = LinearTrajectory(np.tile([0.0, 0.0, 0.0, 1.0], (4, 1)), 0, 50_000_000)
    for model in (Device(), host):
        del calls[:]
        refine_window_poses(model, start, 10, 990, True, 5, (1, 0), prior_weight=0.5)
        assert calls and all(c[0] == "gradient" and c[2].get("prior_weight") == 0.5 for c in calls) and {c[2]["level"] for c in calls} == {0, 1}
        del calls[:]
        refine_window_poses(model, start, 10, 990, True, 5, (1, 0))
        assert calls and all("prior_weight" not in c[2] for c in calls)
    # retirement: whole batches along the whole trajectory; fewer than one batch waits
    del calls[:]
    knots = np.tile([0.0, 0.0, 0.0, 1.0], (5, 1))
    assert retire_events(Device(), knots, 17, 50_000_000, 100, 199, (1, 0)) == 0 and not calls
    assert retire_events(Device(), knots, 17, 50_000_000, 100, 460, (1, 0)) == 300
    (what, (traj, beg, end), kw), = calls
    assert what == "add" and (beg, end) == (100, 460) and kw == dict(levels=(1, 0)) and traj.size() == 5 and (traj.t0_ns, traj.dt_ns) == (17, 50_000_000)
