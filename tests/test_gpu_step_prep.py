"""The steady step without a launch in front of its warp kernel (option step_prep), and texels packed only when they are stale (-m gpu).

Where the accumulator lines are clean and the texels fresh, workgroup 0 of the pixel-order warp kernel forms the K - 1 segment records and hands them to
every other workgroup inside the launch (kernels.h: inline_seg_*).  What can go wrong silently is a wave that reads the PREVIOUS evaluation's records from
the same addresses, or texels of another map or rectangle: every test here compares a context that has a history with a fresh context (no history: its
first step takes the launch in front and the stencil) at the same poses and map.  Records and texels are formed by unchanged arithmetic, so everything
that is not an fp64 atomic sum (ep, count map, active set) must agree BIT FOR BIT; A11, b1 and A22 | b2 are sums of atomics whose arrival order varies and
are held to helpers.assert_close.

Shapes: a 64 x 48 sensor on a 256 x 128 panorama, 20 k events = 318 one-wave workgroups — every XCD, and on a chip that holds them all at once the
hand-off is waited for by nearly every one of them; K = 5 and K = 21.
"""
import copy

import numpy as np
import pytest

from helpers import assert_close, oracle_run, small_workload
from test_gpu_parity import compare_normal_eq

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from emba_amd import build
    build.build_hip()
    return True


@pytest.fixture
def contexts():
    from emba_amd import LEGM
    made = []

    def make(w, events=True, upload=True, **opts):
        m = LEGM(w.sensor_w, w.sensor_h, w.lut, w.C_th, w.pano_w, w.pano_h, device=0)
        made.append(m)
        for k, v in {"step_prep": 1, **opts}.items():      # (the library's default is 0: the hand-off is what these tests are about)
            m.set_option(k, v)
        if events:
            m.set_events(w.events)
        if upload:
            m.upload_map(w.Gx, w.Gy)
        return m

    yield make
    for m in made:
        m.close()


def workload(K):
    return small_workload(n_events=20000, pano_h=128, K=K, dt_knots=0.25 / (K - 1))


def moved(traj, which, eps):
    """A copy of the trajectory with control pose `which` (None: all of them) rotated a little."""
    t = copy.deepcopy(traj)
    k = t.knots_xyzw.copy()
    rows = slice(None) if which is None else slice(which, which + 1)
    k[rows, 0] += eps
    k[rows] /= np.linalg.norm(k[rows], axis=1, keepdims=True)
    t.knots_xyzw = k
    return t


def yawed(traj, angle):
    """Every control pose rotated by `angle` about y (as test_gpu_variants' drift input): the footprint moves across the panorama."""
    from emba_amd.synth import so3_exp_xyzw
    t = copy.deepcopy(traj)
    ex, ey, ez, ew = so3_exp_xyzw(np.array([0.0, angle, 0.0]))
    k = t.knots_xyzw.copy()
    for i in range(k.shape[0]):
        bx, by, bz, bw = k[i]
        q = np.array([ew * bx + ex * bw + ey * bz - ez * by, ew * by + ey * bw + ez * bx - ex * bz,
                      ew * bz + ez * bw + ex * by - ey * bx, ew * bw - ex * bx - ey * by - ez * bz])
        k[i] = q / np.linalg.norm(q)
    t.knots_xyzw = k
    return t


def step(m, w, traj):
    """One resident step and everything it leaves: the equations, ep, the count map; and which form it took."""
    n_inl, P = m.step(traj, w.thres_valid_pixel, w.alpha)
    ne = m._finish(w.alpha, False)
    _, ep, nem = m.eval_finish(want_ep=True, want_map=True)
    return dict(n_inl=n_inl, P=P, ne=ne, ep=ep, nem=nem, in_warp=m.get_option("prep_in_warp"), packed=m.get_option("texels_packed"))


def same(a, b, what):
    assert a["n_inl"] == b["n_inl"] and a["P"] == b["P"], what
    assert np.array_equal(a["nem"], b["nem"]), what + ": count map"
    assert np.array_equal(a["ep"], b["ep"]), what + ": ep differs in some bit"
    assert np.array_equal(a["ne"]["active"], b["ne"]["active"]), what + ": active set"
    for k in ("A11", "b1", "A22", "b2"):      # fp64 atomic sums: the arrival order varies from launch to launch
        assert_close(a["ne"][k], b["ne"][k], f"{k} {what}")


def fresh(contexts, w, traj, Gx=None, Gy=None, **opts):
    """The step of a context without a history, at these poses and this map."""
    ww = w
    if Gx is not None:
        ww = copy.copy(w); ww.Gx, ww.Gy = Gx, Gy
    m = contexts(ww, **opts)
    r = step(m, ww, traj)
    assert r["in_warp"] == 0, "a first step has unclean lines: it takes the launch in front"
    return r


@pytest.mark.parametrize("K", [5, 21])
@pytest.mark.parametrize("prep", [1, 0])
def test_consecutive_steps_never_read_stale_records(gpu, contexts, K, prep):
    """Three consecutive steps on one context at three knot sets, the second differing from the first in ONE control pose, behind the two steps a context needs
    before its texels are fresh (the first packs an empty rectangle, the second the first one's): each equals a fresh context's.  The default takes no launch in
    front of any of the three (asserted), and last step's records sit where this step's are read."""
    w = workload(K)
    trajs = [w.traj, moved(w.traj, K // 2, 2e-3), moved(w.traj, None, -3e-3)]
    m = contexts(w, step_prep=prep)
    for i in range(2):
        assert step(m, w, w.traj)["in_warp"] == 0
    for i, t in enumerate(trajs):
        r = step(m, w, t)
        assert r["in_warp"] == prep, f"step {i}"
        same(r, fresh(contexts, w, t), f"step {i} K {K} step_prep {prep}")
    assert m.get_option("step_prep_fallbacks") == 0


@pytest.mark.parametrize("K", [5, 21])
def test_waves_that_give_up_waiting_form_the_same_records(gpu, contexts, K):
    """step_prep_polls = 0: nobody waits, every wave but workgroup 0's forms the records itself (the bounded wait's exit, counted)."""
    w = workload(K)
    m = contexts(w, step_prep_polls=0)
    step(m, w, w.traj); step(m, w, w.traj)
    t = moved(w.traj, 1, 2e-3)
    r = step(m, w, t)
    assert r["in_warp"] == 1
    n_waves = -(-(w.events.size() + 1) // 63)
    assert 0 < m.get_option("step_prep_fallbacks") <= n_waves
    same(r, fresh(contexts, w, t), f"fallback K {K}")


@pytest.mark.parametrize("prep", [1, 0])
def test_both_forms_against_the_oracle(gpu, contexts, oracle_mod, prep):
    w = workload(21)
    o = oracle_run(oracle_mod, w)
    m = contexts(w, step_prep=prep)
    for i in range(4):
        r = step(m, w, w.traj)
        assert r["in_warp"] == (1 if prep and i >= 2 else 0)
        assert r["n_inl"] == o["ep"].size and r["P"] == o["ne"]["P"]
        assert np.array_equal(r["nem"], o["num_ev_map"])
        assert_close(r["ep"], o["ep"], "ep")
        compare_normal_eq(r["ne"], o["ne"])


def test_texels_follow_the_map_through_every_entry_point(gpu, contexts):
    """Step, change the map through each map-changing call in turn, step again: the texels are packed again (asserted) and the step equals a fresh context's on
    the new map.  Between changes a repeated step packs nothing and takes no launch in front."""
    w = workload(5)
    m = contexts(w)
    step(m, w, w.traj)
    r = step(m, w, w.traj)
    assert (r["packed"], r["in_warp"]) == (1, 0), "the second step packs the first one's rectangle"
    r = step(m, w, w.traj)
    assert (r["packed"], r["in_warp"]) == (0, 1), "same map, same footprint: nothing to pack, no launch in front"

    def changed(what):
        Gx, Gy = m.downloadMap()
        r = step(m, w, w.traj)
        assert (r["packed"], r["in_warp"]) == (1, 0), what
        same(r, fresh(contexts, w, w.traj, Gx, Gy), what)
        r = step(m, w, w.traj)
        assert (r["packed"], r["in_warp"]) == (0, 1), what + ", repeated"
        same(r, fresh(contexts, w, w.traj, Gx, Gy), what + ", repeated")

    m.upload_map(0.5 * w.Gx, w.Gy + 0.25 * w.Gx); changed("emba_upload_map")
    m.median_blur_map(); changed("emba_median_blur3_map")
    for decision in ("accept", "reject"):
        m.step(w.traj, w.thres_valid_pixel, w.alpha)
        _, x2 = m.solveNormalEq(1e-2, fix_first_pose=True)
        m.updateMap(x2, 0.5); changed("emba_update_map (the trial map)")
        if decision == "accept":
            m.acceptMap(); changed("emba_map_accept")
        else:
            m.rejectMap(); changed("emba_map_reject")
    m.step(w.traj, w.thres_valid_pixel, w.alpha)
    m.solveNormalEq(1e-2, fix_first_pose=True, resident_x2=True)
    m.updateMap(None, 0.25); changed("emba_update_map, x2 on the device")


def test_texels_follow_a_map_that_starts_from_nothing(gpu, contexts):
    """The start without a front-end map: a zero map, a step, the map-only solve, its update as the trial map, the acceptance — after each of them the
    texels are packed again and the step equals a fresh context's on the map of that moment."""
    w = workload(5)
    zero = copy.copy(w); zero.Gx, zero.Gy = np.zeros_like(w.Gx), np.zeros_like(w.Gy)
    m = contexts(zero)
    for expect in ((1, 0), (1, 0), (0, 1)):
        r = step(m, zero, w.traj)
        assert (r["packed"], r["in_warp"]) == expect
    same(r, fresh(contexts, zero, w.traj), "the zero map")
    m.solveMapOnly(1e-2, resident_x2=True)
    m.updateMap(None, 1.0)
    for what, then in (("the map-only update", m.acceptMap), ("its acceptance", lambda: None)):
        Gx, Gy = m.downloadMap()
        assert Gx.any() or Gy.any(), "the map-only solve left the zero map"
        r = step(m, w, w.traj)
        assert (r["packed"], r["in_warp"]) == (1, 0), what
        same(r, fresh(contexts, w, w.traj, Gx, Gy), what)
        r = step(m, w, w.traj)
        assert (r["packed"], r["in_warp"]) == (0, 1), what + ", repeated"
        same(r, fresh(contexts, w, w.traj, Gx, Gy), what + ", repeated")
        then()


def test_a_bound_map_is_never_taken_for_unchanged(gpu, contexts):
    """emba_bind_map_dev: the planes are the caller's memory and may change without a call — the texels are packed in every evaluation, the launch stays."""
    import torch
    w = workload(5)
    gx = torch.from_numpy(w.Gx.copy()).cuda(); gy = torch.from_numpy(w.Gy.copy()).cuda()
    m = contexts(w, upload=False)
    m.bind_map_dev(gx.data_ptr(), gy.data_ptr())
    for i in range(3):
        r = step(m, w, w.traj)
        assert r["in_warp"] == 0 and r["packed"] == 1
    gx.mul_(0.5); torch.cuda.synchronize()
    r = step(m, w, w.traj)
    same(r, fresh(contexts, w, w.traj, 0.5 * w.Gx, w.Gy), "bound map changed in place")


def test_the_planes_follow_every_transition(gpu, contexts, oracle_mod):
    """The PLANES after each call that changes or rebinds them (the tests above see them through the texels only): one context walks upload, bind, the blur of
    a bound map, a trial update, a second update before an accept, accept, a reject without a trial, another update, its reject; after each,
    emba_download_map against an expectation kept in numpy.  What only rebinds or copies is compared bit for bit, the blur with its restatement
    (emba_amd.io.median_blur3, exact), an update as test_gpu_parity.test_lm_loop_map_residency does: oracle update_map of the active set, at its tolerance.
    (The dampings are powers of two: damping * x2 is then exact, so that a fused multiply-add gives the bits of a multiply and an add.)"""
    import torch
    from emba_amd import io as eio
    w = workload(5)

    def planes(want, what, exact=True):
        got = m.downloadMap()
        for g, e, n in zip(got, want, ("Gx", "Gy")):
            if exact:
                assert np.array_equal(g, e), f"{n} after {what}"
            else:
                assert np.allclose(g, e, rtol=0, atol=1e-16), f"{n} after {what}"
        return got

    def solved_step():
        """step + solve on the planes the next evaluation reads: the active set and x2 an update is built from"""
        m.step(w.traj, w.thres_valid_pixel, w.alpha)
        ne = m._finish(w.alpha, False)
        _, x2 = m.solveNormalEq(1e-2, fix_first_pose=True)
        assert 0 < ne["P"] < w.Gx.size and x2.any(), "the window has active and inactive pixels, and the solve moves the map"
        return ne["active"], x2

    m = contexts(w)                                                                        # 1. upload
    cur = planes((w.Gx, w.Gy), "emba_upload_map")
    bound = (np.ascontiguousarray(0.5 * w.Gx), np.ascontiguousarray(0.5 * w.Gy + 0.25 * w.Gx))
    gx, gy = (torch.from_numpy(a.copy()).cuda() for a in bound)
    m.bind_map_dev(gx.data_ptr(), gy.data_ptr())                                           # 2. bind, other values
    cur = planes(bound, "emba_bind_map_dev")
    m.median_blur_map()                                                                    # 3. the blur of a bound map: the result is the context's own
    cur = planes((eio.median_blur3(bound[0]), eio.median_blur3(bound[1])), "emba_median_blur3_map on a bound map")
    assert not np.array_equal(cur[0], bound[0])
    torch.cuda.synchronize()
    assert np.array_equal(gx.cpu().numpy(), bound[0]) and np.array_equal(gy.cpu().numpy(), bound[1]), "the blur wrote the caller's tensors"
    active, x2 = solved_step()                                                             # 4. step, solve, update
    m.updateMap(x2, 0.5)
    first = planes(oracle_mod.update_map(active, x2, 0.5, *cur), "emba_update_map", exact=False)
    assert (first[0].ravel()[np.setdiff1d(np.arange(first[0].size), active)] == 0).all()
    m.updateMap(x2, 0.25)                                                                  # 5. again, another damping, no accept: from the CURRENT planes
    second = planes(oracle_mod.update_map(active, x2, 0.25, *cur), "a second emba_update_map before an accept", exact=False)
    from_first = oracle_mod.update_map(active, x2, 0.25, *first)
    assert not np.allclose(second[0], from_first[0], rtol=0, atol=1e-16), "the case cannot tell the current planes from the first trial"
    m.acceptMap()                                                                          # 6. accept: the trial's values
    cur = planes(second, "emba_map_accept")
    m.rejectMap()                                                                          # 7. reject with no trial pending: nothing moves
    planes(cur, "emba_map_reject without a trial")
    active, x2 = solved_step()                                                             # 8. step, solve, update
    m.updateMap(x2, 0.5)
    trial = planes(oracle_mod.update_map(active, x2, 0.5, *cur), "emba_update_map on the accepted map", exact=False)
    assert not np.array_equal(trial[0], cur[0])
    m.rejectMap()                                                                          # 9. reject: the accepted planes again
    planes(cur, "emba_map_reject")


def test_a_footprint_that_leaves_the_packed_rectangle(gpu, contexts):
    """A trajectory whose pixels leave the packed rectangle: that step meets the stencil outside it (same values), the next one packs the new rectangle."""
    w = workload(5)
    m = contexts(w)
    for _ in range(3):
        r = step(m, w, w.traj)
    assert (r["packed"], r["in_warp"]) == (0, 1)
    far = yawed(w.traj, 1.0)
    r = step(m, w, far)
    assert (r["packed"], r["in_warp"]) == (0, 1), "the host cannot know before the step that the footprint will move"
    same(r, fresh(contexts, w, far), "outside the packed rectangle")
    r = step(m, w, far)
    assert (r["packed"], r["in_warp"]) == (1, 0), "the step before reported that its box left the packed one"
    same(r, fresh(contexts, w, far), "rectangle packed again")
    r = step(m, w, far)
    assert (r["packed"], r["in_warp"]) == (0, 1)
    same(r, fresh(contexts, w, far), "fresh again")


def test_paths_that_keep_the_launch_in_front(gpu, contexts, oracle_mod):
    """K = 105 (control poses through the staging buffer), a tile-order window, an empty window and a first evaluation on unclean lines keep the launch."""
    from emba_amd import EventPacket
    w = small_workload(n_events=20000, K=105, dt_knots=0.002)
    m = contexts(w)
    for i in range(3):
        r = step(m, w, w.traj)
        assert r["in_warp"] == 0, "K = 105"
    same(r, fresh(contexts, w, w.traj, step_prep=0), "K = 105")

    w = workload(5)
    m = contexts(w, order=2, texel=3)      # (the rectangle pinned: no texel blocks must mean fresh texels, not another Hessian source)
    for i in range(3):
        r = step(m, w, w.traj)
        assert r["in_warp"] == 0 and m.setup_info()["tile_order"], "tile order"
    assert r["packed"] == 0, "the tile order gets the texels of part 1"
    same(r, fresh(contexts, w, w.traj, order=2, texel=3, step_prep=0), "tile order")

    m = contexts(w)
    step(m, w, w.traj); step(m, w, w.traj)
    ev = w.events
    m.set_events(EventPacket(ev.x[:60].copy(), ev.y[:60].copy(), ev.polarity[:60].copy(), ev.t_ns[:60].copy()))
    n_inl, P = m.step(w.traj, w.thres_valid_pixel, w.alpha)
    assert (n_inl, P) == (0, 0) and m.get_option("prep_in_warp") == 0, "empty window"
    m.set_events(w.events)
    same(step(m, w, w.traj), fresh(contexts, w, w.traj), "the window after the empty one")

    m = contexts(w)       # an evaluation nobody forms leaves its sums in the lines: the next evaluation clears them in the launch in front
    step(m, w, w.traj); step(m, w, w.traj)
    m.eval_launch(moved(w.traj, None, 1e-2)); m.eval_finish(sync=False)
    r = step(m, w, w.traj)
    assert r["in_warp"] == 0, "unclean lines"
    same(r, fresh(contexts, w, w.traj), "unclean lines")
