"""One frame aligned to another on the MI355X, and the rotation graph through its C entry (include/emba_hip.h: emba_frames_pair_eval, emba_frames_pair_align,
emba_rotation_graph_solve) against the numpy forms of the same rules (emba_amd.io: pair_terms, pair_sums, pair_align, rotation_graph_solve).
The seam is uv_out: fed the device's uv, numpy gives the counts as equal integers and the residuals bit for bit; the sums are Jacobian-derived and held to
tests/test_gpu_align.py's bound for its sums, 1e-5 relative to sum |terms| of each sum with a floor of 1e-12 of the array's scale.  Then the loop against the
evaluation and against numpy's loop (tests/pair_cases.py has the figures, measured with numpy), determinism, the chunk edge, every refusal and what a call
leaves alone, the closing case, and examples/run_ba.py --track-close."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import pair_cases as PC
import view_cases as VC
from emba_amd import _lib
from emba_amd import io as eio
from emba_amd import so3, synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_INVALID_ARG = 1
SUM_REL, SUM_FLOOR = 1e-5, 1e-12      # tests/test_gpu_align.py's bound for its sums
ITERS_SLACK = 1                       # tests/track_cases.py's allowance: one trial per item and loop
_dp, _u8p, _i32p, _u64p = (C.POINTER(t) for t in (C.c_double, C.c_uint8, C.c_int32, C.c_uint64))


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from emba_amd import build
    build.build_hip()
    return True


def make_legm(sensor, pano=PC.PANO, lut=None):
    from emba_amd import LEGM
    return LEGM(sensor[0], sensor[1], VC.lut_of(sensor) if lut is None else lut, 0.2, pano[0], pano[1], device=0)


def ptr(a, ty):
    return None if a is None else a.ctypes.data_as(ty)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def sums_distance(got, want, scale):
    allow = SUM_REL * scale + SUM_FLOOR * max(float(np.abs(want).max()), 1e-300)
    return float((np.abs(got - want) / allow).max())


def small_case(sensor, F=4, seed=7):
    """F frames of random smooth bytes (a fifth of them zeroed, so that skip_zero has pixels to mask and to skip), the wide pinhole, a lens, and rotations a
    few pixels apart."""
    sw, sh = sensor
    rng = np.random.default_rng(seed + sw)
    x, y = np.meshgrid(np.arange(sw), np.arange(sh))
    frames = np.array([np.clip(128 + 90 * np.sin(0.3 * x + f) * np.cos(0.4 * y - f) + rng.normal(0, 4, (sh, sw)), 1, 255) for f in range(F)]).astype(np.uint8)
    frames.reshape(-1)[::5] = 0
    calib = eio.pair_calib(0.5 * sw, 0.55 * sw, 0.5 * (sw - 1), 0.5 * (sh - 1), PC.LENS_D)
    return frames, VC.lut_of(sensor), calib


PAIR_SETS = {1: [(0, 1)], 3: [(2, 2), (1, 3), (1, 3)]}      # P = 1; P = 3 with i = j and a pair listed twice


@pytest.mark.parametrize("sensor", ((64, 48), (20, 13)), ids=lambda s: f"sensor{s[0]}x{s[1]}")
@pytest.mark.parametrize("P", (1, 3))
def test_every_evaluation_against_the_numpy_forms(gpu, sensor, P):
    sw, sh = sensor
    frames, lut, calib = small_case(sensor)
    m = make_legm(sensor, lut=lut)
    m.set_option("poison", 1)
    pairs = PAIR_SETS[P]
    rng = np.random.default_rng(P)
    Q = np.array([so3.exp(rng.normal(0, 0.06, 3)) for _ in pairs])
    if P == 3:
        Q[2] = Q[1]
    seen, worst = np.zeros(4, np.int64), 0.0
    for cal in (calib, dict(calib, D=None)):
        for gain, bias in ((None, None), (np.array([0.8, 1.3, 1.3])[:P], np.array([-6.0, 9.0, 9.0])[:P])):      # (the pair listed twice: the same exposure twice)
            for skip_zero in (False, True):
                for huber_k in (0.0, 12.0):
                    what = f"{sensor}, P = {P}, D = {cal['D'] is not None}, exposure = {gain is not None}, skip_zero = {skip_zero}, huber_k = {huber_k}"
                    g = m.pair_eval(frames, pairs, Q, cal, gain=gain, bias=bias, skip_zero=skip_zero, huber_k=huber_k, want_uv=True, want_resid=True)
                    for p, (i, j) in enumerate(pairs):
                        t = eio.pair_terms(frames[i], frames[j], g["uv"][p], lut, Q[p], cal, 1.0 if gain is None else gain[p], 0.0 if bias is None else bias[p],
                                           skip_zero, huber_k)
                        s, n, scale = eio.pair_sums(t, with_scale=True)
                        assert np.array_equal(g["counts"][p], n) and n.sum() == sw * sh, what
                        assert np.array_equal(bits(g["resid"][p]), bits(t["r"])), what
                        d = sums_distance(g["sums"][p], s, scale)
                        worst = max(worst, d)
                        assert d <= 1.0, (what, p, d)
                        seen += n
                    # numpy's own uv agrees with the device's to rounding
                    uv_np = eio.pair_project(lut, Q[0], cal)[1]
                    ok = np.isfinite(uv_np).all(axis=1)
                    assert np.array_equal(ok, np.isfinite(g["uv"][0]).all(axis=1)) and np.abs(uv_np[ok] - g["uv"][0][ok]).max() < 1e-9, what
                    if P == 3:      # the pair listed twice gives the same bits twice
                        assert np.array_equal(bits(g["sums"][1]), bits(g["sums"][2])) and np.array_equal(bits(g["resid"][1]), bits(g["resid"][2])), what
    print(f"{sensor}, P = {P}: worst |sums_device - sums_numpy| = {worst * SUM_REL:.3e} of sum |terms| (allowed {SUM_REL:.0e}); classes seen {seen.tolist()}")
    assert seen[0] > 0 and seen[1] > 0 and seen[2] > 0 and (P == 1 or seen[3] > 0)
    m.close()


def test_identity_pair_on_the_ideal_table(gpu):
    """(i, i) at Q = identity behind the pinhole of focal length 32: uv is the pixel exactly, r = 0 on every used pixel, the counts are the closed form."""
    c = PC.case(False)
    m = make_legm(PC.SENSOR)
    g = m.pair_eval(c["frames"].reshape(PC.F, PC.SH, PC.SW), [(5, 5)], [[0.0, 0.0, 0.0, 1.0]], c["calib"], want_uv=True, want_resid=True)
    xs, ys = np.meshgrid(np.arange(PC.SW, dtype=np.float64), np.arange(PC.SH, dtype=np.float64))
    assert np.array_equal(g["uv"][0, :, 0], xs.ravel()) and np.array_equal(g["uv"][0, :, 1], ys.ravel())
    assert g["counts"][0].tolist() == [(PC.SW - 1) * (PC.SH - 1), PC.SW + PC.SH - 1, 0, 0] and not g["resid"].any() and g["sums"][0, 9] == 0.0 and g["sums"][0, 0] > 0.0
    back = m.pair_eval(c["frames"].reshape(PC.F, PC.SH, PC.SW), [(5, 5)], [[0.0, 1.0, 0.0, 0.0]], c["calib"], want_uv=True)      # half a turn: rb_z < 0 everywhere
    assert back["counts"][0].tolist() == [0, PC.SW * PC.SH, 0, 0] and np.isnan(back["uv"]).all() and not back["sums"].any()
    m.close()


@pytest.mark.parametrize("lens", (False, True))
def test_the_loop_against_the_evaluation_and_numpy(gpu, lens):
    c = PC.case(lens)
    m = make_legm(PC.SENSOR, lut=c["lut"])
    m.set_option("poison", 1)
    fr = c["frames"].reshape(PC.F, PC.SH, PC.SW)
    pairs = list(PC.ALIGN_PAIRS)
    Q0 = np.array([PC.start_off(PC.true_pair(c, *p), PC.START_CELLS * PC.CELL) for p in pairs])
    start = m.pair_eval(fr, pairs, Q0, c["calib"], skip_zero=True)
    r0 = m.pair_align(fr, pairs, Q0, c["calib"], skip_zero=True, **dict(PC.SETTINGS, max_iters=0))
    assert np.array_equal(bits(r0["q"]), bits(Q0)) and (r0["status"] == eio.ALIGN_ITERATIONS).all() and (r0["iters"] == 0).all()
    assert np.array_equal(bits(r0["sums"]), bits(start["sums"])) and np.array_equal(r0["counts"], start["counts"])
    assert np.array_equal(bits(r0["cost0"]), bits(start["sums"][:, 9])) and np.array_equal(r0["n0"], start["counts"][:, 0])
    for iters in (1, 3, PC.SETTINGS["max_iters"]):
        r = m.pair_align(fr, pairs, Q0, c["calib"], skip_zero=True, **dict(PC.SETTINGS, max_iters=iters))
        e = m.pair_eval(fr, pairs, r["q"], c["calib"], skip_zero=True)
        assert np.array_equal(bits(r["sums"]), bits(e["sums"])) and np.array_equal(r["counts"], e["counts"]), iters
    assert np.array_equal(bits(r["info"]), bits(eio.pair_information(r["sums"], r["counts"])))
    for k, pair in enumerate(pairs):
        ref = PC.align_numpy(lens, pair, PC.START_CELLS)
        err = PC.end_angle(lens, pair, r["q"][k])
        print(f"lens {lens} pair {pair}: device {err:.4e} rad, numpy {PC.END_NP[(lens, pair)]:.4e} (bound {PC.angle_bound(lens, pair):.4e}); trials {r['iters'][k]} / "
              f"{ref['iters'][0]}, status {r['status'][k]} / {ref['status'][0]}")
        assert r["status"][k] == ref["status"][0] and abs(int(r["iters"][k]) - int(ref["iters"][0])) <= ITERS_SLACK
        assert err <= PC.angle_bound(lens, pair)
        assert float(eio.rotation_angle_between(ref["q"][0], r["q"][k])[0]) <= PC.angle_bound(lens, pair)
        assert r["n0"][k] == ref["n0"][0] and r["cost0"][k] == pytest.approx(ref["cost0"][0], rel=1e-9)
    m.close()


def test_determinism_and_independence(gpu):
    """The same calls twice, and once more after other stages ran in between: the same bits in every output; a pair's sums do not depend on the pairs around it."""
    c = PC.case(True)
    m = make_legm(PC.SENSOR, lut=c["lut"])
    fr = c["frames"].reshape(PC.F, PC.SH, PC.SW)
    pairs = eio.pair_candidates(*PC.drifted(), **PC.CANDIDATES)
    Q0, a, b = eio.pair_start(PC.drifted()[0], np.linspace(1.0, 1.2, PC.F), np.linspace(0.0, 5.0, PC.F), pairs)
    ev = lambda: m.pair_eval(fr, pairs, Q0, c["calib"], gain=a, bias=b, skip_zero=True, huber_k=9.0, want_uv=True, want_resid=True)      # noqa: E731
    al = lambda: m.pair_align(fr, pairs, Q0, c["calib"], gain=a, bias=b, skip_zero=True, **dict(PC.SETTINGS, huber_k=9.0))      # noqa: E731
    e1, a1, e2, a2 = ev(), al(), ev(), al()
    m.track_frames(fr, c["ts"], levels=(1, 0), max_iters=2)
    e3, a3 = ev(), al()
    assert np.abs(e1["sums"]).max() > 0 and (a1["iters"] > 0).all()
    for x, others in ((e1, (e2, e3)), (a1, (a2, a3))):
        for y in others:
            for k, v in x.items():
                assert np.array_equal(bits(v), bits(y[k])) if v.dtype == np.float64 else np.array_equal(v, y[k]), k
    one = m.pair_eval(fr, pairs[17:18], Q0[17:18], c["calib"], gain=a[17:18], bias=b[17:18], skip_zero=True, huber_k=9.0)
    assert np.array_equal(bits(one["sums"][0]), bits(e1["sums"][17]))
    one = m.pair_align(fr, pairs[17:18], Q0[17:18], c["calib"], gain=a[17:18], bias=b[17:18], skip_zero=True, **dict(PC.SETTINGS, huber_k=9.0))
    assert np.array_equal(bits(one["q"][0]), bits(a1["q"][17])) and one["iters"][0] == a1["iters"][17]
    m.close()


def test_chunk_edge(gpu):
    """65 535 + 2 pairs over two 8 x 8 frames: two chunks.  The pairs on both sides of the cut give the bits of the same pairs in a small call."""
    sensor = (8, 8)
    P = 65535 + 2
    rng = np.random.default_rng(65537)
    frames = rng.integers(0, 256, (2, 8, 8)).astype(np.uint8)
    calib = eio.pair_calib(4.0, 4.0, 3.5, 3.5, PC.LENS_D)
    pairs = rng.integers(0, 2, (P, 2)).astype(np.int32)
    Q = np.array([0.0, 0.0, 0.0, 1.0]) + rng.normal(0, 0.05, (P, 4))
    Q /= np.linalg.norm(Q, axis=1)[:, None]
    gain, bias = rng.uniform(0.8, 1.2, P), rng.uniform(-5, 5, P)
    m = make_legm(sensor, (32, 16))
    m.set_option("poison", 1)
    kw = dict(gain=gain, bias=bias, skip_zero=True, huber_k=20.0)
    big = m.pair_eval(frames, pairs, Q, calib, **kw)
    edge = slice(65535 - 3, P)
    small = m.pair_eval(frames, pairs[edge], Q[edge], calib, gain=gain[edge], bias=bias[edge], skip_zero=True, huber_k=20.0)
    assert np.array_equal(bits(big["sums"][edge]), bits(small["sums"])) and np.array_equal(big["counts"][edge], small["counts"])
    assert (big["counts"].sum(axis=1) == 64).all() and big["counts"][:, 0].sum() > P and np.abs(small["sums"]).max() > 0
    s = dict(PC.SETTINGS, max_iters=2, min_pixels=3, huber_k=20.0)
    bigl = m.pair_align(frames, pairs, Q, calib, gain=gain, bias=bias, skip_zero=True, **s)
    smalll = m.pair_align(frames, pairs[edge], Q[edge], calib, gain=gain[edge], bias=bias[edge], skip_zero=True, **s)
    for k in ("q", "sums", "info"):
        assert np.array_equal(bits(bigl[k][edge]), bits(smalll[k])), k
    for k in ("status", "iters", "counts", "n0"):
        assert np.array_equal(bigl[k][edge], smalll[k]), k
    assert set(bigl["status"].tolist()) <= {1, 2, 3, 4} and (bigl["iters"] <= 2).all() and bigl["iters"].max() == 2
    m.close()


def test_refusals_and_what_a_call_leaves_alone(gpu):
    """Every refusal leaves the outputs untouched, and so it and the calls themselves leave the context: the mosaic's sums, the level planes, the step
    path's ep and the resident map, bit for bit before and after."""
    w = synth.make_scene_workload()          # 64x48 on 256x512
    S, F, P = 64 * 48, 4, 3
    m = make_legm((64, 48), (512, 256), lut=w.lut)
    m.set_events(w.events)
    m.upload_map(w.Gx, w.Gy)
    first = m.step(w.traj, w.thres_valid_pixel, w.alpha)
    ep0, map0 = m.get_ep(), m.downloadMap()
    frames = np.random.default_rng(3).integers(1, 256, (F, 48, 64)).astype(np.uint8)
    m.track_frames(frames, np.array([10, 20, 30, 40], np.int64), levels=(2, 0), batch=2, max_iters=2)
    planes0 = [m.track_level(l) for l in (2, 0)]
    mosaic0 = m.mosaic()
    L = m._L
    out = dict(sums=np.full((P, 10), 4.25), counts=np.full((P, 4), 77, np.uint64), uv=np.full((P, S, 2), -1.5), resid=np.full((P, S), 2.5), q=np.full((P, 4), 3.5),
               status=np.full(P, 9, np.int32), iters=np.full(P, 8, np.int32), cost0=np.full(P, 1.5), n0=np.full(P, 55, np.uint64), info=np.full((P, 6), 6.5))
    vals = dict(sums=4.25, counts=77, uv=-1.5, resid=2.5, q=3.5, status=9, iters=8, cost0=1.5, n0=55, info=6.5)
    pairs = np.array([[0, 1], [2, 2], [3, 0]], np.int32)
    Q = np.tile(np.array([0.0, 0.0, 0.0, 1.0]), (P, 1))
    ones, zeros = np.ones(P), np.zeros(P)
    good = dict(eio.ALIGN_DEFAULTS, max_iters=2)

    def context_untouched():
        planes = [m.track_level(l) for l in (2, 0)]
        mosaic = m.mosaic()
        again = m.step(w.traj, w.thres_valid_pixel, w.alpha)
        map1 = m.downloadMap()
        return (all(np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1]) for x, y in zip(planes0, planes))
                and np.array_equal(mosaic["sum_w"], mosaic0["sum_w"]) and np.array_equal(mosaic["sum_v"], mosaic0["sum_v"])
                and again == first and np.array_equal(bits(m.get_ep()), bits(ep0)) and np.array_equal(bits(map0[0]), bits(map1[0]))
                and np.array_equal(bits(map0[1]), bits(map1[1])))

    def untouched():
        return all((out[k] == v).all() for k, v in vals.items())

    def call_eval(fr=frames, F_=F, pr=pairs, P_=P, Q_=Q, gain=ones, bias=zeros, fu=32.0, fv=32.0, cu=31.5, cv=23.5, D=None, huber_k=0.0):
        return L.emba_frames_pair_eval(m._ctx, ptr(fr, _u8p), F_, ptr(pr, _i32p), P_, ptr(Q_, _dp), ptr(gain, _dp), ptr(bias, _dp), fu, fv, cu, cv, ptr(D, _dp), 1, huber_k,
                                       ptr(out["sums"], _dp), ptr(out["counts"], _u64p), ptr(out["uv"], _dp), ptr(out["resid"], _dp))

    def call_loop(fr=frames, F_=F, pr=pairs, P_=P, Q_=Q, gain=ones, bias=zeros, fu=32.0, fv=32.0, cu=31.5, cv=23.5, D=None, null_settings=False, **kw):
        s = dict(good, **kw)
        cs = _lib.EmbaAlignSettings(int(s["max_iters"]), int(s["min_pixels"]), s["lambda0"], s["lambda_up"], s["lambda_down"], s["lambda_min"], s["lambda_max"],
                                    s["tol_rot"], s["huber_k"])
        return L.emba_frames_pair_align(m._ctx, ptr(fr, _u8p), F_, ptr(pr, _i32p), P_, ptr(Q_, _dp), ptr(gain, _dp), ptr(bias, _dp), fu, fv, cu, cv, ptr(D, _dp), 1,
                                        None if null_settings else C.addressof(cs), ptr(out["q"], _dp), ptr(out["sums"], _dp), ptr(out["counts"], _u64p),
                                        ptr(out["status"], _i32p), ptr(out["iters"], _i32p), ptr(out["cost0"], _dp), ptr(out["n0"], _u64p), ptr(out["info"], _dp))

    nan, inf = float("nan"), float("inf")
    at = lambda base, idx, v: (lambda a: (a.__setitem__(idx, v), a)[1])(base.copy())      # noqa: E731
    refused = [dict(fr=None), dict(pr=None), dict(Q_=None), dict(P_=1 << 31), dict(pr=at(pairs, (1, 0), F)), dict(pr=at(pairs, (2, 1), -1)), dict(F_=2),
               dict(Q_=at(Q, (1, 2), nan)), dict(Q_=at(Q, (0, 0), inf)), dict(Q_=at(Q, 2, 0.0)), dict(gain=at(ones, 1, 0.0)), dict(gain=at(ones, 1, -1.0)),
               dict(gain=at(ones, 0, nan)), dict(gain=at(ones, 2, inf)), dict(bias=at(zeros, 1, nan)), dict(bias=at(zeros, 2, -inf)), dict(fu=0.0), dict(fv=-1.0),
               dict(fu=nan), dict(fv=inf), dict(cu=nan), dict(cv=inf), dict(D=np.array([0.0, nan, 0.0, 0.0, 0.0]))]
    for call in (call_eval, call_loop):
        for kw in refused:
            assert call(**kw) == ERR_INVALID_ARG and untouched(), (call.__name__, kw)
        many = (1 << 30) // S + 1
        assert call(F_=many) == ERR_INVALID_ARG and untouched() and b"resident sequence" in L.emba_last_error(m._ctx)
        assert call(P_=0, fr=None, pr=None, Q_=None) == 0 and untouched()      # P = 0: nothing launched, nothing written
    assert call_eval(huber_k=nan) == ERR_INVALID_ARG and call_loop(huber_k=nan) == ERR_INVALID_ARG and call_loop(null_settings=True) == ERR_INVALID_ARG and untouched()
    for kw in (dict(max_iters=-1), dict(lambda_up=1.0), dict(lambda_down=0.5), dict(lambda0=0.0), dict(lambda0=nan), dict(min_pixels=2), dict(tol_rot=-1.0),
               dict(lambda_min=-1.0), dict(lambda_max=nan)):
        assert call_loop(**kw) == ERR_INVALID_ARG and untouched(), kw
    assert context_untouched()
    # the calls themselves still go, with and without the exposure and the lens, and leave the context alone
    assert call_eval() == 0 and call_loop() == 0 and not untouched()
    assert call_eval(gain=None, bias=None, D=np.array(PC.LENS_D)) == 0 and call_loop(gain=None, bias=None, D=np.array(PC.LENS_D)) == 0
    assert (out["counts"].sum(axis=1) == S).all() and set(out["status"].tolist()) <= {1, 2, 3, 4}
    assert context_untouched()
    m.close()


def test_rotation_graph_through_the_c_entry(gpu):
    """emba_rotation_graph_solve on the recorded closing case, edges from numpy's pairs: within ten times the recorded spread of numpy's solve; the refusals
    by status with the frame they name; the anchor's bits."""
    from emba_amd.legm import LEGM
    r = PC.closing_numpy()
    q, status = PC.drifted()
    k = r["keep"]
    ed, Qe, info = r["pairs"][k], r["align"]["q"][k], r["info"][k]
    g = LEGM.rotation_graph_solve(q, status, ed, Qe, info)
    d = float(eio.rotation_angle_between(r["graph"]["q"], g["q"]).max())
    print(f"C against numpy: {d:.3e} rad (allowed {10.0 * PC.GRAPH_SPREAD:.1e}); worst angle to the truth {PC.worst_angle(g['q']):.4e}; C", {a: b for a, b in g.items() if a != "q"})
    assert d <= 10.0 * PC.GRAPH_SPREAD and g["end"] == r["graph"]["end"] == eio.GRAPH_CONVERGED and np.array_equal(bits(g["q"][0]), bits(q[0]))
    assert PC.worst_angle(g["q"]) == pytest.approx(PC.E_AFTER_NP, rel=1e-3)
    g2 = LEGM.rotation_graph_solve(q, status, ed, Qe, info)
    assert np.array_equal(bits(g["q"]), bits(g2["q"])) and g["cg_iters"] == g2["cg_iters"]
    p = PC.permuted(len(ed))
    gp = LEGM.rotation_graph_solve(q, status, ed[p], Qe[p], info[p])
    assert float(eio.rotation_angle_between(gp["q"], g["q"]).max()) <= 10.0 * PC.GRAPH_SPREAD
    with pytest.raises(_lib.EmbaError, match="no anchor"):
        LEGM.rotation_graph_solve(q, np.full(PC.F, 2, np.int32), ed, Qe, info)
    far = (ed >= 6).all(axis=1)
    with pytest.raises(_lib.EmbaError, match="frame 6 ") as ei:
        LEGM.rotation_graph_solve(q, status, ed[far], Qe[far], info[far])
    assert ei.value.at == 6 and ei.value.status == ERR_INVALID_ARG
    with pytest.raises(_lib.EmbaError, match="outside"):
        LEGM.rotation_graph_solve(q, status, [[0, PC.F]], Qe[:1], info[:1])
    bad = info.copy()
    bad[3, 2] = np.inf
    with pytest.raises(_lib.EmbaError, match="not finite"):
        LEGM.rotation_graph_solve(q, status, ed, Qe, bad)


def test_the_closing_case_on_the_device(gpu):
    """Candidates -> LEGM.pair_align -> the kept pairs -> the graph, through driver.close_tracked_frames: the pairs' codes are numpy's, the trials within the
    allowance, and the worst angle to the truth ends within the project's bound of numpy's figure; the mosaic in the context is the stitch at the new
    rotations."""
    from emba_amd.driver import SequenceSettings, close_tracked_frames
    c = PC.case(False)
    ref = PC.closing_numpy()
    q, status = PC.drifted()
    m = make_legm(PC.SENSOR, lut=c["lut"])
    fr = c["frames"].reshape(PC.F, PC.SH, PC.SW)
    seq = SequenceSettings(1.0, 1.0, track_close=True, close_window=PC.CANDIDATES["window"], close_gap=PC.CANDIDATES["min_gap"], close_angle=PC.CANDIDATES["max_angle"],
                           close_per_frame=PC.CANDIDATES["max_per_frame"], close_min_overlap=PC.MIN_OVERLAP)
    tracked = dict(q=q.copy(), status=status.copy(), tracked=PC.F - 1, lost=0)
    kw = dict(levels=(1, 0), batch=1, skip_zero=True, min_weight=256, min_overlap=0.3, **PC.SETTINGS)
    r = close_tracked_frames(m, fr, c["ts"], tracked, seq, c["calib"], **kw)
    after = PC.worst_angle(r["q"])
    bound = 2.0 * PC.E_AFTER_NP + PC.F * PC.SETTINGS["tol_rot"]
    print(f"device: {len(r['pairs'])} pairs, {int(r['pair_kept'].sum())} kept; worst angle {PC.worst_angle(q):.4e} -> {after:.4e} rad (numpy {PC.E_AFTER_NP:.4e}, bound "
          f"{bound:.4e}); graph {r['graph']}")
    assert np.array_equal(r["pairs"], ref["pairs"]) and np.array_equal(r["pair_status"], ref["align"]["status"]) and r["pair_kept"].all()
    assert after <= bound and after < 0.01 * PC.E_BEFORE_NP and np.array_equal(bits(r["q"][0]), bits(q[0]))
    assert r["graph"]["end"] == eio.GRAPH_CONVERGED
    stitched = [m.track_level(l) for l in (1, 0)]
    m2 = make_legm(PC.SENSOR, lut=c["lut"])
    m2.refit_frames(fr, c["ts"], r["q"], status, sweeps=0, **kw)
    for (a_w, a_v), l in zip(stitched, (1, 0)):
        b_w, b_v = m2.track_level(l)
        assert np.array_equal(a_w, b_w) and np.array_equal(a_v, b_v) and a_w.any()
    same = close_tracked_frames(m, fr, c["ts"], tracked, SequenceSettings(1.0, 1.0), c["calib"], **kw)
    assert same is tracked      # off by default: nothing happens
    m.close()
    m2.close()


def test_run_ba_closes_the_tracked_frames(gpu, tmp_path):
    """examples/run_ba.py --demo with --views-hz writes frames; a second run takes them with --init-poses frames --track-close --init-map frames: it runs to the
    end, frames_pairs.txt has one line per pair with the stated columns, and the flag is refused without --init-poses frames."""
    out1, out2 = tmp_path / "out1", tmp_path / "out2"
    exe = [sys.executable, os.path.join(ROOT, "examples", "run_ba.py")]
    r = subprocess.run(exe + ["--demo", str(out1), "--views-hz", "50", "--window-size", "0.5", "--max-iter", "3"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    lo, hi = open(out1 / "views" / "tone.txt").read().split()
    n_frames = len(open(out1 / "views" / "times.txt").read().splitlines())
    common = ["--frames", str(out1 / "views"), "--init-poses", "frames", "--init-map", "frames", "--track-levels", "3,2,1", "--track-batch", "2", "--track-predict", "1",
              "--track-min-overlap", "0.3", "--track-q0", "0,0,0,1", "--window-size", "0.5", "--frames-log", "0", "--frames-lo", lo, "--frames-hi", hi,
              "--frames-skip-zero", "--max-iter", "3"]
    r = subprocess.run(exe + ["--demo", str(out2)] + common + ["--track-close", "--close-window", "2", "--close-gap", "3", "--close-angle", "0.3", "--close-per-frame", "2",
                                                               "--close-huber", "10"], capture_output=True, text=True, timeout=600)
    print(r.stdout[-3000:])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "init-poses frames:" in r.stdout and "track-close:" in r.stdout and "initial map from" in r.stdout
    lines = open(out2 / "frames_pairs.txt").read().splitlines()
    assert lines[0].startswith("# i j status(")
    rows = [l.split() for l in lines if l and not l.startswith("#")]
    assert len(rows) >= 1 and all(len(x) == 7 for x in rows)
    ij = np.array([[int(x[0]), int(x[1])] for x in rows])
    assert (ij[:, 0] < ij[:, 1]).all() and ij.min() >= 0 and ij.max() < n_frames and {int(x[2]) for x in rows} <= {1, 2, 3, 4} and any(int(x[6]) for x in rows)
    assert all(int(x[3]) >= 0 and float(x[4]) >= 0.0 and float(x[5]) >= 0.0 for x in rows)
    assert (out2 / "refined_traj.txt").exists() and (out2 / "frames_tracked.txt").exists()
    r = subprocess.run(exe + ["--demo", str(tmp_path / "out3"), "--window-size", "0.5", "--track-close"], capture_output=True, text=True, timeout=600)
    assert r.returncode != 0 and "--track-close" in r.stderr
