"""The pair alignment coarse to fine on the MI355X, with the pair's exposure estimated (include/emba_hip.h: emba_frames_pair_level_eval,
emba_frames_pair_align_levels) against the numpy forms of the same rules (emba_amd.io: pair_level_bytes, pair_level_lut, pair_level_calib,
pair_exposure_terms, pair_exposure_sums, pair_align_levels) and against the existing entry points.  The level bytes are equal integers and the level table
has numpy's bits; the seam of an evaluation is uv_out, as in tests/test_gpu_pair.py: fed the device's uv, numpy gives the counts as equal integers and the
residuals bit for bit; the 21 sums are held to that file's bound, 1e-5 relative to sum |terms| of each sum with a floor of 1e-12 of the array's scale.  Then the
two identities, the loop against numpy's (tests/pair_level_cases.py has the figures, measured with numpy), determinism, the chunk edge, every refusal and what
a call leaves alone, the driver and examples/run_ba.py."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import pair_cases as PC
import pair_level_cases as LC
import view_cases as VC
from emba_amd import _lib
from emba_amd import io as eio
from emba_amd import so3, synth
from test_gpu_pair import ERR_INVALID_ARG, ITERS_SLACK, PAIR_SETS, bits, make_legm, ptr, small_case, sums_distance

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_dp, _u8p, _i32p, _u64p = (C.POINTER(t) for t in (C.c_double, C.c_uint8, C.c_int32, C.c_uint64))
LEVELS = {(64, 48): (0, 1, 3), (20, 13): (0, 1, 2)}      # 64 x 48: 8 x 6 at level 3; 20 x 13: 10 x 6 and 5 x 3 (15 pixels, below one wave)


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from emba_amd import build
    build.build_hip()
    return True


def same(x, y, keys=None):
    for k in keys or x.keys():
        v, w = x[k], y[k]
        if v is None:
            assert w is None, k
        else:
            assert np.array_equal(bits(v), bits(w)) if v.dtype == np.float64 else np.array_equal(v, w), k


@pytest.mark.parametrize("sensor", ((64, 48), (20, 13)), ids=lambda s: f"sensor{s[0]}x{s[1]}")
@pytest.mark.parametrize("P", (1, 3))
def test_every_level_against_the_numpy_forms(gpu, sensor, P):
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
    for level in LEVELS[sensor]:
        wl, hl = eio.pair_level_size(sensor, level)
        for cal in (calib, dict(calib, D=None)):
            for gain, bias in ((None, None), (np.array([0.8, 1.3, 1.3])[:P], np.array([-6.0, 9.0, 9.0])[:P])):
                for skip_zero in (False, True):
                    for huber_k in (0.0, 12.0):
                        what = f"{sensor}, level {level}, P = {P}, D = {cal['D'] is not None}, exposure = {gain is not None}, skip_zero = {skip_zero}, huber_k = {huber_k}"
                        g = m.pair_level_eval(frames, pairs, Q, cal, level, gain=gain, bias=bias, skip_zero=skip_zero, huber_k=huber_k, want_uv=True, want_resid=True,
                                              want_level=True)
                        fb, tl, cl = eio.pair_level_bytes(frames, level, skip_zero), eio.pair_level_lut(lut, sensor, level), eio.pair_level_calib(cal, level)
                        assert g["level_bytes"].shape == (len(frames), hl, wl) and np.array_equal(g["level_bytes"], fb), what
                        assert np.array_equal(bits(g["level_lut"]), bits(tl)), what
                        for p, (i, j) in enumerate(pairs):
                            t = eio.pair_exposure_terms(fb[i].reshape(-1), fb[j], g["uv"][p], tl, Q[p], cl, 1.0 if gain is None else gain[p],
                                                        0.0 if bias is None else bias[p], skip_zero, huber_k)
                            s, n, scale = eio.pair_exposure_sums(t, with_scale=True)
                            assert np.array_equal(g["counts"][p], n) and n.sum() == wl * hl, what
                            assert np.array_equal(bits(g["resid"][p]), bits(t["r"])), what
                            d = sums_distance(g["sums"][p], s, scale)
                            worst = max(worst, d)
                            assert d <= 1.0, (what, p, d)
                            seen += n
                        uv_np = eio.pair_project(tl, Q[0], cl)[1]
                        ok = np.isfinite(uv_np).all(axis=1)
                        assert np.array_equal(ok, np.isfinite(g["uv"][0]).all(axis=1)) and np.abs(uv_np[ok] - g["uv"][0][ok]).max() < 1e-9, what
                        if P == 3:      # the pair listed twice gives the same bits twice
                            assert np.array_equal(bits(g["sums"][1]), bits(g["sums"][2])) and np.array_equal(bits(g["resid"][1]), bits(g["resid"][2])), what
                        if level == 0:      # the second identity: level 0 is emba_frames_pair_eval's uv, residuals, counts and ten shared sums bit for bit
                            e = m.pair_eval(frames, pairs, Q, cal, gain=gain, bias=bias, skip_zero=skip_zero, huber_k=huber_k, want_uv=True, want_resid=True)
                            assert np.array_equal(bits(e["uv"]), bits(g["uv"])) and np.array_equal(bits(e["resid"]), bits(g["resid"])), what
                            assert np.array_equal(e["counts"], g["counts"]) and np.array_equal(bits(e["sums"]), bits(g["sums"][:, list(eio.EXPOSURE_SHARED)])), what
    print(f"{sensor}, P = {P}: worst |sums_device - sums_numpy| = {worst * 1e-5:.3e} of sum |terms| (allowed 1e-05); classes seen {seen.tolist()}")
    assert seen[0] > 0 and seen[1] > 0 and seen[2] > 0 and (P == 1 or seen[3] > 0)
    with pytest.raises(_lib.EmbaError, match="level 3 of a 20 x 13" if sensor == (20, 13) else "level 5 of a 64 x 48"):
        m.pair_level_eval(frames, pairs, Q, calib, 3 if sensor == (20, 13) else 5)
    m.close()


@pytest.mark.parametrize("lens", (False, True))
def test_schedule_zero_without_exposure_is_pair_align(gpu, lens):
    """The first identity: the schedule (0) with estimate = 0 is emba_frames_pair_align bit for bit — q, the ten shared sums, counts, status, iters, cost0, n0,
    info — from exposures that are given, under a Huber weight, and at max_iters = 0."""
    c = PC.case(lens)
    m = make_legm(PC.SENSOR, lut=c["lut"])
    m.set_option("poison", 1)
    fr = c["frames"].reshape(PC.F, PC.SH, PC.SW)
    pairs = list(PC.ALIGN_PAIRS) + [(2, 2)]
    Q0 = np.array([PC.start_off(PC.true_pair(c, *p), PC.START_CELLS * PC.CELL) for p in pairs])
    for kw in (dict(skip_zero=True), dict(skip_zero=True, gain=np.array([0.9, 1.1, 1.0]), bias=np.array([3.0, -4.0, 0.5]), huber_k=9.0), dict(max_iters=0)):
        s = dict(PC.SETTINGS, **{k: v for k, v in kw.items() if k in PC.SETTINGS})
        call = {k: v for k, v in kw.items() if k not in PC.SETTINGS}
        a = m.pair_align(fr, pairs, Q0, c["calib"], **call, **s)
        b = m.pair_align_levels(fr, pairs, Q0, c["calib"], levels=(0,), estimate=0, **call, **s)
        same(a, b, ("q", "counts", "status", "iters", "cost0", "n0", "info"))
        assert np.array_equal(bits(a["sums"]), bits(b["sums"][:, list(eio.EXPOSURE_SHARED)])) and (a["iters"] > 0).any() == (s["max_iters"] > 0)
        assert np.array_equal(b["level_status"][:, 0], b["status"]) and np.array_equal(b["level_iters"][:, 0], b["iters"])
        assert np.array_equal(bits(b["gain"]), bits(np.asarray(call.get("gain", np.ones(3))))) and np.array_equal(bits(b["bias"]), bits(np.asarray(call.get("bias", np.zeros(3)))))
    m.close()


@pytest.mark.parametrize("estimate", (0, 1, 2, 3))
def test_the_schedule_against_the_evaluation_and_numpy(gpu, estimate):
    """The loop over (2, 1, 0) on the fine plane, frame j under an exposure the pair is not told: the state the call returns is the evaluation at it on the last
    level; statuses equal numpy's per level, trials within the allowance per level, the angle within the bound around numpy's end, gain and bias within
    tests/pair_level_cases.py's bound."""
    c = LC.case()
    m = make_legm(LC.SENSOR, lut=c["lut"])
    m.set_option("poison", 1)
    fr = LC.exposure_frames().reshape(LC.F, LC.SH, LC.SW)
    Q0 = [LC.start(LC.EXPOSURE_CELLS)]
    ref = LC.align_numpy(LC.SCHEDULE, LC.EXPOSURE_CELLS, estimate, True)
    r = m.pair_align_levels(fr, [LC.PAIR], Q0, c["calib"], levels=LC.SCHEDULE, estimate=estimate, skip_zero=True, **LC.SETTINGS)
    e = m.pair_level_eval(fr, [LC.PAIR], r["q"], c["calib"], LC.SCHEDULE[-1], gain=r["gain"], bias=r["bias"], skip_zero=True)
    assert np.array_equal(bits(r["sums"]), bits(e["sums"])) and np.array_equal(r["counts"], e["counts"])
    assert np.array_equal(bits(r["info"]), bits(eio.pair_information(r["sums"][:, list(eio.EXPOSURE_SHARED)], r["counts"])))
    first = m.pair_level_eval(fr, [LC.PAIR], Q0, c["calib"], LC.SCHEDULE[0], skip_zero=True)
    assert np.array_equal(bits(r["cost0"]), bits(first["sums"][:, 20])) and np.array_equal(r["n0"], first["counts"][:, 0])
    err, d = LC.end_angle(r["q"][0]), float(eio.rotation_angle_between(ref["q"][0], r["q"][0])[0])
    da, db = abs(r["gain"][0] - ref["gain"][0]), abs(r["bias"][0] - ref["bias"][0])
    print(f"estimate {estimate}: device {err:.4e} rad, numpy {LC.end_angle(ref['q'][0]):.4e}, apart {d:.3e} (bound {LC.angle_bound():.4e}); a {r['gain'][0]:.6f} b "
          f"{r['bias'][0]:.4f}, apart {da:.3e} {db:.3e} (bound {LC.ab_bound()}); status {r['level_status'][0].tolist()} / {ref['level_status'][0].tolist()}, trials "
          f"{r['level_iters'][0].tolist()} / {ref['level_iters'][0].tolist()}")
    assert np.array_equal(r["level_status"], ref["level_status"]) and r["status"][0] == ref["status"][0] and r["iters"][0] == r["level_iters"].sum()
    assert (np.abs(r["level_iters"].astype(int) - ref["level_iters"].astype(int)) <= ITERS_SLACK).all()
    assert d <= LC.angle_bound() and da <= LC.ab_bound()[0] and db <= LC.ab_bound()[1]
    assert r["n0"][0] == ref["n0"][0] and r["cost0"][0] == pytest.approx(ref["cost0"][0], rel=1e-9)
    if not estimate & eio.EXPOSURE_GAIN:
        assert r["gain"][0] == 1.0
    if not estimate & eio.EXPOSURE_BIAS:
        assert r["bias"][0] == 0.0
    if estimate == 3 and LC.EXPOSURE_IMPROVES:
        worse = m.pair_align_levels(fr, [LC.PAIR], Q0, c["calib"], levels=LC.SCHEDULE, estimate=0, skip_zero=True, **LC.SETTINGS)
        assert err <= LC.angle_bound() < LC.end_angle(worse["q"][0])
        assert abs(r["gain"][0] - LC.EXPOSURE_AB[0]) < 1e-5 and abs(r["bias"][0] - LC.EXPOSURE_AB[1]) < 1e-3      # (the recorded figures' own digits)
    m.close()


def test_the_basin_widens_on_the_device(gpu):
    """From LC.WIDE_CELLS off, level 0 alone does not come home and the schedule ends at level 0's own end point — asserted because numpy shows it."""
    if not LC.WIDENS:      # (numpy shows no widening: nothing to assert)
        return
    c = LC.case()
    m = make_legm(LC.SENSOR, lut=c["lut"])
    fr = c["frames"].reshape(LC.F, LC.SH, LC.SW)
    kw = dict(skip_zero=True, **LC.SETTINGS)
    own = m.pair_align_levels(fr, [LC.PAIR], [LC.start(1.0)], c["calib"], levels=(0,), **kw)
    alone = m.pair_align_levels(fr, [LC.PAIR], [LC.start(LC.WIDE_CELLS)], c["calib"], levels=(0,), **kw)
    sched = m.pair_align_levels(fr, [LC.PAIR], [LC.start(LC.WIDE_CELLS)], c["calib"], levels=LC.SCHEDULE, **kw)
    ref = LC.align_numpy(LC.SCHEDULE, LC.WIDE_CELLS)
    d = float(eio.rotation_angle_between(own["q"], sched["q"])[0])
    print(f"from {LC.WIDE_CELLS} cells: level 0 alone ends {LC.end_angle(alone['q'][0]):.3e} rad off, the schedule {LC.end_angle(sched['q'][0]):.3e} (bound "
          f"{LC.angle_bound():.3e}), {d:.3e} from level 0's own end point; status {sched['level_status'][0].tolist()} / {ref['level_status'][0].tolist()}")
    assert LC.end_angle(alone["q"][0]) > LC.angle_bound() >= LC.end_angle(sched["q"][0]) and LC.end_angle(own["q"][0]) <= LC.angle_bound()
    assert d <= LC.SETTINGS["tol_rot"] and np.array_equal(sched["level_status"], ref["level_status"])
    m.close()


def test_determinism_degenerate_end_and_other_stages(gpu):
    """The same calls twice, and once more after other stages ran in between: the same bits in every output.  A pair of a frame of one constant byte with
    estimate = 3 ends degenerate at its first level, where it started; the pairs beside it are the pairs of a call without it."""
    c = LC.case()
    m = make_legm(LC.SENSOR, lut=c["lut"])
    fr = LC.exposure_frames().reshape(LC.F, LC.SH, LC.SW).copy()
    fr[0] = 90
    pairs = np.array([(3, 10), (0, 5), (1, 4), (3, 10)], np.int32)
    Q0 = np.array([PC.start_off(PC.true_pair(c, *p), 1.5 * PC.CELL) for p in pairs])
    a0, b0 = np.array([1.0, 1.2, 1.0, 1.0]), np.array([0.0, 3.0, 0.0, 0.0])
    kw = dict(levels=(2, 0, 1), estimate=3, gain=a0, bias=b0, skip_zero=True, **dict(LC.SETTINGS, huber_k=9.0))
    al = lambda: m.pair_align_levels(fr, pairs, Q0, c["calib"], **kw)      # noqa: E731
    ev = lambda: m.pair_level_eval(fr, pairs, Q0, c["calib"], 1, gain=a0, bias=b0, skip_zero=True, huber_k=9.0, want_uv=True, want_resid=True, want_level=True)      # noqa: E731
    a1, e1, a2, e2 = al(), ev(), al(), ev()
    m.track_frames(fr, c["ts"], levels=(1, 0), max_iters=2)
    m.pair_align(fr, pairs, Q0, c["calib"], skip_zero=True, max_iters=2)
    a3, e3 = al(), ev()
    for x, others in ((a1, (a2, a3)), (e1, (e2, e3))):
        for y in others:
            same(x, y)
    assert (a1["iters"][[0, 2, 3]] > 0).all() and np.abs(e1["sums"]).max() > 0
    assert a1["status"][1] == eio.ALIGN_DEGENERATE and a1["level_status"][1].tolist() == [eio.ALIGN_DEGENERATE, 0, 0] and a1["iters"][1] == 0
    assert np.array_equal(bits(a1["q"][1]), bits(Q0[1])) and a1["gain"][1] == 1.2 and a1["bias"][1] == 3.0 and a1["n0"][1] == a1["counts"][1, 0] > 0
    assert (a1["level_status"][[0, 2, 3]] != 0).all() and np.array_equal(bits(a1["q"][0]), bits(a1["q"][3]))
    keep = [0, 2, 3]
    one = m.pair_align_levels(fr, pairs[keep], Q0[keep], c["calib"], **dict(kw, gain=a0[keep], bias=b0[keep]))
    for k in one:
        assert np.array_equal(bits(one[k]), bits(a1[k][keep])) if one[k].dtype == np.float64 else np.array_equal(one[k], a1[k][keep]), k
    m.close()


def test_chunk_edge(gpu):
    """65 535 + 2 pairs over two 8 x 8 frames, schedule (1, 0): two chunks.  The pairs on both sides of the cut give the bits of the same pairs in a small call."""
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
    edge = slice(65535 - 3, P)
    big = m.pair_level_eval(frames, pairs, Q, calib, 1, gain=gain, bias=bias, skip_zero=True, huber_k=20.0)
    small = m.pair_level_eval(frames, pairs[edge], Q[edge], calib, 1, gain=gain[edge], bias=bias[edge], skip_zero=True, huber_k=20.0)
    assert np.array_equal(bits(big["sums"][edge]), bits(small["sums"])) and np.array_equal(big["counts"][edge], small["counts"])
    assert (big["counts"].sum(axis=1) == 16).all() and big["counts"][:, 0].sum() > P and np.abs(small["sums"]).max() > 0
    s = dict(PC.SETTINGS, max_iters=2, min_pixels=3, huber_k=20.0)
    bigl = m.pair_align_levels(frames, pairs, Q, calib, levels=(1, 0), estimate=2, gain=gain, bias=bias, skip_zero=True, **s)
    smalll = m.pair_align_levels(frames, pairs[edge], Q[edge], calib, levels=(1, 0), estimate=2, gain=gain[edge], bias=bias[edge], skip_zero=True, **s)
    for k in bigl:
        assert np.array_equal(bits(bigl[k][edge]), bits(smalll[k])) if bigl[k].dtype == np.float64 else np.array_equal(bigl[k][edge], smalll[k]), k
    assert set(bigl["status"].tolist()) <= {1, 2, 3, 4} and (bigl["level_iters"] <= 2).all() and bigl["iters"].max() >= 2
    m.close()


def test_refusals_and_what_a_call_leaves_alone(gpu):
    """Every refusal, in the order the header states, leaves the outputs untouched, and so it and the calls themselves leave the context: the mosaic's sums,
    the level planes, the step path's ep and the resident map, bit for bit before and after."""
    w = synth.make_scene_workload()          # 64x48 on 256x512
    S, F, P, n = 64 * 48, 4, 3, 2
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
    vals = dict(sums=4.25, counts=77, uv=-1.5, resid=2.5, q=3.5, gain=0.5, bias=7.5, status=9, iters=8, lst=6, lit=5, cost0=1.5, n0=55, info=6.5, lb=3, ll=8.5)
    shapes = dict(sums=(P, 21), counts=(P, 4), uv=(P, S, 2), resid=(P, S), q=(P, 4), gain=(P,), bias=(P,), status=(P,), iters=(P,), lst=(P, n), lit=(P, n),
                  cost0=(P,), n0=(P,), info=(P, 6), lb=(F, S), ll=(S, 3))
    types = dict(counts=np.uint64, n0=np.uint64, status=np.int32, iters=np.int32, lst=np.int32, lit=np.int32, lb=np.uint8)
    out = {k: np.full(shapes[k], v, types.get(k, np.float64)) for k, v in vals.items()}
    pairs = np.array([[0, 1], [2, 2], [3, 0]], np.int32)
    Q = np.tile(np.array([0.0, 0.0, 0.0, 1.0]), (P, 1))
    ones, zeros = np.ones(P), np.zeros(P)
    good = dict(eio.ALIGN_DEFAULTS, max_iters=2)
    lv = np.array([1, 0], np.int32)

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

    def call_eval(fr=frames, F_=F, pr=pairs, P_=P, Q_=Q, gain=ones, bias=zeros, fu=32.0, fv=32.0, cu=31.5, cv=23.5, D=None, huber_k=0.0, level=1):
        return L.emba_frames_pair_level_eval(m._ctx, ptr(fr, _u8p), F_, ptr(pr, _i32p), P_, ptr(Q_, _dp), ptr(gain, _dp), ptr(bias, _dp), fu, fv, cu, cv, ptr(D, _dp), 1,
                                             huber_k, level, ptr(out["sums"], _dp), ptr(out["counts"], _u64p), ptr(out["uv"], _dp), ptr(out["resid"], _dp),
                                             ptr(out["lb"], _u8p), ptr(out["ll"], _dp))

    def call_loop(fr=frames, F_=F, pr=pairs, P_=P, Q_=Q, gain=ones, bias=zeros, fu=32.0, fv=32.0, cu=31.5, cv=23.5, D=None, null_settings=False, levels=lv, n_=n, estimate=3,
                  gain_min=0.25, gain_max=4.0, **kw):
        s = dict(good, **kw)
        cs = _lib.EmbaExposureSettings(_lib.EmbaAlignSettings(int(s["max_iters"]), int(s["min_pixels"]), s["lambda0"], s["lambda_up"], s["lambda_down"], s["lambda_min"],
                                                              s["lambda_max"], s["tol_rot"], s["huber_k"]), gain_min, gain_max)
        return L.emba_frames_pair_align_levels(m._ctx, ptr(fr, _u8p), F_, ptr(pr, _i32p), P_, ptr(Q_, _dp), ptr(gain, _dp), ptr(bias, _dp), fu, fv, cu, cv, ptr(D, _dp), 1,
                                               ptr(levels, _i32p), n_, estimate, None if null_settings else C.addressof(cs), ptr(out["q"], _dp), ptr(out["gain"], _dp),
                                               ptr(out["bias"], _dp), ptr(out["sums"], _dp), ptr(out["counts"], _u64p), ptr(out["status"], _i32p), ptr(out["iters"], _i32p),
                                               ptr(out["lst"], _i32p), ptr(out["lit"], _i32p), ptr(out["cost0"], _dp), ptr(out["n0"], _u64p), ptr(out["info"], _dp))

    nan, inf = float("nan"), float("inf")
    at = lambda base, idx, v: (lambda a: (a.__setitem__(idx, v), a)[1])(base.copy())      # noqa: E731
    err = lambda: L.emba_last_error(m._ctx)      # noqa: E731
    refused = [dict(fr=None), dict(pr=None), dict(Q_=None), dict(P_=1 << 31), dict(pr=at(pairs, (1, 0), F)), dict(pr=at(pairs, (2, 1), -1)), dict(F_=2),
               dict(Q_=at(Q, (1, 2), nan)), dict(Q_=at(Q, 2, 0.0)), dict(gain=at(ones, 1, 0.0)), dict(gain=at(ones, 0, nan)), dict(bias=at(zeros, 2, -inf)), dict(fu=0.0),
               dict(fv=inf), dict(cu=nan), dict(cv=inf), dict(D=np.array([0.0, nan, 0.0, 0.0, 0.0]))]
    for call in (call_eval, call_loop):
        for kw in refused:
            assert call(**kw) == ERR_INVALID_ARG and untouched(), (call.__name__, kw)
        many = (1 << 30) // S + 1
        assert call(F_=many) == ERR_INVALID_ARG and untouched() and b"resident sequence" in err()
        assert call(P_=0, fr=None, pr=None, Q_=None) == 0 and untouched()      # P = 0: nothing launched, nothing written
    assert call_eval(huber_k=nan) == ERR_INVALID_ARG and call_loop(huber_k=nan) == ERR_INVALID_ARG and untouched()
    # the level and the schedule, each with every later refusal also wrong: the first is reported
    later = dict(estimate=4, gain_min=2.0, min_pixels=2, F_=(1 << 30) // S + 1)
    assert call_eval(level=8) == ERR_INVALID_ARG and b"outside 0" in err() and call_eval(level=-1) == ERR_INVALID_ARG and untouched()
    assert call_eval(level=5, F_=many) == ERR_INVALID_ARG and b"level 5 of a 64 x 48" in err() and untouched()
    assert call_loop(huber_k=nan, levels=None, **later) == ERR_INVALID_ARG and b"huber_k" in err()
    assert call_loop(levels=None, **later) == ERR_INVALID_ARG and b"levels NULL" in err() and call_loop(n_=0, **later) == ERR_INVALID_ARG and b"levels NULL" in err()
    assert call_loop(levels=np.zeros(9, np.int32), n_=9, **later) == ERR_INVALID_ARG and b"n_levels = 9" in err()
    assert call_loop(levels=np.array([5, 8], np.int32), **later) == ERR_INVALID_ARG and b"levels[1] = 8" in err()
    assert call_loop(levels=np.array([0, 5], np.int32), **later) == ERR_INVALID_ARG and b"level 5 of a 64 x 48" in err()
    assert call_loop(**later) == ERR_INVALID_ARG and b"estimate = 4" in err() and call_loop(estimate=-1) == ERR_INVALID_ARG
    assert call_loop(**dict(later, estimate=3)) == ERR_INVALID_ARG and b"gain_min" in err() and call_loop(gain_max=nan) == ERR_INVALID_ARG
    assert call_loop(**dict(later, estimate=3, gain_min=0.25)) == ERR_INVALID_ARG and b"min_pixels" in err() and call_loop(null_settings=True) == ERR_INVALID_ARG
    assert call_loop(F_=many) == ERR_INVALID_ARG and b"resident sequence" in err() and untouched()
    for kw in (dict(max_iters=-1), dict(lambda_up=1.0), dict(lambda0=nan), dict(tol_rot=-1.0), dict(lambda_max=nan)):
        assert call_loop(**kw) == ERR_INVALID_ARG and untouched(), kw
    assert context_untouched()
    # the calls themselves still go, with and without the exposure and the lens, and leave the context alone
    assert call_eval() == 0 and call_loop() == 0 and not untouched()
    assert call_eval(gain=None, bias=None, D=np.array(PC.LENS_D)) == 0 and call_loop(gain=None, bias=None, D=np.array(PC.LENS_D), estimate=0) == 0
    assert (out["counts"].sum(axis=1) == S).all() and set(out["status"].tolist()) <= {1, 2, 3, 4} and (out["gain"] == 1.0).all() and (out["bias"] == 0.0).all()
    assert context_untouched()
    m.close()


def test_the_closing_case_through_the_driver(gpu):
    """driver.close_tracked_frames with close_levels = (1, 0) closes tests/pair_cases.py's drifted loop as the default does, and returns the pairs' exposures
    and level statuses; with the defaults it is today's result bit for bit (the calls LEGM.pair_align makes)."""
    from emba_amd.driver import SequenceSettings, close_tracked_frames
    c = PC.case(False)
    q, status = PC.drifted()
    fr = c["frames"].reshape(PC.F, PC.SH, PC.SW)
    common = dict(track_close=True, close_window=PC.CANDIDATES["window"], close_gap=PC.CANDIDATES["min_gap"], close_angle=PC.CANDIDATES["max_angle"],
                  close_per_frame=PC.CANDIDATES["max_per_frame"], close_min_overlap=PC.MIN_OVERLAP)
    tracked = dict(q=q.copy(), status=status.copy(), tracked=PC.F - 1, lost=0)
    kw = dict(levels=(1, 0), batch=1, skip_zero=True, min_weight=256, min_overlap=0.3, **PC.SETTINGS)
    m = make_legm(PC.SENSOR, lut=c["lut"])
    base = close_tracked_frames(m, fr, c["ts"], tracked, SequenceSettings(1.0, 1.0, **common), c["calib"], **kw)
    # ... against the calls themselves: LEGM.pair_align from io.pair_start's starts, the gate, the floored information and the graph
    S = PC.SW * PC.SH
    pairs = eio.pair_candidates(q, status, **PC.CANDIDATES)
    Q0, a0, b0 = eio.pair_start(q, None, None, pairs)
    al = m.pair_align(fr, pairs, Q0, c["calib"], gain=a0, bias=b0, skip_zero=True, **dict(PC.SETTINGS, huber_k=0.0))
    n = al["counts"][:, 0]
    keep = ((al["status"] == eio.ALIGN_CONVERGED) | (al["status"] == eio.ALIGN_ITERATIONS)) & (n >= PC.MIN_OVERLAP * S)
    g = m.rotation_graph_solve(q, status, pairs[keep], al["q"][keep], eio.pair_information(al["sums"], al["counts"], floor=eio.PAIR_NOISE_FLOOR)[keep])
    want = dict(q=g["q"], pairs=pairs, pair_status=al["status"], pair_n=n, pair_cost=al["sums"][:, 9] / np.maximum(n, 1), pair_kept=keep,
                pair_moved=eio.rotation_angle_between(Q0, al["q"]))
    assert "pair_gain" not in base and "pair_level_status" not in base and keep.all()
    for k, v in want.items():
        assert np.array_equal(bits(base[k]), bits(v)) if v.dtype == np.float64 else np.array_equal(base[k], v), k
    r = close_tracked_frames(m, fr, c["ts"], tracked, SequenceSettings(1.0, 1.0, close_levels=(1, 0), close_exposure="bias", **common), c["calib"], **kw)
    after = PC.worst_angle(r["q"])
    print(f"(1, 0), bias: {len(r['pairs'])} pairs, {int(r['pair_kept'].sum())} kept; worst angle {PC.worst_angle(q):.4e} -> {after:.4e} rad (level 0 alone "
          f"{PC.worst_angle(base['q']):.4e}); |bias| <= {np.abs(r['pair_bias']).max():.3f}; graph {r['graph']}")
    assert np.array_equal(r["pairs"], base["pairs"]) and r["pair_kept"].all() and r["pair_level_status"].shape == (len(r["pairs"]), 2) and (r["pair_last_level"] == 0).all()
    assert (r["pair_gain"] == 1.0).all() and np.abs(r["pair_bias"]).max() < 1.0 and r["graph"]["end"] == eio.GRAPH_CONVERGED
    assert after < 0.01 * PC.E_BEFORE_NP and np.array_equal(bits(r["q"][0]), bits(q[0]))
    m.close()


def test_run_ba_closes_coarse_to_fine(gpu, tmp_path):
    """examples/run_ba.py --track-close --close-levels 1,0 --close-exposure bias end to end: frames_pairs.txt gains the columns gain, bias and the last level;
    both flags are refused without --track-close."""
    out1, out2 = tmp_path / "out1", tmp_path / "out2"
    exe = [sys.executable, os.path.join(ROOT, "examples", "run_ba.py")]
    r = subprocess.run(exe + ["--demo", str(out1), "--views-hz", "50", "--window-size", "0.5", "--max-iter", "3"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    lo, hi = open(out1 / "views" / "tone.txt").read().split()
    common = ["--frames", str(out1 / "views"), "--init-poses", "frames", "--init-map", "frames", "--track-levels", "3,2,1", "--track-batch", "2", "--track-predict", "1",
              "--track-min-overlap", "0.3", "--track-q0", "0,0,0,1", "--window-size", "0.5", "--frames-log", "0", "--frames-lo", lo, "--frames-hi", hi,
              "--frames-skip-zero", "--max-iter", "3"]
    r = subprocess.run(exe + ["--demo", str(out2)] + common + ["--track-close", "--close-window", "2", "--close-gap", "3", "--close-angle", "0.3", "--close-per-frame", "2",
                                                               "--close-huber", "10", "--close-levels", "1,0", "--close-exposure", "bias"],
                       capture_output=True, text=True, timeout=600)
    print(r.stdout[-3000:])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "track-close:" in r.stdout
    lines = open(out2 / "frames_pairs.txt").read().splitlines()
    assert lines[0].startswith("# i j status(") and lines[0].endswith("kept gain bias last_level")
    rows = [l.split() for l in lines if l and not l.startswith("#")]
    assert len(rows) >= 1 and all(len(x) == 10 for x in rows) and any(int(x[6]) for x in rows)
    assert all(float(x[7]) == 1.0 and np.isfinite(float(x[8])) and int(x[9]) in (0, 1) for x in rows) and (out2 / "refined_traj.txt").exists()
    # a flag given at its default value: level 0 alone, the exposure as given — and the three columns all the same
    for k, flag in enumerate((["--close-levels", "0"], ["--close-exposure", "none"])):
        out = tmp_path / f"out_default{k}"
        r = subprocess.run(exe + ["--demo", str(out)] + common + ["--track-close", "--close-window", "2", "--close-gap", "3", "--close-angle", "0.3", "--close-per-frame", "2",
                                                                  "--close-huber", "10"] + flag, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
        lines = open(out / "frames_pairs.txt").read().splitlines()
        rows0 = [l.split() for l in lines if l and not l.startswith("#")]
        assert lines[0].endswith("kept gain bias last_level") and len(rows0) >= 1 and all(len(x) == 10 and float(x[7]) == 1.0 and float(x[8]) == 0.0 and int(x[9]) == 0 for x in rows0)
    for flag in (["--close-levels", "1,0"], ["--close-exposure", "bias"]):
        r = subprocess.run(exe + ["--demo", str(tmp_path / "out3"), "--window-size", "0.5"] + flag, capture_output=True, text=True, timeout=600)
        assert r.returncode != 0 and "--track-close" in r.stderr
