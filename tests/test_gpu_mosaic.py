"""The mosaic of intensity frames on the MI355X (include/emba_hip.h: emba_mosaic_frames, emba_mosaic_get, emba_mosaic_map, emba_mosaic_clear)
against the numpy forms of the same rules (emba_amd.io: mosaic_votes, mosaic_mean, mosaic_log, gradient_from_plane).  Every case feeds numpy the call's own
pm_out: the sums, the counters, the covered cells and the mean are compared with array_equal (the mean by its bits) — a difference is a bug in one of the
two forms, never a tolerance.  The one tolerance is the logarithm's: device and numpy each document <= 1 ulp, so |dL| <= 4 * 2^-52 * max(1, |L|).  Then the
chunk edge, accumulate / clear / skip_zero, the map made resident, the loop plane -> views -> mosaic -> map closed on the device, every refusal, what a
call leaves alone, and examples/run_ba.py on the files of another run."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import mosaic_cases as MC
import view_cases as VC
from emba_amd import io as eio
from emba_amd import so3, synth
from emba_amd.legm import EventWindow, LinearTrajectory

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_INVALID_ARG, ERR_TIME_RANGE, ERR_STATE = 1, 4, 5
LOG_TOL = 4.0 * 2.0 ** -52
_dp, _u8p, _i64p, _u64p = (C.POINTER(t) for t in (C.c_double, C.c_uint8, C.c_int64, C.c_uint64))


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from emba_amd import build
    build.build_hip()
    return True


@pytest.fixture(scope="module")
def scene():
    return synth.make_scene_workload()          # 64x48 on 256x512, K = 6: 38 965 events


def make_legm(sensor, pano, lut=None):
    from emba_amd import LEGM
    return LEGM(sensor[0], sensor[1], VC.lut_of(sensor) if lut is None else lut, 0.2, pano[0], pano[1], device=0)


def ptr(a, ty):
    return None if a is None else a.ctypes.data_as(ty)


def traj_of(kind):
    return LinearTrajectory(np.ascontiguousarray(VC.knots_of(kind)), VC.T0_NS, VC.DT_NS)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def check_against_numpy(m, frames, pm, pano, skip_zero, got, what, min_weight=256, fill=-2.5):
    """The device's mosaic against the numpy form fed the device's own pm: every integer, the covered cells and the bits of the mean.  Returns numpy's."""
    W, H = pano
    sw, sv, dropped, skipped = eio.mosaic_votes(frames, pm, W, H, skip_zero)
    mean, cov = eio.mosaic_mean(sw, sv, min_weight, fill)
    g = m.mosaic(min_weight, fill)
    assert np.array_equal(g["sum_w"], sw) and np.array_equal(g["sum_v"], sv), what
    assert got is None or (got["dropped"], got["skipped"]) == (dropped, skipped), what
    assert np.array_equal(g["covered"], cov) and g["n_covered"] == int(cov.sum()), what
    assert np.array_equal(bits(g["mean"]), bits(mean)), what
    return g


def check_map(m, g, lo, hi, eps, what, worst, min_weight=256):
    """emba_mosaic_map against io.mosaic_log of the device's mean and io.gradient_from_plane of the device's L."""
    for take_log in (False, True):
        r = m.mosaic_map(min_weight, lo, hi, eps, take_log)
        L_np, cov = eio.mosaic_log(g["mean"], g["covered"], lo, hi, eps, take_log)
        if not take_log:
            assert np.array_equal(bits(r["L"]), bits(L_np)), what
        else:
            d = np.abs(r["L"] - L_np) / np.maximum(1.0, np.abs(L_np))
            worst[0] = max(worst[0], float(d.max()) / 2.0 ** -52)
            assert d.max() <= LOG_TOL, (what, float(d.max()))
            assert not r["L"][~cov].any()
        Gx, Gy = eio.gradient_from_plane(r["L"], cov)
        assert np.array_equal(bits(r["Gx"]), bits(Gx)) and np.array_equal(bits(r["Gy"]), bits(Gy)), (what, take_log)
        assert not r["Gy"][0].any()
    return r


@pytest.mark.parametrize("pano", MC.PANOS, ids=lambda p: f"pano{p[1]}x{p[0]}")
@pytest.mark.parametrize("sensor", MC.SENSORS, ids=lambda s: f"sensor{s[0]}x{s[1]}")
def test_every_case_against_the_numpy_forms(gpu, sensor, pano):
    W, H = pano
    sw_, sh_ = sensor
    m = make_legm(sensor, pano)
    m.set_option("poison", 1)      # a cell that is read before it is written shows
    worst = [0.0]
    seen_dropped = seen_skipped = seen_wrapped = 0
    for kind in MC.KINDS:
        for F in MC.FRAMES:
            c = MC.case(sensor, pano, kind, F)
            for skip_zero in (True, False):
                what = f"{sensor} on {pano}, {kind}, F = {F}, skip_zero = {skip_zero}"
                got = m.mosaic_frames(c["frames"].reshape(F, sh_, sw_), c["ts"], traj_of(kind), skip_zero=skip_zero, want_pm=True)
                assert got["pm"].shape == (F, sw_ * sh_, 2), what
                g = check_against_numpy(m, c["frames"], got["pm"], pano, skip_zero, got, what)
                check_against_numpy(m, c["frames"], got["pm"], pano, skip_zero, None, what, min_weight=1, fill=0.0)
                seen_dropped += got["dropped"]
                seen_skipped += got["skipped"]
                if kind == "identity" and F == 65:
                    assert int(g["sum_w"].max()) >= 65 * 64, what                       # every frame on the same cells
            r = check_map(m, g, c["lo"], c["hi"], 1.0 / 255.0, what, worst)
            both = g["covered"][:, 0] & g["covered"][:, W - 1]
            if kind == "yaw_pi" and both.any():
                assert (r["Gx"][both, 0] == r["L"][both, 0] - r["L"][both, W - 1]).all(), what      # column 0's left neighbour is column W - 1
                seen_wrapped += 1
    # row 0 covered: a view pitched upwards (device pm only: no pole-row exclusion is needed)
    knots = np.array([so3.mul(so3.exp(np.array([0.0, 0.2 * i, 0.0])), so3.exp(np.array([1.25, 0.0, 0.0]))) for i in range(VC.K)])
    frames = np.random.default_rng(7).integers(1, 256, (3, sh_, sw_)).astype(np.uint8)
    got = m.mosaic_frames(frames, VC.frame_times(3), LinearTrajectory(knots, VC.T0_NS, VC.DT_NS), want_pm=True)
    g = check_against_numpy(m, frames, got["pm"], pano, False, got, "pitched upwards", min_weight=1)
    r = check_map(m, g, 0.5, 2.0, 0.01, "pitched upwards", worst, min_weight=1)
    assert g["covered"][0].any() and r["Gx"][0].any() and not r["Gy"][0].any()
    print(f"{sensor} on {pano}: worst |L_device - L_numpy| / max(1, |L|) = {worst[0]:.3f} * 2^-52")
    assert seen_dropped > 0 and seen_skipped > 0 and seen_wrapped > 0
    m.close()


def test_chunk_edge(gpu):
    """F = 65 535 + 3 frames of the 7 x 5 sensor: two chunks.  Random bytes, yaw_pi, times spread over the accepted range."""
    sensor, pano = (7, 5), (32, 16)
    F = 65535 + 3
    m = make_legm(sensor, pano)
    m.set_option("poison", 1)
    frames = np.random.default_rng(65538).integers(0, 256, (F, 5, 7)).astype(np.uint8)
    ts = VC.T0_NS + (np.arange(F, dtype=np.int64) * (VC.T_LAST_NS - VC.T0_NS)) // (F - 1)
    traj = traj_of("yaw_pi")
    got = m.mosaic_frames(frames, ts, traj, skip_zero=True, want_pm=True)
    g = check_against_numpy(m, frames, got["pm"], pano, True, got, "one call")
    assert got["skipped"] == int((frames == 0).sum()) and got["dropped"] == 0 and int(g["sum_w"].sum()) == 256 * (frames.size - got["skipped"])
    # two accumulated calls, split at a frame that is not the chunk edge
    a = m.mosaic_frames(frames[:40000], ts[:40000], traj, skip_zero=True)
    b = m.mosaic_frames(frames[40000:], ts[40000:], traj, skip_zero=True, accumulate=True)
    g2 = m.mosaic()
    assert np.array_equal(g2["sum_w"], g["sum_w"]) and np.array_equal(g2["sum_v"], g["sum_v"])
    assert a["dropped"] + b["dropped"] == got["dropped"] and a["skipped"] + b["skipped"] == got["skipped"]
    m.close()


def test_accumulate_clear_and_skip_zero(gpu):
    from emba_amd import EmbaError
    sensor, pano = (20, 13), (48, 24)
    c = MC.case(sensor, pano, "pitch", 65)
    fr = c["frames"].reshape(65, 13, 20)
    traj = traj_of("pitch")
    m = make_legm(sensor, pano)
    with pytest.raises(EmbaError) as ei:
        m.mosaic()
    assert ei.value.status == ERR_STATE
    one = m.mosaic_frames(fr, c["ts"], traj, skip_zero=True, want_pm=True)
    whole = check_against_numpy(m, c["frames"], one["pm"], pano, True, one, "one call")
    # three pieces, the first without accumulate: what was there is gone
    m.mosaic_frames(fr[:5], c["ts"][:5], traj, skip_zero=False)
    p0 = m.mosaic_frames(fr[:23], c["ts"][:23], traj, skip_zero=True)
    p1 = m.mosaic_frames(fr[23:24], c["ts"][23:24], traj, skip_zero=True, accumulate=True)
    p2 = m.mosaic_frames(fr[24:], c["ts"][24:], traj, skip_zero=True, accumulate=True)
    g = m.mosaic()
    assert np.array_equal(g["sum_w"], whole["sum_w"]) and np.array_equal(g["sum_v"], whole["sum_v"])
    assert sum(p["skipped"] for p in (p0, p1, p2)) == one["skipped"] == int((c["frames"] == 0).sum())
    # accumulate with no frame adds nothing; without accumulate it clears
    m.mosaic_frames(fr[:0], c["ts"][:0], traj, accumulate=True)
    assert np.array_equal(m.mosaic()["sum_w"], whole["sum_w"])
    # skip_zero off: the zero bytes vote with their weight and a value of zero
    plain = m.mosaic_frames(fr, c["ts"], traj, skip_zero=False, want_pm=True)
    gp = check_against_numpy(m, c["frames"], plain["pm"], pano, False, plain, "skip_zero off")
    assert plain["skipped"] == 0 and np.array_equal(gp["sum_v"], whole["sum_v"]) and int(gp["sum_w"].sum()) > int(whole["sum_w"].sum())
    # clear: nothing accumulated; accumulate onto nothing starts from zero
    m.mosaic_clear()
    for call in (m.mosaic, m.mosaic_map):
        with pytest.raises(EmbaError) as ei:
            call()
        assert ei.value.status == ERR_STATE
    assert m._L.emba_mosaic_get(m._ctx, 256, 0.0, None, None, None, None, None) == ERR_STATE
    m.mosaic_frames(fr, c["ts"], traj, skip_zero=True, accumulate=True)
    assert np.array_equal(m.mosaic()["sum_w"], whole["sum_w"])
    m.mosaic_frames(fr[:0], c["ts"][:0], traj)
    with pytest.raises(EmbaError):
        m.mosaic()
    m.close()


def views_of_the_scene_map(m, w, F=40):
    """F frames of bytes of the panorama of the resident map along the scene's trajectory, with their times and tone."""
    t_end = w.traj.t0_ns + w.traj.dt_ns * (w.K - 1) - 1
    ts = w.traj.t0_ns + (np.arange(F, dtype=np.int64) * (t_end - w.traj.t0_ns)) // (F - 1)
    lo, hi = m.normalizeRobust(m.reconstructIntensity(), with_range=True)[1]
    r = m.render_views(ts, w.traj.knots_xyzw, w.traj.t0_ns, w.traj.dt_ns, want_u8=True, lo=lo, hi=hi)
    return r["u8"], ts, lo, hi


def test_make_resident_is_an_upload_of_the_same_planes(gpu, scene):
    """ep of an evaluation right after emba_mosaic_map(make_resident = 1) against ep after emba_upload_map of the downloaded Gx, Gy in a second context."""
    w = scene
    a = make_legm((64, 48), (512, 256), lut=w.lut)
    a.set_events(w.events)
    a.upload_map(w.Gx, w.Gy)
    frames, ts, lo, hi = views_of_the_scene_map(a, w)
    a.mosaic_frames(frames, ts, w.traj, skip_zero=True)
    r = a.mosaic_map(256, lo, hi, take_log=False, resident=True)
    assert np.abs(r["Gx"]).max() > 0 and np.abs(r["Gy"]).max() > 0
    first = a.step(w.traj, w.thres_valid_pixel, w.alpha)
    ep_a = a.get_ep()
    gx, gy = a.downloadMap()
    assert np.array_equal(bits(gx), bits(r["Gx"])) and np.array_equal(bits(gy), bits(r["Gy"]))
    b = make_legm((64, 48), (512, 256), lut=w.lut)
    b.set_events(w.events)
    b.upload_map(r["Gx"], r["Gy"])
    second = b.step(w.traj, w.thres_valid_pixel, w.alpha)
    ep_b = b.get_ep()
    assert first == second and ep_a.size > 1000 and np.array_equal(bits(ep_a), bits(ep_b))
    assert a.last_counts() == b.last_counts()
    a.close(); b.close()


def test_the_loop_closed_on_the_device(gpu):
    """plane -> LEGM.render_views (bytes, lo / hi of the plane) -> mosaic_frames(skip_zero) -> mosaic_map(take_log = False) on 64 x 48 / 128 x 64: the
    gradient correlation with the plane's backward differences is >= 0.95, the figure of tests/test_mosaic_cpu.py (numpy alone on this pair: 0.983 - 0.995
    with this linear tone)."""
    sensor, pano = MC.E2E_LARGE[0]
    P = MC.smooth_plane(pano)
    lo, hi = float(P.min()), float(P.max())
    ref = MC.backward_differences(P)
    m = make_legm(sensor, pano)
    for kind in MC.KINDS:
        for F in MC.FRAMES:
            knots, ts = VC.knots_of(kind), VC.frame_times(F)
            v = m.render_views(ts, knots, VC.T0_NS, VC.DT_NS, plane=P, want_u8=True, lo=lo, hi=hi)
            got = m.mosaic_frames(v["u8"], ts, traj_of(kind), skip_zero=True)
            r = m.mosaic_map(256, lo, hi, take_log=False)
            both = MC.gradient_mask(m.mosaic()["covered"])
            corr = MC.correlation((r["Gx"], r["Gy"]), ref, both)
            print(f"{kind}, F = {F}: correlation {corr:.4f} over {int(both.sum())} cells, {got['skipped']} skipped")
            assert got["skipped"] >= int(v["outside"].sum()) and both.sum() >= 300 and corr >= MC.E2E_MIN_CORRELATION, (kind, F, corr)
    m.close()


def test_every_refusal_by_status(gpu, scene):
    w = scene
    S = 64 * 48
    m = make_legm((64, 48), (512, 256), lut=w.lut)
    m.set_events(w.events)
    m.upload_map(w.Gx, w.Gy)
    first = m.step(w.traj, w.thres_valid_pixel, w.alpha)
    ep0 = m.get_ep()
    knots = np.ascontiguousarray(w.traj.knots_xyzw)
    t0, dt, K = w.traj.t0_ns, w.traj.dt_ns, w.K
    t_last = t0 + dt * (K - 1) - 1
    frames = np.random.default_rng(3).integers(0, 256, (3, 48, 64)).astype(np.uint8)
    ts = np.array([t0, (t0 + t_last) // 2, t_last], np.int64)
    u64 = lambda: C.c_uint64(77)
    L = m._L
    # nothing accumulated yet
    shape = (256, 512)
    out = dict(sw=np.full(shape, 5, np.uint64), sv=np.full(shape, 6, np.uint64), mean=np.full(shape, 4.25), cov=np.full(shape, 9, np.uint8), n=u64(),
               L=np.full(shape, 1.5), gx=np.full(shape, 2.5), gy=np.full(shape, 3.5), pm=np.full((3, S, 2), -1.5), dropped=u64(), skipped=u64())

    def untouched():
        return ((out["sw"] == 5).all() and (out["sv"] == 6).all() and (out["mean"] == 4.25).all() and (out["cov"] == 9).all() and out["n"].value == 77
                and (out["L"] == 1.5).all() and (out["gx"] == 2.5).all() and (out["gy"] == 3.5).all() and (out["pm"] == -1.5).all()
                and out["dropped"].value == 77 and out["skipped"].value == 77)

    def call_frames(fr=frames, t=ts, F=3, kn=knots, k=K, d=dt, accumulate=0):
        return L.emba_mosaic_frames(m._ctx, ptr(fr, _u8p), ptr(t, _i64p), F, ptr(kn, _dp), k, t0, d, 1, accumulate, C.byref(out["dropped"]), C.byref(out["skipped"]),
                                    ptr(out["pm"], _dp))

    def call_get(min_weight=256, fill=0.0):
        return L.emba_mosaic_get(m._ctx, min_weight, fill, ptr(out["sw"], _u64p), ptr(out["sv"], _u64p), ptr(out["mean"], _dp), ptr(out["cov"], _u8p), C.byref(out["n"]))

    def call_map(min_weight=256, lo=0.0, hi=1.0, eps=0.0, resident=1):
        return L.emba_mosaic_map(m._ctx, min_weight, lo, hi, eps, 0, ptr(out["L"], _dp), ptr(out["gx"], _dp), ptr(out["gy"], _dp), resident)

    assert call_get() == ERR_STATE and call_map() == ERR_STATE and untouched()
    m.mosaic_frames(frames, ts, w.traj, skip_zero=True)
    before = m.mosaic()
    map0 = m.downloadMap()

    def unchanged(st, want):
        g = m.mosaic()
        now = m.downloadMap()
        again = m.step(w.traj, w.thres_valid_pixel, w.alpha)      # the context still evaluates its window, on the map it had
        return (st == want and untouched() and np.array_equal(g["sum_w"], before["sum_w"]) and np.array_equal(g["sum_v"], before["sum_v"])
                and np.array_equal(now[0], map0[0]) and np.array_equal(now[1], map0[1]) and again == first and np.array_equal(bits(m.get_ep()), bits(ep0)))
    nan, inf = float("nan"), float("inf")
    for accumulate in (0, 1):
        assert unchanged(call_frames(fr=None, accumulate=accumulate), ERR_INVALID_ARG)
        assert unchanged(call_frames(t=None, accumulate=accumulate), ERR_INVALID_ARG)
        assert unchanged(call_frames(kn=None, accumulate=accumulate), ERR_INVALID_ARG)
        assert unchanged(call_frames(k=1, accumulate=accumulate), ERR_INVALID_ARG)
        assert unchanged(call_frames(d=0, accumulate=accumulate), ERR_INVALID_ARG)
        assert unchanged(call_frames(d=-dt, accumulate=accumulate), ERR_INVALID_ARG)
        assert unchanged(call_frames(F=1 << 31, accumulate=accumulate), ERR_INVALID_ARG)
        assert unchanged(call_frames(F=(1 << 36) // S + 1 - (3 if accumulate else 0), accumulate=accumulate), ERR_INVALID_ARG)      # the 2^36 bound, with what is there
        for bad_t in (t_last + 1, t0 - 1):
            assert unchanged(call_frames(t=np.array([t0, bad_t, t_last], np.int64), accumulate=accumulate), ERR_TIME_RANGE)
    assert unchanged(call_get(min_weight=0), ERR_INVALID_ARG)
    assert unchanged(call_get(fill=nan), ERR_INVALID_ARG) and unchanged(call_get(fill=-inf), ERR_INVALID_ARG)
    assert unchanged(call_map(min_weight=0), ERR_INVALID_ARG)
    for lo, hi, eps in ((nan, 1.0, 0.0), (0.0, inf, 0.0), (0.0, 1.0, nan), (-inf, 1.0, 0.0), (1.0, 1.0, 0.0), (2.0, 1.0, 0.0)):
        assert unchanged(call_map(lo=lo, hi=hi, eps=eps), ERR_INVALID_ARG), (lo, hi, eps)
    # the calls themselves still go
    assert call_frames(accumulate=1) == 0 and call_get() == 0 and not untouched()
    assert np.array_equal(out["sw"], 2 * before["sum_w"]) and np.array_equal(out["sv"], 2 * before["sum_v"])
    assert call_map(resident=0) == 0 and np.array_equal(m.downloadMap()[0], map0[0])
    m.mosaic_clear()
    assert call_get() == ERR_STATE and call_map() == ERR_STATE
    m.close()


def test_a_call_in_between_changes_nothing(gpu, scene):
    """The panorama of warped events, a step evaluation and the resident map after the four mosaic calls (make_resident = 0): bit-equal to the same calls on
    a context that never made them."""
    w = scene
    t_end = w.traj.t0_ns + w.traj.dt_ns * (w.K - 1) - 1
    ts = np.array([w.traj.t0_ns, t_end], np.int64)
    frames = np.random.default_rng(9).integers(0, 256, (2, 48, 64)).astype(np.uint8)
    other = LinearTrajectory(np.ascontiguousarray(w.traj.knots_xyzw[:3]), w.traj.t0_ns, 4 * w.traj.dt_ns)      # other knots than the calls around it
    got = []
    for between in (False, True):
        m = make_legm((64, 48), (512, 256), lut=w.lut)
        n = m.set_sequence(w.events)
        m.set_events(EventWindow(0, n))
        m.upload_map(w.Gx, w.Gy)
        first = m.step(w.traj, w.thres_valid_pixel, w.alpha)
        if between:
            m.mosaic_frames(frames, ts, other, skip_zero=True, want_pm=True)
            m.mosaic()
            m.mosaic_map(1, -1.0, 1.0, 0.5, True)
        pano = m.event_panorama(w.traj, 300, 20000, signed=True, want_pm=True)
        if between:
            m.mosaic_frames(frames, ts, w.traj, accumulate=True)
            m.mosaic_map(256, 0.0, 1.0, take_log=False)
            m.mosaic_clear()
        second = m.step(w.traj, w.thres_valid_pixel, w.alpha)
        got.append((first, pano, second, m.get_ep(), m.last_counts(), m.event_counts(), m.downloadMap(), m.sequence_size()))
        m.close()
    a, b = got
    assert a[0] == b[0] and a[2] == b[2] and a[4] == b[4] and a[5] == b[5] and a[7] == b[7] and a[0][0] > 1000
    assert np.array_equal(bits(a[3]), bits(b[3]))
    assert np.array_equal(a[1]["image"], b[1]["image"]) and np.array_equal(bits(a[1]["pm"]), bits(b[1]["pm"]))
    assert all(a[1][k] == b[1][k] for k in ("J", "sum", "nonzero", "dropped"))
    assert np.array_equal(bits(a[6][0]), bits(b[6][0])) and np.array_equal(bits(a[6][1]), bits(b[6][1])) and np.array_equal(a[6][0], w.Gx)


def test_run_ba_on_the_frames_of_another_run(gpu, tmp_path):
    """examples/run_ba.py --demo with --views-hz writes frames; a second run takes them as --frames, starts from their mosaic (--init-map frames) with the
    first run's tone and writes frame_mosaic.pgm."""
    out1, out2 = tmp_path / "out1", tmp_path / "out2"
    exe = [sys.executable, os.path.join(ROOT, "examples", "run_ba.py")]
    r = subprocess.run(exe + ["--demo", str(out1), "--views-hz", "50", "--window-size", "0.5", "--max-iter", "3"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    lo, hi = open(out1 / "views" / "tone.txt").read().split()
    n_frames = len(open(out1 / "views" / "times.txt").read().splitlines())
    assert n_frames >= 20 and (out1 / "views" / ("frame_%06d.pgm" % (n_frames - 1))).exists()
    r = subprocess.run(exe + ["--demo", str(out2), "--frames", str(out1 / "views"), "--init-map", "frames", "--frames-log", "0", "--frames-lo", lo, "--frames-hi", hi,
                              "--frames-skip-zero", "--max-iter", "3"], capture_output=True, text=True, timeout=600)
    print(r.stdout[-3000:])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "initial map from" in r.stdout and "frame mosaic:" in r.stdout
    for f in ("refined_traj.txt", "Gx.bin", "Gy.bin", "map_poisson_opt.pgm", "frame_mosaic.pgm", "frame_mosaic_covered.pgm"):
        assert (out2 / f).exists(), f
    mosaic, covered = eio.load_pgm(str(out2 / "frame_mosaic.pgm")), eio.load_pgm(str(out2 / "frame_mosaic_covered.pgm"))
    assert mosaic.shape == (512, 1024) and covered.shape == (512, 1024) and 1000 < int((covered == 255).sum()) < covered.size and len(np.unique(mosaic[covered == 255])) > 20
    # --init-map frames refuses without --frames
    r = subprocess.run(exe + ["--demo", str(tmp_path / "out3"), "--init-map", "frames"], capture_output=True, text=True, timeout=600)
    assert r.returncode != 0 and "--frames" in r.stderr
    # ... and along a trajectory that carries the timing only
    r = subprocess.run(exe + ["--demo", str(tmp_path / "out3"), "--frames", str(out1 / "views"), "--init-map", "frames", "--init-poses", "identity", "--window-size", "0.5"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode != 0 and "given poses" in r.stderr
