"""emba_seq_filter on the MI355X (include/emba_hip.h; sequence_kernels.h: emba_filter_*): the resident sequence, the statistics and the hot-pixel mask
after the filter against the plain loops of tests/filter_ref.py, exactly (integers), on the cases of tests/test_filter_cpu.py; that a registered
window is left alone; that a window cut from the filtered sequence is the window of the pre-filtered recording; and the group form.  Every context is
built with option poison = 1: a read of never-written workspace shows."""
import ctypes as C

import numpy as np
import pytest

import filter_ref as FR
from emba_amd import synth
from emba_amd.legm import EventPacket, EventWindow
from emba_amd.sharded import shard_events, window_shard_ranges
from helpers import assert_close_elementwise, small_workload
from test_filter_cpu import MS, case, case_names, reference

pytestmark = pytest.mark.gpu
ERR_INVALID_ARG, ERR_STATE = 1, 5


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from emba_amd import build
    build.build_hip()
    return True


def make_sensor_legm(sw, sh):
    """A context for a sensor of that size (the panorama plays no part in the filter), every new allocation poisoned."""
    from emba_amd import LEGM
    m = LEGM(sw, sh, synth.pinhole_bearing_lut(sw, sh, 60.0, 60.0, sw / 2.0, sh / 2.0), 0.2, 128, 64, device=0)
    m.set_option("poison", 1)
    return m


def make_legm(w):
    from emba_amd import LEGM
    m = LEGM(w.sensor_w, w.sensor_h, w.lut, w.C_th, w.pano_w, w.pano_h, device=0)
    m.set_option("poison", 1)
    return m


def assert_sequence_equals(m, want):
    n = len(want[3])
    assert m.sequence_size() == n
    got = m.sequence_events(0, n)
    for g, o in zip((got.x, got.y, got.polarity, got.t_ns), want):
        assert np.array_equal(g, o)


# ---- a ... g, i: the cases -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", case_names())
def test_filter_equals_the_loops(gpu, name):
    c = case(name)
    want, stats, hot = reference(name)
    m = make_sensor_legm(c.sw, c.sh)
    assert m.set_sequence(c.ev, 1) == c.ev.size()
    got_stats = m.filter_sequence(*c.args(), c.rate)
    print(name, [int(v) for v in got_stats], stats)
    assert [int(v) for v in got_stats] == stats
    assert_sequence_equals(m, want)
    assert np.array_equal(m.sequence_hot_pixels(), hot)
    if name.startswith("f-off"):      # filters off with rate r: emba_seq_upload(..., r) of the same host arrays
        m2 = make_sensor_legm(c.sw, c.sh)
        kept = m2.set_sequence(c.ev, c.rate)
        assert kept == stats[5]
        up = m2.sequence_events(0, kept)
        assert_sequence_equals(m, (up.x, up.y, up.polarity, up.t_ns))
        m2.close()
    m.close()


def test_a_second_filter_runs_on_the_survivors(gpu):
    """The fresh arrays are swapped in, then swapped back: a second call filters what the first one left (buffers of both generations in use)."""
    c = case("f-all-r1")
    m = make_sensor_legm(c.sw, c.sh)
    m.set_sequence(c.ev, 1)
    m.filter_sequence(*c.args(), 1)
    x, y, pol, t = reference("f-all-r1")[0]
    want, stats, hot = FR.filter_loops(x, y, pol, t, c.sw, c.sh, 2.0, 2 * MS, 40 * MS, 2)
    assert [int(v) for v in m.filter_sequence(2.0, 2 * MS, 40 * MS, 2)] == stats and 0 < stats[5] < len(t) // 2
    assert_sequence_equals(m, want)
    assert np.array_equal(m.sequence_hot_pixels(), hot)
    m.close()


# ---- h: states and arguments -----------------------------------------------------------------------------------------------------------------------------
def test_states_and_arguments(gpu):
    from emba_amd import EmbaError
    c = case("h-all-removed")
    m = make_sensor_legm(c.sw, c.sh)
    with pytest.raises(EmbaError) as ei:
        m.filter_sequence(3.0, 0, 0, 1)
    assert ei.value.status == ERR_STATE                              # no sequence
    with pytest.raises(EmbaError) as ei:
        m.sequence_hot_pixels()
    assert ei.value.status == ERR_STATE                              # no filter yet
    m.set_sequence(c.ev, 1)
    with pytest.raises(EmbaError) as ei:
        m.filter_sequence(float("nan"), MS, MS, 1)
    assert ei.value.status == ERR_INVALID_ARG and "NaN" in str(ei.value)
    assert_sequence_equals(m, (c.ev.x, c.ev.y, c.ev.polarity, c.ev.t_ns))      # intact
    # all tests off, rate <= 1: unchanged
    assert [int(v) for v in m.filter_sequence(0.0, 0, 0, 1)] == [500, 0, 0, 0, 0, 500]
    assert_sequence_equals(m, (c.ev.x, c.ev.y, c.ev.polarity, c.ev.t_ns))
    assert not m.sequence_hot_pixels().any()
    # everything removed: EMBA_OK, size 0, and no sequence is resident afterwards
    st = m.filter_sequence(*c.args(), 1)
    assert int(st[5]) == 0 and int(st[4]) == 500 and m.sequence_size() == 0
    with pytest.raises(EmbaError) as ei:
        m.filter_sequence(3.0, 0, 0, 1)
    assert ei.value.status == ERR_STATE
    assert m.set_sequence(c.ev, 1) == 500                            # the context is usable afterwards
    assert [int(v) for v in m.filter_sequence(0.0, 1 * MS, 0, 1)] == FR.filter_loops(c.ev.x, c.ev.y, c.ev.polarity, c.ev.t_ns, c.sw, c.sh, 0.0, 1 * MS, 0, 1)[1]
    m.close()


# ---- a registered window is not disturbed ------------------------------------------------------------------------------------------------------------
def noisy_workload():
    w = small_workload(n_events=20_000)
    noisy, hot = synth.add_sensor_noise(w.events, (w.sensor_w, w.sensor_h), n_hot=3, hot_events_each=1500, n_background=0, seed=3)
    return w, noisy, hot


def test_filter_leaves_the_registered_window_alone(gpu):
    w, noisy, hot = noisy_workload()
    m = make_legm(w)
    n = m.set_sequence(noisy, 1)
    m.set_events(EventWindow(0, n))
    nem1 = np.zeros((w.pano_h, w.pano_w), dtype=np.int32)
    ep1 = m.evaluateDataError(w.traj, w.Gx, w.Gy, None, True, nem1).copy()
    stats = m.filter_sequence(4.0, 100_000, 20 * MS, 2)
    assert 0 < int(stats[5]) < n // 2 and int(stats[1]) == 3 and m.sequence_size() == int(stats[5])
    nem2 = np.zeros_like(nem1)
    ep2 = m.evaluateDataError(w.traj, None, None, None, True, nem2)      # the same window, not registered again
    assert ep1.size > 1000 and np.array_equal(ep1, ep2) and np.array_equal(nem1, nem2)
    m.close()


# ---- a window of the filtered sequence is the window of the pre-filtered recording -----------------------------------------------------------------------
def test_window_of_the_filtered_sequence_matches_the_prefiltered_upload(gpu):
    w, noisy, hot = noisy_workload()
    args = (4.0, 100_000, 20 * MS)
    want, stats, mask = FR.filter_loops(noisy.x, noisy.y, noisy.polarity, noisy.t_ns, w.sensor_w, w.sensor_h, *args, 1)
    assert np.array_equal(np.flatnonzero(mask), hot) and stats[3] > 0 and stats[4] > 0 and stats[5] > 10_000
    t = want[3]
    t_beg, t_end = int(t[2000]) - MS, int(t[-2000]) + MS
    res = []
    for filtered_on_device in (True, False):
        m = make_legm(w)
        if filtered_on_device:
            m.set_sequence(noisy, 1)
            assert [int(v) for v in m.filter_sequence(*args, 1)] == stats
        else:
            m.set_sequence(EventPacket(*want), 1)
        beg, end = m.sequence_window(t_beg, t_end)
        m.set_events(EventWindow(beg, end))
        nem = np.zeros((w.pano_h, w.pano_w), dtype=np.int32)
        ep = m.evaluateDataError(w.traj, w.Gx, w.Gy, None, True, nem)
        m.formNormalEq(None, w.K, nem, w.thres_valid_pixel)
        ne = m.applyL2Reg(w.alpha)
        res.append(dict(range=(beg, end), ep=ep.copy(), nem=nem, ne=ne, counts=m.event_counts()))
        m.close()
    dev, host = res
    assert dev["range"] == host["range"] and dev["range"][0] > 0 and dev["range"][1] - dev["range"][0] > 5000
    assert dev["counts"] == host["counts"] and np.array_equal(dev["nem"], host["nem"]) and dev["ep"].shape == host["ep"].shape and dev["ep"].size > 1000
    assert_close_elementwise(dev["ep"], host["ep"], "ep")
    assert np.array_equal(dev["ne"]["active"], host["ne"]["active"])
    for k in ("A11", "b1", "A22", "b2"):
        assert_close_elementwise(dev["ne"][k], host["ne"][k], k)


# ---- the group ----------------------------------------------------------------------------------------------------------------------------------------
def _arr(a, ty):
    return a.ctypes.data_as(ty)


def test_group_filters_every_ranks_copy(gpu):
    from emba_amd import _lib
    L = _lib.load()
    w, noisy, hot = noisy_workload()
    args = (4.0, 100_000, 20 * MS)
    want, stats, mask = FR.filter_loops(noisy.x, noisy.y, noisy.polarity, noisy.t_ns, w.sensor_w, w.sensor_h, *args, 2)
    fx, fy, fp, ft = want
    nk = stats[5]
    x, y, pol, t = (np.ascontiguousarray(a, d) for a, d in ((noisy.x, np.uint16), (noisy.y, np.uint16), (noisy.polarity, np.uint8), (noisy.t_ns, np.int64)))
    lut = np.ascontiguousarray(w.lut, dtype=np.float64)
    cfg = _lib.EmbaCfg(w.sensor_w, w.sensor_h, w.pano_w, w.pano_h, _arr(lut, _lib._dp), float(w.C_th), 100, 10.0, 0, None)
    g = C.c_void_p()
    world = 2
    devs = (C.c_int32 * world)(0, 0)
    assert L.emba_group_create(C.byref(cfg), devs, world, C.byref(g)) == 0, L.emba_group_last_error(None)
    try:
        assert L.emba_group_set_option(g, b"poison", 1) == 0
        st6 = (C.c_uint64 * 6)()
        assert L.emba_group_seq_filter(g, *args, 2, st6) == ERR_STATE                      # no sequence yet
        kept = C.c_size_t(0)
        assert L.emba_group_seq_upload(g, _arr(x, _lib._u16p), _arr(y, _lib._u16p), _arr(pol, _lib._u8p), _arr(t, _lib._i64p), x.size, 1, C.byref(kept)) == 0
        assert L.emba_group_seq_filter(g, *args, 2, st6) == 0, L.emba_group_last_error(g)
        assert list(st6) == stats
        size = C.c_size_t(0)
        assert L.emba_group_seq_size(g, C.byref(size)) == 0 and size.value == nk
        for r in range(world):
            ctx = L.emba_group_ctx(g, r)
            sx, sy, sp, st_ = np.empty(nk, np.uint16), np.empty(nk, np.uint16), np.empty(nk, np.uint8), np.empty(nk, np.int64)
            assert L.emba_seq_get(ctx, 0, nk, _arr(sx, _lib._u16p), _arr(sy, _lib._u16p), _arr(sp, _lib._u8p), _arr(st_, _lib._i64p)) == 0
            assert np.array_equal(sx, fx) and np.array_equal(sy, fy) and np.array_equal(sp, fp) and np.array_equal(st_, ft)
            hm = np.zeros(w.sensor_w * w.sensor_h, np.uint8)
            assert L.emba_seq_hot_pixels(ctx, _arr(hm, _lib._u8p)) == 0 and np.array_equal(hm, mask)
        beg, end = 300, nk - 57
        assert L.emba_group_set_events_seq(g, beg, end) == 0, L.emba_group_last_error(g)
        lo1 = window_shard_ranges(beg, end, world)[1][0]
        nh = C.c_size_t(0)
        ctx1 = L.emba_group_ctx(g, 1)
        assert L.emba_seq_halo(ctx1, beg, lo1, None, None, None, 0, C.byref(nh)) == 0
        hx, hy, hbt = np.empty(nh.value, np.uint16), np.empty(nh.value, np.uint16), np.empty(nh.value, np.int64)
        assert L.emba_seq_halo(ctx1, beg, lo1, _arr(hx, _lib._u16p), _arr(hy, _lib._u16p), _arr(hbt, _lib._i64p), nh.value, C.byref(nh)) == 0
        _, halo = shard_events(EventPacket(fx[beg:end], fy[beg:end], fp[beg:end], ft[beg:end]), w.sensor_w, 1, world)
        assert nh.value == len(halo[0]) > 100
        assert np.array_equal(hx, halo[0]) and np.array_equal(hy, halo[1]) and np.array_equal(hbt, halo[2])
    finally:
        L.emba_group_destroy(g)
