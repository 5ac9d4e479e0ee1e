"""The sensor-noise filters on the CPU: emba_amd.io.filter_events against the plain loops of tests/filter_ref.py bit for bit, the driver's use of them
on the oracle model, and synth.add_sensor_noise.  tests/test_gpu_filter.py runs the same cases through emba_seq_filter on the device."""
import dataclasses
import functools

import numpy as np
import pytest

import filter_ref as FR
from emba_amd import io as eio, synth
from emba_amd.driver import SequenceSettings, run_sequence
from emba_amd.legm import EventPacket
from emba_amd.solver import BASettings, LMSettings
from helpers import OracleModel
from test_sequence_cpu import raw_poses, three_window_case

MS = 1_000_000
T_SPAN = 400 * MS
# hot_sigma, refractory_ns, support_ns
ALL3 = (3.0, 1 * MS, 25 * MS)
PARAMS = {"hot": (3.0, 0, 0), "refr": (0.0, 1 * MS, 0), "supp": (0.0, 0, 25 * MS), "all": ALL3}


@dataclasses.dataclass
class Case:
    name: str
    sw: int
    sh: int
    ev: EventPacket
    hot_sigma: float = 0.0
    refractory_ns: int = 0
    support_ns: int = 0
    rate: int = 1

    def args(self):
        return self.hot_sigma, self.refractory_ns, self.support_ns


# ---- inputs shared with tests/test_gpu_filter.py ---------------------------------------------------------------------------------------------------
def noisy_packet(n, sw, sh, seed, n_busy=3):
    """70 % of the events uniform over the sensor, 30 % on n_busy pixels (about 0.1 n events each in 400 ms: hot, and inside each other's refractory
    period); timestamps random, sorted, with ties."""
    rng = np.random.default_rng(seed)
    pix = rng.integers(0, sw * sh, n)
    busy = rng.choice(sw * sh, size=n_busy, replace=False)
    on_busy = rng.random(n) < 0.3
    pix[on_busy] = busy[rng.integers(0, n_busy, int(on_busy.sum()))]
    t = np.sort(rng.integers(10**9, 10**9 + T_SPAN, size=n)).astype(np.int64)
    return EventPacket((pix % sw).astype(np.uint16), (pix // sw).astype(np.uint16), rng.integers(0, 2, n).astype(np.uint8), t)


def one_pixel_packet(n=9000, sw=64, sh=48):
    """c: every event at one pixel — the longest chain.  Steps of 0 ... 2 ms around the 1-ms refractory period."""
    rng = np.random.default_rng(5)
    t = 10**9 + np.cumsum(rng.integers(0, 2 * MS, n)).astype(np.int64)
    return EventPacket(np.full(n, 17, np.uint16), np.full(n, 29, np.uint16), rng.integers(0, 2, n).astype(np.uint8), t)


def border_packet(n=3000, sw=64, sh=48):
    """d: events only at the four corners and along the borders — every neighbourhood is clipped."""
    rng = np.random.default_rng(6)
    border = [(x, y) for x in range(sw) for y in (0, sh - 1)] + [(x, y) for y in range(1, sh - 1) for x in (0, sw - 1)]
    corners = [(0, 0), (sw - 1, 0), (0, sh - 1), (sw - 1, sh - 1)]
    pick = rng.integers(0, len(border), n)
    xy = np.array([border[i] for i in pick])
    at_corner = rng.random(n) < 0.2
    xy[at_corner] = np.array(corners)[rng.integers(0, 4, int(at_corner.sum()))]
    t = np.sort(rng.integers(10**9, 10**9 + T_SPAN, size=n)).astype(np.int64)
    return EventPacket(xy[:, 0].astype(np.uint16), xy[:, 1].astype(np.uint16), rng.integers(0, 2, n).astype(np.uint8), t)


def ties_packet(n=5000, sw=64, sh=48):
    """e: blocks of equal timestamps, one across the tile boundary at index 4096 — equal times are ordered by index."""
    ev = noisy_packet(n, sw, sh, seed=8)
    t = ev.t_ns.copy()
    t[4000:4200] = t[4000]
    t[100:140] = t[100]
    t[4090:4100] = t[4090]
    t = np.maximum.accumulate(t)
    # a few pixels that fire twice inside a block, and neighbours inside a block
    x, y = ev.x.copy(), ev.y.copy()
    x[4095], y[4095] = 10, 10
    x[4096], y[4096] = 10, 10
    x[4097], y[4097] = 11, 10
    x[4094], y[4094] = 11, 11
    return EventPacket(x, y, ev.polarity, t)


def hot_supporter_packet(sw=16, sh=12):
    """g: pixel A = (5, 5) is hot (400 events); B = (6, 5) fires 2 ms behind events of A and has no other neighbour with events: its only supporter is
    a hot pixel, so with the hot test on B's events fail support, with it off they pass.  C = (12, 8) / D = (13, 8): an ordinary supported pair.  A
    thin uniform background keeps the statistics sane (200 pixels with a handful of events)."""
    rng = np.random.default_rng(9)
    ta = 10**9 + np.arange(400, dtype=np.int64) * MS
    tb = ta[::40] + 2 * MS
    tc = 10**9 + np.arange(6, dtype=np.int64) * 50 * MS + 7
    td = tc + 3 * MS
    nbg = 300
    bg_pix = rng.integers(0, sw * sh, nbg)
    bg_pix = bg_pix[~np.isin(bg_pix, [4 * sw + 4 + dx + dy * sw for dx in range(4) for dy in range(3)])][:250]      # none around A and B
    tbg = rng.integers(10**9, 10**9 + T_SPAN, bg_pix.size)
    x = np.concatenate([np.full(400, 5), np.full(tb.size, 6), np.full(6, 12), np.full(6, 13), bg_pix % sw])
    y = np.concatenate([np.full(400, 5), np.full(tb.size, 5), np.full(6, 8), np.full(6, 8), bg_pix // sw])
    t = np.concatenate([ta, tb, tc, td, tbg])
    order = np.argsort(t, kind="stable")
    return EventPacket(x[order].astype(np.uint16), y[order].astype(np.uint16), np.zeros(t.size, np.uint8), t[order].astype(np.int64))


@functools.lru_cache(maxsize=None)
def cases():
    cs = []
    for n in (0, 1, 99, 100):                                            # a
        cs.append(Case(f"a-n{n}", 16, 12, noisy_packet(n, 16, 12, seed=n + 1), *ALL3))
    for n in (4095, 4096, 4097, 3 * 4096 + 17):                          # b: one or several scan and sort tiles
        cs.append(Case(f"b-n{n}", 64, 48, noisy_packet(n, 64, 48, seed=n), *ALL3))
    cs.append(Case("b-16x12", 16, 12, noisy_packet(4097, 16, 12, seed=31), 3.0, 1 * MS, 2 * MS))      # one radix pass (8 bits)
    cs.append(Case("b-300x200", 300, 200, noisy_packet(3 * 4096 + 17, 300, 200, seed=32), 3.0, 1 * MS, 150 * MS))      # two (16 bits)
    cs.append(Case("c-one-pixel", 64, 48, one_pixel_packet(), 0.0, 1 * MS, 0))                         # c
    cs.append(Case("c-one-pixel-all", 64, 48, one_pixel_packet(), 3.0, 1 * MS, 25 * MS))
    cs.append(Case("d-borders", 64, 48, border_packet(), 0.0, 0, 30 * MS))                             # d
    cs.append(Case("d-borders-all", 64, 48, border_packet(), 2.0, 1 * MS, 30 * MS))
    cs.append(Case("e-ties", 64, 48, ties_packet(), *ALL3))                                            # e
    cs.append(Case("e-ties-refr", 64, 48, ties_packet(), 0.0, 1, 0))       # refractory 1 ns: exactly the equal-time successors fail
    f_ev = noisy_packet(6000, 64, 48, seed=40)                                                         # f
    for pname, p in PARAMS.items():
        for rate in (1, 2, 7):
            cs.append(Case(f"f-{pname}-r{rate}", 64, 48, f_ev, *p, rate))
    for rate in (1, 2, 7, 0):
        cs.append(Case(f"f-off-r{rate}", 64, 48, f_ev, 0.0, 0, 0, rate))
    cs.append(Case("g-hot-supporter", 16, 12, hot_supporter_packet(), 3.0, 0, 5 * MS))                 # g
    cs.append(Case("g-hot-off", 16, 12, hot_supporter_packet(), 0.0, 0, 5 * MS))
    cs.append(Case("h-all-removed", 64, 48, one_pixel_packet(500), 0.0, 0, 1 * MS))                    # h: one pixel has no neighbour support
    return cs


def case_names():
    return [c.name for c in cases()]


def case(name):
    return next(c for c in cases() if c.name == name)


@functools.lru_cache(maxsize=None)
def reference(name):
    """The loop reference of a case, computed once per session and shared (read-only)."""
    c = case(name)
    ev = c.ev
    (x, y, pol, t), stats, hot = FR.filter_loops(ev.x, ev.y, ev.polarity, ev.t_ns, c.sw, c.sh, c.hot_sigma, c.refractory_ns, c.support_ns, c.rate)
    for a in (x, y, pol, t, hot):
        a.setflags(write=False)
    return (x, y, pol, t), stats, hot


def noisy_scene(K=6, n_steps=4000, n_hot=4, hot_events_each=3000, n_background=1500, seed=17):
    """The committed small scene (synth.make_scene_workload defaults) plus injected noise; returns (workload with the noisy events, clean events, hot)."""
    w = synth.make_scene_workload(K=K, n_steps=n_steps)
    noisy, hot = synth.add_sensor_noise(w.events, (w.sensor_w, w.sensor_h), n_hot, hot_events_each, n_background, seed)
    return dataclasses.replace(w, events=noisy), w.events, hot


# ---- 1. the numpy form equals the loops ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", case_names())
def test_filter_events_equals_the_loops(name):
    c = case(name)
    want, stats, hot = reference(name)
    got, gstats, ghot = eio.filter_events(c.ev, c.sw, c.sh, *c.args())
    got = eio.downsample_events(got, c.rate)
    for g, o in zip((got.x, got.y, got.polarity, got.t_ns), want):
        assert np.array_equal(g, o) and g.dtype == o.dtype
    assert [int(v) for v in gstats[:5]] == stats[:5] and got.size() == stats[5]
    assert np.array_equal(ghot, hot) and ghot.dtype == np.uint8
    if not (c.hot_sigma > 0 or c.refractory_ns > 0 or c.support_ns > 0):
        assert eio.filter_events(c.ev, c.sw, c.sh)[0] is c.ev


def test_the_cases_exercise_every_test():
    """What the cases are built for, spelled out on the loop reference."""
    st = {n: reference(n)[1] for n in case_names()}
    for n in ("b-n4095", "b-n4096", "b-n4097", "b-n12305", "b-16x12", "b-300x200", "e-ties", "f-all-r1", "d-borders-all"):
        s = st[n]
        assert s[1] > 0 and s[2] > 0 and s[3] > 0 and 0 < s[4] < s[0] and 0 < s[5] < s[0], (n, s)
    assert st["a-n0"] == [0] * 6 and st["a-n1"][0] == 1
    s = st["c-one-pixel"]
    assert 3000 < s[3] < 6000 and s[5] == 9000 - s[3]
    assert st["c-one-pixel-all"][5] == 0 and st["h-all-removed"][5] == 0 and st["h-all-removed"][4] == 500
    assert 0 < st["d-borders"][4] < 3000
    ties = case("e-ties").ev.t_ns
    assert st["e-ties-refr"][3] > 0 and (np.diff(ties) == 0).sum() >= st["e-ties-refr"][3]
    assert st["f-hot-r1"][3] == st["f-hot-r1"][4] == 0 and st["f-refr-r1"][1] == 0 and st["f-all-r7"][5] == st["f-all-r1"][5] // 7
    assert st["f-off-r2"] == [6000, 0, 0, 0, 0, 3000] and st["f-off-r0"][5] == 6000
    # g: B's 10 events lose their only supporter when A is hot, and keep it when the hot test is off
    g_on, g_off = st["g-hot-supporter"], st["g-hot-off"]
    assert g_on[1] == 1 and g_on[2] == 400 and g_on[4] - g_off[4] == 10
    (x, y, _, _), _, _ = reference("g-hot-supporter")
    assert not ((x == 6) & (y == 5)).any() and ((x == 13) & (y == 8)).sum() == 6
    (x, y, _, _), _, _ = reference("g-hot-off")
    assert ((x == 6) & (y == 5)).sum() == 10


def test_nan_sigma_is_refused():
    c = case("a-n100")
    with pytest.raises(ValueError, match="NaN"):
        eio.filter_events(c.ev, c.sw, c.sh, float("nan"))


# ---- 2. synthetic noise ------------------------------------------------------------------------------------------------------------------------------
def test_add_sensor_noise_is_sorted_inside_the_sensor_and_reproducible():
    base = noisy_packet(5000, 64, 48, seed=3)
    a, hot_a = synth.add_sensor_noise(base, (64, 48), n_hot=3, hot_events_each=700, n_background=900, seed=4)
    b, hot_b = synth.add_sensor_noise(base, (64, 48), n_hot=3, hot_events_each=700, n_background=900, seed=4)
    for p, q in zip((a.x, a.y, a.polarity, a.t_ns, hot_a), (b.x, b.y, b.polarity, b.t_ns, hot_b)):
        assert np.array_equal(p, q)
    assert a.size() == 5000 + 3 * 700 + 900 and (np.diff(a.t_ns) >= 0).all() and a.t_ns.dtype == np.int64
    assert a.x.dtype == np.uint16 and (a.x < 64).all() and (a.y < 48).all() and set(np.unique(a.polarity)) <= {0, 1}
    assert a.t_ns[0] == base.t_ns[0] and a.t_ns[-1] == base.t_ns[-1]
    assert hot_a.size == 3 and np.unique(hot_a).size == 3
    pix = a.y.astype(np.int64) * 64 + a.x
    for p in hot_a:                                                  # uniformly spaced over the recording
        tp = a.t_ns[pix == p]
        assert tp.size >= 700 and np.isin(base.t_ns[0] + (np.arange(700) * (base.t_ns[-1] - base.t_ns[0])) // 700, tp).all()
    c, _ = synth.add_sensor_noise(base, (64, 48), n_hot=3, hot_events_each=700, n_background=900, seed=5)
    assert not np.array_equal(a.x, c.x)
    # the recording's own events keep their order (stable merge)
    d, _ = synth.add_sensor_noise(base, (64, 48), 0, 0, 0, seed=4)
    assert np.array_equal(d.t_ns, base.t_ns) and np.array_equal(d.x, base.x)


def test_injected_hot_pixels_are_exactly_the_hot_mask():
    """Construction: m pixels fire, H = 4 of them are injected with E = 3000 events each on top of a scene whose busiest pixel has C events.  With
    h = H / m, thr -> E (h + sigma sqrt(h (1 - h))) as E grows: an injected pixel (>= E events) exceeds it while sigma < sqrt((1 - h) / h) (27 for
    4 of 3072), and a scene pixel stays below sigma E sqrt(h (1 - h)) (540 at sigma 5) as long as C does.  The margins are asserted below."""
    w, clean, hot = noisy_scene()
    ev = w.events
    pix = ev.y.astype(np.int64) * w.sensor_w + ev.x
    counts = np.bincount(pix, minlength=w.sensor_w * w.sensor_h)
    c = counts[counts > 0].astype(np.float64)
    thr = c.mean() + 5.0 * c.std()
    others = np.delete(counts, hot)
    assert counts[hot].min() > 1.5 * thr and others.max() < 0.5 * thr, (counts[hot].min(), others.max(), thr)
    (x, y, pol, t), stats, mask = FR.filter_loops(ev.x, ev.y, ev.polarity, ev.t_ns, w.sensor_w, w.sensor_h, 5.0, 0, 0, 1)
    assert np.array_equal(np.flatnonzero(mask), hot) and stats[1] == 4 and stats[2] == counts[hot].sum() and stats[5] == ev.size() - stats[2]
    got, gstats, gmask = eio.filter_events(ev, w.sensor_w, w.sensor_h, 5.0)
    assert np.array_equal(gmask, mask) and np.array_equal(got.t_ns, t) and np.array_equal(got.x, x) and [int(v) for v in gstats] == stats


# ---- 3. the driver -----------------------------------------------------------------------------------------------------------------------------------
def noisy_three_window_case():
    w, pose_t, pose_q, seq = three_window_case()
    noisy, hot = synth.add_sensor_noise(w.events, (w.sensor_w, w.sensor_h), n_hot=4, hot_events_each=3000, n_background=1500, seed=17)
    seq = dataclasses.replace(seq, hot_pixel_sigma=5.0, refractory_period=20e-6, support_time=0.02, event_sampling_rate=2)
    return dataclasses.replace(w, events=noisy), pose_t, pose_q, seq, hot


def test_run_sequence_filters_like_a_prefiltered_recording(oracle_mod):
    w, pose_t, pose_q, seq, hot = noisy_three_window_case()
    ba, lm = BASettings(alpha=1.0), LMSettings(max_num_iter=2)
    ev = w.events
    (x, y, pol, t), stats, mask = FR.filter_loops(ev.x, ev.y, ev.polarity, ev.t_ns, w.sensor_w, w.sensor_h, 5.0, 20_000, 20 * MS, 1)
    assert np.array_equal(np.flatnonzero(mask), hot) and stats[3] > 0 and stats[4] > 0
    r = run_sequence(OracleModel(oracle_mod, w), ev, pose_t, pose_q, w.Gx, w.Gy, seq, ba, lm, resident=False)
    off = dataclasses.replace(seq, hot_pixel_sigma=0.0, refractory_period=0.0, support_time=0.0)
    r0 = run_sequence(OracleModel(oracle_mod, w), EventPacket(x, y, pol, t), pose_t, pose_q, w.Gx, w.Gy, off, ba, lm, resident=False)
    assert r0.filter_stats is None and [int(v) for v in r.filter_stats] == stats[:5] + [stats[5] // 2]
    assert r.n_events == r0.n_events == stats[5] // 2 and len(r.windows) == len(r0.windows) == 3
    for a, b in zip(r.windows, r0.windows):
        assert (a.beg, a.end) == (b.beg, b.end) and a.result.log == b.result.log
        assert np.array_equal(a.result.traj.knots_xyzw, b.result.traj.knots_xyzw)
    assert np.array_equal(r.traj.knots_xyzw, r0.traj.knots_xyzw)


class Recorder:
    """A model that keeps a sequence and records every call the driver makes before the first window."""

    def __init__(self):
        self.calls = []

    def set_sequence(self, events, sampling_rate=1):
        self.calls.append(("set_sequence", events.size(), sampling_rate))
        return events.size() // max(sampling_rate, 1)

    def filter_sequence(self, hot_sigma, refractory_ns, support_ns, sampling_rate):
        self.calls.append(("filter_sequence", hot_sigma, refractory_ns, support_ns, sampling_rate))
        return np.array([10, 0, 0, 0, 0, 5], np.uint64)

    def sequence_window(self, t_beg_ns, t_end_ns):
        self.calls.append(("sequence_window", t_beg_ns, t_end_ns))
        raise StopIteration


def test_defaults_change_no_call():
    """Filters off (the default): set_sequence(events, rate) and nothing else before the first window, filter_stats None.  Filters on: an upload at rate 1,
    then the filter with the rate, the two times as integer nanoseconds."""
    w = synth.make_scene_workload(n_steps=200)
    pose_t, pose_q = raw_poses(w.traj)
    seq = SequenceSettings(time_window_size=0.25, sliding_window_stride=0.25, t_start=0.1, t_end=0.35, event_sampling_rate=3, median_blur=False)
    assert (seq.hot_pixel_sigma, seq.refractory_period, seq.support_time) == (0.0, 0.0, 0.0)
    m = Recorder()
    with pytest.raises(StopIteration):
        run_sequence(m, w.events, pose_t, pose_q, w.Gx, w.Gy, seq)
    assert m.calls == [("set_sequence", w.events.size(), 3), ("sequence_window", 100 * MS, 350 * MS)]
    m = Recorder()
    with pytest.raises(StopIteration):
        run_sequence(m, w.events, pose_t, pose_q, w.Gx, w.Gy, dataclasses.replace(seq, hot_pixel_sigma=4.0, refractory_period=1e-3, support_time=0.01))
    assert m.calls == [("set_sequence", w.events.size(), 1), ("filter_sequence", 4.0, MS, 10 * MS, 3), ("sequence_window", 100 * MS, 350 * MS)]
    from emba_amd.driver import SequenceResult
    assert SequenceResult(None).filter_stats is None
