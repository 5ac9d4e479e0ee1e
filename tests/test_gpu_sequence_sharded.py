"""Time shards of a window of the resident sequence on the MI355X (include/emba_hip.h: emba_set_events_seq_shard, emba_seq_halo, emba_group_seq_*,
emba_group_set_events_seq, emba_group_median_blur3_map): the halo the device builds against the host's (emba_amd.sharded.shard_events on the downloaded
slice) bit for bit, the shard registration against the host-slice registration and the oracle, the group, and a two-window run of emba_amd/driver.py over
two rank threads.  Ranks are threads or a group on device 0, as in tests/test_gpu_sharded.py."""
import ctypes as C
import dataclasses
import threading

import numpy as np
import pytest

from emba_amd import io as eio
from emba_amd.legm import EventPacket, EventWindow
from emba_amd.sharded import batch_mid_ns, batch_ranges, merge_ep, shard_events, window_shard_ranges
from helpers import assert_close, oracle_run, small_workload

pytestmark = pytest.mark.gpu
ERR_INVALID_ARG, ERR_CAPACITY = 1, 6
MS = 1_000_000


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from emba_amd import build
    build.build_hip()
    return True


def make_legm(w, **options):
    from emba_amd import LEGM
    m = LEGM(w.sensor_w, w.sensor_h, w.lut, w.C_th, w.pano_w, w.pano_h, device=0)
    for k, v in options.items():
        m.set_option(k, v)
    return m


# ---- 1. the halo ------------------------------------------------------------------------------------------------------------------------------
HAND_SENSOR = (8, 6)
HAND_N = 1000
HAND_WIN_BEGS = (0, 137)
# the first event of every rank >= 1 of worlds 2 and 3 on the window [win_beg, 1000): batch_ranges(1000, .) and 137 + batch_ranges(863, .)
HAND_LOS = {0: (500, 400, 700), 137: (537, 437, 737)}


def hand_built_packet():
    """1000 events on an 8 x 6 sensor, sensor pixel p = y * 8 + x.  Pixel roles (every other event falls on the pixels 10 ... 47):
        0   one event, index 0: for win_beg = 0 the window's first event and the pixel's only one (offset 0 against the table's "none");
            for win_beg = 137 an event in front of the window, to be ignored
        1   one event, index 137: the same for win_beg = 137
        2   the event lo - 1 of every lo of HAND_LOS
        3   every index that is no multiple of 3 and carries no other role: hundreds of events in front of every lo (atomic contention)
        4   events at 737, 800 and 950 only: at or behind every lo
        6   299 and 300 with EQUAL timestamps: the two sides of a batch boundary of the grid of win_beg = 0 (the later index wins: another midpoint)
        7   336 and 337 with equal timestamps: the same on the grid of win_beg = 137
        8   5, 50 and 120 only: in front of win_beg = 137"""
    rng = np.random.default_rng(41)
    n, sw = HAND_N, HAND_SENSOR[0]
    pix = rng.integers(10, 48, n)
    idx = np.arange(n)
    pix[(idx % 3 != 0) & (idx >= 2) & (idx < 900)] = 3
    for los in HAND_LOS.values():
        for lo in los:
            pix[lo - 1] = 2
    pix[[737, 800, 950]] = 4
    pix[[299, 300]] = 6
    pix[[336, 337]] = 7
    pix[[5, 50, 120]] = 8
    pix[0], pix[137] = 0, 1
    t = 10**9 + np.cumsum(rng.integers(1, 5000, n)).astype(np.int64)      # irregular steps: the midpoints round
    t[300], t[337] = t[299], t[336]
    assert (np.diff(t) >= 0).all()
    return EventPacket((pix % sw).astype(np.uint16), (pix // sw).astype(np.uint16), rng.integers(0, 2, n).astype(np.uint8), t), pix


def test_hand_built_packet_holds_what_it_is_built_for():
    """(no device: the packet itself)"""
    ev, pix = hand_built_packet()
    at = lambda p: np.flatnonzero(pix == p)
    assert list(at(0)) == [0] and list(at(1)) == [137]
    for wb, los in HAND_LOS.items():
        n = HAND_N - wb
        assert sorted(los) == sorted(wb + batch_ranges(n, w)[r][0] for w in (2, 3) for r in range(1, w))
        for lo in los:
            assert pix[lo - 1] == 2
            assert np.count_nonzero(pix[wb:lo] == 3) >= 170
            assert at(4).min() >= lo
    assert pix[299] == pix[300] == 6 and ev.t_ns[299] == ev.t_ns[300] and at(6).size == 2
    assert pix[336] == pix[337] == 7 and ev.t_ns[336] == ev.t_ns[337] and at(7).size == 2
    assert at(8).max() < 137


def check_halos(m, n, sw, win_begs, worlds=(2, 3)):
    """sequence_halo(win_beg, lo) of every rank against shard_events on the DOWNLOADED slice [win_beg, n)."""
    seen = 0
    for wb in win_begs:
        ev = m.sequence_events(wb, n)
        for world in worlds:
            ranges = window_shard_ranges(wb, n, world)
            for rank in range(world):
                _, (hx, hy, hbt) = shard_events(ev, sw, rank, world)
                gx, gy, gbt = m.sequence_halo(wb, ranges[rank][0])
                assert gx.dtype == np.uint16 and gy.dtype == np.uint16 and gbt.dtype == np.int64
                assert gx.size == hx.size, (wb, world, rank, gx.size, hx.size)
                assert np.array_equal(gx, hx) and np.array_equal(gy, hy) and np.array_equal(gbt, hbt), (wb, world, rank)
                if rank == 0:
                    assert gx.size == 0
                else:
                    assert gx.size > 0
                seen += 1
    return seen


@pytest.mark.parametrize("poison", [0, 1])
def test_halo_of_the_hand_built_packet_equals_the_hosts(gpu, poison):
    ev, pix = hand_built_packet()
    sw, sh = HAND_SENSOR
    w = small_workload(n_events=2000, pano_h=64, sensor=HAND_SENSOR, focal=8.0)
    m = make_legm(w, poison=poison)
    assert m.set_sequence(ev, 1) == HAND_N
    assert check_halos(m, HAND_N, sw, HAND_WIN_BEGS) == 2 * (2 + 3)
    # the roles, spelled out (the host's halo has them too: this names what a wrong answer would have got wrong)
    t = ev.t_ns
    entry = lambda h, p: [(int(b)) for x, y, b in zip(*h) if int(y) * sw + int(x) == p]
    h = m.sequence_halo(0, 400)
    assert entry(h, 0) == [batch_mid_ns(t[0], t[99])]                              # offset 0 is an event, not "none"
    assert entry(h, 2) == [batch_mid_ns(t[300], t[399])] and (int(h[0][-1]), int(h[1][-1])) == (2, 0)      # lo - 1: the last entry
    assert entry(h, 6) == [batch_mid_ns(t[300], t[399])] != [batch_mid_ns(t[200], t[299])]                 # 300 wins over 299
    assert entry(h, 4) == [] and entry(h, 1) == [batch_mid_ns(t[100], t[199])] and len(entry(h, 3)) == 1 and entry(h, 8) == [batch_mid_ns(t[100], t[199])]
    h = m.sequence_halo(137, 437)
    assert entry(h, 0) == [] and entry(h, 8) == []                                 # in front of the window
    assert entry(h, 1) == [batch_mid_ns(t[137], t[236])]                           # the WINDOW's grid
    assert entry(h, 7) == [batch_mid_ns(t[337], t[436])] and entry(h, 6) == [batch_mid_ns(t[237], t[336])]
    assert len(h[0]) == np.unique(pix[137:437]).size
    m.close()


@pytest.mark.parametrize("sensor", [(64, 48), (50, 37)])
def test_halo_of_a_random_packet_equals_the_hosts(gpu, sensor):
    """30 050 events: several blocks of every pass and a ragged tail; 50 x 37: a sensor that is no multiple of anything."""
    sw, sh = sensor
    n = 30_050
    rng = np.random.default_rng(43)
    ev = EventPacket(rng.integers(0, sw, n).astype(np.uint16), rng.integers(0, sh, n).astype(np.uint16), rng.integers(0, 2, n).astype(np.uint8),
                     np.sort(rng.integers(10**9, 10**9 + 400 * MS, size=n)).astype(np.int64))
    w = small_workload(n_events=2000, sensor=sensor)
    m = make_legm(w, poison=1)
    assert m.set_sequence(ev, 1) == n
    assert check_halos(m, n, sw, HAND_WIN_BEGS) == 10
    m.close()


# ---- 2. the shard registration: rank threads ------------------------------------------------------------------------------------------------------
class _Shared:
    def __init__(self, world):
        self.world = world
        self.barrier = threading.Barrier(world)
        self.slots = [None] * world
        self.errors = []


class _ThreadDist:
    """torch.distributed-like handle for one rank-thread (the pattern of tests/test_gpu_sharded.py)."""

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


def run_rank_threads(world, target, *args, timeout=180):
    shared, results = _Shared(world), [None] * world

    def guarded(rank):
        try:
            results[rank] = target(shared, rank, *args)
        except Exception as e:  # noqa: BLE001
            shared.errors.append((rank, repr(e)))
            shared.barrier.abort()
            raise

    th = [threading.Thread(target=guarded, args=(r,)) for r in range(world)]
    [t.start() for t in th]
    [t.join(timeout=timeout) for t in th]
    assert not shared.errors, shared.errors
    assert all(r is not None for r in results)
    return results


def sharded_legm(shared, rank, w, K, **options):
    import torch
    from emba_amd.sharded import HipEngine, ShardedLEGM
    dev = torch.device("cuda", 0)
    npix = w.pano_h * w.pano_w
    m = make_legm(w, **options)
    count = torch.zeros(npix, dtype=torch.int32, device=dev)
    pack = torch.zeros(9 * K * K + 3 * K + 5 * npix, dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    return m, ShardedLEGM(HipEngine(m, check_stream=False), _ThreadDist(shared, rank, m.sync), count, pack, w.sensor_w, None), count


def embedded_sequence(w, n_front=1237, n_back=700, seed=5):
    """w.events with n_front events in front (win_beg > 0 and no multiple of 100) and n_back behind, on the same sensor."""
    rng = np.random.default_rng(seed)
    ev = w.events

    def extra(n, t_lo, t_hi):
        return (rng.integers(0, w.sensor_w, n).astype(np.uint16), rng.integers(0, w.sensor_h, n).astype(np.uint16), rng.integers(0, 2, n).astype(np.uint8),
                np.sort(rng.integers(t_lo, t_hi, n)).astype(np.int64))

    a = extra(n_front, int(ev.t_ns[0]) - 50 * MS, int(ev.t_ns[0]))
    b = extra(n_back, int(ev.t_ns[-1]) + 1, int(ev.t_ns[-1]) + 20 * MS)
    cat = [np.concatenate([p, q, r]) for p, q, r in zip(a, (ev.x, ev.y, ev.polarity, ev.t_ns), b)]
    return EventPacket(*cat), n_front, n_front + ev.size()


def _registration_rank(shared, rank, w, seq_ev, beg, end, resident, lam, fix):
    m, sh, count = sharded_legm(shared, rank, w, w.K, poison=1)
    if resident:
        assert sh.set_sequence(seq_ev, 1) == seq_ev.size()
        win = sh.set_events(EventWindow(beg, end))
        local = m.sequence_events(win.beg, win.end)
    else:
        local = sh.set_events(w.events)
    m.upload_map(w.Gx, w.Gy)
    out = None
    for _ in range(2):                    # twice: the second evaluation runs on what the first one left
        n_inl, out = sh.iteration(w.traj, w.thres_valid_pixel, w.alpha, download=True)
    x1, x2 = sh.solveNormalEq(lam, fix)
    d = m.dump_state(fields=("inlier_idx",))
    _, ep, _ = m.eval_finish(want_ep=True)
    pix = local.y.astype(np.int64) * w.sensor_w + local.x
    ep_pix = np.zeros(ep.size, dtype=np.int64)
    sel = d["inlier_idx"] >= 0
    ep_pix[d["inlier_idx"][sel]] = pix[: sel.size][sel]
    res = dict(ne=out, count=count.cpu().numpy().astype(np.int32), ep=ep.copy(), ep_pix=ep_pix, n_inl=n_inl, x1=x1, x2=x2, n_local=sh.n_local, n_max=sh.n_max,
               setup=m.setup_info(), n_halo=len(m.sequence_halo(beg, win.beg)[0]) if resident else None)
    m.close()
    return res


@pytest.fixture(scope="module")
def registration_case(oracle_mod):
    """The workload, the sequence around it and the oracle's answers on the slice: computed once, shared by the worlds."""
    w = small_workload(n_events=30050, pano_h=256, K=11, sensor=(64, 48), focal=60.0)
    seq_ev, beg, end = embedded_sequence(w)
    o = oracle_run(oracle_mod, w, dense_A12=True)
    lam, fix = 1e-2, True
    ox1, ox2 = oracle_mod.solve_normal_eq(o["ne"], lam, fix)
    return dict(w=w, seq_ev=seq_ev, beg=beg, end=end, o=o, lam=lam, fix=fix, ox1=ox1, ox2=ox2)


@pytest.mark.parametrize("world", [2, 3])
def test_shard_registration_matches_the_host_slices_and_the_oracle(gpu, registration_case, world):
    c = registration_case
    w, o = c["w"], c["o"]
    assert c["beg"] > 0 and c["beg"] % 100 != 0 and c["end"] - c["beg"] == 30050
    runs = {}
    for resident in (True, False):
        runs[resident] = run_rank_threads(world, _registration_rank, w, c["seq_ev"], c["beg"], c["end"], resident, c["lam"], c["fix"])
    dev, host = runs[True], runs[False]
    merged = {k: merge_ep([r["ep"] for r in v], [r["ep_pix"] for r in v]) for k, v in runs.items()}
    ranges = window_shard_ranges(c["beg"], c["end"], world)
    for r in range(world):
        g, h = dev[r], host[r]
        # what is integer or bit-exact today
        assert g["n_local"] == h["n_local"] and g["n_max"] == h["n_max"] and g["n_inl"] == h["n_inl"]
        assert g["setup"]["entries"] == h["setup"]["entries"] == g["n_local"] + g["n_halo"] and g["setup"]["set_events_ms"] > 0
        assert (g["n_halo"] == 0) == (r == 0) and ranges[r][1] - ranges[r][0] - g["n_local"] == (50 if r == world - 1 else 0)
        assert np.array_equal(g["count"], h["count"]) and np.array_equal(g["count"].reshape(w.pano_h, w.pano_w), o["num_ev_map"])
        assert np.array_equal(g["ne"]["active"], h["ne"]["active"]) and np.array_equal(g["ne"]["active"], o["ne"]["active"])
        assert np.array_equal(g["ep"], h["ep"]) and np.array_equal(g["ep_pix"], h["ep_pix"])      # a rank's residuals: the same kernels on the same structure
        for name in ("A11", "b1", "A22", "b2"):
            print(f"world {world} rank {r} {name}: vs host slices {np.abs(g['ne'][name] - h['ne'][name]).max():.3e}, vs oracle {np.abs(g['ne'][name] - o['ne'][name]).max():.3e}")
            assert_close(g["ne"][name], h["ne"][name], f"rank{r} host-sliced {name}")
            assert_close(g["ne"][name], o["ne"][name], f"rank{r} {name}")
        for name, ref in (("x1", c["ox1"]), ("x2", c["ox2"])):
            print(f"world {world} rank {r} {name}: vs host slices {np.abs(g[name] - h[name]).max():.3e}, vs oracle {np.abs(g[name] - ref).max():.3e} of {np.abs(ref).max():.3e}")
            assert_close(g[name], h[name], f"rank{r} host-sliced {name}")
            assert_close(g[name], ref, f"rank{r} {name}")
    assert np.array_equal(merged[True], merged[False])
    assert_close(merged[True], o["ep"], "merged ep")
    assert sum(r["n_inl"] for r in dev) == o["ep"].size


# ---- 3. the group -----------------------------------------------------------------------------------------------------------------------------------
def _arr(a, ty):
    return a.ctypes.data_as(ty)


@pytest.mark.parametrize("world,rate", [(2, 1), (3, 3), (2, 3), (3, 1)])
def test_group_registers_a_window_of_its_resident_sequence(gpu, registration_case, world, rate):
    from emba_amd import _lib
    L = _lib.load()
    w = registration_case["w"]
    ev = registration_case["seq_ev"]
    n = ev.size()
    x, y, pol, t = (np.ascontiguousarray(a, d) for a, d in ((ev.x, np.uint16), (ev.y, np.uint16), (ev.polarity, np.uint8), (ev.t_ns, np.int64)))
    lut = np.ascontiguousarray(w.lut, dtype=np.float64)
    knots = np.ascontiguousarray(w.traj.knots_xyzw, np.float64)
    Gx, Gy = np.ascontiguousarray(w.Gx), np.ascontiguousarray(w.Gy)
    npix = w.pano_h * w.pano_w
    t_beg, t_end = int(w.events.t_ns[0]) - MS, int(w.events.t_ns[-1]) - 5 * MS      # (the window ends inside the trajectory's time range)
    # a single context's answers
    m = make_legm(w)
    assert m.set_sequence(ev, rate) == n // rate
    want_win = m.sequence_window(t_beg, t_end)
    m.close()
    cfg = _lib.EmbaCfg(w.sensor_w, w.sensor_h, w.pano_w, w.pano_h, _arr(lut, _lib._dp), float(w.C_th), 100, 10.0, 0, None)
    g = C.c_void_p()
    devs = (C.c_int32 * world)(*([0] * world))
    assert L.emba_group_create(C.byref(cfg), devs, world, C.byref(g)) == 0, L.emba_group_last_error(None)
    try:
        assert L.emba_group_set_option(g, b"poison", 1) == 0
        kept, size = C.c_size_t(0), C.c_size_t(0)
        assert L.emba_group_seq_upload(g, _arr(x, _lib._u16p), _arr(y, _lib._u16p), _arr(pol, _lib._u8p), _arr(t, _lib._i64p), n, rate, C.byref(kept)) == 0, L.emba_group_last_error(g)
        assert L.emba_group_seq_size(g, C.byref(size)) == 0 and kept.value == size.value == n // rate
        b, e = C.c_size_t(0), C.c_size_t(0)
        assert L.emba_group_seq_window(g, t_beg, t_end, C.byref(b), C.byref(e)) == 0, L.emba_group_last_error(g)
        beg, end = b.value, e.value
        assert (beg, end) == want_win and beg > 0 and end - beg > 9000
        # every rank holds the whole sequence: the slice, downloaded from the LAST rank's copy
        m_slice = end - beg
        sx, sy, sp, st_ = np.empty(m_slice, np.uint16), np.empty(m_slice, np.uint16), np.empty(m_slice, np.uint8), np.empty(m_slice, np.int64)
        assert L.emba_seq_get(L.emba_group_ctx(g, world - 1), beg, end, _arr(sx, _lib._u16p), _arr(sy, _lib._u16p), _arr(sp, _lib._u8p), _arr(st_, _lib._i64p)) == 0
        want = tuple(a[rate - 1::rate][: n // rate][beg:end] for a in (x, y, pol, t)) if rate > 1 else (x[beg:end], y[beg:end], pol[beg:end], t[beg:end])
        assert all(np.array_equal(p, q) for p, q in zip((sx, sy, sp, st_), want))
        assert L.emba_group_upload_map(g, _arr(Gx, _lib._dp), _arr(Gy, _lib._dp)) == 0

        def step_and_fetch():
            n_inl, P = C.c_size_t(0), C.c_size_t(0)
            for _ in range(2):
                st = L.emba_group_step(g, _arr(knots, _lib._dp), w.K, int(w.traj.t0_ns), int(w.traj.dt_ns), w.thres_valid_pixel, 0, 0.0, w.alpha, C.byref(n_inl), C.byref(P))
                assert st == 0, L.emba_group_last_error(g)
            K, Pn = w.K, P.value
            A11, b1 = np.zeros((3 * K, 3 * K)), np.zeros(3 * K)
            act, A22, b2 = np.zeros(Pn, np.uint32), np.zeros(4 * Pn), np.zeros(2 * Pn)
            assert L.emba_group_download(g, _arr(A11, _lib._dp), _arr(b1, _lib._dp), _arr(act, _lib._u32p), Pn, _arr(A22, _lib._dp), _arr(b2, _lib._dp)) == 0, L.emba_group_last_error(g)
            ep, n2 = np.full(m_slice, np.nan), C.c_size_t(0)
            assert L.emba_group_get_ep(g, _arr(ep, _lib._dp), ep.size, C.byref(n2)) == 0, L.emba_group_last_error(g)
            assert n2.value == n_inl.value and not np.isnan(ep[: n2.value]).any()
            setup = []
            for r in range(world):
                ne_, ms = C.c_size_t(0), C.c_double(0)
                assert L.emba_last_setup_ms(L.emba_group_ctx(g, r), C.byref(ms), None, None, C.byref(ne_), None) == 0
                setup.append((ne_.value, ms.value))
            return dict(n_inl=n_inl.value, P=Pn, A11=A11, b1=b1, active=act, A22=A22, b2=b2, ep=ep[: n2.value].copy(), setup=setup)

        assert L.emba_group_set_events_seq(g, beg, end) == 0, L.emba_group_last_error(g)
        dev = step_and_fetch()
        assert L.emba_group_set_events(g, _arr(sx, _lib._u16p), _arr(sy, _lib._u16p), _arr(sp, _lib._u8p), _arr(st_, _lib._i64p), m_slice) == 0, L.emba_group_last_error(g)
        host = step_and_fetch()
        assert dev["n_inl"] == host["n_inl"] > 0 and dev["P"] == host["P"] > 0
        assert [s[0] for s in dev["setup"]] == [s[0] for s in host["setup"]] and all(s[1] > 0 for s in dev["setup"])      # events + halo entries of every rank
        assert np.array_equal(dev["active"], host["active"]) and np.array_equal(dev["ep"], host["ep"])
        for name in ("A11", "b1", "A22", "b2"):
            assert_close(dev[name], host[name], f"group {name}")
        # a range that is none: the registered window stays
        assert L.emba_group_set_events_seq(g, beg, n // rate + 1) == ERR_INVALID_ARG
        # the median blur of every replica
        assert L.emba_group_upload_map(g, _arr(Gx, _lib._dp), _arr(Gy, _lib._dp)) == 0
        assert L.emba_group_median_blur3_map(g) == 0, L.emba_group_last_error(g)
        bx, by = np.empty_like(Gx), np.empty_like(Gy)
        assert L.emba_group_download_map(g, _arr(bx, _lib._dp), _arr(by, _lib._dp)) == 0
        assert np.array_equal(bx, eio.median_blur3(Gx)) and np.array_equal(by, eio.median_blur3(Gy)) and not np.array_equal(bx, Gx)
        for r in range(world):
            rx, ry = np.empty(npix), np.empty(npix)
            assert L.emba_download_map(L.emba_group_ctx(g, r), _arr(rx, _lib._dp), _arr(ry, _lib._dp)) == 0
            assert np.array_equal(rx.reshape(Gx.shape), bx) and np.array_equal(ry.reshape(Gy.shape), by)
        assert L.emba_group_seq_free(g) == 0 and L.emba_group_seq_size(g, C.byref(size)) == 0 and size.value == 0
    finally:
        L.emba_group_destroy(g)


# ---- 4. two sliding windows over two rank threads ------------------------------------------------------------------------------------------------------
def _sequence_rank(shared, rank, w, pose_t, pose_q, seq, ba, lm, resident_sequence):
    from emba_amd.driver import run_sequence
    from emba_amd.sharded import ShardedModel
    m, sh, _ = sharded_legm(shared, rank, w, 13)
    model = ShardedModel(sh, m)
    kw = {} if resident_sequence is None else dict(resident_sequence=resident_sequence)
    r = run_sequence(model, w.events, pose_t, pose_q, w.Gx, w.Gy, seq, ba, lm, resident=True, **kw)
    last = r.windows[-1]
    lo, hi = window_shard_ranges(last.beg, last.end, shared.world)[rank]
    res = dict(run=r, maps=model.downloadMap(), n_seq=m.sequence_size(), setup=m.setup_info(), lo=lo, hi=hi,
               n_halo=len(m.sequence_halo(last.beg, lo)[0]) if m.sequence_size() else None)
    m.close()
    return res


def test_two_sliding_windows_over_two_rank_threads_stay_on_the_device(gpu, monkeypatch):
    from emba_amd import _lib
    from emba_amd.solver import BASettings, LMSettings
    from test_sequence_cpu import three_window_case
    w, pose_t, pose_q, seq = three_window_case()
    seq = dataclasses.replace(seq, t_end=0.55)                 # [0.1, 0.4] and [0.25, 0.55]
    ba, lm = BASettings(alpha=1.0), LMSettings(max_num_iter=5)
    world = 2
    L = _lib.load()
    calls = []
    real = L.emba_set_events
    monkeypatch.setattr(L, "emba_set_events", lambda *a: (calls.append(1), real(*a))[1])
    dev = run_rank_threads(world, _sequence_rank, w, pose_t, pose_q, seq, ba, lm, None, timeout=300)
    assert calls == [], "the resident run registered a window from host arrays"
    host = run_rank_threads(world, _sequence_rank, w, pose_t, pose_q, seq, ba, lm, False, timeout=300)
    assert len(calls) == 2 * world
    for r in range(world):
        g, h = dev[r], host[r]
        assert len(g["run"].windows) == len(h["run"].windows) == 2 and g["n_seq"] == w.events.size() and h["n_seq"] == 0
        for k, (a, b) in enumerate(zip(g["run"].windows, h["run"].windows)):
            assert (a.beg, a.end) == (b.beg, b.end) and a.end > a.beg, k                   # sequence_window against io.event_window
            assert [e[4] for e in a.result.log] == [e[4] for e in b.result.log], f"rank {r} window {k}: accept/reject sequence differs"
            assert a.result.iterations == b.result.iterations and a.result.converged == b.result.converged
            assert a.setup_ms > 0
        assert any(e[4] for wr in g["run"].windows for e in wr.result.log), "no LM step was accepted"
        # setup_info() reports this rank's registration of the last window: its whole batches + its halo
        assert g["setup"]["entries"] == ((g["hi"] - g["lo"]) // 100) * 100 + g["n_halo"] == h["setup"]["entries"] and (g["n_halo"] > 0) == (r > 0)
        print(f"rank {r}: knots differ by {np.abs(g['run'].traj.knots_xyzw - h['run'].traj.knots_xyzw).max():.3e}, "
              f"maps by {max(np.abs(p - q).max() for p, q in zip(g['maps'], h['maps'])):.3e}")
        assert_close(g["run"].traj.knots_xyzw, h["run"].traj.knots_xyzw, f"rank{r} knots")
        for name, p, q in zip(("Gx", "Gy"), g["maps"], h["maps"]):
            assert_close(p, q, f"rank{r} {name}")
        if r:
            assert np.array_equal(g["run"].traj.knots_xyzw, dev[0]["run"].traj.knots_xyzw)


# ---- 5. argument errors ---------------------------------------------------------------------------------------------------------------------------------
def test_shard_argument_errors_leave_the_window_usable(gpu, registration_case):
    from emba_amd import EmbaError, _lib
    L = _lib.load()
    c = registration_case
    w, beg, end = c["w"], c["beg"], c["end"]
    n = c["seq_ev"].size()
    m = make_legm(w)
    assert m.set_sequence(c["seq_ev"], 1) == n
    lo, hi = window_shard_ranges(beg, end, 2)[1]
    m.set_events_seq_shard(beg, lo, hi)
    nem = np.zeros((w.pano_h, w.pano_w), np.int32)
    ep = m.evaluateDataError(w.traj, w.Gx, w.Gy, None, True, nem).copy()
    entries = m.setup_info()["entries"]
    assert ep.size > 0 and entries > hi - lo - 100
    # off the window's batch grid; lo in front of the window; hi behind the sequence; lo behind hi
    for bad in ((beg, lo + 1, hi), (beg, lo - 50, hi), (lo + 100, lo, hi), (beg, lo, n + 1), (beg, hi + 100, hi)):
        with pytest.raises(EmbaError) as ei:
            m.set_events_seq_shard(*bad)
        assert ei.value.status == ERR_INVALID_ARG, bad
    for bad in ((beg, lo + 1), (lo + 100, lo), (beg, beg + 100 * ((n - beg) // 100 + 1))):
        with pytest.raises(EmbaError) as ei:
            m.sequence_halo(*bad)
        assert ei.value.status == ERR_INVALID_ARG, bad
    nem2 = np.zeros_like(nem)
    assert np.array_equal(m.evaluateDataError(w.traj, None, None, None, True, nem2), ep) and np.array_equal(nem2, nem) and m.setup_info()["entries"] == entries
    # lo == win_beg is emba_set_events_seq
    m.set_events_seq_shard(beg, beg, end)
    a = m.evaluateDataError(w.traj, None, None, None, True, nem2).copy()
    m.set_events(EventWindow(beg, end))
    assert np.array_equal(m.evaluateDataError(w.traj, None, None, None, True, nem), a) and np.array_equal(nem, nem2)
    # the halo's capacity
    hx, hy, hbt = m.sequence_halo(beg, lo)
    nh = hx.size
    assert nh > 1
    cnt = C.c_size_t(0)
    assert L.emba_seq_halo(m._ctx, beg, lo, None, None, None, 0, C.byref(cnt)) == 0 and cnt.value == nh          # the count only
    sx, sy, sb = np.zeros(nh, np.uint16), np.zeros(nh, np.uint16), np.zeros(nh, np.int64)
    cnt = C.c_size_t(0)
    st = L.emba_seq_halo(m._ctx, beg, lo, _arr(sx, _lib._u16p), _arr(sy, _lib._u16p), _arr(sb, _lib._i64p), nh - 1, C.byref(cnt))
    assert st == ERR_CAPACITY and cnt.value == nh and not sx.any() and not sb.any()
    assert L.emba_seq_halo(m._ctx, beg, lo, _arr(sx, _lib._u16p), _arr(sy, _lib._u16p), _arr(sb, _lib._i64p), nh, C.byref(cnt)) == 0
    assert np.array_equal(sx, hx) and np.array_equal(sy, hy) and np.array_equal(sb, hbt)
    m.close()
