"""Loop-closure pairs found by appearance on the MI355X (include/emba_hip.h: emba_frames_match_eval, emba_frames_match_search) against the
numpy forms of the same rule (emba_amd.io: match_sums, match_best, match_search on pair_level_bytes).  Everything is held exactly: the six sums of every shift
as equal integers, the score of every pair bit for bit, shifts, counts and partners as equal integers.  Then the search's rules, the chunk edge at 2^20 pairs,
determinism, every refusal and what a call leaves alone, the driver and examples/run_ba.py.  tests/match_cases.py has the cases and the figures, measured with
numpy."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import match_cases as MC
import pair_cases as PC
from emba_amd import _lib
from emba_amd import io as eio
from emba_amd import synth
from test_gpu_pair import ERR_INVALID_ARG, PAIR_SETS, bits, make_legm, ptr, small_case

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_dp, _u8p, _i32p, _u64p = (C.POINTER(t) for t in (C.c_double, C.c_uint8, C.c_int32, C.c_uint64))
# 64 x 48 at level 2: 16 x 12, a width that is a multiple of 4; 20 x 13 at level 0: rows that do not fill a dword, an odd height; 9 x 7 at level 0 with the
# widest range allowed: the overlap shrinks to one pixel and n_min decides
SHAPES = (((64, 48), 2, 6, 4), ((20, 13), 0, 3, 2), ((9, 7), 0, 8, 6))


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from emba_amd import build
    build.build_hip()
    return True


def frames_of(sensor):
    """tests/test_gpu_pair.py's small frames (a fifth of the bytes zero), with zero bytes in the corners where the overlap of the widest shifts lies"""
    fr = small_case(sensor)[0].copy()
    fr[:, 0, 0] = fr[:, -1, -1] = fr[1, 0, -1] = 0
    return fr


def same_search(got, want):
    return (np.array_equal(got["partner"], want["partner"]) and np.array_equal(bits(got["score"]), bits(want["score"])) and np.array_equal(got["shift"], want["shift"])
            and np.array_equal(got["n"], want["n"]))


@pytest.mark.parametrize("sensor,level,rx,ry", SHAPES, ids=lambda v: str(v).replace(" ", ""))
@pytest.mark.parametrize("P", (1, 3))
def test_pair_lists_against_numpy(gpu, sensor, level, rx, ry, P):
    fr = frames_of(sensor)
    m = make_legm(sensor)
    m.set_option("poison", 1)
    pairs = PAIR_SETS[P]
    wl, hl = eio.pair_level_size(sensor, level)
    scored = 0
    for skip_zero in (False, True):
        th = eio.pair_level_bytes(fr, level, skip_zero)
        for n_min in (1, wl * hl // 3):
            what = f"{sensor}, level {level}, range ({rx}, {ry}), P = {P}, skip_zero = {skip_zero}, n_min = {n_min}"
            g = m.match_eval(fr, pairs, level, rx, ry, skip_zero=skip_zero, n_min=n_min, want_sums=True)
            assert g["sums"].shape == (P, (2 * rx + 1) * (2 * ry + 1), 6), what
            for p, (i, j) in enumerate(pairs):
                b = eio.match_best(th[i], th[j], rx, ry, skip_zero, n_min)
                assert np.array_equal(g["sums"][p], b["sums"]), (what, p)
                assert bits(g["score"][p]) == bits(b["score"]) and g["shift"][p].tolist() == [b["dx"], b["dy"]] and g["n"][p] == b["n"], (what, p, g["score"][p], b)
                scored += b["n"] > 0
                if i == j:
                    assert g["score"][p] == 1.0 or b["n"] == 0, what
            if P == 3:      # the pair listed twice gives the same bits twice
                assert bits(g["score"][1]) == bits(g["score"][2]) and np.array_equal(g["sums"][1], g["sums"][2]), what
            h = m.match_eval(fr, pairs, level, rx, ry, skip_zero=skip_zero, n_min=n_min)      # without the sums: the same records
            assert h["sums"] is None and np.array_equal(bits(h["score"]), bits(g["score"])) and np.array_equal(h["shift"], g["shift"]) and np.array_equal(h["n"], g["n"])
    assert scored > 0
    m.close()


def test_one_shift_and_frames_without_a_score(gpu):
    """rx = ry = 0 is one shift; a frame against itself scores exactly 1.0 at (0, 0); a constant frame, and under skip_zero an all-zero frame, are unscored:
    -2, (0, 0), 0."""
    sensor = (20, 13)
    fr = frames_of(sensor)
    fr[2] = 77
    fr[3] = 0
    m = make_legm(sensor)
    m.set_option("poison", 1)
    pairs = [(0, 0), (0, 1), (1, 0), (2, 0), (0, 2), (3, 0), (3, 3), (2, 2)]
    for skip_zero in (False, True):
        g = m.match_eval(fr, pairs, 0, 0, 0, skip_zero=skip_zero, n_min=1, want_sums=True)
        assert g["sums"].shape == (len(pairs), 1, 6) and g["score"][0] == 1.0 and not g["shift"].any()
        assert bits(g["score"][1]) == bits(g["score"][2]) and g["n"][1] == g["n"][2]      # (one shift: the sums are symmetric)
        assert bits(g["score"][1]) == bits(eio.match_best(fr[0], fr[1], 0, 0, skip_zero, 1)["score"])
        assert (g["score"][3:] == eio.MATCH_UNSCORED).all() and not g["n"][3:].any()
        w = m.match_eval(fr, pairs, 0, 3, 2, skip_zero=skip_zero, n_min=20)
        assert w["score"][0] == 1.0 and w["shift"][0].tolist() == [0, 0] and (w["score"][3:] == eio.MATCH_UNSCORED).all() and not w["shift"][3:].any() and not w["n"][3:].any()
    m.close()


def test_the_search_against_numpy(gpu):
    """F = 12 of tests/match_cases.py: numpy's [F, k] partners, scores, shifts and counts exactly, k = 1 and k = 3, at level 1 and level 2; a lost frame is
    never a partner; min_gap = F - 2 leaves one pair, F - 1 none; identical frames tie to the lower index; score_min above every score gives all -1."""
    fr = MC.frames3()
    status = MC.drifted()[1]
    m = make_legm(MC.SENSOR, lut=MC.case()["lut"])
    m.set_option("poison", 1)
    for level in (1, 2):
        rx, ry = MC.RANGE[level]
        kw = dict(level=level, rx=rx, ry=ry, min_gap=MC.GAP, skip_zero=True, n_min=MC.N_MIN[level], score_min=MC.SCORE_MIN)
        for k in (1, 3):
            got, want = m.match_search(fr, status, k=k, **kw), eio.match_search(fr, status, k=k, **kw)
            assert same_search(got, want), (level, k)
        got = m.match_search(fr, status, k=MC.K, **kw)
        assert same_search(got, MC.search_numpy(level))
        found = [tuple(p) for p in eio.match_pairs(got).tolist()]
        if MC.FINDS:      # what numpy showed, on the device: the search finds true loops where the rotations propose none
            assert len(found) == MC.N_MATCHED[level] and all(p in MC.true_loops() for p in found) and len([p for p in found if p not in MC.SAME_BYTES]) == MC.N_DISTINCT[level]
        for a, b in MC.SAME_BYTES:      # the same bytes: exactly 1 at (0, 0), each the other's first partner
            assert got["partner"][a, 0] == b and got["partner"][b, 0] == a and got["score"][a, 0] == 1.0 and not got["shift"][a, 0].any()
    kw = dict(level=2, rx=6, ry=4, skip_zero=True, n_min=48)
    lost = status.copy()
    lost[[3, 9]] = 3
    got, want = m.match_search(fr, lost, min_gap=2, score_min=-1.0, k=4, **kw), eio.match_search(fr, lost, min_gap=2, score_min=-1.0, k=4, **kw)
    assert same_search(got, want) and not np.isin(got["partner"], (3, 9)).any() and (got["partner"][[3, 9]] == -1).all() and (got["partner"][0] >= 0).all()
    got = m.match_search(fr, None, min_gap=MC.F - 2, score_min=-1.0, k=2, **kw)
    assert same_search(got, eio.match_search(fr, None, min_gap=MC.F - 2, score_min=-1.0, k=2, **kw)) and eio.match_pairs(got).tolist() == [[0, MC.F - 1]]
    m.enable_kernel_timing(True)
    m.match_search(fr, None, min_gap=0, score_min=-1.0, k=1, **kw)
    m.sync()
    t7 = m.timer_ms(7)
    got = m.match_search(fr, None, min_gap=MC.F - 1, score_min=-1.0, k=2, **kw)      # no candidate pair: nothing is launched, the timer keeps its events
    m.sync()
    assert (got["partner"] == -1).all() and (got["score"] == eio.MATCH_UNSCORED).all() and not got["shift"].any() and not got["n"].any() and m.timer_ms(7) == t7 and t7 > 0
    m.enable_kernel_timing(False)
    got = m.match_search(fr, status, min_gap=MC.GAP, score_min=1.5, k=2, **kw)
    assert (got["partner"] == -1).all() and (got["score"] == eio.MATCH_UNSCORED).all()
    same = fr[[0, 5, 0, 0, 7, 0]]      # identical frames: ties to the lower partner index
    got = m.match_search(same, None, min_gap=0, score_min=0.0, k=3, **kw)
    assert same_search(got, eio.match_search(same, None, min_gap=0, score_min=0.0, k=3, **kw)) and got["partner"][0].tolist() == [2, 3, 5] and got["partner"][3].tolist() == [0, 2, 5]
    m.close()


def test_chunk_edge(gpu):
    """8 x 8 frames at level 0, rx = ry = 1, F = 1450: 1 050 525 pairs, 1 949 more than one launch's 2^20.  The [F, 1] result equals numpy's for every frame —
    the frames whose pairs straddle the cut among them."""
    F, cut = 1450, 1 << 20
    rng = np.random.default_rng(8)
    base = rng.integers(0, 256, (40, 8, 8)).astype(np.uint8)
    fr = np.clip(base[rng.integers(0, 40, F)].astype(np.int64) + rng.integers(-20, 21, (F, 8, 8)), 0, 255).astype(np.uint8)
    rows = np.cumsum([0] + [F - 1 - i for i in range(F - 1)])      # the first table index of every row
    i_cut = int(np.searchsorted(rows, cut, side="right") - 1)
    j_cut = i_cut + 1 + cut - int(rows[i_cut])
    assert rows[-1] == F * (F - 1) // 2 == 1050525 and 0 < i_cut < F - 2 and i_cut < j_cut < F      # the cut lies inside row i_cut
    m = make_legm((8, 8))
    m.set_option("poison", 1)
    kw = dict(level=0, rx=1, ry=1, min_gap=0, skip_zero=True, n_min=16, score_min=-1.0, k=1)
    got, want = m.match_search(fr, None, **kw), eio.match_search(fr, None, **kw)
    assert (got["partner"] >= 0).all()
    for f in (0, i_cut - 1, i_cut, i_cut + 1, j_cut - 1, j_cut, F - 2, F - 1):
        assert got["partner"][f, 0] == want["partner"][f, 0] and bits(got["score"][f, 0]) == bits(want["score"][f, 0]), f
    assert same_search(got, want)
    # the pairs on both sides of the cut, as a list, are the table's records
    pr = [(i_cut, j_cut - 1), (i_cut, j_cut), (i_cut, min(j_cut + 1, F - 1))]
    e = m.match_eval(fr, pr, 0, 1, 1, skip_zero=True, n_min=16)
    for p, (i, j) in enumerate(pr):
        b = eio.match_best(fr[i], fr[j], 1, 1, True, 16)
        assert bits(e["score"][p]) == bits(b["score"]) and e["shift"][p].tolist() == [b["dx"], b["dy"]] and e["n"][p] == b["n"]
    m.close()


def test_determinism_and_independence(gpu):
    sensor, level, rx, ry = SHAPES[0]
    fr = frames_of(sensor)
    m = make_legm(sensor)
    pairs = [(0, 1), (2, 2), (1, 3), (3, 0)]
    a = m.match_eval(fr, pairs, level, rx, ry, skip_zero=True, n_min=8, want_sums=True)
    s = m.match_search(fr, None, level=level, rx=rx, ry=ry, min_gap=0, skip_zero=True, n_min=8, score_min=-1.0, k=2)
    m.pair_level_eval(fr, [(0, 1)], [[0.0, 0.0, 0.0, 1.0]], PC.PINHOLE, 1, skip_zero=True)      # another stage's call in between
    m.match_eval(fr[::-1].copy(), pairs, 0, 1, 1)
    b = m.match_eval(fr, pairs, level, rx, ry, skip_zero=True, n_min=8, want_sums=True)
    t = m.match_search(fr, None, level=level, rx=rx, ry=ry, min_gap=0, skip_zero=True, n_min=8, score_min=-1.0, k=2)
    assert np.array_equal(bits(a["score"]), bits(b["score"])) and np.array_equal(a["shift"], b["shift"]) and np.array_equal(a["n"], b["n"]) and np.array_equal(a["sums"], b["sums"])
    assert same_search(s, t)
    m.close()


def test_refusals_and_what_a_call_leaves_alone(gpu):
    """Every refusal, in the order the header states, leaves the outputs untouched, and so it and the calls themselves leave the context: the mosaic's sums,
    the level planes, the step path's ep and the resident map, bit for bit before and after."""
    w = synth.make_scene_workload()          # 64x48 on 256x512
    S, F, P, K = 64 * 48, 4, 3, 2
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
    shifts = 13 * 9
    vals = dict(score=4.25, shift=7, n=77, sums=55, partner=9, kscore=2.5, kshift=6, kn=5)
    shapes = dict(score=(P,), shift=(P, 2), n=(P,), sums=(P, shifts, 6), partner=(F, K), kscore=(F, K), kshift=(F, K, 2), kn=(F, K))
    types = dict(shift=np.int32, n=np.uint64, sums=np.uint64, partner=np.int32, kshift=np.int32, kn=np.uint64)
    out = {k: np.full(shapes[k], v, types.get(k, np.float64)) for k, v in vals.items()}
    pairs = np.array([[0, 1], [2, 2], [3, 0]], np.int32)
    status = np.array([1, 2, 2, 2], np.int32)

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

    def call_eval(fr=frames, F_=F, pr=pairs, P_=P, level=2, rx=6, ry=4, n_min=8, **_):
        return L.emba_frames_match_eval(m._ctx, ptr(fr, _u8p), F_, ptr(pr, _i32p), P_, level, rx, ry, 1, n_min, ptr(out["score"], _dp), ptr(out["shift"], _i32p),
                                        ptr(out["n"], _u64p), ptr(out["sums"], _u64p))

    def call_search(fr=frames, F_=F, st=status, level=2, rx=6, ry=4, n_min=8, k=K, min_gap=0, score_min=0.0, **_):
        return L.emba_frames_match_search(m._ctx, ptr(fr, _u8p), F_, ptr(st, _i32p), level, rx, ry, min_gap, 1, n_min, score_min, k, ptr(out["partner"], _i32p),
                                          ptr(out["kscore"], _dp), ptr(out["kshift"], _i32p), ptr(out["kn"], _u64p))

    nan = float("nan")
    at = lambda base, idx, v: (lambda a: (a.__setitem__(idx, v), a)[1])(base.copy())      # noqa: E731
    err = lambda: L.emba_last_error(m._ctx)      # noqa: E731
    many = (1 << 30) // S + 1
    # each refusal with every later one also wrong: the first is reported
    later = [dict(fr=None), dict(F_=0), dict(F_=1 << 31), dict(pr=None), dict(P_=1 << 31), dict(pr=at(pairs, (1, 0), F)), dict(pr=at(pairs, (2, 1), -1)), dict(level=8),
             dict(level=-1), dict(level=5), dict(rx=-1), dict(rx=16), dict(ry=12), dict(n_min=0), dict(k=0), dict(k=65), dict(min_gap=-1), dict(score_min=nan), dict(F_=many)]
    words = [b"frames NULL", b"F = 0", b"31 bits", b"pairs NULL", b"P = ", b"pairs[1]", b"pairs[2]", b"level = 8", b"level = -1", b"level 5 of a 64 x 48", b"rx = -1",
             b"rx = 16", b"ry = 12", b"n_min = 0", b"k = 0", b"k = 65", b"min_gap", b"score_min", b"resident sequence"]
    only_list, only_search = {3, 4, 5, 6}, {14, 15, 16, 17}
    for call, skip in ((call_eval, only_search), (call_search, only_list)):
        for n in range(len(later)):
            if n in skip:
                continue
            kw = {}
            for later_kw in reversed(later[n:]):      # (the earliest setting of an argument wins: it is the refusal under test)
                kw.update(later_kw)
            if n in (5, 6):
                kw.pop("F_")      # (the frame a pair names is outside the true F)
            assert call(**kw) == ERR_INVALID_ARG and untouched() and words[n] in err(), (call.__name__, n, err())
    # 240 x 180 at level 0 does not fit a thumbnail, and the message names the level that does; the table of a search is bounded
    big = make_legm((240, 180))
    fb = np.ones((2, 180, 240), np.uint8)
    for lvl, word in ((0, b"smallest level that fits is 1"), (7, b"level 7 of a 240 x 180")):
        rc = big._L.emba_frames_match_eval(big._ctx, ptr(fb, _u8p), 2, ptr(pairs[:1], _i32p), 1, lvl, -1, 0, 1, 0, ptr(out["score"], _dp), None, None, None)
        assert rc == ERR_INVALID_ARG and word in big._L.emba_last_error(big._ctx) and untouched()
    big.close()
    tiny = make_legm((8, 8))
    rc = tiny._L.emba_frames_match_search(tiny._ctx, ptr(np.ones(64, np.uint8), _u8p), 9460, None, 0, 1, 1, 0, 1, 1, 0.0, 1, ptr(out["partner"], _i32p), None, None, None)
    assert rc == ERR_INVALID_ARG and b"table of a search" in tiny._L.emba_last_error(tiny._ctx) and untouched()
    tiny.close()
    assert call_eval(P_=0, pr=None) == 0 and untouched()      # P = 0: nothing launched, nothing written
    assert context_untouched()
    # the calls themselves go, write every output and leave the context alone
    assert call_eval() == 0 and call_search() == 0 and not any((out[k] == v).all() for k, v in vals.items())
    th = eio.pair_level_bytes(frames, 2, True)
    for p, (i, j) in enumerate(pairs):
        assert np.array_equal(out["sums"][p], eio.match_best(th[i], th[j], 6, 4, True, 8)["sums"])
    want = eio.match_search(frames, status, 2, 6, 4, 0, True, 8, 0.0, K)
    assert np.array_equal(out["partner"], want["partner"]) and np.array_equal(bits(out["kscore"]), bits(want["score"])) and np.array_equal(out["kshift"], want["shift"])
    assert call_search(st=None) == 0 and call_search(min_gap=3) == 0 and (out["partner"] == -1).all()      # (no candidate: the outputs say "none")
    assert context_untouched()
    m.close()


def test_the_driver(gpu):
    """close_search = "rotations" makes exactly the parent's calls and returns its arrays on tests/pair_cases.py's closing case; "appearance" on
    tests/match_cases.py's case gives numpy's pairs, sources and starts, and what the cases assert."""
    from emba_amd.driver import SequenceSettings, close_tracked_frames
    c = PC.case(False)
    q, status = PC.drifted()
    fr = c["frames"].reshape(PC.F, PC.SH, PC.SW)
    common = dict(track_close=True, close_window=PC.CANDIDATES["window"], close_gap=PC.CANDIDATES["min_gap"], close_angle=PC.CANDIDATES["max_angle"],
                  close_per_frame=PC.CANDIDATES["max_per_frame"], close_min_overlap=PC.MIN_OVERLAP)
    tracked = dict(q=q.copy(), status=status.copy(), tracked=PC.F - 1, lost=0)
    kw = dict(levels=(1, 0), batch=1, skip_zero=True, min_weight=256, min_overlap=0.3, **PC.SETTINGS)
    m = make_legm(PC.SENSOR, lut=c["lut"])
    calls = []
    for name in ("match_search", "pair_align", "pair_align_levels"):
        setattr(m, name, (lambda fn, name: lambda *a, **k: (calls.append(name), fn(*a, **k))[1])(getattr(m, name), name))
    base = close_tracked_frames(m, fr, c["ts"], tracked, SequenceSettings(1.0, 1.0, close_search="rotations", **common), c["calib"], **kw)
    assert calls == ["pair_align"]
    pairs = eio.pair_candidates(q, status, **PC.CANDIDATES)
    Q0, a0, b0 = eio.pair_start(q, None, None, pairs)
    al = m.pair_align(fr, pairs, Q0, c["calib"], gain=a0, bias=b0, skip_zero=True, **dict(PC.SETTINGS, huber_k=0.0))
    n = al["counts"][:, 0]
    keep = ((al["status"] == eio.ALIGN_CONVERGED) | (al["status"] == eio.ALIGN_ITERATIONS)) & (n >= PC.MIN_OVERLAP * PC.SW * PC.SH)
    g = m.rotation_graph_solve(q, status, pairs[keep], al["q"][keep], eio.pair_information(al["sums"], al["counts"], floor=eio.PAIR_NOISE_FLOOR)[keep])
    want = dict(q=g["q"], pairs=pairs, pair_status=al["status"], pair_n=n, pair_cost=al["sums"][:, 9] / np.maximum(n, 1), pair_kept=keep,
                pair_moved=eio.rotation_angle_between(Q0, al["q"]))
    for k, v in want.items():
        assert np.array_equal(bits(base[k]), bits(v)) if v.dtype == np.float64 else np.array_equal(base[k], v), k
    assert np.array_equal(base["pair_source"], np.where(pairs[:, 1] - pairs[:, 0] <= PC.CANDIDATES["window"], 0, 1)) and (base["pair_match_score"] == eio.MATCH_UNSCORED).all()
    m.close()
    # the new case: the drift hides every loop from the rotations
    c = MC.case()
    q, status = MC.drifted()
    fr = MC.frames3()
    tracked = dict(q=q.copy(), status=status.copy(), tracked=MC.F - 1, lost=0)
    m = make_legm(MC.SENSOR, lut=c["lut"])
    ends = {}
    for mode in ("rotations", "appearance"):
        seq = SequenceSettings(1.0, 1.0, track_close=True, close_search=mode, close_levels=MC.SCHEDULE, close_match_level=2, close_match_range=MC.RANGE[2],
                               close_match_score=MC.SCORE_MIN, close_match_per_frame=MC.K, close_match_min_overlap=0.25, close_min_overlap=MC.MIN_OVERLAP)
        r = close_tracked_frames(m, fr, c["ts"], tracked, seq, c["calib"], **kw)
        pairs, source, Q0, score, shift = MC.closing_pairs(mode)
        assert np.array_equal(r["pairs"], pairs) and np.array_equal(r["pair_source"], source) and np.array_equal(bits(r["pair_match_score"]), bits(score))
        assert np.array_equal(r["pair_match_shift"], shift) and r["graph"]["end"] == eio.GRAPH_CONVERGED and np.array_equal(bits(r["q"][0]), bits(q[0]))
        ends[mode] = MC.worst_angle(r["q"])
        print(f"{mode}: {len(r['pairs'])} pairs, sources {np.bincount(r['pair_source'], minlength=3).tolist()}, {int(r['pair_kept'].sum())} kept; worst angle "
              f"{MC.worst_angle(q):.4e} -> {ends[mode]:.4e} rad (numpy: {MC.E_ROTATIONS if mode == 'rotations' else MC.E_APPEARANCE:.4e})")
    if MC.FINDS:
        assert (r["pair_source"] == 2).sum() == MC.N_MATCHED[2] and r["pair_kept"][r["pair_source"] == 2].any()
    if MC.IMPROVES:
        assert ends["appearance"] < ends["rotations"] < MC.worst_angle(q)
    m.close()


def test_run_ba_closes_by_appearance(gpu, tmp_path):
    """examples/run_ba.py --track-close --close-search appearance end to end: frames_pairs.txt gains the columns source, match score, dx, dy; the flags are
    refused without --track-close."""
    out1, out2 = tmp_path / "out1", tmp_path / "out2"
    exe = [sys.executable, os.path.join(ROOT, "examples", "run_ba.py")]
    r = subprocess.run(exe + ["--demo", str(out1), "--views-hz", "50", "--window-size", "0.5", "--max-iter", "3"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    lo, hi = open(out1 / "views" / "tone.txt").read().split()
    common = ["--frames", str(out1 / "views"), "--init-poses", "frames", "--init-map", "frames", "--track-levels", "3,2,1", "--track-batch", "2", "--track-predict", "1",
              "--track-min-overlap", "0.3", "--track-q0", "0,0,0,1", "--window-size", "0.5", "--frames-log", "0", "--frames-lo", lo, "--frames-hi", hi,
              "--frames-skip-zero", "--max-iter", "3"]
    r = subprocess.run(exe + ["--demo", str(out2)] + common + ["--track-close", "--close-window", "2", "--close-gap", "3", "--close-huber", "10", "--close-levels", "2,1,0",
                                                               "--close-search", "appearance", "--close-match-level", "3", "--close-match-range", "6,4",
                                                               "--close-match-score", "0.3", "--close-match-per-frame", "2"],
                       capture_output=True, text=True, timeout=600)
    print(r.stdout[-3000:])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "track-close:" in r.stdout and "search appearance" in r.stdout
    lines = open(out2 / "frames_pairs.txt").read().splitlines()
    assert lines[0].startswith("# i j status(") and lines[0].endswith("match_score dx dy")
    rows = [l.split() for l in lines if l and not l.startswith("#")]
    assert len(rows) >= 1 and all(len(x) == 14 and int(x[10]) in (0, 2) and np.isfinite(float(x[11])) for x in rows) and (out2 / "refined_traj.txt").exists()
    assert all((int(x[10]) == 2) == (int(x[1]) - int(x[0]) > 3) for x in rows)
    for flag in (["--close-search", "appearance"], ["--close-match-level", "1"], ["--close-match-range", "2,2"]):
        r = subprocess.run(exe + ["--demo", str(tmp_path / "out3"), "--window-size", "0.5"] + flag, capture_output=True, text=True, timeout=600)
        assert r.returncode != 0 and "--track-close" in r.stderr
