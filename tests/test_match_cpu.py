"""Loop-closure pairs found by appearance, in numpy (emba_amd.io.match_*): the sums against a triple loop in Python integers, the score and the
best of a pair, the search and its tie rules, match_start against the C entry bit for bit, the driver's settings, and the cases of tests/match_cases.py with
the figures recorded there."""
import os

import numpy as np
import pytest

import match_cases as MC
import pair_cases as PC
from emba_amd import io as eio

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def test_abi_declares_the_match_stage(hip_lib):
    from emba_amd import _lib
    header = open(os.path.join(ROOT, "include", "emba_hip.h")).read()
    for name in ("emba_frames_match_eval", "emba_frames_match_search", "emba_match_start"):
        assert hasattr(hip_lib, name) and name in _lib.SIGNATURES and f"emba_status {name}(" in header
    assert hip_lib.emba_abi_version() == 2


def loop_sums(A, B, rx, ry, skip_zero):
    """the six sums of every shift by a triple loop in Python integers"""
    h, w = len(A), len(A[0])
    out = []
    for dy in range(-ry, ry + 1):
        for dx in range(-rx, rx + 1):
            s = [0] * 6
            for y in range(h):
                for x in range(w):
                    if not (0 <= x + dx < w and 0 <= y + dy < h):
                        continue
                    a, b = int(A[y][x]), int(B[y + dy][x + dx])
                    if skip_zero and (a == 0 or b == 0):
                        continue
                    s = [s[0] + 1, s[1] + a, s[2] + b, s[3] + a * a, s[4] + b * b, s[5] + a * b]
            out.append(s)
    return out


@pytest.mark.parametrize("shape,rx,ry", (((7, 9), 8, 6), ((13, 20), 3, 2), ((2, 3), 1, 1)))
def test_sums_against_a_triple_loop(shape, rx, ry):
    rng = np.random.default_rng(shape[0])
    A, B = (rng.integers(0, 256, shape).astype(np.uint8) for _ in range(2))
    A[rng.random(shape) < 0.2] = 0
    B[0, 0] = B[-1, -1] = 0
    for skip_zero in (False, True):
        got = eio.match_sums(A, B, rx, ry, skip_zero)
        want = loop_sums(A.tolist(), B.tolist(), rx, ry, skip_zero)
        assert got.dtype == np.uint64 and got.shape == ((2 * rx + 1) * (2 * ry + 1), 6) and got.tolist() == want
        # the score from the same integers in Python's own arithmetic: exact integers, then four correctly rounded operations
        score, scored = eio.match_score(got, n_min=2)
        for s, (n, sa, sb, saa, sbb, sab) in enumerate(want):
            cov, va, vb = n * sab - sa * sb, n * saa - sa * sa, n * sbb - sb * sb
            if n < 2 or va == 0 or vb == 0:
                assert not scored[s] and score[s] == eio.MATCH_UNSCORED
            else:
                assert scored[s] and bits(score[s]) == bits((float(cov) * abs(float(cov))) / (float(va) * float(vb)))
        # ... and the table form (matrix products in fp64) gives the same best
        b = eio.match_best(A, B, rx, ry, skip_zero, n_min=2)
        tb, ts, tn = eio.match_table(np.stack([A, B]), rx, ry, skip_zero, n_min=2)
        assert bits(tb[0, 1]) == bits(b["score"]) and ts[0, 1].tolist() == [b["dx"], b["dy"]] and tn[0, 1] == b["n"]
    assert eio.match_shifts(1, 1).tolist()[:4] == [[-1, -1], [0, -1], [1, -1], [-1, 0]]


def test_self_constant_zero_and_the_tie():
    rng = np.random.default_rng(5)
    T = rng.integers(1, 256, (13, 20)).astype(np.uint8)
    b = eio.match_best(T, T, 3, 2, True, 8)
    assert b["score"] == 1.0 and (b["dx"], b["dy"], b["n"]) == (0, 0, 260)
    for a, c, skip in ((np.full_like(T, 77), T, False), (T, np.full_like(T, 77), True), (np.zeros_like(T), T, True)):
        b = eio.match_best(a, c, 3, 2, skip, 1)
        assert (b["score"], b["dx"], b["dy"], b["n"]) == (eio.MATCH_UNSCORED, 0, 0, 0)
    P = np.tile(np.array([50, 200], np.uint8), (4, 4))      # period 2 in x: dx = -2, 0, 2 all score 1; the lowest index is dx = -2
    b = eio.match_best(P, P, 2, 0)
    assert (b["score"], b["dx"], b["shift"]) == (1.0, -2, 0)
    with pytest.raises(ValueError, match="smallest level that fits is 1"):
        eio.match_check((240, 180), 0, 1, 1)
    with pytest.raises(ValueError, match="0 <= rx < 16"):
        eio.match_check((64, 48), 2, 16, 0)
    with pytest.raises(ValueError, match="n_min"):
        eio.match_check((64, 48), 2, 1, 1, 0)
    with pytest.raises(ValueError, match="2 x 2"):
        eio.match_check((64, 48), 5, 0, 0)


def test_search_rules_on_small_frames():
    """identical frames tie to the lower index; a lost frame is never a partner; min_gap = F - 2 leaves one pair, F - 1 none; score_min above every score"""
    rng = np.random.default_rng(2)
    base = rng.integers(1, 256, (8, 8)).astype(np.uint8)
    fr = np.stack([base, rng.integers(1, 256, (8, 8)).astype(np.uint8), base, base, rng.integers(1, 256, (8, 8)).astype(np.uint8), base])
    r = eio.match_search(fr, None, 0, 1, 1, 0, False, 8, -1.0, 3)
    assert r["partner"][0].tolist() == [2, 3, 5] and (r["score"][0] == 1.0).all() and r["partner"][3].tolist() == [0, 2, 5] and (r["shift"][0] == 0).all()
    st = np.array([1, 2, 3, 2, 2, 2])
    r = eio.match_search(fr, st, 0, 1, 1, 0, False, 8, -1.0, 5)
    assert not (r["partner"] == 2).any() and (r["partner"][2] == -1).all() and r["partner"][0, :2].tolist() == [3, 5] and (r["partner"][:, 4] == -1).all()
    r = eio.match_search(fr, None, 0, 1, 1, 4, False, 8, -1.0, 2)
    assert r["partner"][0].tolist() == [5, -1] and r["partner"][5].tolist() == [0, -1] and (r["partner"][1:5] == -1).all()
    assert eio.match_pairs(r).tolist() == [[0, 5]]
    r = eio.match_search(fr, None, 0, 1, 1, 5, False, 8, -1.0, 2)
    assert (r["partner"] == -1).all() and (r["score"] == eio.MATCH_UNSCORED).all() and not r["n"].any() and eio.match_pairs(r).shape == (0, 2)
    r = eio.match_search(fr, None, 0, 1, 1, 0, False, 8, 1.5, 2)
    assert (r["partner"] == -1).all()
    for bad in (dict(k=0), dict(k=65), dict(min_gap=-1), dict(score_min=float("nan"))):
        with pytest.raises(ValueError):
            eio.match_search(fr, None, 0, 1, 1, **dict(dict(min_gap=0, score_min=0.0, k=1), **bad))


def test_match_start_against_the_c_entry_bit_for_bit(hip_lib):
    from emba_amd import LEGM
    rng = np.random.default_rng(11)
    for _ in range(200):
        sw, sh = int(rng.integers(2, 400)), int(rng.integers(2, 300))
        l = int(rng.integers(0, 4))
        cal = eio.pair_calib(rng.uniform(20, 300), rng.uniform(20, 300), rng.uniform(0, sw), rng.uniform(0, sh))
        dx, dy = int(rng.integers(-40, 41)), int(rng.integers(-40, 41))
        q = eio.match_start(dx, dy, l, cal["fu"], cal["fv"], cal["cu"], cal["cv"], sw, sh)
        assert np.array_equal(bits(q), bits(LEGM.match_start(dx, dy, l, cal, (sw, sh)))), (dx, dy, l, cal, sw, sh)
        assert abs(np.linalg.norm(q) - 1.0) < 1e-15
    assert np.array_equal(bits(eio.match_start(0, 0, 2, 32.0, 35.2, 31.5, 23.5, 64, 48)), bits([0.0, 0.0, 0.0, 1.0]))
    from emba_amd import _lib
    with pytest.raises(_lib.EmbaError):
        LEGM.match_start(1, 1, 8, PC.PINHOLE, PC.SENSOR)
    with pytest.raises(ValueError):
        eio.match_start(1, 1, 8, 32.0, 32.0, 31.5, 23.5, 64, 48)


def test_settings_of_the_driver():
    from emba_amd.driver import SequenceSettings
    s = SequenceSettings(1.0, 1.0)
    assert s.close_search == "rotations" and s.close_match_level == 2 and s.close_match_range == (6, 4) and s.close_match_per_frame == 2
    for bad in (dict(close_search="bytes"), dict(close_match_level=8), dict(close_match_range=(1,)), dict(close_match_range=(-1, 0)), dict(close_match_per_frame=0),
                dict(close_match_score=float("nan")), dict(close_match_min_overlap=1.5)):
        with pytest.raises(ValueError):
            SequenceSettings(1.0, 1.0, **bad)


def test_the_cases_are_what_numpy_measured():
    """tests/match_cases.py's figures: the rotations propose no loop, the appearance search finds true loops at level 1 and at level 2 with starts inside §27's
    basin, and closing with them ends nearer the truth than closing without."""
    q, status = MC.drifted()
    rot = eio.pair_candidates(q, status, window=MC.WINDOW, min_gap=MC.GAP, max_angle=MC.ANGLE, max_per_frame=MC.PER_FRAME)
    assert int((rot[:, 1] - rot[:, 0] > MC.WINDOW).sum()) == MC.ROTATION_LOOPS == 0 and len(MC.true_loops()) == MC.N_TRUE_LOOPS
    for level in (1, 2):
        r = MC.search_numpy(level)
        mp, ms, md = eio.match_pairs(r, with_info=True)
        found = [tuple(p) for p in mp.tolist()]
        distinct = [p for p in found if p not in MC.SAME_BYTES]
        print(f"level {level}: {len(found)} matched pairs, {len(distinct)} of distinct bytes; shifts {md.tolist()}")
        assert len(found) == MC.N_MATCHED[level] and len(distinct) == MC.N_DISTINCT[level]
        if MC.FINDS:
            assert all(p in MC.true_loops() for p in found) and len(distinct) > 0
        worst = max(MC.start_error(level, p, d) for p, d in zip(found, md)) / MC.CELL
        assert abs(worst - MC.START_ERROR[level]) < 0.01 and worst < 12.0
        for p in MC.SAME_BYTES:      # the same bytes: score exactly 1 at shift 0, and each is the other's first partner
            assert r["partner"][p[0], 0] == p[1] and r["partner"][p[1], 0] == p[0] and r["score"][p[0], 0] == 1.0 and not r["shift"][p[0], 0].any()
        # the tie rule: frame 6 is the turning point and sees frames 5 and 7, 4 and 8 ... as equals; nothing here depends on which lane looked first
        one = MC.search_numpy(level, 1)
        assert np.array_equal(one["partner"][:, 0], r["partner"][:, 0]) and np.array_equal(bits(one["score"][:, 0]), bits(r["score"][:, 0]))
    before = MC.worst_angle(q)
    ends = {}
    for mode in ("rotations", "appearance", "both"):
        c = MC.closing_numpy(mode)
        ends[mode] = MC.worst_angle(c["graph"]["q"])
        print(f"{mode}: {len(c['pairs'])} pairs, {int(c['keep'].sum())} kept, worst angle {before:.4e} -> {ends[mode]:.4e}")
        assert len(c["pairs"]) == MC.N_PAIRS[mode] and int(c["keep"].sum()) == MC.N_KEPT[mode]
    assert abs(before / MC.E_BEFORE - 1) < 1e-3 and abs(ends["rotations"] / MC.E_ROTATIONS - 1) < 1e-3 and abs(ends["appearance"] / MC.E_APPEARANCE - 1) < 1e-3
    assert set(MC.closing_numpy("appearance")["source"].tolist()) == {0, 2} and ends["both"] == ends["appearance"]
    if MC.IMPROVES:
        assert ends["appearance"] < ends["rotations"] < before
