"""The rotation graph in numpy (emba_amd.io.rotation_graph_solve) and, on the CPU, through the C entry (it needs no device): the closing case
of tests/pair_cases.py — candidates, pairs, graph with frame 0 the anchor — and the refusals."""
import numpy as np
import pytest

import pair_cases as PC
from emba_amd import io as eio
from emba_amd import so3


def test_closing_case_figures():
    """The out-and-back trajectory with 0.35 cells of drift per frame: numpy's pairs all converge, and the graph brings the worst angle to the truth from
    E_BEFORE_NP to E_AFTER_NP.  numpy shows an improvement (IMPROVES), so it is asserted."""
    r = PC.closing_numpy()
    q, status = PC.drifted()
    before, after = PC.worst_angle(q), PC.worst_angle(r["graph"]["q"])
    print(f"pairs {len(r['pairs'])}, kept {int(r['keep'].sum())}; worst angle {before:.4e} -> {after:.4e} rad; graph",
          {k: v for k, v in r["graph"].items() if k != "q"})
    assert len(r["pairs"]) == PC.N_PAIRS_NP and r["keep"].all() and (r["align"]["status"] == eio.ALIGN_CONVERGED).all()
    assert before == pytest.approx(PC.E_BEFORE_NP, rel=1e-3) and after == pytest.approx(PC.E_AFTER_NP, rel=1e-3)
    assert PC.IMPROVES == (True,) and after < 0.01 * before
    assert r["graph"]["end"] == eio.GRAPH_CONVERGED and r["graph"]["cost"] < 1e-5 * r["graph"]["cost0"]
    assert np.array_equal(r["graph"]["q"][0], q[0])      # the anchor keeps its bits
    same = [k for k, (i, j) in enumerate(r["pairs"].tolist()) if i + j == PC.F]
    # frames f and 12 - f are the same bytes: their pairs end at a cost that is rounding alone, and only the noise floor keeps their information in bounds
    assert len(same) == 4 and (r["align"]["sums"][same, 9] < 1e-15).all() and (np.abs(r["align"]["info"][same]).max(axis=1) > 1e20).all()
    assert np.abs(r["info"]).max() < 12.0 * np.abs(r["align"]["sums"][:, :6]).max() * 1.0001


def test_permuted_edges_and_tighter_tolerances_stay_within_the_spread():
    r = PC.closing_numpy()
    q, status = PC.drifted()
    k = r["keep"]
    ed, Qe, info = r["pairs"][k], r["align"]["q"][k], r["info"][k]
    p = PC.permuted(len(ed))
    assert sorted(p.tolist()) == list(range(len(ed)))
    g1 = eio.rotation_graph_solve(q, status, ed[p], Qe[p], info[p])
    g2 = eio.rotation_graph_solve(q, status, ed, Qe, info, tol=1e-12, cg_tol=1e-12)
    s1, s2 = (float(eio.rotation_angle_between(r["graph"]["q"], g["q"]).max()) for g in (g1, g2))
    print(f"permuted {s1:.3e} rad, tighter {s2:.3e} rad; recorded {PC.GRAPH_PERMUTED_NP:.1e}, spread {PC.GRAPH_SPREAD:.1e}")
    assert s1 <= PC.GRAPH_SPREAD and s2 <= PC.GRAPH_SPREAD


def test_c_entry_against_numpy_on_the_cpu(hip_lib):
    """emba_rotation_graph_solve needs no context and no device: held to numpy within ten times the recorded spread, here as on the GPU machine."""
    from emba_amd.legm import LEGM
    r = PC.closing_numpy()
    q, status = PC.drifted()
    k = r["keep"]
    from emba_amd import _lib
    nan_q, zero_Q = np.array(q), r["align"]["q"][k].copy()
    nan_q[4, 1] = np.nan
    zero_Q[2] = 0.0
    for args, text in (((nan_q, np.full(PC.F, 2), r["pairs"][k], zero_Q, r["info"][k]), r"q_xyzw\[4\]"), ((q, status, r["pairs"][k], zero_Q, r["info"][k]), r"Q_xyzw\[2\]")):
        with pytest.raises(_lib.EmbaError, match=text):      # the same refusals in the same order as numpy's
            LEGM.rotation_graph_solve(*args)
    g = LEGM.rotation_graph_solve(q, status, r["pairs"][k], r["align"]["q"][k], r["info"][k])
    d = float(eio.rotation_angle_between(r["graph"]["q"], g["q"]).max())
    print(f"C against numpy: {d:.3e} rad; C", {a: b for a, b in g.items() if a != "q"})
    assert d <= 10.0 * PC.GRAPH_SPREAD and g["end"] == r["graph"]["end"] and g["iters"] == r["graph"]["iters"] and g["cg_iters"] >= g["iters"]
    assert g["cost0"] == pytest.approx(r["graph"]["cost0"], rel=1e-12) and g["cost"] == pytest.approx(r["graph"]["cost"], rel=1e-9)
    assert np.array_equal(g["q"][0], q[0])


def test_exact_edges_recover_the_truth_and_refusals():
    c = PC.case(False)
    q, status = PC.drifted()
    ed = np.array([(i, j) for i in range(PC.F) for j in range(i + 1, min(i + 3, PC.F))] + [(1, 10), (2, 9)], dtype=np.int32)
    Qe = np.array([PC.true_pair(c, i, j) for i, j in ed])
    info = np.tile([500.0, 10.0, -5.0, 400.0, 8.0, 300.0], (len(ed), 1))
    g = eio.rotation_graph_solve(q, status, ed, Qe, info)
    assert PC.worst_angle(g["q"]) < 1e-9 and g["end"] == eio.GRAPH_CONVERGED
    # a second anchor, displaced, is held exactly
    st = status.copy()
    st[7] = eio.TRACK_ANCHOR
    g = eio.rotation_graph_solve(q, st, ed, Qe, info)
    assert np.array_equal(g["q"][7], q[7]) and np.array_equal(g["q"][0], q[0]) and g["cost"] > 0.0
    # a frame without an edge keeps its input
    g = eio.rotation_graph_solve(q, status, ed[(ed != 11).all(axis=1)], Qe[(ed != 11).all(axis=1)], info[(ed != 11).all(axis=1)])
    assert np.array_equal(g["q"][11], q[11])
    with pytest.raises(ValueError, match="no anchor"):
        eio.rotation_graph_solve(q, np.full(PC.F, 2), ed, Qe, info)
    far = (ed >= 6).all(axis=1)
    with pytest.raises(ValueError, match="frame 6 "):
        eio.rotation_graph_solve(q, status, ed[far], Qe[far], info[far])
    with pytest.raises(ValueError, match="outside"):
        eio.rotation_graph_solve(q, status, [[0, PC.F]], Qe[:1], info[:1])
    bad = info.copy()
    bad[3, 2] = np.inf
    with pytest.raises(ValueError, match="not finite"):
        eio.rotation_graph_solve(q, status, ed, Qe, bad)
    # the refusals graph_args_ok has beside these, in its order: the settings, then a bad q before the missing anchor, a bad edge Q before a bad info
    nan_q, zero_Q = np.array(q), Qe.copy()
    nan_q[4, 1] = np.nan
    zero_Q[2] = 0.0
    with pytest.raises(ValueError, match="settings"):
        eio.rotation_graph_solve(nan_q, np.full(PC.F, 2), ed, zero_Q, bad, lambda_up=1.0)
    with pytest.raises(ValueError, match=r"q_xyzw\[4\]"):
        eio.rotation_graph_solve(nan_q, np.full(PC.F, 2), ed, zero_Q, bad)
    with pytest.raises(ValueError, match=r"Q_xyzw\[2\]"):
        eio.rotation_graph_solve(q, status, ed, zero_Q, bad)
    assert np.allclose(eio.graph_jr_inv(np.zeros(3)), np.eye(3))
    e = np.array([0.3, -1.1, 0.7])
    h = 1e-6
    num = np.stack([(eio.graph_log(so3.mul(so3.exp(e), so3.exp(h * d))) - eio.graph_log(so3.mul(so3.exp(e), so3.exp(-h * d)))) / (2 * h) for d in np.eye(3)], axis=1)
    assert np.allclose(num, eio.graph_jr_inv(e), atol=1e-8)
