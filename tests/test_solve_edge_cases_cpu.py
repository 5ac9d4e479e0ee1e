"""The conditions of the solvers' capacity cases (tests/solve_edge_cases.py), on the CPU oracle alone: what tests/test_gpu_solve_capacity.py relies on its
workloads to have.  A change of a builder that breaks one fails here, not on the device."""
import numpy as np
import pytest

import solve_edge_cases as E
from helpers import oracle_run


def test_the_constants_follow_from_the_lds_footprints():
    """72 * 3K and 16 * 3K bytes against 64 KB and 160 KB (the figures the comments of solve_rule.h and solve_host.h state)"""
    assert (E.K_SCHUR_NO_RAISE, E.K_SCHUR_RAISE, E.K_SCHUR_LAST, E.K_SCHUR_REFUSED) == (303, 304, 758, 759)
    assert (E.K_CG_NO_RAISE, E.K_CG_RAISE, E.K_CG_LAST, E.K_CG_REFUSED) == (1365, 1366, 3413, 3414)
    assert 72 * 3 * 303 == 65448 and 72 * 3 * 304 == 65664 and 72 * 3 * 758 == 163728 == 160 * 1024 - 112 and 72 * 3 * 759 == 163944
    assert 16 * 3 * 1365 == 65520 and 16 * 3 * 1366 == 65568 and 16 * 3 * 3413 == 163824 and 16 * 3 * 3414 == 163872
    assert set(E.N_EVENTS) == {303, 304, 758, 759, 1365, 1366, 3413, 3414}


@pytest.mark.parametrize("K", sorted(E.N_EVENTS))
def test_every_control_pose_is_observed_and_the_column_order_is_in_play(oracle_mod, K):
    w = E.workload(K)
    assert w.K == K and w.events.size() == E.N_EVENTS[K]
    ne = oracle_run(oracle_mod, w)["ne"]
    d = np.diag(ne["A11"])
    assert d.shape == (3 * K,) and (d > 0).all(), f"K = {K}: {(d <= 0).sum()} diagonal entries of A11 are not positive"
    assert ne["P"] >= 512                       # four slices of 128 pixels: the column order (solve_perm) and the slices of the block-sparse product are in play
    assert 3 * K >= 384 or K < 128              # ... and from K = 128 the auto rule of the column order decides by itself


@pytest.mark.parametrize("K", E.SCHUR_PARITY_KS)
def test_the_rows_a_pixel_touches(oracle_mod, K):
    """From the oracle's dense A12: per pixel (column pair) the non-zero rows.  At K >= 683 (3K >= 2049) some pixel's records reach a row >= 2048 — row block >= 32
    (bit 32 of rows_mask / slice_mask), 16-row group >= 128 (bit 7 of a byte of SchurBuildParams::range) —, and every row block of S is touched."""
    w = E.workload(K)
    ne = oracle_run(oracle_mod, w, dense_A12=True)["ne"]
    lo, hi = E.touched_rows(ne["A12"])
    assert (lo <= hi).all()                     # every active pixel has a record
    blocks = np.zeros((3 * K + 63) // 64, dtype=bool)
    nz_rows = ((ne["A12"] != 0).any(axis=1)).nonzero()[0]
    blocks[nz_rows // 64] = True
    assert blocks.all()
    if K >= 683:
        assert hi.max() >= 2048 and (hi.max() >> 6) >= 32 and (hi.max() >> 4) >= 128
        assert (3 * K + 63) // 64 == 36 and (hi.max() >> 4) == 142 and (hi.max() >> 4) < 256      # K = 758: 36 row blocks, group indices up to 142 in 8 bits
    else:
        assert hi.max() < 2048
