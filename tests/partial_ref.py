"""TEST INFRASTRUCTURE: numpy references of the two partial solves (emba_solve_map_only, emba_solve_poses_only) on the dict OracleLEGM.form_normal_eq
returns (after apply_l2), the oracle model that offers them to emba_amd.solver.solve_time_window, and the gloo stand-in engine that computes them from its
all-reduced pack."""
import numpy as np

from helpers import OracleModel
from shard_engine import OracleShardEngine


def _blocks(ne):
    """(xx, xy, yy, bx, by) per active pixel from A22 [P, 2, 2] and b2 [2P]"""
    A22 = np.asarray(ne["A22"], dtype=np.float64).reshape(-1, 2, 2)
    b2 = np.asarray(ne["b2"], dtype=np.float64).reshape(-1, 2)
    return A22[:, 0, 0], A22[:, 0, 1], A22[:, 1, 1], b2[:, 0], b2[:, 1]


def solve_map_only(ne, lam):
    """x2_i = (A22_i + lam diag A22_i)^-1 b2_i in closed form -> (x2 [2P], number of blocks failing `xx > 0 and det > 0`); a failing block's entries are
    whatever the division gives (inf / nan), as the reference's inverse() would."""
    xx, xy, yy, bx, by = _blocks(ne)
    mxx, myy = xx + lam * xx, yy + lam * yy
    det = mxx * myy - xy * xy
    bad = ~((mxx > 0) & (det > 0))
    with np.errstate(divide="ignore", invalid="ignore"):
        x2 = np.stack([(myy * bx - xy * by) / det, (mxx * by - xy * bx) / det], axis=1)
    return x2.reshape(-1), int(bad.sum())


def solve_poses_only(ne, lam, fix_first_pose):
    """(A11 + lam diag A11) x1 = b1 with the first pose's rows / columns trimmed (solver.cpp:156-165) -> x1 [3K], zeros for a fixed first pose"""
    A11 = np.asarray(ne["A11"], dtype=np.float64)
    b1 = np.asarray(ne["b1"], dtype=np.float64)
    sk = 3 if fix_first_pose else 0
    A = A11 + lam * np.diag(np.diag(A11))
    x1 = np.zeros(b1.size)
    x1[sk:] = np.linalg.solve(A[sk:, sk:], b1[sk:])
    return x1


class PartialOracleModel(OracleModel):
    """OracleModel + the two partial solves.  A map-only solve with a block that is not positive definite raises like the device (status EMBA_ERR_NUMERIC)."""

    n_bad_blocks = 0        # failing blocks over every solveMapOnly of this model

    def solveMapOnly(self, lam):
        from emba_amd._lib import ERR_NUMERIC, EmbaError
        x2, bad = solve_map_only(self.ne, lam)
        self.n_bad_blocks += bad
        if bad:
            raise EmbaError(ERR_NUMERIC, f"{bad} blocks of A22 + lambda diag(A22) are not positive definite")
        return np.zeros(3 * self.K), x2

    def solvePosesOnly(self, lam, fix_first_pose=False):
        return solve_poses_only(self.ne, lam, fix_first_pose), None


class PartialShardEngine(OracleShardEngine):
    """The gloo stand-in engine + the two partial solves, computed in numpy from the pack the ranks have all-reduced (a replica on every rank)."""

    def _ne(self):
        K, P = self.K, self.P
        pk = self.pack[: self.pack_len].numpy()
        q = pk[9 * K * K + 3 * K:].reshape(P, 5)
        A22 = np.stack([q[:, 0], q[:, 1], q[:, 1], q[:, 2]], axis=1).reshape(P, 2, 2)
        return dict(A11=pk[:9 * K * K].reshape(3 * K, 3 * K, order="F"), b1=pk[9 * K * K:9 * K * K + 3 * K], A22=A22, b2=q[:, 3:5].ravel(), P=P)

    def solve_map_only(self, lam, resident_x2=False):
        from emba_amd._lib import ERR_NUMERIC, EmbaError
        x2, bad = solve_map_only(self._ne(), lam)
        if bad:
            raise EmbaError(ERR_NUMERIC, f"{bad} blocks of A22 + lambda diag(A22) are not positive definite")
        return x2

    def solve_poses_only(self, lam, fix_first_pose=False):
        return solve_poses_only(self._ne(), lam, fix_first_pose)

    def rejectMap(self):
        if getattr(self, "_cur", None) is not None:      # (a rejected pose-only step: no trial map, like the device's emba_map_reject)
            super().rejectMap()
