"""TEST INFRASTRUCTURE (no HIP in here): the solvers at their capacity edges in the number of control poses K — the K constants, derived from the kernels'
LDS footprints and NOT copied from solve_rule.h, and the builders of the workloads tests/test_solve_edge_cases_cpu.py (their conditions, on the oracle) and
tests/test_gpu_solve_capacity.py (the device) share.

emba_schur_build_kernel stages (2 * 4 + 1) columns of 3K doubles per workgroup: 72 * 3K bytes of dynamic LDS.  emba_cg_pixel_kernel keeps two 3K-vectors:
16 * 3K bytes.  A launch takes up to 64 KB of dynamic LDS as it is, more only after hipFuncAttributeMaxDynamicSharedMemorySize was raised, and a CU has 160 KB."""
import numpy as np

from helpers import small_workload

LDS_DEFAULT = 64 * 1024       # dynamic LDS a launch gets without the attribute
LDS_CU = 160 * 1024           # LDS of a CU (gfx950)

SCHUR_BUILD_BYTES_PER_POSE = 72 * 3      # (2 * kBuildWaves + 1) * 8 bytes per row, three rows per control pose
CG_PIXEL_BYTES_PER_POSE = 16 * 3         # two doubles per row

K_SCHUR_NO_RAISE = LDS_DEFAULT // SCHUR_BUILD_BYTES_PER_POSE      # 303: 65 448 B, the last launch without the raise
K_SCHUR_RAISE = K_SCHUR_NO_RAISE + 1                              # 304: 65 664 B
K_SCHUR_LAST = LDS_CU // SCHUR_BUILD_BYTES_PER_POSE               # 758: 163 728 B, 112 B under the CU's 160 KB
K_SCHUR_REFUSED = K_SCHUR_LAST + 1                                # 759: 163 944 B
K_CG_NO_RAISE = LDS_DEFAULT // CG_PIXEL_BYTES_PER_POSE            # 1365: 65 520 B
K_CG_RAISE = K_CG_NO_RAISE + 1                                    # 1366: 65 568 B
K_CG_LAST = LDS_CU // CG_PIXEL_BYTES_PER_POSE                     # 3413: 163 824 B
K_CG_REFUSED = K_CG_LAST + 1                                      # 3414: 163 872 B

# events per case: about 200 per control pose, so that every control pose is observed (A11 has no zero on its diagonal)
N_EVENTS = {K_SCHUR_NO_RAISE: 61000, K_SCHUR_RAISE: 61000, K_SCHUR_LAST: 152000, K_SCHUR_REFUSED: 152000,
            K_CG_NO_RAISE: 274000, K_CG_RAISE: 274000, K_CG_LAST: 683000, K_CG_REFUSED: 683000}

SCHUR_PARITY_KS = (K_SCHUR_NO_RAISE, K_SCHUR_RAISE, K_SCHUR_LAST)
SOLVES = ((1e-2, True), (3.0, False))      # (lambda, fix_first_pose) of every Schur parity case; the second call re-uses the cached lists


def workload(K):
    """the window of half a second with K control poses on a 32 x 24 sensor over a 128-row panorama (P about 1800 active pixels)"""
    return small_workload(n_events=N_EVENTS[K], pano_h=128, K=K, sensor=(32, 24), focal=30.0, dt_knots=0.5 / (K - 1), thres_valid_pixel=3)


def touched_rows(A12):
    """per pixel (column pair of the dense A12 [3K, 2P]) the first and the last non-zero row -> (lo [P], hi [P]); lo > hi: no entry"""
    n, c = A12.shape
    nz = (A12[:, 0::2] != 0) | (A12[:, 1::2] != 0)
    any_ = nz.any(axis=0)
    lo = np.where(any_, nz.argmax(axis=0), n)
    hi = np.where(any_, n - 1 - nz[::-1].argmax(axis=0), -1)
    return lo, hi


def damped_residual(ne, lam, fix, x1, x2):
    """The residual of the full damped system [A11m A12; A12^T A22m] [x1; x2] = [b1; b2] in np.longdouble, from the dense A12 of the oracle's equations:
    (max |pose rows| / max |b1|, max |map rows| / max |b2|); the rows of a fixed first pose do not count."""
    ld = np.longdouble
    sk = 3 if fix else 0
    A11 = np.asarray(ne["A11"])
    A12 = np.asarray(ne["A12"])
    b1 = np.asarray(ne["b1"]).astype(ld); b2 = np.asarray(ne["b2"]).astype(ld)
    X1 = np.asarray(x1).astype(ld); X2 = np.asarray(x2).astype(ld)
    r1 = b1 - _matvec_ld(A11, X1) - ld(lam) * np.diag(A11).astype(ld) * X1 - _matvec_ld(A12, X2)
    A22 = np.asarray(ne["A22"]).reshape(-1, 2, 2).astype(ld)
    v = X2.reshape(-1, 2)
    t = _matvec_ld(A12.T, X1).reshape(-1, 2)
    m0 = (A22[:, 0, 0] + ld(lam) * A22[:, 0, 0]) * v[:, 0] + A22[:, 0, 1] * v[:, 1]
    m1 = A22[:, 1, 0] * v[:, 0] + (A22[:, 1, 1] + ld(lam) * A22[:, 1, 1]) * v[:, 1]
    r2 = b2.reshape(-1, 2) - t - np.stack([m0, m1], axis=1)
    return float(np.abs(r1[sk:]).max() / np.abs(b1).max()), float(np.abs(r2).max() / np.abs(b2).max())


def _matvec_ld(A, x, rows=256):
    """A x in np.longdouble without a long-double copy of A (65 MB of A12 at K = 758 would be 130 MB): row blocks at a time"""
    out = np.zeros(A.shape[0], dtype=np.longdouble)
    for r0 in range(0, A.shape[0], rows):
        out[r0:r0 + rows] = A[r0:r0 + rows].astype(np.longdouble) @ x
    return out


def refine_once(ne, lam, fix, x1, x2):
    """One step of iterative refinement of (x1, x2) on the dense damped system: the residual in np.longdouble, the correction from a float64 solve of the Schur
    system (numpy) -> the refined (x1, x2) as float64.  What the tolerance of the parity tests is measured with: the oracle's own distance from it."""
    ld = np.longdouble
    sk = 3 if fix else 0
    A11 = np.asarray(ne["A11"]); A12 = np.asarray(ne["A12"])
    b1 = np.asarray(ne["b1"]).astype(ld); b2 = np.asarray(ne["b2"]).astype(ld)
    X1 = np.asarray(x1).astype(ld); X2 = np.asarray(x2).astype(ld)
    d11 = np.diag(A11)
    r1 = b1 - _matvec_ld(A11, X1) - ld(lam) * d11.astype(ld) * X1 - _matvec_ld(A12, X2)
    A22 = np.asarray(ne["A22"]).reshape(-1, 2, 2)
    a, b, c = A22[:, 0, 0] * (1 + lam), A22[:, 0, 1], A22[:, 1, 1] * (1 + lam)
    v = X2.reshape(-1, 2)
    t = _matvec_ld(A12.T, X1).reshape(-1, 2)
    r2 = b2.reshape(-1, 2) - t - np.stack([a.astype(ld) * v[:, 0] + b.astype(ld) * v[:, 1], b.astype(ld) * v[:, 0] + c.astype(ld) * v[:, 1]], axis=1)
    r1 = r1.astype(np.float64); r2 = r2.astype(np.float64)
    r1[:sk] = 0.0
    det = a * c - b * b
    inv = np.stack([c / det, -b / det, -b / det, a / det], axis=1).reshape(-1, 2, 2)        # A22m^-1 per pixel

    def apply_inv(w):           # A22m^-1 on [2P] or [2P, m]
        w2 = w.reshape(inv.shape[0], 2, -1)
        return np.einsum("pij,pjm->pim", inv, w2).reshape(w.shape)

    S = A11 + lam * np.diag(d11) - A12 @ apply_inv(np.ascontiguousarray(A12.T))
    rhs = r1 - A12 @ apply_inv(r2.reshape(-1))
    d1 = np.zeros_like(r1)
    d1[sk:] = np.linalg.solve(S[sk:, sk:], rhs[sk:])
    d2 = apply_inv(r2.reshape(-1) - A12.T @ d1)
    return np.asarray(x1) + d1, np.asarray(x2) + d2


def spread(x, ref):
    """max |x - ref| / max |ref|"""
    return float(np.abs(np.asarray(x) - np.asarray(ref)).max() / np.abs(ref).max())
