"""Boundary EMBA_POISSON_WRAP_X on a CPU: the numpy form of the rule (tests/poisson_wrap_ref.py) pinned by the equation it solves, by its invariance
under a roll of the columns and on integrable fields; and the closing step of the cyclic systems (emba_amd/csrc/poisson_rule.h) against dense
elimination (tests/cpp/poisson_rule_test.cpp)."""
import os
import subprocess

import numpy as np
import pytest

import poisson_wrap_ref as PW

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(5, 3), (24, 48), (75, 150), (64, 128)]


def fields(shape):
    rng = np.random.default_rng(shape[0])
    return rng.normal(size=shape), rng.normal(size=shape)


@pytest.mark.parametrize("shape", SHAPES)
def test_reference_solves_the_wrapped_equation(shape):
    Gx, Gy = fields(shape)
    F = PW.divergence(Gx, Gy)
    H, W = shape
    assert (F[-1] == 0).all()
    for i, j in ((0, 0), (H - 2, W - 1), (1, W - 2)):
        assert F[i, j] == Gx[i, (j + 1) % W] - Gx[i, j] + Gy[i + 1, j] - Gy[i, j]
    M = PW.solve(F)
    res = np.abs(PW.laplacian(M) - F).max()
    print(f"{H}x{W}: residual {res:.3e}, max|F| {np.abs(F).max():.3e}")
    assert res <= 1e-12 * np.abs(F).max()
    # the equation written out at a corner: the left neighbour of column 0 is column W-1, the row above row 0 is 0
    assert abs(M[1, 0] + M[0, W - 1] + M[0, 1] - 4.0 * M[0, 0] - F[0, 0]) <= 1e-12 * np.abs(F).max()


@pytest.mark.parametrize("shape", SHAPES)
def test_a_rolled_map_gives_the_rolled_panorama(shape):
    Gx, Gy = fields(shape)
    W = shape[1]
    M = PW.reconstruct_from_gradient(Gx, Gy)
    for k in (1, W // 3, W - 1):
        Mk = PW.reconstruct_from_gradient(np.roll(Gx, k, axis=1), np.roll(Gy, k, axis=1))
        err = np.abs(Mk - np.roll(M, k, axis=1)).max()
        print(f"{shape[0]}x{W} k={k}: {err:.3e}")
        assert err <= 1e-12 * np.abs(M).max()


@pytest.mark.parametrize("shape", SHAPES)
def test_integrable_fields(shape):
    """Where the reference returns the image a gradient field came from.  The divergence takes FORWARD differences of Gx and Gy, so it is the 5-point
    operator at (i, j) exactly when the field holds BACKWARD differences of an image M0 (zero rows beyond the poles):
        Gx[i][j] = M0[i][j] - M0[i][(j-1) mod W],   Gy[i][j] = M0[i][j] - M0[i-1][j]      =>      F[i][j] = (lap M0)[i][j]   for i < H-1.
    Row H-1 of F is 0 whatever M0 is.  Hence, for ANY such M0, M - M0 solves the equation with a right-hand side that is -(lap M0)[H-1] in row H-1 and 0
    elsewhere: lap M equals lap M0 in every row the right-hand side is defined in, and 0 in the last.  M is M0 itself exactly when (lap M0)[H-1] = 0.
    The field of the forward differences Gx = M0[:, j+1 mod W] - M0, Gy[i] = M0[i+1] - M0[i] is the same statement for two DIFFERENT images (M0 rolled by
    one column in Gx, moved up one row in Gy), which no single image satisfies: F is then the x second difference at (i, j+1) plus the y one at (i+1, j)."""
    H, W = shape
    rng = np.random.default_rng(100 + H)
    M0 = rng.normal(size=shape)
    back = lambda A: (A - np.roll(A, 1, axis=1), A - np.pad(A, ((1, 0), (0, 0)))[:-1])
    Gx, Gy = back(M0)
    L0 = PW.laplacian(M0)
    scale = np.abs(L0).max()
    assert np.abs(PW.divergence(Gx, Gy)[:-1] - L0[:-1]).max() <= 1e-14 * scale
    M = PW.reconstruct_from_gradient(Gx, Gy)
    L = PW.laplacian(M)
    assert np.abs(L[:-1] - L0[:-1]).max() <= 1e-12 * scale and np.abs(L[-1]).max() <= 1e-12 * scale
    assert np.abs(M - M0).max() > 1e-3          # the last row's defect is felt: a random M0 is not returned
    # an image whose last row is harmonic given the row above it, (lap M0)[H-1] = 0: returned as it is
    mu = -4.0 * np.sin(np.pi * np.arange(W) / W) ** 2
    M0[-1] = np.fft.ifft(np.fft.fft(-M0[-2]) / (mu - 2.0)).real
    assert np.abs(PW.laplacian(M0)[-1]).max() <= 1e-13 * scale
    M = PW.reconstruct_from_gradient(*back(M0))
    err = np.abs(M - M0).max()
    print(f"{H}x{W}: max|M - M0| = {err:.3e}")
    assert err <= 1e-12 * np.abs(M0).max()
    # the forward differences of the same image: the shifted stencil, and what the reference solves then
    Gx = np.roll(M0, -1, axis=1) - M0
    Gy = np.pad(M0, ((0, 1), (0, 0)))[1:] - M0
    dxx = np.roll(M0, -2, axis=1) - 2.0 * np.roll(M0, -1, axis=1) + M0
    P = np.pad(M0, ((0, 2), (0, 0)))
    dyy = P[2:] - 2.0 * P[1:-1] + P[:-2]
    F = PW.divergence(Gx, Gy)
    assert np.abs(F[:-1] - (dxx + dyy)[:-1]).max() <= 1e-14 * scale and (F[-1] == 0).all()


def test_poisson_rule_on_the_cpu(tmp_path):
    """The boundary check, the wrapped column, and the cyclic systems (C_W + (beta + 2) I) x = g solved by the rule — Thomas sweeps of T_{W-1} for p and q by the
    recurrence the kernels use, then poisson_wrap_pivot and poisson_wrap_close — against dense elimination with partial pivoting, at W = 3, 4, 5, 129, 130 and
    beta from -2 - 1e-6 to -6."""
    exe = str(tmp_path / "poisson_rule_test")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", os.path.join(ROOT, "tests", "cpp", "poisson_rule_test.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout[-3000:], r.stderr)
    assert r.returncode == 0 and r.stdout.strip().splitlines()[-1] == "OK poisson_rule", r.stdout[-3000:] + r.stderr


def test_python_hosts_pass_the_boundary_through():
    """The argument's names, and the recorder: a model is asked for a boundary only where it is not the reference's."""
    from emba_amd.legm import POISSON_BOUNDARIES, poisson_boundary
    from emba_amd.solver import BASettings, MapRecorder
    assert POISSON_BOUNDARIES == {"dirichlet": 0, "wrap": 1} and BASettings().panorama_boundary == "dirichlet"
    with pytest.raises(ValueError):
        poisson_boundary("periodic")
    import inspect
    assert inspect.signature(MapRecorder.record).parameters["boundary"].default == "dirichlet"
