"""The intensity panorama under boundary EMBA_POISSON_WRAP_X (include/emba_hip.h) in numpy — test infrastructure only, and the definition the device
form is compared with.  Columns wrap (column W-1 is the neighbour of column 0); the rows beyond the poles are 0, as in the reference's Dirichlet solve.

    F[i][j] = Gx[i][(j+1) mod W] - Gx[i][j] + Gy[i+1][j] - Gy[i][j]          i < H-1, every j;  row H-1 is 0
    M[i-1][j] + M[i+1][j] + M[i][(j-1) mod W] + M[i][(j+1) mod W] - 4 M[i][j] = F[i][j],      M[-1][:] = M[H][:] = 0

The sine vectors along H and the Fourier vectors along W diagonalise the two second differences, eigenvalues lambda1[i] = -4 sin^2(pi (i+1) / (2 (H+1)))
and mu[k] = -4 sin^2(pi k / W):

    M = DST-I_H( FFT_W^-1( FFT_W(DST-I_H(F)) / (lambda1[i] + mu[k]) ) ) / (2 (H+1))

(scipy's type-1 DST is the unnormalised one: applied twice it multiplies by 2 (H+1)).  lambda1[i] + mu[k] <= lambda1[0] < 0: nothing to regularise."""
import numpy as np
from scipy import fft as sfft


def divergence(Gx, Gy):
    """F of the rule above."""
    Gx, Gy = np.asarray(Gx, dtype=np.float64), np.asarray(Gy, dtype=np.float64)
    F = np.zeros(Gx.shape)
    F[:-1] = np.roll(Gx, -1, axis=1)[:-1] - Gx[:-1] + Gy[1:] - Gy[:-1]
    return F


def laplacian(M):
    """The left-hand side of the equation: 5 points, columns wrapped, zero rows beyond the poles."""
    P = np.pad(M, ((1, 1), (0, 0)))
    return P[2:] + P[:-2] + np.roll(M, 1, axis=1) + np.roll(M, -1, axis=1) - 4.0 * M


def solve(F):
    """M of the spectral form above."""
    H, W = F.shape
    lam1 = -4.0 * np.sin(np.pi * (np.arange(H) + 1) / (2.0 * (H + 1))) ** 2
    mu = -4.0 * np.sin(np.pi * np.arange(W) / W) ** 2
    R = np.fft.fft(sfft.dst(F, type=1, axis=0), axis=1)
    U = np.fft.ifft(R / (lam1[:, None] + mu[None, :]), axis=1).real
    return sfft.dst(U, type=1, axis=0) / (2.0 * (H + 1))


def reconstruct_from_gradient(Gx, Gy):
    return solve(divergence(Gx, Gy))
