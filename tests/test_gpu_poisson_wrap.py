"""Boundary EMBA_POISSON_WRAP_X of the intensity panorama on the MI355X (include/emba_hip.h: emba_reconstruct_intensity_bc, emba_render_map_images_bc;
DESIGN.md §16) against the numpy form of the same rule, tests/poisson_wrap_ref.py.  The gradient planes are the random ones of
test_gpu_parity.py::test_poisson_reconstruction_matches_oracle, seed = H; the bounds are that test's: assert_close(tight=1e-10) and a residual of the
5-point equation below 1e-9 max|Gx| W."""
import ctypes as C

import numpy as np
import pytest

import poisson_wrap_ref as PW
from emba_amd import io as eio
from helpers import assert_close, rel_err

pytestmark = pytest.mark.gpu
ERR_INVALID_ARG, ERR_STATE = 1, 5
DIRICHLET, WRAP = 0, 1
dp, u8p = C.POINTER(C.c_double), C.POINTER(C.c_uint8)


def fresh(H, W, **options):
    from emba_amd import LEGM
    from emba_amd.synth import pinhole_bearing_lut
    m = LEGM(8, 8, pinhole_bearing_lut(8, 8, 10, 10, 4, 4), 0.2, W, H, device=0)
    for k, v in options.items():
        m.set_option(k, v)
    return m


def planes(H, W):
    rng = np.random.default_rng(H)
    return rng.normal(size=(H, W)), rng.normal(size=(H, W))


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from emba_amd import build
    build.build_hip()
    return True


@pytest.fixture(scope="module")
def case64(gpu):
    """One context at 64 x 128 for the module, its planes, the numpy panorama (left unchanged) and the device's."""
    H, W = 64, 128
    m = fresh(H, W)
    Gx, Gy = planes(H, W)
    Mo = PW.reconstruct_from_gradient(Gx, Gy)
    Mo.setflags(write=False)
    M = m.reconstructIntensity(Gx, Gy, boundary="wrap")
    yield m, Gx, Gy, Mo, M
    m.close()


def ptr(a, t=dp):
    return None if a is None else a.ctypes.data_as(t)


def raw_reconstruct(m, Gx, Gy, boundary, bc=True):
    """The C entry point with the output pre-filled: (status, M)."""
    M = np.full((m.H, m.W), 7.5)
    if bc:
        st = m._L.emba_reconstruct_intensity_bc(m._ctx, ptr(Gx), ptr(Gy), ptr(M), boundary)
    else:
        st = m._L.emba_reconstruct_intensity(m._ctx, ptr(Gx), ptr(Gy), ptr(M))
    return st, M


def raw_render(m, boundary, bc=True):
    """emba_render_map_images[_bc] with every image given and pre-filled: (status, gx, gy, rgb, poisson)."""
    n = m.H * m.W
    out = [np.full(n, 75, np.uint8), np.full(n, 75, np.uint8), np.full(3 * n, 75, np.uint8), np.full(n, 75, np.uint8)]
    if bc:
        st = m._L.emba_render_map_images_bc(m._ctx, 0.1, *(ptr(o, u8p) for o in out), boundary)
    else:
        st = m._L.emba_render_map_images(m._ctx, 0.1, *(ptr(o, u8p) for o in out))
    return (st, *out)


def last_error(m):
    return m._L.emba_last_error(m._ctx).decode()


# W - 1 rows go through the sweeps' kTriChunks = 128 chunks: 47 leaves chunks empty, 149 and 129 make two-element chunks with a ragged tail, 127 and 128 one
# element per chunk, 2047 the 16-element chunks of the benchmark panorama.  A context admits any width, so 65 x 129 and 65 x 130 are taken as they stand.
CASES = [(24, 48, {}), (75, 150, {}), (75, 150, {"poisson": 2}), (75, 150, {"gemm64": 1}), (64, 128, {}), (64, 128, {"poisson": 2}), (64, 128, {"gemm64": 1}),
         (65, 129, {}), (65, 130, {}), (1024, 2048, {})]


@pytest.mark.parametrize("H,W,options", CASES, ids=[f"{h}x{w}" + "".join(f"-{k}{v}" for k, v in o.items()) for h, w, o in CASES])
def test_wrap_matches_the_numpy_rule(gpu, H, W, options):
    m = fresh(H, W, **options)
    Gx, Gy = planes(H, W)
    M = m.reconstructIntensity(Gx, Gy, boundary="wrap")
    m.close()
    Mo = PW.reconstruct_from_gradient(Gx, Gy)
    res = np.abs(PW.laplacian(M) - PW.divergence(Gx, Gy)).max()
    print(f"{H}x{W} {options}: relative error {rel_err(M, Mo):.3e}, residual {res:.3e} (bound {1e-9 * np.abs(Gx).max() * W:.3e})")
    assert_close(M, Mo, "intensity panorama, wrapped", tight=1e-10)
    assert res < 1e-9 * np.abs(Gx).max() * W


def test_a_rolled_map_gives_the_rolled_panorama(case64):
    """The wrapped panorama does not know where the seam is; the reference's boundary does, by construction."""
    m, Gx, Gy, Mo, M = case64
    k = 43
    rx, ry = np.roll(Gx, k, axis=1), np.roll(Gy, k, axis=1)
    assert_close(m.reconstructIntensity(rx, ry, boundary="wrap"), np.roll(M, k, axis=1), "intensity panorama of the rolled map", tight=1e-10)
    D, Dr = m.reconstructIntensity(Gx, Gy), m.reconstructIntensity(rx, ry)
    print(f"dirichlet: rolled map against rolled panorama {rel_err(Dr, np.roll(D, k, axis=1)):.3e}")
    with pytest.raises(AssertionError):
        assert_close(Dr, np.roll(D, k, axis=1), "the reference's boundary under a roll", tight=1e-10, elementwise=False)


def test_resident_map_and_images(case64):
    m, Gx, Gy, Mo, M = case64
    assert_close(M, Mo, "intensity panorama, wrapped", tight=1e-10)
    m.upload_map(Gx, Gy)
    assert np.array_equal(m.reconstructIntensity(boundary="wrap"), M)
    imgs = m.renderMapImages(0.1, boundary="wrap")
    assert np.array_equal(imgs["map_poisson"], eio.normalize_robust(M, 0.1))
    ref = m.renderMapImages(0.1)
    assert all(np.array_equal(imgs[k], ref[k]) for k in ("Gx", "Gy", "G_hsv"))
    assert np.array_equal(ref["map_poisson"], eio.normalize_robust(m.reconstructIntensity(), 0.1)) and not np.array_equal(ref["map_poisson"], imgs["map_poisson"])


def test_nothing_existing_moved(case64):
    """Boundary 0 through the _bc entry points is the old entry points bit for bit, and the two boundaries share scratch planes and tables without a trace."""
    m, Gx, Gy, Mo, M = case64
    m.upload_map(Gx, Gy)
    st, old = raw_reconstruct(m, Gx, Gy, DIRICHLET, bc=False)
    assert st == 0
    st, new = raw_reconstruct(m, Gx, Gy, DIRICHLET)
    assert st == 0 and np.array_equal(new, old)
    r_old, r_new = raw_render(m, DIRICHLET, bc=False), raw_render(m, DIRICHLET)
    assert r_old[0] == 0 and r_new[0] == 0 and all(np.array_equal(a, b) for a, b in zip(r_old[1:], r_new[1:]))
    for planes_ in ((Gx, Gy), (None, None)):
        st, w1 = raw_reconstruct(m, *planes_, WRAP)
        assert st == 0 and np.array_equal(w1, M)
        st, d1 = raw_reconstruct(m, *planes_, DIRICHLET)
        assert st == 0 and np.array_equal(d1, old)
        st, w2 = raw_reconstruct(m, *planes_, WRAP)
        assert st == 0 and np.array_equal(w2, M)
    # a context whose first call is the wrapped one: the same bits as one that began with the reference's
    f = fresh(m.H, m.W)
    assert np.array_equal(f.reconstructIntensity(Gx, Gy, boundary="wrap"), M) and np.array_equal(f.reconstructIntensity(Gx, Gy), old)
    f.close()


def test_refusals_leave_everything_untouched(case64):
    m, Gx, Gy, Mo, M = case64
    m.upload_map(Gx, Gy)

    def untouched(out):
        return all((o == o.flat[0]).all() and o.flat[0] in (7.5, 75) for o in out)

    for boundary in (2, -1, 1 << 20):
        st, out = raw_reconstruct(m, Gx, Gy, boundary)
        assert st == ERR_INVALID_ARG and untouched([out]) and "boundary" in last_error(m), boundary
        r = raw_render(m, boundary)
        assert r[0] == ERR_INVALID_ARG and untouched(r[1:]) and "boundary" in last_error(m), boundary
    for half in ((Gx, None), (None, Gy)):
        st, out = raw_reconstruct(m, *half, WRAP)
        assert st == ERR_INVALID_ARG and untouched([out]) and "both" in last_error(m)
    m.set_option("poisson", 1)
    st, out = raw_reconstruct(m, Gx, Gy, WRAP)
    assert st == ERR_STATE and untouched([out]) and "poisson" in last_error(m)
    r = raw_render(m, WRAP)
    assert r[0] == ERR_STATE and untouched(r[1:]) and "poisson" in last_error(m)
    m.set_option("poisson", 0)
    from emba_amd import EmbaError
    with pytest.raises(ValueError):
        m.reconstructIntensity(Gx, Gy, boundary="periodic")
    # the context is as it was: the resident map, both boundaries
    assert np.array_equal(m.reconstructIntensity(boundary="wrap"), M) and np.array_equal(m.downloadMap()[0], Gx)
    # no map resident
    f = fresh(m.H, m.W)
    st, out = raw_reconstruct(f, None, None, WRAP)
    assert st == ERR_STATE and untouched([out]) and "no map" in last_error(f)
    r = raw_render(f, WRAP)
    assert r[0] == ERR_STATE and untouched(r[1:])
    with pytest.raises(EmbaError) as ei:
        f.reconstructIntensity(boundary="wrap")
    assert ei.value.status == ERR_STATE
    assert np.array_equal(f.reconstructIntensity(Gx, Gy, boundary="wrap"), M)
    f.close()
    # a panorama of two columns: every column's two neighbours would be the same column
    n = fresh(8, 2)
    gx, gy = planes(8, 2)
    st, out = raw_reconstruct(n, gx, gy, WRAP)
    assert st == ERR_INVALID_ARG and untouched([out]) and "pano_w" in last_error(n)
    st, out = raw_reconstruct(n, gx, gy, DIRICHLET)
    assert st == 0 and np.isfinite(out).all()
    n.close()


def test_poisoned_workspace(case64):
    """Option poison on a fresh context: every new allocation — the scratch planes, the q table and the buffers around it — reads as 0xFF bytes (NaN).  The
    wrapped call is the first the context sees, with planes and then on the resident map: the bits of the context that was not poisoned."""
    m, Gx, Gy, Mo, M = case64
    f = fresh(m.H, m.W, poison=1)
    assert np.array_equal(f.reconstructIntensity(Gx, Gy, boundary="wrap"), M)
    f.upload_map(Gx, Gy)
    assert np.array_equal(f.reconstructIntensity(boundary="wrap"), M)
    assert np.array_equal(f.renderMapImages(0.1, boundary="wrap")["map_poisson"], eio.normalize_robust(M, 0.1))
    f.close()
    # the unfolded form at an odd height, where the last transform takes the second scratch plane
    g, h = fresh(75, 150), fresh(75, 150, poison=1)
    gx, gy = planes(75, 150)
    assert np.array_equal(h.reconstructIntensity(gx, gy, boundary="wrap"), g.reconstructIntensity(gx, gy, boundary="wrap"))
    g.close(); h.close()
