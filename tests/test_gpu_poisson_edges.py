"""The intensity panorama on the MI355X at every tile, fold and sweep-chunk edge of its launch plan (emba_amd/csrc/poisson_rule.h): the three
fp64 MFMA GEMM kernels with tails in M, N and K on their scalar and 16-byte operand paths, the folded DST's strided operand at ragged half lengths, the
backward Thomas sweep replayed from the factor table (W > 4096), and the narrowest wrapped planes.  The cases and the plan each takes: tests/poisson_edge_cases.py;
what the table covers is asserted on a CPU by tests/test_poisson_edge_cases_cpu.py.  The references are oracle/poisson.py and tests/poisson_wrap_ref.py, the
bounds those of test_gpu_parity.py::test_poisson_reconstruction_matches_oracle: assert_close(tight=1e-10), and a residual of the 5-point equation below
1e-9 max|Gx| W.  Nothing on this path is atomic: a dropped k-slice, row or column shows at 1e-6 or worse."""
import numpy as np
import pytest

import poisson_edge_cases as E
from helpers import assert_close, rel_err

pytestmark = pytest.mark.gpu


def fresh(H, W, **options):
    from emba_amd import LEGM
    from emba_amd.synth import pinhole_bearing_lut
    m = LEGM(8, 8, pinhole_bearing_lut(8, 8, 10, 10, 4, 4), 0.2, W, H, device=0)
    for k, v in options.items():
        m.set_option(k, v)
    return m


@pytest.fixture(scope="module")
def n_cu():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from emba_amd import build
    build.build_hip()
    return torch.cuda.get_device_properties(0).multi_processor_count      # what emba_create reads (hipDeviceAttributeMultiprocessorCount)


@pytest.mark.parametrize("case", E.CASES, ids=[c.id for c in E.CASES])
def test_edge_case_matches_the_numpy_reference(n_cu, case):
    plan = case.plan(n_cu)
    forms = {p[6] for p in plan["products"]}
    assert forms == set(case.forms), f"{case.id}: on {n_cu} compute units the products run on {sorted(forms)}, the table names {sorted(case.forms)}: {plan}"
    Gx, Gy, Mo, ref_res = E.reference(case.H, case.W, case.boundary)
    m = fresh(case.H, case.W, **case.options)
    M = m.reconstructIntensity(Gx, Gy, boundary=case.boundary)
    m.close()
    res, bound = E.residual(M, Gx, Gy, case.boundary), E.residual_bound(Gx, case.W)
    print(f"{case.id}: plan {plan}\n{case.id}: relative error {rel_err(M, Mo):.3e}, residual {res:.3e} = {res / ref_res:.2f} x the numpy form's {ref_res:.3e} "
          f"(bound {bound:.3e})")
    assert_close(M, Mo, "intensity panorama, " + case.id, tight=1e-10)
    assert res < bound


TWICE = [(66, 131, E.DIRICHLET), (66, 131, E.WRAP), (24, 4097, E.DIRICHLET), (24, 4098, E.WRAP)]      # a ragged fold; the sweeps' table branch (wrapped: Wt = 4097)


@pytest.mark.parametrize("H,W,boundary", TWICE, ids=[f"{h}x{w}-{b}" for h, w, b in TWICE])
def test_cached_tables_and_the_resident_map(n_cu, H, W, boundary):
    """A second call on the same context finds the sine matrices, the Thomas factors and the q table in place: the same bits.  The resident map goes the same
    way as planes passed in.  The other boundary in between leaves no trace."""
    Gx, Gy = E.planes(H, W)
    m = fresh(H, W)
    first = m.reconstructIntensity(Gx, Gy, boundary=boundary)
    assert np.array_equal(m.reconstructIntensity(Gx, Gy, boundary=boundary), first)
    m.upload_map(Gx, Gy)
    assert np.array_equal(m.reconstructIntensity(boundary=boundary), first)
    other = E.WRAP if boundary == E.DIRICHLET else E.DIRICHLET
    assert not np.array_equal(m.reconstructIntensity(boundary=other), first)
    assert np.array_equal(m.reconstructIntensity(boundary=boundary), first)
    m.close()
