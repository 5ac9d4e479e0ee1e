"""emba_amd/csrc/cost_rule.h on a CPU: the summand of one residual, the factors behind the sums and the grid of the cost launch
(tests/cpp/cost_rule_test.cpp), and single residuals against the oracle's dataCost."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cost_rule_on_the_cpu(tmp_path, oracle_mod):
    """cost_term at e = 0, against closed forms for the quadratic, Huber and Cauchy cost and just below, at and just above Huber's threshold; cost_scale
    and reg_scale; the grid at n_pm and npix of 0, 1, 255, 256, 257 and 2^31 for four chip sizes (every block has work or is the one block there must be,
    nb_data <= n_cu, nb_reg <= 2 n_cu, nb_reg = 0 exactly when the regulariser is not asked for, never an empty launch).  Then cost_scale * cost_term of the
    single residuals the program prints against oracle.data_cost of the one-element vector, at the rel = 1e-10 of test_gpu_parity.py::test_irls_parity."""
    exe = str(tmp_path / "cost_rule_test")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", os.path.join(ROOT, "tests", "cpp", "cost_rule_test.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout[-3000:], r.stderr)
    lines = r.stdout.strip().splitlines()
    assert r.returncode == 0 and lines[-1] == "OK cost_rule", r.stdout[-3000:] + r.stderr
    terms = [l.split()[1:] for l in lines if l.startswith("TERM ")]
    assert len(terms) == 3 * 2 * 11
    for irls, eta, e, got in terms:
        irls, eta, e, got = int(irls), float(eta), float(e), float(got)
        want = oracle_mod.data_cost(np.array([e]), irls, eta)
        assert got == pytest.approx(want, rel=1e-10, abs=0.0), (irls, eta, e, got, want)
        assert (got == 0.0) == (e == 0.0)
