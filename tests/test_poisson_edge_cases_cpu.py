"""The case table of the intensity panorama's edge tests (tests/poisson_edge_cases.py) on a CPU: its Python statement of the launch plan against
emba_amd/csrc/poisson_rule.h (tests/cpp/poisson_rule_test.cpp, argument `plan`), what the table covers at 256 compute units, asserted path by path, and the
numpy references' own residuals, which tests/test_gpu_poisson_edges.py takes as exact against the suite's bounds."""
import os
import subprocess

import numpy as np
import pytest

import poisson_edge_cases as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FORMS = ("k64x64", "k64x128", "k128x128")


@pytest.fixture(scope="module")
def rule_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("poisson_rule") / "poisson_rule_test")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", os.path.join(ROOT, "tests", "cpp", "poisson_rule_test.cpp"), "-o", exe])
    return exe


def cpp_plans(exe, lines):
    r = subprocess.run([exe, "plan"], input="".join(lines), capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr
    return r.stdout


def test_the_python_plan_is_the_rule_headers(rule_exe):
    """Every case of the table, at 256 compute units and at counts that move the kernel choice, and a sweep of shapes around every threshold."""
    asked = []      # (H, W, n_cu, gemm64, poisson, boundary)
    for c in E.CASES:
        for n_cu in (E.N_CU, 304, 64, 1):
            asked.append((c.H, c.W, n_cu, c.options.get("gemm64", 0), c.options.get("poisson", 0), c.boundary))
    for H in (61, 62, 63, 64, 65, 66, 127, 128, 129, 2047, 2048, 2049):
        for W in (3, 4, 127, 128, 129, 130, 4095, 4096, 4097, 4098, 4224, 4225, 8192, 8193):
            for gemm64, poisson, boundary in ((0, 0, E.DIRICHLET), (1, 0, E.WRAP), (0, 2, E.WRAP), (1, 1, E.DIRICHLET)):
                asked.append((H, W, E.N_CU, gemm64, poisson, boundary))
    lines = [f"{H} {W} {n_cu} {g} {p} {int(b == E.WRAP)}\n" for H, W, n_cu, g, p, b in asked]
    want = "".join(E.plan_text(*a) for a in asked)
    got = cpp_plans(rule_exe, lines)
    assert got.count("case ") == len(asked)
    assert got == want, next((a, b) for a, b in zip(got.splitlines(), want.splitlines()) if a != b)
    print(cpp_plans(rule_exe, [f"{c.H} {c.W} {E.N_CU} {c.options.get('gemm64', 0)} {c.options.get('poisson', 0)} {int(c.boundary == E.WRAP)}\n" for c in E.CASES]))


def test_the_python_tiles_are_the_rule_headers(rule_exe):
    """TILE and THREAD_COLS against the one tile table of poisson_rule.h (gemm_tile), which the kernel's instantiations, gemm_form and gemm_tiles read."""
    r = subprocess.run([rule_exe, "tiles"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr
    print(r.stdout)
    rows = {f[0]: tuple(int(v) for v in f[1:]) for f in (line.split() for line in r.stdout.splitlines())}
    assert set(rows) == set(FORMS) == set(E.TILE) == set(E.THREAD_COLS)
    for form, (bm, bn, threads, b_per_thread) in rows.items():
        assert (bm, bn) == E.TILE[form] and b_per_thread == E.THREAD_COLS[form], form
        assert b_per_thread * threads == E.GEMM_BK * bn and 4 * bm == threads, form      # the staging: a B tile of 16 x bn, an A tile of bm x 16 in fours


def test_every_case_takes_the_form_its_row_names():
    for c in E.CASES:
        assert {p[6] for p in c.plan()["products"]} == set(c.forms), c


def test_every_gemm_form_meets_every_operand_path_with_all_three_tails():
    """Per kernel: the scalar and the 16-byte operand paths, with A read at stride 1 and at stride 2, on products whose M, N and K are no multiples of the
    tile — and, on the 16-byte path at stride 2, an N whose last vector of B straddles the edge."""
    met = {f: set() for f in FORMS}
    for c in E.CASES:
        for prod in c.plan()["products"]:
            M, N, K, lda, stride, vec, form = prod
            tm, tn, tk, straddles = E.tails(prod)
            if not (tm and tn and tk):
                continue
            if stride == 1 and not vec:
                met[form].add("stride 1, vec 0")
            if stride == 1 and vec:
                met[form].add("stride 1, vec 1, ragged N")
            if stride == 2 and not vec:
                met[form].add("stride 2, vec 0")
            if stride == 2 and vec and straddles and tn < E.THREAD_COLS[form]:
                met[form].add("stride 2, vec 1, N tail narrower than a thread's vector")
    print(met)
    every = {"stride 1, vec 0", "stride 1, vec 1, ragged N", "stride 2, vec 0", "stride 2, vec 1, N tail narrower than a thread's vector"}
    for f in FORMS:
        assert met[f] == every, (f, every - met[f])
    # a vector of B that straddles the edge inside a tile that is ragged as a whole: h = 50, columns 48 to 51 of 50
    assert any(p[6] == "k64x64" and p[4] == 2 and p[5] and E.tails(p)[3] and E.tails(p)[1] > E.THREAD_COLS["k64x64"] for c in E.CASES for p in c.plan()["products"])
    # the dense form's eigen-solve epilogue on partial tiles
    dense = [c for c in E.CASES if c.options.get("poisson") == 1]
    assert dense and all(all(E.tails(p)[:3]) for c in dense for p in c.plan()["products"])
    # a second tile column of a single column (h = 65), and a single row (M = W = 4097 = 32 * 128 + 1)
    prods = [p for c in E.CASES for p in c.plan()["products"]]
    assert any(p[6] == "k64x64" and p[1] == 65 for p in prods) and all(any(p[6] == f and p[0] % E.TILE[f][0] == 1 for p in prods) for f in ("k64x128", "k128x128"))


def test_both_replay_forms_under_both_boundaries_and_the_chunk_edges():
    sweeps = {(c.boundary, c.plan()["sweep"]) for c in E.CASES if c.plan()["sweep"]}
    for boundary in (E.DIRICHLET, E.WRAP):
        assert {s[2] for b, s in sweeps if b == boundary} == {"registers", "table"}, boundary
        # the two widths at the threshold, under each boundary (wrapped: the sweeps run over W - 1 rows)
        assert {(4096, 32, "registers"), (4097, 33, "table")} <= {s for b, s in sweeps if b == boundary}, boundary
    table = [s for _, s in sweeps if s[2] == "table"]
    sizes = {s[0]: E.chunk_sizes(s[0]) for s in table}
    assert all(sum(v) == Wt for Wt, v in sizes.items())
    assert sizes[4097][124] == 5 and sizes[4097][125:] == [0, 0, 0] and sizes[4097][:124] == [33] * 124      # a partial chunk and empty ones, from the table
    assert sizes[4224] == [33] * 128 and max(sizes[8192]) == 64 and sizes[4225][-1] == 0 and 0 < sizes[4225][124] < 34
    assert any(c.H % E.TRI_SYS and c.plan()["sweep"][2] == "table" for c in E.CASES if c.plan()["sweep"])
    # the narrowest wrapped planes: two and three live chunks of one row
    assert {(2, 1, "registers"), (3, 1, "registers")} <= {s for b, s in sweeps if b == E.WRAP}
    assert E.chunk_sizes(2) == [1, 1] + [0] * 126


@pytest.mark.parametrize("shape", E.SHAPES, ids=[f"{h}x{w}-{b}" for h, w, b in E.SHAPES])
def test_the_numpy_reference_is_far_inside_the_bounds(shape):
    """The residual of the numpy panorama on the 5-point equation of its boundary: at most 1e-3 of the suite's bound 1e-9 max|Gx| W on the device's residual."""
    H, W, boundary = shape
    Gx, Gy, Mo, res = E.reference(H, W, boundary)
    bound = E.residual_bound(Gx, W)
    print(f"{H}x{W} {boundary}: residual {res:.3e} = {res / bound:.2e} of the bound {bound:.3e}")
    assert np.isfinite(Mo).all() and res <= 1e-3 * bound
