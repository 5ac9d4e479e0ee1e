"""The emba_set_option table against tests/option_matrix.py (CPU): every option has a GPU parity test for the values that select another
kernel or host branch, or a stated exemption."""
import ast
import os
import re

import pytest

import option_matrix as OM

TESTS = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def table():
    return {o["name"]: o for o in OM.parse_options()}


def test_option_table_parses(table):
    assert len(table) >= 31, sorted(table)
    for o in table.values():
        assert o["lo"] <= o["hi"], o


def test_every_option_is_covered_or_exempt(table):
    listed = set(OM.COVERED) | set(OM.EXEMPT)
    missing = sorted(set(table) - listed)
    assert not missing, f"options without a parity test or a stated exemption in tests/option_matrix.py: {missing}"
    unknown = sorted(listed - set(table))
    assert not unknown, f"tests/option_matrix.py names options the library does not have: {unknown}"
    both = sorted(set(OM.COVERED) & set(OM.EXEMPT))
    assert not both, f"options both covered and exempt: {both}"
    for name, why in OM.EXEMPT.items():
        assert why.strip(), name


def test_covered_values_are_in_range_and_include_every_branch(table):
    assert set(OM.REQUIRED) == set(OM.COVERED), sorted(set(OM.REQUIRED) ^ set(OM.COVERED))
    for name, (values, _) in OM.COVERED.items():
        lo, hi = table[name]["lo"], table[name]["hi"]
        out = [v for v in values if not lo <= v <= hi]
        assert not out, f"option {name}: covered values {out} outside [{lo}, {hi}]"
        need = [v for v in OM.REQUIRED[name] if v not in values]
        assert not need, f"option {name}: values {need} select a kernel or branch that no test runs"


def _test_sources(mod):
    """test name -> its source with its decorators and the source of every module-level function or value it refers to (transitively): the
    helpers it calls, the parameter lists its decorators name."""
    with open(os.path.join(TESTS, mod)) as f:
        text = f.read()
    tree = ast.parse(text)
    top = {}
    for node in tree.body:
        if isinstance(node, (ast.FunctionDef, ast.ClassDef)):
            top[node.name] = node
        elif isinstance(node, ast.Assign):
            for t in node.targets:
                if isinstance(t, ast.Name):
                    top[t.id] = node

    def segment(node):
        lo = min([node.lineno] + [d.lineno for d in getattr(node, "decorator_list", [])])
        return "\n".join(text.splitlines()[lo - 1:node.end_lineno])

    out = {}
    for name, node in top.items():
        if not (isinstance(node, ast.FunctionDef) and name.startswith("test_")):
            continue
        seen, todo, parts = {name}, [node], []
        while todo:
            n = todo.pop()
            parts.append(segment(n))
            for sub in ast.walk(n):
                if isinstance(sub, ast.Name) and sub.id in top and sub.id not in seen:
                    seen.add(sub.id)
                    todo.append(top[sub.id])
        out[name] = "\n".join(parts)
    return text, out


def test_covering_tests_exist_and_set_their_option():
    """Every test COVERED credits with an option exists in a GPU module and names the option (in its body, its decorators, or a helper or
    parameter list of its module that it refers to)."""
    mods = {}
    for name, (_, tests) in OM.COVERED.items():
        assert tests, name
        for t in tests:
            mod, fn = t.split("::")
            if mod not in mods:
                mods[mod] = _test_sources(mod)
            text, srcs = mods[mod]
            assert re.search(r"\bpytest\.mark\.gpu\b", text), f"{mod} is not a GPU module"
            assert fn in srcs, f"option {name}: {t} does not exist"
            assert re.search(r"\b%s\b" % name, srcs[fn]), f"option {name}: {t} never names it"


def test_tile_chunk_round_is_covered():
    """tile_chunk's "one round" case is kWarpNew x kTileWaves of the current kernels.h."""
    assert OM.tile_round() in OM.COVERED["tile_chunk"][0] and OM.tile_round() in OM.REQUIRED["tile_chunk"]


def test_tile_shapes_parse():
    shapes = OM.parse_tile_shapes()
    assert len(shapes) == 4 == OM.parse_constants()["kNumTileShapes"]
    for s in shapes:
        assert s["tw"] * s["th"] == 1152, s
        assert 0 < s["fine_pw"] <= s["pw"] <= s["tw"] and 0 < s["fine_ph"] <= s["ph"] <= s["th"], s
    # reserve 5 on the 96 x 12 tile leaves a 2-px pitch in y (the narrowest geometry the tests run)
    assert OM.tile_geometry(2, False, 5)["pitch_y"] == 2


def test_parser_names_a_new_option(tmp_path):
    """A new entry in the table (here a dummy one) is reported by name."""
    with open(OM.OPTIONS_SRC) as f:
        src = f.read()
    head = "kOptions[] = {"
    assert src.count(head) == 1
    p = tmp_path / "options_host.h"
    p.write_text(src.replace(head, head + '\n    {"foo", &emba_ctx::step_ep, 0, 1, false},'))
    names = {o["name"] for o in OM.parse_options(str(p))}
    assert "foo" in names and sorted(names - set(OM.COVERED) - set(OM.EXEMPT)) == ["foo"]
