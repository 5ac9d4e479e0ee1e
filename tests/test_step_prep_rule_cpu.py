"""emba_amd/csrc/step_rule.h on a CPU: when the packed texels are stale and when the launch in front of the warp kernel is dropped (tests/cpp/step_prep_rule_test.cpp)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_step_prep_rules_on_the_cpu(tmp_path):
    """rect_contained on both sides of its slack on every side and with empty boxes, texels_stale for each reason a pack is due, texel_blocks, and
    prep_inside_warp for the steady step and for every case that keeps the launch (K = 105, tile order, the pose table, an empty window, unclean
    lines, stale texels, the full pack, the option)."""
    import option_matrix as OM
    assert OM.parse_constants()["kInlineKnots"] == 104      # (the value the rule test passes in)
    exe = str(tmp_path / "step_prep_rule_test")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", os.path.join(ROOT, "tests", "cpp", "step_prep_rule_test.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and r.stdout.strip().splitlines()[-1] == "OK step_prep_rule", r.stdout + r.stderr


def test_the_step_prep_options_have_their_gpu_tests():
    """step_prep and step_prep_polls are entries of the one option table (kOptions of options_host.h, read by tests/option_matrix.py).  As for every option,
    the values that select another kernel or host branch are run against a fresh context and the oracle: tests/test_gpu_step_prep.py must exist as a GPU
    module and set each of them."""
    import re
    import option_matrix as OM
    names = [o["name"] for o in OM.parse_options() if o["name"].startswith("step_prep")]
    assert names == ["step_prep", "step_prep_polls"], names
    for n in names:
        assert all(t.startswith("test_gpu_step_prep.py::") for t in OM.COVERED[n][1]), OM.COVERED[n]
    with open(os.path.join(ROOT, "tests", "test_gpu_step_prep.py")) as f:
        text = f.read()
    assert re.search(r"\bpytest\.mark\.gpu\b", text)
    assert re.search(r'parametrize\("prep", \[1, 0\]\)', text) and "step_prep=prep" in text          # both values of step_prep
    assert "step_prep_polls=0" in text                                                               # nobody waits: the bounded wait's exit
