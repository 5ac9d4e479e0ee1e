"""emba_amd/csrc/pair_level_rule.h on a CPU: the pair alignment coarse to fine with the pair's exposure estimated — the refusals, the sizes,
bytes, table and camera of a level, min_pixels per level and the schedule, through tests/cpp/pair_level_rule_test.cpp."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_pair_level_rule_on_the_cpu(tmp_path):
    """pair_level_rule.h (plain C++17, no HIP): tests/cpp/pair_level_rule_test.cpp checks the refusals in their order, the level sizes of 64 x 48, 20 x 13 and
    8 x 8, the byte rule against a direct sum (the rounding tie, a zero in the box, with and without skip_zero, the cascade of boxes), the level camera at
    level 0 bit for bit and a point's u_l, the level table behind a pinhole against the analytic centre, Ju at a level against central differences,
    min_pixels per level, the schedule's hand-over, level 0 with estimate = 0 against align_step's loop bit for bit, and the degenerate end on a frame of
    one constant byte.  Built twice: plain, and as a stand-alone program under -fsanitize=address,undefined."""
    src = os.path.join(ROOT, "tests", "cpp", "pair_level_rule_test.cpp")
    outs = []
    for name, extra in (("pair_level_rule_test", []), ("pair_level_rule_test_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])):
        exe = str(tmp_path / name)
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-ffp-contract=off"] + extra + [src, "-o", exe])
        r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
        print(r.stdout[-3000:], r.stderr)
        assert r.returncode == 0 and r.stdout.strip().splitlines()[-1] == "OK pair_level_rule", r.stdout[-3000:] + r.stderr
        outs.append(r.stdout)
    assert outs[0] == outs[1]
