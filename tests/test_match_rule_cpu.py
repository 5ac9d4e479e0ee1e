"""emba_amd/csrc/match_rule.h on a CPU: loop-closure pairs found by appearance — the refusals, the launch arithmetic, the sums, the score, the
best of a pair, the search and the start of a matched pair, through tests/cpp/match_rule_test.cpp."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_match_rule_on_the_cpu(tmp_path):
    """match_rule.h (plain C++17, no HIP): tests/cpp/match_rule_test.cpp checks every refusal in its order, the shift count and the index <-> (i, j) map of
    the triangular table at F = 2, 3, 7, 4096 and 2^31 - 1, the chunks at 2^20 - 1, 2^20 and 2^20 + 1 pairs, the six sums of a hand-made 3 x 2 pair, a frame
    against itself scoring exactly 1.0, a constant and an all-zero frame being unscored, n_min where the overlap is one pixel, the tie going to the lower
    shift index and to the lower partner, and match_start: the identity bit for bit at d = 0, b_i turned onto b_j by R(Q).  Built twice: plain, and as a
    stand-alone program under -fsanitize=address,undefined."""
    src = os.path.join(ROOT, "tests", "cpp", "match_rule_test.cpp")
    outs = []
    for name, extra in (("match_rule_test", []), ("match_rule_test_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])):
        exe = str(tmp_path / name)
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-ffp-contract=off"] + extra + [src, "-o", exe])
        r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
        print(r.stdout[-3000:], r.stderr)
        assert r.returncode == 0 and r.stdout.strip().splitlines()[-1] == "OK match_rule", r.stdout[-3000:] + r.stderr
        outs.append(r.stdout)
    assert outs[0] == outs[1]
