"""emba_amd/csrc/track_rule.h on a CPU: the argument checks of the frame tracker, the geometry of a level, the batches, the prediction, one
pixel against a level's two integer sums and the verdict, through tests/cpp/track_rule_test.cpp."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_track_rule_on_the_cpu(tmp_path):
    """track_rule.h (plain C++17, no HIP): tests/cpp/track_rule_test.cpp checks every argument refusal in the order the C ABI reports them, the level geometry
    at l = 0 and at the last allowed level with a non-divisible W and H_l = 1, the batch plan at F = 1, F = batch, F = batch + 1 and with a chunk edge inside a
    batch, the prediction with zero, one and two tracked frames, across a lost frame and with unequal gaps, the classes of a pixel against two sums, and the
    verdict at overlap == min_overlap and behind a degenerate last level.  Built twice: plain, and as a stand-alone program under
    -fsanitize=address,undefined."""
    src = os.path.join(ROOT, "tests", "cpp", "track_rule_test.cpp")
    outs = []
    for name, extra in (("track_rule_test", []), ("track_rule_test_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])):
        exe = str(tmp_path / name)
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-ffp-contract=off"] + extra + [src, "-o", exe])
        r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
        print(r.stdout[-3000:], r.stderr)
        assert r.returncode == 0 and r.stdout.strip().splitlines()[-1] == "OK track_rule", r.stdout[-3000:] + r.stderr
        outs.append(r.stdout)
    assert outs[0] == outs[1]
