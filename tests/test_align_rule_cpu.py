"""emba_amd/csrc/align_rule.h on a CPU: the argument checks of the frame alignment, the sample with its gradient, the classes of a pixel, the
Huber weight, the 3 x 3 solve and the Levenberg-Marquardt step of one frame, through tests/cpp/align_rule_test.cpp."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_align_rule_on_the_cpu(tmp_path):
    """align_rule.h (plain C++17, no HIP): tests/cpp/align_rule_test.cpp checks the argument enums in the order the C ABI reports them, the sample gradient on a
    hand-written 3 x 4 plane at the wrapped column and at both row limits and against a finite difference of view_sample, the precedence outside / masked /
    skipped, the Huber branches at |r| = k, a known 3 x 3 system, every non-positive pivot, n < min_pixels, and accept / reject / lambda with every status.
    Built twice: plain, and as a stand-alone program under -fsanitize=address,undefined."""
    src = os.path.join(ROOT, "tests", "cpp", "align_rule_test.cpp")
    outs = []
    for name, extra in (("align_rule_test", []), ("align_rule_test_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])):
        exe = str(tmp_path / name)
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-ffp-contract=off"] + extra + [src, "-o", exe])
        r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
        print(r.stdout[-3000:], r.stderr)
        assert r.returncode == 0 and r.stdout.strip().splitlines()[-1] == "OK align_rule", r.stdout[-3000:] + r.stderr
        outs.append(r.stdout)
    assert outs[0] == outs[1]
