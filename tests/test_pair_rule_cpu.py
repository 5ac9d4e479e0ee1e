"""emba_amd/csrc/pair_rule.h on a CPU: one frame aligned to another — the argument checks, the projection through the plumb_bob model with
its Jacobians, the sample of the other frame's bytes, the classes, the term, pair_start and pair_information, through tests/cpp/pair_rule_test.cpp."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_pair_rule_on_the_cpu(tmp_path):
    """pair_rule.h (plain C++17, no HIP): tests/cpp/pair_rule_test.cpp checks every refusal in the order the C ABI reports them, D = 0 against the plain
    pinhole bit for bit, the projection's Jacobian and Ju against central differences under a strong lens, the sample at integer (u, v), every outside edge
    (ix = -1, ix = sw - 2 against sw - 1, rb_z <= 0, a NaN, 2^31), the class precedence, the exposure in the residual, the identity pair of a frame with
    itself, pair_start and pair_information.  Built twice: plain, and as a stand-alone program under -fsanitize=address,undefined."""
    src = os.path.join(ROOT, "tests", "cpp", "pair_rule_test.cpp")
    outs = []
    for name, extra in (("pair_rule_test", []), ("pair_rule_test_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])):
        exe = str(tmp_path / name)
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-ffp-contract=off"] + extra + [src, "-o", exe])
        r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
        print(r.stdout[-3000:], r.stderr)
        assert r.returncode == 0 and r.stdout.strip().splitlines()[-1] == "OK pair_rule", r.stdout[-3000:] + r.stderr
        outs.append(r.stdout)
    assert outs[0] == outs[1]
