"""emba_amd/csrc/refit_rule.h on a CPU: the argument checks of the refit, the un-vote, the selectors, the sweep order, the start of a frame,
the refit codes and the rotation change, through tests/cpp/refit_rule_test.cpp."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_refit_rule_on_the_cpu(tmp_path):
    """refit_rule.h (plain C++17, no HIP): tests/cpp/refit_rule_test.cpp checks every refusal in the order the C ABI reports them, the un-vote of a vote as
    the identity on uint64 (a sum that wraps among it), which frames a launch serves, the order of a sweep with `alternate`, the start of a frame (its own
    values bit for bit; track_predict's formula between two voting frames, across a run of lost frames; one side only; none), the code table and the rotation
    change.  Built twice: plain, and as a stand-alone program under -fsanitize=address,undefined."""
    src = os.path.join(ROOT, "tests", "cpp", "refit_rule_test.cpp")
    outs = []
    for name, extra in (("refit_rule_test", []), ("refit_rule_test_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])):
        exe = str(tmp_path / name)
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-ffp-contract=off"] + extra + [src, "-o", exe])
        r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
        print(r.stdout[-3000:], r.stderr)
        assert r.returncode == 0 and r.stdout.strip().splitlines()[-1] == "OK refit_rule", r.stdout[-3000:] + r.stderr
        outs.append(r.stdout)
    assert outs[0] == outs[1]
