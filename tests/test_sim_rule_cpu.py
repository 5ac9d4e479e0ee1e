"""emba_amd/csrc/sim_rule.h on a CPU: what one sensor pixel of the event simulator does with one more sample, the cut of F steps into
chunks and the passes of the sort, through tests/cpp/sim_rule_test.cpp."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_sim_rule_on_the_cpu(tmp_path):
    """sim_rule.h (plain C++17, no HIP): tests/cpp/sim_rule_test.cpp checks one step of one pixel with |cur - ref| just below, at and above C in both
    directions with c_on != c_off, the cap at 1 and 2 with the carry into the next step, cur == prev with a carried difference (frac NaN, -inf and +inf),
    frac == 1 giving off == d - 1, d == 1 and d == 2^52 - 1, disarming and arming around an outside sample, the chunk cutter at F = 1, at one chunk exactly
    and at one chunk plus one step, and the sort's passes at the 2^32 ns edge.  Built twice: plain, and as a stand-alone program under
    -fsanitize=address,undefined."""
    src = os.path.join(ROOT, "tests", "cpp", "sim_rule_test.cpp")
    outs = []
    for name, extra in (("sim_rule_test", []), ("sim_rule_test_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])):
        exe = str(tmp_path / name)
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-ffp-contract=off"] + extra + [src, "-o", exe])
        r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
        print(r.stdout[-3000:], r.stderr)
        assert r.returncode == 0 and r.stdout.strip().splitlines()[-1] == "OK sim_rule", r.stdout[-3000:] + r.stderr
        outs.append(r.stdout)
    assert outs[0] == outs[1]
