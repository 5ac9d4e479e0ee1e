"""emba_amd/csrc/exposure_rule.h on a CPU: the per-frame gain and bias of the frame alignment — the argument checks, the 21 sums, the
compensated byte, the step under each estimate mask, the gain bounds and the gauge, through tests/cpp/exposure_rule_test.cpp."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_exposure_rule_on_the_cpu(tmp_path):
    """exposure_rule.h (plain C++17, no HIP): tests/cpp/exposure_rule_test.cpp checks the index of each of the 15 + 5 sums and the ten shared with
    align_accumulate, the pixel against align_pixel at gain 1 and bias 0, exposure_byte at its ties and both clamps, the step on a hand-written H, b under
    each of the four estimate masks, the leading block against align_solve and align_step bit for bit, the constant-byte frame degenerate under mask 3 and
    not under mask 0, the gain bounds and the gauge.  Built twice: plain, and as a stand-alone program under -fsanitize=address,undefined."""
    src = os.path.join(ROOT, "tests", "cpp", "exposure_rule_test.cpp")
    outs = []
    for name, extra in (("exposure_rule_test", []), ("exposure_rule_test_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])):
        exe = str(tmp_path / name)
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-ffp-contract=off"] + extra + [src, "-o", exe])
        r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
        print(r.stdout[-3000:], r.stderr)
        assert r.returncode == 0 and r.stdout.strip().splitlines()[-1] == "OK exposure_rule", r.stdout[-3000:] + r.stderr
        outs.append(r.stdout)
    assert outs[0] == outs[1]
