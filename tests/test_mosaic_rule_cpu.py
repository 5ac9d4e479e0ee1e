"""emba_amd/csrc/mosaic_rule.h on a CPU: the argument checks of the frame mosaic, its chunks, the bound that keeps its integer sums exact,
and the mean, the log-intensity and the gradient map of a plane with holes, through tests/cpp/mosaic_rule_test.cpp."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_mosaic_rule_on_the_cpu(tmp_path):
    """mosaic_rule.h (plain C++17, no HIP): tests/cpp/mosaic_rule_test.cpp checks the argument enums in the order the C ABI reports them, the chunk cut at
    65 535 + 3 frames of 7 x 5 and at 240 x 180, the 2^36 bound at its last accepted count and where F * S leaves 64 bits, and mean, log and gradient on a
    hand-written 3 x 4 plane with holes, the wrapped column and row 0.  Built twice: plain, and as a stand-alone program under
    -fsanitize=address,undefined."""
    src = os.path.join(ROOT, "tests", "cpp", "mosaic_rule_test.cpp")
    outs = []
    for name, extra in (("mosaic_rule_test", []), ("mosaic_rule_test_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])):
        exe = str(tmp_path / name)
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-ffp-contract=off"] + extra + [src, "-o", exe])
        r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
        print(r.stdout[-3000:], r.stderr)
        assert r.returncode == 0 and r.stdout.strip().splitlines()[-1] == "OK mosaic_rule", r.stdout[-3000:] + r.stderr
        outs.append(r.stdout)
    assert outs[0] == outs[1]
