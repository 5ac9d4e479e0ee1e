"""emba_amd/csrc/view_rule.h on a CPU: the sample of a panorama plane at a projected sensor pixel, its 8-bit tone, the frame of a
timestamp and the cut of F frames into chunks, through tests/cpp/view_rule_test.cpp."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_view_rule_on_the_cpu(tmp_path):
    """view_rule.h (plain C++17, no HIP): tests/cpp/view_rule_test.cpp checks view_sample at the four corners of a cell, at ax = 0 across the seam
    (ix = W - 1), at iy = -1, H - 2 and H - 1 and at a pm that is not finite; view_u8 at lo == hi, below lo and above hi; view_frame_of on and between the
    edges; the chunk cutter at F = 0, 1, 65 535 and 65 536.  Built twice: plain, and as a stand-alone program under -fsanitize=address,undefined — every
    plane of the test is exactly as large as the rule says it reads."""
    src = os.path.join(ROOT, "tests", "cpp", "view_rule_test.cpp")
    outs = []
    for name, extra in (("view_rule_test", []), ("view_rule_test_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])):
        exe = str(tmp_path / name)
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-ffp-contract=off"] + extra + [src, "-o", exe])
        r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
        print(r.stdout[-3000:], r.stderr)
        assert r.returncode == 0 and r.stdout.strip().splitlines()[-1] == "OK view_rule", r.stdout[-3000:] + r.stderr
        outs.append(r.stdout)
    assert outs[0] == outs[1]
