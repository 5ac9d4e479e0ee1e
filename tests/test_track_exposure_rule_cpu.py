"""emba_amd/csrc/track_exposure_rule.h on a CPU: the argument checks of the frame tracker with exposure, one pixel against a level's two integer
sums under a gain and a bias, and the start of a frame's gain and bias, through tests/cpp/track_exposure_rule_test.cpp."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_track_exposure_rule_on_the_cpu(tmp_path):
    """track_exposure_rule.h (plain C++17, no HIP): tests/cpp/track_exposure_rule_test.cpp checks the refusals of the bounds and of `estimate` in the order the
    C ABI reports them, track_exposure_pixel against track_pixel bit for bit at a = 1, b = 0 (and the ten shared sums against align_accumulate's), against
    exposure_pixel on the materialised mean plane of level 0 under non-trivial gains and biases, the precedence outside / masked / skipped with skipped
    testing the raw byte, and the start gain and bias across lost frames.  Built twice: plain, and as a stand-alone program under
    -fsanitize=address,undefined."""
    src = os.path.join(ROOT, "tests", "cpp", "track_exposure_rule_test.cpp")
    outs = []
    for name, extra in (("track_exposure_rule_test", []), ("track_exposure_rule_test_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])):
        exe = str(tmp_path / name)
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-ffp-contract=off"] + extra + [src, "-o", exe])
        r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
        print(r.stdout[-3000:], r.stderr)
        assert r.returncode == 0 and r.stdout.strip().splitlines()[-1] == "OK track_exposure_rule", r.stdout[-3000:] + r.stderr
        outs.append(r.stdout)
    assert outs[0] == outs[1]
