"""emba_amd/csrc/graph_rule.h on a CPU: the rotation graph — the refusals, Jr^-1, and the damped Gauss-Newton solve by preconditioned
conjugate gradients with the anchors held exactly, through tests/cpp/graph_rule_test.cpp."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_graph_rule_on_the_cpu(tmp_path):
    """graph_rule.h (plain C++17, no HIP): tests/cpp/graph_rule_test.cpp checks every refusal in the order the C ABI reports them (no anchor and the first
    unreachable frame among them), Jr^-1 against central differences at 1e-7, 1e-3, 0.4, 1.7, 3.0 and 3.14 rad, exact edges from a perturbed start (the truth
    to 1e-9 rad, the anchor's and an edgeless frame's bits kept), a second anchor held, nothing free, and a permuted edge list on noisy edges within the
    spread it prints.  Built twice: plain, and as a stand-alone program under -fsanitize=address,undefined."""
    src = os.path.join(ROOT, "tests", "cpp", "graph_rule_test.cpp")
    outs = []
    for name, extra in (("graph_rule_test", []), ("graph_rule_test_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])):
        exe = str(tmp_path / name)
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-ffp-contract=off"] + extra + [src, "-o", exe])
        r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
        print(r.stdout[-3000:], r.stderr)
        assert r.returncode == 0 and r.stdout.strip().splitlines()[-1] == "OK graph_rule", r.stdout[-3000:] + r.stderr
        outs.append(r.stdout)
    assert outs[0] == outs[1]
