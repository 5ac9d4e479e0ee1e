"""The pair-aligned plan of the Gram launch on a CPU (emba_amd/csrc/step_rule.h: gram_pair_cuts, gram_paired)."""
import os
import re
import subprocess

import option_matrix as OM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_gram_pair_rule_on_the_cpu(tmp_path):
    """tests/cpp/gram_pair_rule_test.cpp cuts a few thousand vectors of pair sizes (random ones with empty pairs, K = 2, K = 3 with an empty pair, pairs shorter
    than a share, more pairs than blocks, a pair over many shares, the benchmark's shape; 12 ... 16 streaming waves, four chip sizes) into wave ranges:
    every slot exactly once, no range across the start of a pair's run, the share within its bounds, the grid within gram_plan's unless the runs alone
    outnumber its wave slots; and the rule on both sides of each of its clauses."""
    consts = OM.parse_constants()
    with open(OM.KERNELS_H) as f:
        consts["kEpTailBlk"] = OM._eval_int(re.search(r"constexpr\s+int\s+kEpTailBlk\s*=\s*([^;]+);", f.read()).group(1), consts)
    defs = dict(GRAM_BLOCK="kGramBlock", GRAM_CHUNK="kGramChunk", GRAM_CHUNK_MIN="kGramChunkMin", EP_TAIL_BLK="kEpTailBlk")
    exe = str(tmp_path / "gram_pair_rule_test")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror"] + ["-D%s=%d" % (k, consts[v]) for k, v in defs.items()] +
                          [os.path.join(ROOT, "tests", "cpp", "gram_pair_rule_test.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout[-3000:], r.stderr)
    assert r.returncode == 0 and r.stdout.strip().splitlines()[-1] == "OK gram_pair_rule", r.stdout[-3000:] + r.stderr
