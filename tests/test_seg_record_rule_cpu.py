"""emba_amd/csrc/seg_record_rule.h on a CPU: the segment records the host forms for a steady step (option step_prep = 2) against the oracle's restatement of
the reference's spline, on the control-pose pairs of the golden cases (tests/golden/so3_spline_n2.npz); and the option's entry in the option table.

The bound is MEASURED (tests/cpp/seg_record_rule_test.cpp states it): tests/golden/seg_records_device_gfx950.npz holds the records the device's launch in front of
the warp kernel (step_prep = 0) formed for the same pairs — tests/test_gpu_step_prep_host.py checks on the GPU that it still forms exactly these —, `differences`
below measures them against the oracle, and the bound on each quantity is 4 x the largest difference found in it (none above 4 x the largest of all)."""
import os
import re
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "so3_spline_n2.npz")
DEVICE = os.path.join(ROOT, "tests", "golden", "seg_records_device_gfx950.npz")
SRC = os.path.join(ROOT, "tests", "cpp", "seg_record_rule_test.cpp")
# the largest |device record - oracle| on the golden pairs, per quantity (tests/cpp/seg_record_rule_test.cpp; the largest of all: Jl^-1, 7.77e-16) ...
MEASURED = dict(delta=2.0 ** -52, r1=2.0 ** -53, k=2.0 ** -52, jinv=7 * 2.0 ** -53, q=2.0 ** -53)
TOL = {k: 4 * v for k, v in MEASURED.items()}      # ... and the bounds, absolute: 8.9e-16, 4.4e-16, 8.9e-16, 3.1e-15 (r2, through Jl^-1), 4.4e-16
WORD_TOL = np.array([0.0] * 4 + [TOL["delta"]] * 3 + [TOL["r1"]] + [TOL["k"]] * 3 + [TOL["jinv"]])      # a record's 12 words, one form against another


def _normalize(q):
    n2 = (q[0] * q[0] + q[2] * q[2]) + (q[1] * q[1] + q[3] * q[3])
    return q / np.sqrt(n2)


def _mul(a, b):
    """SO3 product with the normalising constructor (so3.hpp:324-339, :481-487): the operations of the oracle, in its order."""
    ax, ay, az, aw = a; bx, by, bz, bw = b
    return _normalize(np.array([aw * bx + ax * bw + ay * bz - az * by, aw * by + ay * bw + az * bx - ax * bz,
                                aw * bz + az * bw + ax * by - ay * bx, aw * bw - ax * bx - ay * by - az * bz]))


def _matrix(q):
    x, y, z, w = q
    tx, ty, tz = 2 * x, 2 * y, 2 * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    return np.array([[1 - (tyy + tzz), txy - twz, txz + twy], [txy + twz, 1 - (txx + tzz), tyz - twx], [txz - twy, tyz + twx, 1 - (txx + tyy)]])


def _hat(p):
    return np.array([[0, -p[2], p[1]], [p[2], 0, -p[0]], [-p[1], p[0], 0]])


def differences(O, g, rec):
    """Records `rec` (cases x (K - 1) x 12) of the golden control poses against the oracle, the largest absolute difference per quantity: delta against the oracle's
    logarithm of the oracle-order product; r1 against -theta / 2 of the oracle's delta; k against R0 times the oracle's unit axis; Jl^-1 = I + r1 A + r2 A^2,
    A = hat(delta / theta) of the record, against the oracle's Jl^-1 of the record's delta (r2: |A^2| has entries of order 1); q = p0 exp(u delta) of the case's
    own query against the reference's recorded q.  p0 is a copy and r1 is -theta / 2 of the record's own delta: exact, asserted.  Also counts the branches."""
    knots = g["knots"]
    n_case, K = knots.shape[0], knots.shape[1]
    t0, dt = int(g["t0_ns"]), int(g["dt_ns"])
    branches = dict(zero=0, small=0, general=0, near_pi=0)
    worst = dict(delta=0.0, r1=0.0, k=0.0, jinv=0.0, q=0.0)
    for c in range(n_case):
        for s in range(K - 1):
            p0, p1, seg = knots[c, s], knots[c, s + 1], rec[c, s]
            assert np.array_equal(seg[:4], p0)
            p0inv = _normalize(np.array([-p0[0], -p0[1], -p0[2], p0[3]]))
            delta = O.so3_log(_mul(p0inv, p1))
            worst["delta"] = max(worst["delta"], np.abs(seg[4:7] - delta).max())
            th_o = np.sqrt((delta[0] * delta[0] + delta[1] * delta[1]) + delta[2] * delta[2])
            worst["r1"] = max(worst["r1"], abs(seg[7] + 0.5 * th_o))
            n2 = (seg[4] * seg[4] + seg[5] * seg[5]) + seg[6] * seg[6]
            th = np.sqrt(n2)
            assert seg[7] == -0.5 * th
            if th == 0.0:
                branches["zero"] += 1
                assert not seg[8:].any()
                continue
            if th_o > 0.0:
                worst["k"] = max(worst["k"], np.abs(seg[8:11] - _matrix(p0) @ (delta / th_o)).max())
            A = _hat(seg[4:7] / th)
            jinv = np.eye(3) + seg[7] * A + seg[11] * (A @ A)
            branches["small" if n2 <= 1e-10 else ("general" if th < np.pi - 1e-5 else "near_pi")] += 1
            worst["jinv"] = max(worst["jinv"], np.abs(jinv - O.left_jacobian(seg[4:7])[1]).max())
        # the case's own query: q = p0 exp(u delta) with the record of its segment
        st = int(g["t"][c]) - t0
        s, u = st // dt, float(st % dt) / float(dt)
        seg = rec[c, s]
        q = _mul(seg[:4], O.so3_exp(seg[4:7] * u))
        worst["q"] = max(worst["q"], np.abs(q - g["q"][c]).max())
    return {k: float(v) for k, v in worst.items()}, branches


def host_records(tmp_path, knots, compiler=("g++",)):
    """tests/cpp/seg_record_rule_test.cpp compiled without contraction and run on every pair of neighbouring control poses (its hand cases run too)."""
    exe = str(tmp_path / "seg_record_rule_test")
    subprocess.check_call(list(compiler) + ["-std=c++17", "-O2", "-Wall", "-Werror", "-ffp-contract=off", "-DEMBA_FP_CONTRACT_OFF", SRC, "-o", exe])
    n_case, K = knots.shape[0], knots.shape[1]
    pairs = np.concatenate([knots[:, :-1], knots[:, 1:]], axis=2).reshape(-1, 8)
    fin, fout = tmp_path / "pairs.bin", tmp_path / "records.bin"
    with open(fin, "wb") as f:
        f.write(np.int32(pairs.shape[0]).tobytes()); f.write(np.ascontiguousarray(pairs).tobytes())
    r = subprocess.run([exe, str(fin), str(fout)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.strip().splitlines()[-1] == "OK seg_record_rule", r.stdout + r.stderr
    return np.fromfile(fout).reshape(n_case, K - 1, 12)


def test_the_bound_is_four_times_the_device_records_distance_from_the_oracle(oracle_mod):
    """TOL is not chosen: it is 4 x the largest difference between the oracle and the records the device's own launch forms for the golden pairs."""
    g = np.load(GOLD)
    dev = np.load(DEVICE)
    assert np.array_equal(dev["knots"], g["knots"])
    worst, branches = differences(oracle_mod, g, dev["seg"])
    print("device records against the oracle:", worst, branches)
    assert branches["zero"] and branches["small"] and branches["general"] and branches["near_pi"], branches
    assert worst == MEASURED, (worst, MEASURED)


def test_host_segment_records_against_the_oracle(tmp_path, oracle_mod):
    """Every pair of neighbouring control poses of the golden cases through the small-angle, general and near-pi branches (counted): every quantity of the host's
    records within its bound of the oracle; and every word within its bound of the device's records."""
    g = np.load(GOLD)
    rec = host_records(tmp_path, g["knots"])
    worst, branches = differences(oracle_mod, g, rec)
    d = np.abs(rec - np.load(DEVICE)["seg"]).max(axis=(0, 1))
    print("host records against the oracle:", worst, branches, "bound", TOL)
    print("host records against the device's, per word:", d)
    assert branches["zero"] and branches["small"] and branches["general"] and branches["near_pi"], branches
    for k, v in worst.items():
        assert v <= TOL[k], (k, v, TOL[k])
    assert (d <= WORD_TOL).all(), (d, WORD_TOL)


def test_host_compile_of_the_library_forms_the_same_records(tmp_path, oracle_mod):
    """The library's host side is compiled by hipcc (clang), not g++.  The same header through hipcc's host compiler: everything that feeds the rounded pixel
    (p0, delta) and r1, k in the same bits; r2 = 1 - theta (1 + cos theta) / (2 sin theta) may differ in its last bit (observed: 4 of 1300 records, 2^-52 —
    the compilers are free to take sin and cos from one call or from two), so it is held to its bound like any other form; and the same bounds against the oracle."""
    from emba_amd import build
    g = np.load(GOLD)
    a = host_records(tmp_path, g["knots"])
    b = host_records(tmp_path, g["knots"], compiler=(build.hipcc(), "-x", "c++"))
    assert np.array_equal(a[..., :11], b[..., :11])
    assert np.abs(a[..., 11] - b[..., 11]).max() <= WORD_TOL[11]
    worst, _ = differences(oracle_mod, g, b)
    for k, v in worst.items():
        assert v <= TOL[k], (k, v, TOL[k])
    assert (np.abs(b - np.load(DEVICE)["seg"]).max(axis=(0, 1)) <= WORD_TOL).all()


def test_step_prep_2_is_in_the_option_table_and_has_its_gpu_test():
    """step_prep's third value selects another kernel instantiation and another host branch: the table admits it, and tests/test_gpu_step_prep_host.py — a GPU
    module — sets it against step_prep = 0 and against the oracle (tests/option_matrix.py lists the values 0 and 1 with tests/test_gpu_step_prep.py)."""
    import option_matrix as OM
    o = {x["name"]: x for x in OM.parse_options()}["step_prep"]
    assert (o["lo"], o["hi"], o["reorders"]) == (0, 2, False)
    with open(os.path.join(ROOT, "tests", "test_gpu_step_prep_host.py")) as f:
        text = f.read()
    assert re.search(r"^pytestmark = pytest\.mark\.gpu$", text, re.M)
    assert 'set_option("step_prep", 2)' in text and 'set_option("step_prep", 0)' in text and "step_prep=2" in text
    for name in ("test_host_records_against_the_launch", "test_trial_rejection_between_two_steps", "test_host_records_against_the_oracle"):
        assert re.search(r"^def %s\(" % name, text, re.M), name
