"""The C++ host's record_data hook (tests/cpp/record_test.cpp): emba_host::solveTimeWindow calls its record callback at the reference's three
points, and emba_host::ShardedLEGM::render_map_images renders rank 0's replica — the same images on one rank and on two ranks of one device."""
import subprocess

import numpy as np
import pytest

from emba_amd import io as eio
from helpers import oracle_run, small_workload
from test_cpp_host import _build, _write_case


def test_cpp_record_compiles_and_links(tmp_path, hip_lib):
    exe = _build(tmp_path, hip_lib, "record_test")
    assert subprocess.run([exe], capture_output=True).returncode == 2


def _run(exe, case, devices, max_iter, out_dir=""):
    r = subprocess.run([exe, str(case), devices, str(max_iter), str(out_dir)], capture_output=True, text=True, timeout=300)
    print(r.stdout[-4000:], r.stderr[-4000:])
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.strip().splitlines()
    rec = [ln.split()[1:] for ln in lines if ln.startswith("REC ")]
    lm = [ln for ln in lines if ln.startswith("LM ")]
    end = [ln.split() for ln in lines if ln.startswith("END ")][-1]
    return rec, lm, int(end[1]), int(end[2])


@pytest.mark.gpu
def test_cpp_record_points_and_images(tmp_path, hip_lib, oracle_mod):
    exe = _build(tmp_path, hip_lib, "record_test")
    w = small_workload(n_events=30000)
    o = oracle_run(oracle_mod, w)
    case = tmp_path / "in.bin"
    _write_case(case, w, o)
    out = tmp_path / "rec"
    out.mkdir()
    rec, lm, iters, converged = _run(exe, case, "0", 4, out)
    # an evo record at every loop iteration (iter 0 .. N-1), then one final record (evo + opt) with iter N
    assert len(lm) == iters
    assert [(int(a), int(b), int(c)) for a, b, c, _ in rec] == [(i, i, 0) for i in range(iters)] + [(iters, iters, 1)]
    H, W = w.pano_h, w.pano_w
    for k in range(len(rec)):
        b = str(out / f"rec_{k}")
        mp = np.fromfile(b + ".map").reshape(2, H, W)
        assert np.array_equal(np.fromfile(b + ".gx", np.uint8).reshape(H, W), eio.normalize_robust(mp[0], 0.1))
        assert np.array_equal(np.fromfile(b + ".gy", np.uint8).reshape(H, W), eio.normalize_robust(mp[1], 0.1))
        assert np.fromfile(b + ".rgb", np.uint8).size == 3 * H * W and np.fromfile(b + ".poisson", np.uint8).size == H * W
    # two ranks on one device: rank 0's replica renders, and the images are those of one rank wherever the two loops' maps agree
    out2 = tmp_path / "rec2"
    out2.mkdir()
    rec2, lm2, iters2, _ = _run(exe, case, "0,0", 4, out2)
    assert iters2 == iters and [r[:3] for r in rec2] == [r[:3] for r in rec]
    for k in range(len(rec)):
        m1, m2 = np.fromfile(str(out / f"rec_{k}.map")), np.fromfile(str(out2 / f"rec_{k}.map"))
        mp = m2.reshape(2, H, W)
        assert np.array_equal(np.fromfile(str(out2 / f"rec_{k}.gx"), np.uint8).reshape(H, W), eio.normalize_robust(mp[0], 0.1))
        if np.array_equal(m1, m2):
            assert rec2[k][3] == rec[k][3]
    assert np.array_equal(np.fromfile(str(out / "rec_0.map")), np.fromfile(str(out2 / "rec_0.map")))    # the uploaded map
    assert rec2[0][3] == rec[0][3]
