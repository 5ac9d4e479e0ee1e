"""Generates tests/golden/ref_build_vectors.npz: what the REFERENCE build under oracle/_ref (oracle/Makefile: libref_basalt.so, libref_eigen.so)
returns for the inputs of the two live tests of tests/test_oracle_pinned.py, so that both also hold where oracle/_ref cannot be built:

    prim_*   so3_exp, so3_log, left_jacobian (Jl, Jl^-1) of the reference's basalt/Sophus headers   test_primitives_match_reference_build_bitwise
    ldlt_*   S.ldlt().solve(rhs) on random SPD / semi-definite / indefinite systems                 test_solver_restatements_live_against_the_reference_eigen_build
    inv2_*   Matrix2d::inverse()
    cg_*     solveNormalEqCG assembled by the reference's eigen_utils on a small oracle workload

The inputs are drawn exactly as the tests draw them and stored beside the outputs.

Run where oracle/_ref is built:   make -C oracle && python tests/golden/make_ref_build_golden.py
The fixture holds inputs and the reference build's outputs; it is data, not source."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", ".."))
sys.path.insert(0, os.path.join(HERE, ".."))
from oracle import oracle as O  # noqa: E402
from helpers import small_workload, oracle_run  # noqa: E402
import test_oracle_pinned as T  # noqa: E402


def main():
    assert O.ref_available() and O.ref_eigen() is not None, "oracle/_ref is not built"
    out = {}
    W = T.primitive_inputs()
    out["prim_w"] = W
    out["prim_exp"] = np.array([O.so3_exp(w, use_ref=True) for w in W])
    out["prim_log"] = np.array([O.so3_log(q, use_ref=True) for q in out["prim_exp"]])
    jl = [O.left_jacobian(w, use_ref=True) for w in W]
    out["prim_jl"] = np.array([j[0] for j in jl]); out["prim_jl_inv"] = np.array([j[1] for j in jl])

    systems, A2 = T.solver_inputs()
    out["ldlt_n"] = np.array([S.shape[0] for S, _ in systems])
    out["ldlt_S"] = np.concatenate([S.reshape(-1) for S, _ in systems]); out["ldlt_rhs"] = np.concatenate([r for _, r in systems])
    res = [O.ref_ldlt_solve(S, r) for S, r in systems]
    out["ldlt_x"] = np.concatenate([b[0] for b in res]); out["ldlt_piv"] = np.concatenate([np.asarray(b[2]).reshape(-1) for b in res])
    out["ldlt_info"] = np.array([b[3] for b in res])
    out["inv2_A"] = A2; out["inv2_out"] = np.array([O.ref_inverse2(A) for A in A2])

    w = small_workload(**T.CG_WORKLOAD)
    ne = oracle_run(O, w, dense_A12=True)["ne"]
    for i, (lam, skip) in enumerate(T.CG_CASES):
        x1r, x2r, itr, errr, _ = O.ref_solve_normal_eq_cg(ne["A11"][skip:, skip:], ne["A12"][skip:, :], ne["A22"], ne["b1"][skip:], ne["b2"], lam)
        out[f"cg{i}_x"] = np.concatenate([x1r, x2r]); out[f"cg{i}_iters"] = np.array(itr); out[f"cg{i}_err"] = np.array(errr)
    path = os.path.join(HERE, "ref_build_vectors.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
