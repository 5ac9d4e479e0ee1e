"""TEST INFRASTRUCTURE (no HIP in here): the intensity panorama (emba_amd/csrc/poisson_host.h, poisson_kernels.h) at every tile, fold and sweep-chunk edge —
the launch plan of emba_amd/csrc/poisson_rule.h restated in Python, the case table tests/test_poisson_edge_cases_cpu.py (the plan, its coverage, the numpy
references) and tests/test_gpu_poisson_edges.py (the device) share, and the suite's random planes.

The plan, once.  The solve works on the transposed plane (W x H), so every product of the Fourier form has M = W:
    dense (option poisson = 1)   four products H x W x {W, H, W, H}, no sweeps
    unfolded                     two products W x H x H, A's row stride H
    folded (H even, H >= 64, option poisson = 0), h = H / 2
                                 four products W x h x h whose A operand reads every other column of the W x H plane: stride 2, row stride H
A product runs on the 128 x 128 kernel where that gives every CU a tile, else on the 64 x 128 kernel where that gives every CU two, else on the 64 x 64 one;
it loads 16 bytes at a time where K and N are even.  A thread stages THREAD_COLS consecutive columns of B, so a vector load straddles the edge of B exactly
where N is no multiple of that.  The Thomas sweeps cut the Wt = W (wrapped: W - 1) rows into 128 chunks of q = ceil(Wt / 128) rows; the backward sweep replays
a chunk from registers up to q = 32 and from the factor table beyond."""
import functools

import numpy as np

GEMM_BK = 16
TILE = {"k64x64": (64, 64), "k64x128": (64, 128), "k128x128": (128, 128)}      # block tile (rows, columns) of the three kernels
THREAD_COLS = {"k64x64": 4, "k64x128": 8, "k128x128": 4}                        # B doubles a thread stages per k: BN / 16 at 256 threads, 128 / 32 at 512
TRI_SYS, TRI_CHUNKS, TRI_MAX_Q = 8, 128, 32
FOLD_MIN_H = 64
N_CU = 256                    # compute units of an MI355X: what the table below was laid out for
DIRICHLET, WRAP = "dirichlet", "wrap"


def ceil_div(a, b):
    return -(-a // b)


def poisson_folds(H, poisson):
    return poisson != 1 and H % 2 == 0 and H >= FOLD_MIN_H and poisson != 2


def gemm_form(M, N, n_cu, gemm64):
    if ceil_div(M, 128) * ceil_div(N, 128) >= n_cu and not gemm64:
        return "k128x128"
    if ceil_div(M, 64) * ceil_div(N, 128) >= 2 * n_cu:
        return "k64x128"
    return "k64x64"


def gemm_vec(K, N):
    return int(K % 2 == 0 and N % 2 == 0)


def tri_chunk_len(W):
    return ceil_div(W, TRI_CHUNKS)


def tri_replay_from_table(W):
    return tri_chunk_len(W) > TRI_MAX_Q


def products(H, W, poisson):
    """(M, N, K, lda, stride) of every product of one solve, in launch order"""
    if poisson == 1:
        return [(H, W, W, W, 1), (H, W, H, H, 1), (H, W, W, W, 1), (H, W, H, H, 1)]
    if poisson_folds(H, poisson):
        return [(W, H // 2, H // 2, H, 2)] * 4
    return [(W, H, H, H, 1)] * 2


def plan(H, W, n_cu=N_CU, gemm64=0, poisson=0, boundary=DIRICHLET):
    """{"fold", "products": [(M, N, K, lda, stride, vec, form)], "sweep": (Wt, q, "registers" | "table") or None (the dense form has no sweeps)}"""
    prods = [(M, N, K, lda, s, gemm_vec(K, N), gemm_form(M, N, n_cu, gemm64)) for M, N, K, lda, s in products(H, W, poisson)]
    sweep = None
    if poisson != 1:
        Wt = W - 1 if boundary == WRAP else W
        sweep = (Wt, tri_chunk_len(Wt), "table" if tri_replay_from_table(Wt) else "registers")
    return {"fold": poisson_folds(H, poisson), "products": prods, "sweep": sweep}


def plan_text(H, W, n_cu=N_CU, gemm64=0, poisson=0, boundary=DIRICHLET):
    """the plan as tests/cpp/poisson_rule_test.cpp prints it for the line `H W n_cu gemm64 poisson boundary`"""
    p = plan(H, W, n_cu, gemm64, poisson, boundary)
    lines = [f"case {H} {W} {n_cu} {gemm64} {poisson} {int(boundary == WRAP)}", f"fold {int(p['fold'])}"]
    lines += ["product " + " ".join(str(v) for v in prod) for prod in p["products"]]
    lines.append("sweep none" if p["sweep"] is None else "sweep {} {} {}".format(*p["sweep"]))
    return "\n".join(lines) + "\n"


def tails(prod):
    """(M, N, K) remainders of a product against its kernel's block tile, and whether a thread's vector of B straddles the edge of B"""
    M, N, K, _, _, _, form = prod
    bm, bn = TILE[form]
    return M % bm, N % bn, K % GEMM_BK, N % THREAD_COLS[form] != 0


def chunk_sizes(Wt):
    """rows of each of the 128 chunks of a sweep over Wt rows"""
    q = tri_chunk_len(Wt)
    return [max(0, min(Wt, (c + 1) * q) - c * q) for c in range(TRI_CHUNKS)]


class Case:
    def __init__(self, H, W, boundary=DIRICHLET, forms=("k64x64",), **options):
        self.H, self.W, self.boundary, self.options, self.forms = H, W, boundary, options, frozenset(forms)
        self.id = f"{H}x{W}-{boundary}" + "".join(f"-{k}{v}" for k, v in options.items())

    def plan(self, n_cu=N_CU):
        return plan(self.H, self.W, n_cu, self.options.get("gemm64", 0), self.options.get("poisson", 0), self.boundary)

    def plan_text(self, n_cu=N_CU):
        return plan_text(self.H, self.W, n_cu, self.options.get("gemm64", 0), self.options.get("poisson", 0), self.boundary)

    def __repr__(self):
        return self.id


# Large: 33 x 9 = 297 tiles of 128 x 128 (>= 256 CUs), 65 x 9 = 585 of 64 x 128 (>= 512) under gemm64.  Each gemm64 row follows its shape's row, so that one
# numpy panorama serves both.  No smaller plane reaches the 128 x 128 kernel with all three tails: its tile count ceil(W / 128) ceil(N / 128) >= 256 needs
# W N >= 4.2 M whatever the shape, and these have W N = 4.2 M.
LARGE = []
for _H, _W, _o in [(1025, 4097, {}),                    # unfolded, stride 1, vec 0; tails M 1, N 1, K 1; q = 33
                   (1026, 4100, {"poisson": 2}),        # unfolded, stride 1, vec 1; N tail 2: narrower than a thread's vector
                   (2050, 4097, {}),                    # folded, stride 2, h = 1025, vec 0
                   (2052, 4100, {})]:                   # folded, stride 2, h = 1026, vec 1, N tail 2
    LARGE += [Case(_H, _W, DIRICHLET, ("k128x128",), **_o), Case(_H, _W, DIRICHLET, ("k64x128",), gemm64=1, **_o)]

SMALL = []
for _H, _W in [(62, 125),            # even H below the fold threshold: stride 1, vec 1
               (66, 131),            # the smallest ragged fold: h = 33, vec 0
               (100, 203),           # h = 50: vec 1, K tail 2, N = 50 = 12 vectors of 4 and a half
               (130, 67),            # taller than wide: h = 65, a second N tile of one column
               (132, 69)]:           # h = 66: vec 1 with a second N tile of two columns, half a thread's vector (the large cases' tail, on the 64 x 64 kernel)
    SMALL += [Case(_H, _W, DIRICHLET), Case(_H, _W, WRAP)]
SMALL.append(Case(66, 131, DIRICHLET, poisson=1))       # the dense form: stride 1, vec 0, epilogue 1 on partial tiles

SWEEP = [Case(24, 4096, DIRICHLET),      # q = 32: the last width replayed from registers
         Case(24, 4097, DIRICHLET),      # q = 33: the first replayed from the table; chunk 124 holds five rows, chunks 125 to 127 none
         Case(65, 4224, DIRICHLET),      # q = 33 with every chunk full; H no multiple of the 8 systems of a workgroup
         Case(24, 4225, DIRICHLET),      # q = 34
         Case(24, 8192, DIRICHLET),      # q = 64
         Case(24, 4097, WRAP),           # Wt = 4096: registers
         Case(24, 4098, WRAP),           # Wt = 4097: p and the q table through the table branch
         Case(5, 3, WRAP), Case(5, 4, WRAP)]      # the narrowest widths the wrapped boundary admits: sweeps over 2 and 3 rows

CASES = LARGE + SMALL + SWEEP
SHAPES = sorted({(c.H, c.W, c.boundary) for c in CASES})


def planes(H, W):
    """the suite's random gradient planes (test_gpu_parity.py::test_poisson_reconstruction_matches_oracle): seed = H"""
    rng = np.random.default_rng(H)
    return rng.normal(size=(H, W)), rng.normal(size=(H, W))


def divergence(Gx, Gy, boundary):
    import poisson_wrap_ref as PW
    from oracle import poisson as OP
    return PW.divergence(Gx, Gy) if boundary == WRAP else OP.divergence(Gx, Gy)


def laplacian(M, boundary):
    """the 5-point operator of the case's boundary: zero values all round, or columns wrapped and zero rows beyond the poles"""
    if boundary == WRAP:
        import poisson_wrap_ref as PW
        return PW.laplacian(M)
    P = np.pad(M, 1)
    return P[2:, 1:-1] + P[:-2, 1:-1] + P[1:-1, 2:] + P[1:-1, :-2] - 4.0 * M


def residual(M, Gx, Gy, boundary):
    return float(np.abs(laplacian(M, boundary) - divergence(Gx, Gy, boundary)).max())


def residual_bound(Gx, W):
    """the suite's bound on the residual of the 5-point equation"""
    return 1e-9 * float(np.abs(Gx).max()) * W


@functools.lru_cache(maxsize=1)
def reference(H, W, boundary):
    """(Gx, Gy, the numpy panorama, its residual), read-only; the last shape asked for is kept, which is what the order of CASES needs"""
    import poisson_wrap_ref as PW
    from oracle import poisson as OP
    Gx, Gy = planes(H, W)
    Mo = (PW if boundary == WRAP else OP).reconstruct_from_gradient(Gx, Gy)
    for a in (Gx, Gy, Mo):
        a.setflags(write=False)
    return Gx, Gy, Mo, residual(Mo, Gx, Gy, boundary)
