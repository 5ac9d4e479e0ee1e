// emba_amd/csrc/solve_rule.h — the host arithmetic of the solvers (solve_host.h), as functions of plain values: the sizes of the augmented Schur matrix, a
// rank's pixel range, the path of the optical axis, who gets the panorama column order, and the shape of the block-sparse product S -= U U^T.
//
// No HIP in here: plain C++17, so that tests/cpp/solve_rule_test.cpp checks it on a CPU in milliseconds.  The kernels' sizes come in as values —
// `slice_pix`: kSyrkSlicePix, `build_waves`: kBuildWaves of solve_kernels.h.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <cmath>

namespace emba {

// the pose block and the augmented Schur matrix S_aug of K control poses (the CG solvers take n and skip from it)
struct SchurDims {
    int n, na, skip; long lds;   // n = 3K; na = n + 1: row n carries y / the right-hand side; lds: leading dimension of S_aug and of U; skip: the fixed first pose's rows
    explicit SchurDims(int K, int fix_first_pose = 0) : n(3 * K), na(n + 1), skip(fix_first_pose ? 3 : 0), lds((na + 15) / 16 * 16) {}
    size_t size() const { return (size_t)lds * na; }
};

// pixels per chunk of U (two columns of lds doubles each): <= 6 GB of U
inline size_t schur_u_chunk(long lds, size_t n_pix) { return std::max<size_t>(1, std::min<size_t>(std::max<size_t>(n_pix, 1), (size_t)(6ull << 30) / (16ull * (size_t)lds))); }

// K <= 21 (22 with the first pose fixed): the Cholesky factorisation and both substitutions fit one launch of one workgroup
inline bool chol_single_launch(int n, int skip) { return n - skip + 1 <= 64 && skip <= 64; }

// the active pixels rank `rank` of `n_ranks` owns in a sharded solve: [lo, hi) of P
struct ShardRange { size_t lo, hi; };
inline ShardRange shard_range(size_t P, int rank, int n_ranks) { return {(P * (size_t)rank) / n_ranks, (P * ((size_t)rank + 1)) / n_ranks}; }

// azimuth / elevation path length (rad) of the optical axis over K control poses (unit quaternions x y z w); have: there is one (two poses at the least)
struct AxisPath { bool have; double az, el; };
inline AxisPath axis_path(const double* knots_xyzw, int K)
{
    if (!knots_xyzw || K < 2) return {false, 0.0, 0.0};
    double path_az = 0.0, path_el = 0.0, az0 = 0.0, el0 = 0.0;
    for (int i = 0; i < K; ++i) {
        const double x = knots_xyzw[4 * i], y = knots_xyzw[4 * i + 1], z = knots_xyzw[4 * i + 2], w = knots_xyzw[4 * i + 3];
        const double ax = 2.0 * (x * z + w * y), ay = 2.0 * (y * z - w * x), az_ = 1.0 - 2.0 * (x * x + y * y);      // R (0, 0, 1)
        const double az = atan2(ax, az_), el = asin(std::max(-1.0, std::min(1.0, ay)));
        if (i) { double d = az - az0; while (d > M_PI) d -= 2.0 * M_PI; while (d < -M_PI) d += 2.0 * M_PI; path_az += fabs(d); path_el += fabs(el - el0); }
        az0 = az; el0 = el;
    }
    return {true, path_az, path_el};
}

// The column order of U for the local solve (emba_perm_keys_kernel): panorama columns first when the camera mostly pans (azimuth path of the optical axis
// over the control poses >= its elevation path), the compact order otherwise.  mode: option solve_perm — -1 auto, 0 off, 1 on.
// Measured (device time of one solve, with / without; the U build reads its pixels' records out of sequence and pays 5 % for it): config 2's shape (K = 201,
// 10 M events over 10 s) 3.96 / 4.16 ms — SYRK 1.25 / 1.52, 5.8 / 7.9 products per slice —; 10 M events at K = 97: 2.81 / 2.79; 1 M events over 1 s at
// K = 201 (every pixel sees the whole window: nothing to gain) 2.27 / 2.24.  From six row blocks (K >= 128) up, unless option solve_perm forces it.
inline bool solve_perm_size_ok(int mode, size_t P, int K, int slice_pix)
{
    return !(mode == 0 || P < 4 * (size_t)slice_pix || (mode < 0 && 3 * K < 384) || 3 * K < 256);
}
inline bool solve_perm_wanted(int mode, size_t P, int K, int slice_pix, double path_az, double path_el, bool have_path)
{
    if (!solve_perm_size_ok(mode, P, K, slice_pix)) return false;
    return mode >= 0 || (have_path && path_az >= path_el);      // (auto, mostly tilting: a panorama row is the better slice already)
}

// What one call of schur_accumulate is given: the matrix, the pixels, the chip, the options syrk_* and what is known of the camera's motion.
struct SyrkShape {
    int n; long lds; size_t n_pix;      // rows of S (3K), leading dimension of S_aug and U, pixels (two columns of U each)
    int n_cu, slice_pix, build_waves;
    int syrk_dense, syrk_lists, syrk_min_cols, syrk_item_cap;
    double fov_x, fov_y; AxisPath path;
};

enum SyrkStatus { kSyrkOk = 0, kSyrkBuildLds, kSyrkItemChunks };   // the two capacity limits: the U build's column staging in LDS; the item form's grid

// The shape of S -= U U^T for one call and the U chunk that begins at pixel p0.
struct SyrkPlan {
    // the call
    size_t chunk;                    // pixels per U chunk (schur_u_chunk)
    int nb64, nbp, nks_max;          // 64-row blocks of S, pairs of them, most K slabs per pair
    size_t build_lds; bool build_lds_raise;   // dynamic LDS of the U build; above 64 KB the launch needs the attribute raised
    bool sparse;                     // the block-sparse product
    double in_view; int band_blocks; // fraction of the control poses a pixel is in view for, and the row blocks that makes
    bool items_form;                 // the item form of the block-sparse product (else its lists form)
    size_t slab, item_slab;          // doubles of split-K slabs: every form, and what the item form asks for on top
    // the chunk [p0, p1)
    size_t p0, p1; long kc; int n_slices;     // its columns and slices of slice_pix pixels
    int nks; bool direct;            // K slabs per pair; the product writes S itself (one slab, not the item form)
    int item_chunk, n_item_chunks;   // item form: slices per item, items per pair
    SyrkStatus status;
};

inline SyrkPlan syrk_plan(const SyrkShape& in, size_t p0)
{
    SyrkPlan q{};
    const int n = in.n;
    q.chunk = schur_u_chunk(in.lds, in.n_pix);
    q.nb64 = (n + 63) / 64; q.nbp = q.nb64 * (q.nb64 + 1) / 2;
    q.nks_max = std::max(1, (4 * in.n_cu + q.nbp - 1) / q.nbp);   // enough (tile pair, K slab) blocks to fill the chip ...
    q.slab = (size_t)q.nks_max * q.nbp * 4096;
    q.build_lds = (size_t)(2 * in.build_waves + 1) * n * sizeof(double);
    q.build_lds_raise = q.build_lds > 64 * 1024;
    if (q.build_lds > 160 * 1024) q.status = kSyrkBuildLds;
    // Block-sparse SYRK (>= 4 row blocks, i.e. K >= 64): the columns of a slice of slice_pix consecutive active pixels — a piece of a
    // panorama row — are non-zero only in the rows of the control poses in view while the camera looked there; over a long window
    // (config 2: 10 s, K = 201) that is a band, and only the (row-block pair, slice) products with both blocks populated are formed.
    // Option syrk_dense switches it off (comparison).
    q.sparse = q.nb64 >= 4 && q.nb64 <= 64 && !in.syrk_dense;
    // Where the item form pays: a BANDED U — a pixel is in view for the fraction fov / (path of the optical axis over the window) of the control poses, and an
    // operand block is read once per pair of its band.  With a dense band (every pixel sees the whole window: 1 s at any K) there is nothing to re-use that the
    // lists form does not get from its longer runs (measured: 10 M events / K = 97 over 1 s 3.14 vs 3.38 ms per solve, 1 M / K = 201 over 1 s 2.5 vs 2.75; config 2's
    // shape, 10 s: 4.15 vs 3.93).  Option syrk_lists: 0 auto, 1 the lists form always, 2 the item form always.
    q.in_view = 1.0;
    if (in.path.have) q.in_view = std::min(1.0, (in.path.az >= in.path.el ? in.fov_x : in.fov_y) / std::max(std::max(in.path.az, in.path.el), 1e-9));
    q.band_blocks = std::min(q.nb64, (int)std::ceil(q.in_view * q.nb64) + 1);
    q.items_form = q.sparse && (in.syrk_lists == 2 || (in.syrk_lists == 0 && 2 * q.band_blocks <= q.nb64));

    q.p0 = p0; q.p1 = std::min(in.n_pix, p0 + q.chunk);
    q.kc = (long)(2 * (q.p1 - q.p0));
    q.n_slices = (int)((q.p1 - q.p0 + in.slice_pix - 1) / in.slice_pix);
    q.nks = (int)std::max<long>(1, std::min<long>(q.nks_max, q.kc / in.syrk_min_cols));   // ... but >= 512 columns each (option syrk_min_cols): a block pays a fixed LDS combine + 32-KB slab write
    // ... and whole rounds of one block per CU.  Measured at K = 21, 137 k columns on 256 CUs: 268 blocks of 512 columns took 57 us, 255 blocks of 536 columns 44 us
    // (this rule makes it 137 000 / 512 = 267 -> 256 blocks of 535 columns)
    if ((long)q.nbp * q.nks > in.n_cu) q.nks = (int)std::max<long>(1, ((long)q.nbp * q.nks / in.n_cu) * in.n_cu / q.nbp);
    if (q.sparse) q.nks = std::max(1, std::min(q.nks_max, q.n_slices));      // (the lists form: a workgroup per (pair, part) walks every nks-th slice of the pair's list)
    q.direct = q.nks == 1 && !q.items_form;
    // ITEM form of the block-sparse product (round 5, SyrkParams::items): workgroups = (block pair, chunk of slices) in chunk-major order.  Option syrk_lists = 1
    // keeps the round-3/4 form.  Its slabs: option syrk_item_cap (4096; tests force the overflow branch with 8) — items beyond them add to S by global atomics.
    if (q.items_form) {
        const long pairs_est = (long)q.band_blocks * (q.band_blocks + 1) / 2;
        q.item_chunk = (int)std::min<long>(64, std::max<long>(4, ((long)q.n_slices * pairs_est * 3 / 2 + 2999) / 3000));
        q.n_item_chunks = (q.n_slices + q.item_chunk - 1) / q.item_chunk;
        if (!q.status && (q.n_item_chunks > 65535 || q.nbp > 65535)) q.status = kSyrkItemChunks;
        q.item_slab = std::max<size_t>((size_t)q.nks_max * q.nbp, (uint32_t)in.syrk_item_cap) * 4096;
    }
    return q;
}

}  // namespace emba
