// The host arithmetic of the solvers (emba_amd/csrc/solve_rule.h) on a CPU: cases computed by hand (the comment on each shows the arithmetic), and a sweep of
// the plan of the block-sparse product against the expressions schur_accumulate held before they moved into syrk_plan, restated here once.
// Prints "OK ..." and returns 0, or names what failed.
#include "../../emba_amd/csrc/solve_rule.h"

#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace emba;

namespace {

int g_fail = 0;
#define CHECK(cond, ...)                                          \
    do {                                                          \
        if (!(cond)) {                                            \
            if (++g_fail <= 20) {                                 \
                std::printf("FAIL %s:%d: %s -- ", __FILE__, __LINE__, #cond); \
                std::printf(__VA_ARGS__);                         \
                std::printf("\n");                                \
            }                                                     \
        }                                                         \
    } while (0)

#ifndef SYRK_SLICE_PIX
#define SYRK_SLICE_PIX 128      // kSyrkSlicePix of solve_kernels.h (tests/test_cpp_host.py passes the current values; the sweep runs with them)
#endif
#ifndef SCHUR_BUILD_WAVES
#define SCHUR_BUILD_WAVES 4     // kBuildWaves
#endif

// the hand-computed cases are worked out for slices of 128 pixels, 4 build waves, 256 CUs and the options' defaults
SyrkShape shape(int K, size_t n_pix)
{
    const SchurDims d(K);
    SyrkShape in{};
    in.n = d.n; in.lds = d.lds; in.n_pix = n_pix; in.n_cu = 256; in.slice_pix = 128; in.build_waves = 4;
    in.syrk_dense = 0; in.syrk_lists = 0; in.syrk_min_cols = 512; in.syrk_item_cap = 4096;
    in.fov_x = 1.0; in.fov_y = 1.0; in.path = AxisPath{false, 0.0, 0.0};
    return in;
}

void check_dims()
{
    // K = 21: n = 63, na = 64, lds = 64 (already a multiple of 16); m + 1 = 64 <= 64: the last K whose Cholesky is one launch
    SchurDims d(21);
    CHECK(d.n == 63 && d.na == 64 && d.lds == 64 && d.skip == 0 && d.size() == 4096, "K = 21");
    CHECK(chol_single_launch(63, 0), "K = 21: m + 1 = 64");
    // K = 22: n = 66, na = 67 -> lds = 80; m + 1 = 67 — the panel loop; with the first pose fixed m = 63 again: one launch
    d = SchurDims(22, 1);
    CHECK(d.n == 66 && d.na == 67 && d.lds == 80 && d.skip == 3 && d.size() == 80 * 67, "K = 22");
    CHECK(!chol_single_launch(66, 0) && chol_single_launch(66, 3) && !chol_single_launch(69, 3), "K = 22 / 23");
    // K = 100: n = 300, na = 301 -> lds = 304;  K = 201: n = 603, na = 604 -> lds = 608
    CHECK(SchurDims(100).lds == 304 && SchurDims(201).lds == 608 && SchurDims(201).size() == (size_t)608 * 604, "lds");
}

void check_plan()
{
    // K = 21: one row block, one pair; 4 x 256 blocks fill the chip: nks_max = 1024; LDS 9 x 63 x 8 = 4536
    SyrkPlan q = syrk_plan(shape(21, 1000), 0);
    CHECK(q.nb64 == 1 && q.nbp == 1 && q.nks_max == 1024 && !q.sparse && !q.items_form && q.build_lds == 4536 && !q.build_lds_raise && q.status == kSyrkOk, "K = 21");
    // ... 1000 pixels: 2000 columns / 512 = 3 slabs, 3 blocks <= 256 CUs: no rounding; with syrk_min_cols = 64: 31
    CHECK(q.chunk == 1000 && q.p1 == 1000 && q.kc == 2000 && q.n_slices == 8 && q.nks == 3 && !q.direct && q.slab == (size_t)1024 * 4096, "K = 21, 1000 pixels: nks %d", q.nks);
    SyrkShape in = shape(21, 1000); in.syrk_min_cols = 64;
    CHECK(syrk_plan(in, 0).nks == 31, "syrk_min_cols = 64");
    CHECK(syrk_plan(shape(21, 255), 0).nks == 1 && syrk_plan(shape(21, 255), 0).direct, "510 columns: one slab, written straight into S");
    // The rounding comment's case — K = 21, 137 k columns on 256 CUs: 137 000 / 512 = 267 blocks > 256 CUs -> (267 / 256) x 256 / 1 = 256 blocks (of 535 columns).
    // The comment's measurement compared 268 blocks of 512 columns with 255 of 536: the rule gives 256, not 255 (137 216 = 268 x 512 columns: 256 as well).
    CHECK(syrk_plan(shape(21, 68500), 0).nks == 256 && syrk_plan(shape(21, 68608), 0).nks == 256, "whole rounds of one block per CU: %d", syrk_plan(shape(21, 68500), 0).nks);
    in = shape(21, 68500); in.n_cu = 64;      // 64 CUs: nks_max = 256 < 267; 256 blocks are four whole rounds already
    CHECK(syrk_plan(in, 0).nks_max == 256 && syrk_plan(in, 0).nks == 256, "64 CUs");
    // K = 22: two row blocks, three pairs, nks_max = (1024 + 2) / 3 = 342; 3 x 267 = 801 blocks -> 3 rounds = 768 -> 256 per pair
    q = syrk_plan(shape(22, 68500), 0);
    CHECK(q.nb64 == 2 && q.nbp == 3 && q.nks_max == 342 && q.nks == 256, "K = 22: nks %d", q.nks);
    // K = 64: n = 192, three row blocks — dense; six pairs, nks_max = (1024 + 5) / 6 = 171 < 267; 6 x 171 = 1026 blocks -> 4 rounds = 1024 -> 170 per pair
    q = syrk_plan(shape(64, 68500), 0);
    CHECK(q.nb64 == 3 && q.nbp == 6 && !q.sparse && q.nks_max == 171 && q.nks == 170, "K = 64: nks %d", q.nks);
    // K = 65: n = 195, four row blocks — block-sparse; ten pairs, nks_max = 103; 68 500 pixels = 536 slices (535.2): nks = min(103, 536)
    q = syrk_plan(shape(65, 68500), 0);
    CHECK(q.nb64 == 4 && q.nbp == 10 && q.sparse && q.nks_max == 103 && q.n_slices == 536 && q.nks == 103, "K = 65");
    in = shape(65, 68500); in.syrk_dense = 1;
    CHECK(!syrk_plan(in, 0).sparse && !syrk_plan(in, 0).items_form, "option syrk_dense");
    // K = 100, the shape of the GPU SYRK tests: n = 300, five row blocks, 15 pairs, nks_max = (1024 + 14) / 15 = 69; LDS 9 x 300 x 8 = 21 600.
    // No path known: in view 1 -> band = min(5, 5 + 1) = 5 blocks, 10 > 5: the lists form.  1000 pixels = 8 slices: nks = 8
    q = syrk_plan(shape(100, 1000), 0);
    CHECK(q.nb64 == 5 && q.nbp == 15 && q.nks_max == 69 && q.build_lds == 21600 && q.sparse && q.in_view == 1.0 && q.band_blocks == 5 && !q.items_form, "K = 100");
    CHECK(q.n_slices == 8 && q.nks == 8 && !q.direct && q.slab == (size_t)69 * 15 * 4096 && q.item_slab == 0 && q.item_chunk == 0 && q.n_item_chunks == 0, "K = 100, 1000 pixels");
    CHECK(syrk_plan(shape(100, 128), 0).nks == 1 && syrk_plan(shape(100, 128), 0).direct && syrk_plan(shape(100, 129), 0).nks == 2, "one slice: one slab");
    // K = 201: n = 603, ten row blocks, 55 pairs, nks_max = (1024 + 54) / 55 = 19; LDS 43 416
    q = syrk_plan(shape(201, 1000), 0);
    CHECK(q.nb64 == 10 && q.nbp == 55 && q.nks_max == 19 && q.build_lds == 43416 && q.sparse, "K = 201");
    // K = 1365: n = 4095, 64 row blocks — still block-sparse; K = 1366: n = 4098, 65 — dense again (the slice masks hold 64 bits).  Both are past the LDS limit:
    CHECK(syrk_plan(shape(1365, 1000), 0).nb64 == 64 && syrk_plan(shape(1365, 1000), 0).sparse, "K = 1365");
    q = syrk_plan(shape(1366, 1000), 0);
    CHECK(q.nb64 == 65 && q.nbp == 2145 && !q.sparse && q.nks_max == 1 && q.status == kSyrkBuildLds, "K = 1366");
    // ... the build's LDS, 72 n bytes: above 64 KB from n = 912 (K = 304: 65 664; K = 303: 65 448), above 160 KB from n = 2277 (K = 759: 163 944; K = 758: 163 728)
    CHECK(!syrk_plan(shape(303, 1000), 0).build_lds_raise && syrk_plan(shape(304, 1000), 0).build_lds_raise && syrk_plan(shape(304, 1000), 0).build_lds == 65664, "64 KB");
    CHECK(syrk_plan(shape(758, 1000), 0).status == kSyrkOk && syrk_plan(shape(758, 1000), 0).build_lds_raise && syrk_plan(shape(759, 1000), 0).status == kSyrkBuildLds, "160 KB");
    // The shapes tests/test_gpu_solve_capacity.py runs on the device (tests/solve_edge_cases.py: about 1800 active pixels), with the K its constants derive from
    // 72 x 3K bytes against 64 KB and 160 KB — one statement per edge, so that a failure names it
    CHECK(!syrk_plan(shape(303, 1751), 0).build_lds_raise && syrk_plan(shape(303, 1751), 0).build_lds == 65448 && syrk_plan(shape(303, 1751), 0).status == kSyrkOk, "K = 303: no raise");
    CHECK(syrk_plan(shape(304, 1751), 0).build_lds_raise && syrk_plan(shape(304, 1751), 0).status == kSyrkOk, "K = 304: the raise");
    q = syrk_plan(shape(758, 1781), 0);      // n = 2274: 36 row blocks, 666 pairs, nks_max = (1024 + 665) / 666 = 2; 1781 pixels = 14 slices
    CHECK(q.status == kSyrkOk && q.build_lds == 163728 && q.build_lds == 160 * 1024 - 112 && q.build_lds_raise, "K = 758: 112 bytes under the CU's LDS");
    CHECK(q.nb64 == 36 && q.nbp == 666 && q.sparse && q.nks_max == 2 && q.n_slices == 14 && q.nks == 2 && !q.items_form, "K = 758: 36 row blocks, block-sparse");
    CHECK(syrk_plan(shape(759, 1781), 0).status == kSyrkBuildLds && syrk_plan(shape(759, 1781), 0).build_lds == 163944, "K = 759: refused");
    CHECK(solve_perm_size_ok(-1, 1751, 303, 128) && solve_perm_size_ok(-1, 1781, 758, 128) && !solve_perm_size_ok(-1, 511, 758, 128), "the column order's size rule decides by itself there");
}

void check_forms()
{
    // K = 201, ten row blocks: the item form needs 2 x band <= 10, band = ceil(10 x in view) + 1.
    // A pan of 1 rad seen through 0.375 rad: in view 0.375 -> ceil(3.75) + 1 = 5 blocks, 10 <= 10: items.  Through 0.4375 rad: ceil(4.375) + 1 = 6, 12 > 10: lists
    SyrkShape in = shape(201, 1000);
    in.path = AxisPath{true, 1.0, 0.25}; in.fov_x = 0.375; in.fov_y = 9.0;
    SyrkPlan q = syrk_plan(in, 0);
    CHECK(q.in_view == 0.375 && q.band_blocks == 5 && q.items_form, "in view 0.375");
    in.fov_x = 0.4375;
    q = syrk_plan(in, 0);
    CHECK(q.in_view == 0.4375 && q.band_blocks == 6 && !q.items_form, "in view 0.4375");
    in.syrk_lists = 2;      // forced
    CHECK(syrk_plan(in, 0).items_form, "syrk_lists = 2");
    in.fov_x = 0.375; in.syrk_lists = 1;
    CHECK(!syrk_plan(in, 0).items_form, "syrk_lists = 1");
    in.syrk_lists = 2; in.syrk_dense = 1;
    CHECK(!syrk_plan(in, 0).items_form, "no item form of the dense product");
    // mostly tilting: the elevation path and the vertical field of view decide — 0.5 rad through 4 rad of path: 0.125 -> ceil(1.25) + 1 = 3
    in = shape(201, 1000); in.path = AxisPath{true, 1.0, 4.0}; in.fov_x = 9.0; in.fov_y = 0.5;
    CHECK(syrk_plan(in, 0).in_view == 0.125 && syrk_plan(in, 0).band_blocks == 3 && syrk_plan(in, 0).items_form, "tilt");
    in.path = AxisPath{true, 0.0, 0.0};      // a camera at rest: the path is floored at 1e-9, in view 1, band = min(10, 11)
    CHECK(syrk_plan(in, 0).in_view == 1.0 && syrk_plan(in, 0).band_blocks == 10, "no motion");

    // item_chunk = (slices x pairs of the band x 3 / 2 + 2999) / 3000, in [4, 64].  Band 5 -> 15 pairs.
    in = shape(201, 1000); in.path = AxisPath{true, 1.0, 0.25}; in.fov_x = 0.375;
    q = syrk_plan(in, 0);      // 8 slices: (180 + 2999) / 3000 = 1 -> 4; (8 + 3) / 4 = 2 items per pair; one slab per workgroup-sized item: direct is off
    CHECK(q.item_chunk == 4 && q.n_item_chunks == 2 && q.nks == 8 && !q.direct && q.item_slab == (size_t)4096 * 4096 && q.slab == (size_t)19 * 55 * 4096, "item_chunk, lower clamp");
    in.syrk_item_cap = 8;      // fewer item slabs than the lists form's: 19 x 55 = 1045 stay
    CHECK(syrk_plan(in, 0).item_slab == (size_t)1045 * 4096, "syrk_item_cap = 8");
    in.n_pix = 128; in.syrk_item_cap = 4096;      // (one slice, nks = 1: the item form never writes S directly)
    CHECK(syrk_plan(in, 0).nks == 1 && !syrk_plan(in, 0).direct, "direct");
    // the U chunk: lds = 608 -> 6 GB / (16 x 608 = 9728) = 662 258 pixels (remainder 5120).  8 M pixels: 13 chunks, the last one 8 000 000 - 12 x 662 258 = 52 904 pixels
    in.n_pix = 8000000;
    q = syrk_plan(in, 0);      // 662 258 pixels = 5174 slices (5173.9): (5174 x 15 x 3 / 2 = 116 415 + 2999) / 3000 = 39; (5174 + 38) / 39 = 133
    CHECK(q.chunk == 662258 && q.p0 == 0 && q.p1 == 662258 && q.kc == 1324516 && q.n_slices == 5174 && q.item_chunk == 39 && q.n_item_chunks == 133 && q.nks == 19, "U chunk");
    CHECK(schur_u_chunk(608, 8000000) == 662258 && schur_u_chunk(608, 662258) == 662258 && schur_u_chunk(608, 5) == 5 && schur_u_chunk(608, 0) == 1, "schur_u_chunk");
    q = syrk_plan(in, (size_t)12 * 662258);      // 52 904 pixels = 414 slices (413.3): (9315 + 2999) / 3000 = 4
    CHECK(q.p0 == 7947096 && q.p1 == 8000000 && q.kc == 105808 && q.n_slices == 414 && q.item_chunk == 4 && q.n_item_chunks == 104, "last U chunk");
    // upper clamp — K = 65 (lds = 208: chunks of 1 935 832 pixels = 15 124 slices), no path: band 4 -> 10 pairs, item form forced:
    // (15 124 x 10 x 3 / 2 = 226 860 + 2999) / 3000 = 76 -> 64; (15 124 + 63) / 64 = 237
    in = shape(65, 2000000); in.syrk_lists = 2;
    q = syrk_plan(in, 0);
    CHECK(q.chunk == 1935832 && q.n_slices == 15124 && q.band_blocks == 4 && q.item_chunk == 64 && q.n_item_chunks == 237 && q.status == kSyrkOk, "item_chunk, upper clamp");
    // The 65 535 items per pair that the grid allows: with slices of 128 pixels and 6 GB of U a chunk has 15 124 slices at the most (above), far from 64 x 65 535 —
    // the limit is met with slices of one pixel and a leading dimension of 16 only (chunks of 25 165 824 pixels): 4 194 240 slices = 65 535 items of 64, one more = 65 536
    in = shape(100, (size_t)65535 * 64); in.lds = 16; in.slice_pix = 1; in.syrk_lists = 2;
    q = syrk_plan(in, 0);
    CHECK(q.chunk == (size_t)65535 * 64 && q.item_chunk == 64 && q.n_item_chunks == 65535 && q.status == kSyrkOk, "65535 items per pair");
    in.n_pix += 1;
    CHECK(syrk_plan(in, 0).n_item_chunks == 65536 && syrk_plan(in, 0).status == kSyrkItemChunks, "65536 items per pair");
}

void check_shards()
{
    // the ranks' ranges tile [0, P): P not divisible, fewer pixels than ranks, none
    const size_t Ps[] = {0, 1, 5, 7, 1000, 1001, 4194301};
    const int ranks[] = {1, 2, 3, 7, 8, 1024};
    for (size_t P : Ps)
        for (int n : ranks) {
            size_t at = 0, longest = 0, shortest = (size_t)-1;
            for (int r = 0; r < n; ++r) {
                const ShardRange s = shard_range(P, r, n);
                CHECK(s.lo == at && s.hi >= s.lo, "P %zu, rank %d of %d: [%zu, %zu) after %zu", P, r, n, s.lo, s.hi, at);
                at = s.hi; longest = std::max(longest, s.hi - s.lo); shortest = std::min(shortest, s.hi - s.lo);
            }
            CHECK(at == P && longest - shortest <= 1, "P %zu over %d ranks: covered up to %zu, shares of %zu ... %zu", P, n, at, shortest, longest);
        }
    // 7 pixels over 3 ranks: 7 r / 3 = 0, 2, 4, 7
    CHECK(shard_range(7, 0, 3).hi == 2 && shard_range(7, 1, 3).hi == 4 && shard_range(7, 2, 3).lo == 4 && shard_range(7, 2, 3).hi == 7, "7 over 3");
}

// K poses turned by angles[i] about the vertical (y) axis — the optical axis R (0, 0, 1) = (sin a, 0, cos a): azimuth a — or about the x axis:
// (0, -sin a, cos a): elevation -a
std::vector<double> turned(const std::vector<double>& angles, bool about_x, double scale = 1.0)
{
    std::vector<double> q;
    for (double a : angles) {
        const double s = scale * sin(0.5 * a), c = scale * cos(0.5 * a);
        q.insert(q.end(), {about_x ? s : 0.0, about_x ? 0.0 : s, 0.0, c});
    }
    return q;
}

void check_axis_path()
{
    std::vector<double> a;
    for (int i = 0; i <= 15; ++i) a.push_back(0.1 * i);      // 0 ... 1.5 rad
    AxisPath p = axis_path(turned(a, false).data(), 16);
    CHECK(p.have && fabs(p.az - 1.5) < 1e-12 && fabs(p.el) < 1e-12, "pan: (%.15g, %.15g)", p.az, p.el);
    for (double& v : a) v += 2.5;                            // 2.5 ... 4.0 rad: the azimuth jumps from +pi to -pi on the way
    p = axis_path(turned(a, false).data(), 16);
    CHECK(p.have && fabs(p.az - 1.5) < 1e-12 && fabs(p.el) < 1e-12, "pan across +-pi: (%.15g, %.15g)", p.az, p.el);
    p = axis_path(turned({0.0, 0.3, 0.8, 0.5}, true).data(), 4);      // up 0.8, back 0.3: a path of 1.1
    CHECK(p.have && fabs(p.az) < 1e-12 && fabs(p.el - 1.1) < 1e-12, "tilt: (%.15g, %.15g)", p.az, p.el);
    // a quaternion a little longer than 1 looking straight down: sin > 1 is clamped, the elevation stays pi / 2
    p = axis_path(turned({0.0, M_PI / 2}, true, 1.0000001).data(), 2);
    CHECK(p.have && fabs(p.el - M_PI / 2) < 1e-12, "asin clamp: %.15g", p.el);
    CHECK(!axis_path(turned({0.4}, false).data(), 1).have && !axis_path(nullptr, 16).have && !axis_path(turned({0.4}, false).data(), 0).have, "no path without two poses");
}

void check_perm()
{
    // forced (1): from 3K >= 256 — K = 85: 255, K = 86: 258; auto (-1): from 3K >= 384 — K = 127: 381, K = 128: 384
    CHECK(!solve_perm_wanted(1, 100000, 85, 128, 0, 0, false) && solve_perm_wanted(1, 100000, 86, 128, 0, 0, false), "3K = 255 / 258, forced");
    CHECK(!solve_perm_wanted(-1, 100000, 127, 128, 2.0, 1.0, true) && solve_perm_wanted(-1, 100000, 128, 128, 2.0, 1.0, true), "3K = 381 / 384, auto");
    CHECK(solve_perm_wanted(1, 100000, 127, 128, 2.0, 1.0, true), "forced between the two");
    // at least four slices of pixels
    CHECK(!solve_perm_wanted(-1, 511, 201, 128, 2.0, 1.0, true) && solve_perm_wanted(-1, 512, 201, 128, 2.0, 1.0, true) && !solve_perm_wanted(1, 511, 201, 128, 2.0, 1.0, true), "P < 4 slices");
    // auto asks the path: mostly tilting, or no path known — no; forced does not ask
    CHECK(!solve_perm_wanted(-1, 100000, 201, 128, 1.0, 2.0, true) && solve_perm_wanted(-1, 100000, 201, 128, 1.0, 1.0, true) && !solve_perm_wanted(-1, 100000, 201, 128, 2.0, 1.0, false), "path");
    CHECK(solve_perm_wanted(1, 100000, 201, 128, 1.0, 2.0, true) && solve_perm_wanted(1, 100000, 201, 128, 0, 0, false), "forced");
    CHECK(!solve_perm_wanted(0, 100000, 201, 128, 2.0, 1.0, true) && !solve_perm_size_ok(0, 100000, 201, 128) && solve_perm_size_ok(-1, 512, 128, 128), "off");
}

// ---- the sweep: schur_accumulate's own expressions as they stood before syrk_plan (context fields spelled as SyrkShape's), for the U chunk at p0 --------------
struct Ref {
    size_t chunk, lds_bytes, slab, item_slab, u_doubles, p1; int nb64, nbp, nks_max, n_slices, nks, band_blocks, item_chunk, n_item_chunks, direct;
    long kc; bool raise, sparse, items_form; double in_view; int fail;      // fail: 1 the LDS message, 2 the item-chunk message
};
Ref reference(const SyrkShape& c, size_t p0)
{
    Ref r{};
    const int n = c.n; const long lds_ = c.lds; const size_t n_pix = c.n_pix;
    const size_t chunk = std::max<size_t>(1, std::min<size_t>(std::max<size_t>(n_pix, 1), (size_t)(6ull << 30) / (16ull * (size_t)lds_)));   // <= 6 GB of U
    const int nb64 = (n + 63) / 64, nbp = nb64 * (nb64 + 1) / 2;
    const int nks_max = std::max(1, (4 * c.n_cu + nbp - 1) / nbp);
    r.u_doubles = (size_t)lds_ * 2 * chunk; r.slab = (size_t)nks_max * nbp * 4096;
    const size_t lds_bytes = (size_t)(2 * c.build_waves + 1) * n * sizeof(double);
    if (lds_bytes > 160 * 1024) r.fail = 1;
    r.raise = lds_bytes > 64 * 1024;
    const bool sparse = nb64 >= 4 && nb64 <= 64 && !c.syrk_dense;
    const size_t p1 = std::min(n_pix, p0 + chunk);
    const long kc = (long)(2 * (p1 - p0));
    const int n_slices = (int)((p1 - p0 + c.slice_pix - 1) / c.slice_pix);
    int nks = (int)std::max<long>(1, std::min<long>(nks_max, kc / c.syrk_min_cols));
    if ((long)nbp * nks > c.n_cu) nks = (int)std::max<long>(1, ((long)nbp * nks / c.n_cu) * c.n_cu / nbp);
    double paz = c.path.az, pel = c.path.el, in_view = 1.0;
    if (c.path.have) in_view = std::min(1.0, (paz >= pel ? c.fov_x : c.fov_y) / std::max(std::max(paz, pel), 1e-9));
    const int band_blocks = std::min(nb64, (int)std::ceil(in_view * nb64) + 1);
    const bool items_form = sparse && (c.syrk_lists == 2 || (c.syrk_lists == 0 && 2 * band_blocks <= nb64));
    if (sparse) nks = std::max(1, std::min(nks_max, n_slices));
    int item_chunk = 0, n_item_chunks = 0;
    const uint32_t item_cap = (uint32_t)c.syrk_item_cap;
    if (items_form) {
        const long pairs_est = (long)band_blocks * (band_blocks + 1) / 2;
        item_chunk = (int)std::min<long>(64, std::max<long>(4, ((long)n_slices * pairs_est * 3 / 2 + 2999) / 3000));
        n_item_chunks = (n_slices + item_chunk - 1) / item_chunk;
        if (!r.fail && (n_item_chunks > 65535 || nbp > 65535)) r.fail = 2;
        r.item_slab = std::max<size_t>((size_t)nks_max * nbp, item_cap) * 4096;
    }
    r.direct = (nks == 1);
    if (items_form) r.direct = 0;
    r.chunk = chunk; r.lds_bytes = lds_bytes; r.p1 = p1; r.nb64 = nb64; r.nbp = nbp; r.nks_max = nks_max; r.n_slices = n_slices; r.nks = nks; r.band_blocks = band_blocks;
    r.item_chunk = item_chunk; r.n_item_chunks = n_item_chunks; r.kc = kc; r.sparse = sparse; r.items_form = items_form; r.in_view = in_view;
    return r;
}

bool same(const SyrkPlan& q, const Ref& r, const SchurDims& d, size_t n_pix)
{
    return q.chunk == r.chunk && q.nb64 == r.nb64 && q.nbp == r.nbp && q.nks_max == r.nks_max && q.build_lds == r.lds_bytes && q.build_lds_raise == r.raise &&
           q.sparse == r.sparse && q.in_view == r.in_view && q.band_blocks == r.band_blocks && q.items_form == r.items_form && q.slab == r.slab && q.item_slab == r.item_slab &&
           q.p1 == r.p1 && q.kc == r.kc && q.n_slices == r.n_slices && q.nks == r.nks && (int)q.direct == r.direct && q.item_chunk == r.item_chunk &&
           q.n_item_chunks == r.n_item_chunks && (int)q.status == r.fail && (size_t)d.lds * 2 * schur_u_chunk(d.lds, n_pix) == r.u_doubles;
}

void check_sweep()
{
    const size_t pixels[] = {1, 129, 1000, 68500, 662259, 8000000};
    const AxisPath paths[] = {{false, 0.0, 0.0}, {true, 0.9, 0.2}, {true, 0.7, 6.5}};      // unknown; a short pan: everything in view; a long tilt: a band
    size_t plans = 0, items = 0, lists = 0, dense = 0, chunks = 0;
    for (int K = 1; K <= 1400; ++K) {
        const SchurDims d(K);
        for (size_t n_pix : pixels)
            for (int n_cu : {256, 64})
                for (int dn : {0, 1}) for (int ls : {0, 1, 2}) for (int mc : {512, 64}) for (int cap : {4096, 8})
                    for (const AxisPath& path : paths) {
                        SyrkShape in{d.n, d.lds, n_pix, n_cu, SYRK_SLICE_PIX, SCHUR_BUILD_WAVES, dn, ls, mc, cap, 1.2, 0.9, path};
                        const size_t chunk = schur_u_chunk(d.lds, n_pix), last = (n_pix - 1) / chunk * chunk;
                        for (size_t p0 : {(size_t)0, last}) {      // the first U chunk and the (ragged) last one
                            const SyrkPlan q = syrk_plan(in, p0);
                            CHECK(same(q, reference(in, p0), d, n_pix) && q.p0 == p0, "K %d, %zu pixels from %zu, %d CUs, dense %d lists %d min_cols %d item_cap %d, path %d %.1f %.1f", K,
                                  n_pix, p0, n_cu, dn, ls, mc, cap, (int)path.have, path.az, path.el);
                            ++plans; items += q.items_form; lists += q.sparse && !q.items_form; dense += !q.sparse; chunks += p0 != 0;
                            if (!last) break;
                        }
                    }
    }
    CHECK(items > 1000 && lists > 1000 && dense > 1000 && chunks > 1000, "coverage: %zu item, %zu lists, %zu dense plans, %zu last chunks", items, lists, dense, chunks);
    std::printf("sweep: %zu plans (%zu item form, %zu lists form, %zu dense; %zu of a last U chunk)\n", plans, items, lists, dense, chunks);
}

}  // namespace

int main()
{
    check_dims();
    check_plan();
    check_forms();
    check_shards();
    check_axis_path();
    check_perm();
    check_sweep();
    if (g_fail) { std::printf("%d checks failed\n", g_fail); return 1; }
    std::printf("OK solve_rule\n");
    return 0;
}
