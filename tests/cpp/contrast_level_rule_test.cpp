// tests/cpp/contrast_level_rule_test.cpp — the level additions of emba_amd/csrc/contrast_rule.h on a CPU (plain C++17, no HIP;
// tests/test_contrast_pyramid_cpu.py builds and runs it, once plain and once with -fsanitize=address,undefined): the grid of a level, the levels that are
// refused, the scaled vote against the unscaled one (level 0: the same bits; level l: contrast_vote of the scaled pm on the level's grid), the plan that
// names the vote kernel at its boundary, and the shares of the persistent workgroups (a partition of the events, whatever their number).
// Prints the votes of a few pm at a few levels ("LVOTE pm_x pm_y W H level | four cells | four weights | dwx | dwy"): the Python side compares them with
// io.contrast_votes on io.contrast_level.
#include "../../emba_amd/csrc/contrast_rule.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>

using namespace emba;

static int g_fail = 0;
#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #cond); ++g_fail; } \
    } while (0)

static void test_grids_and_refusals()
{
    for (int l = 0; l <= kContrastMaxLevel; ++l) {
        CHECK(contrast_level_ok(1024, 512, l) == ContrastLevelStatus::ok);
        const ContrastLevel g = contrast_level_grid(1024, 512, l);
        CHECK(g.W == 1024 >> l && g.H == 512 >> l && g.scale * (double)(1 << l) == 1.0);
    }
    const ContrastLevel g0 = contrast_level_grid(512, 256, 0);
    CHECK(g0.W == 512 && g0.H == 256 && g0.scale == 1.0);
    CHECK(contrast_level_ok(512, 256, -1) == ContrastLevelStatus::bad_level);
    CHECK(contrast_level_ok(1 << 20, 1 << 19, kContrastMaxLevel + 1) == ContrastLevelStatus::bad_level);
    CHECK(contrast_level_ok(512, 256, 8) == ContrastLevelStatus::too_few_rows);       // one row left
    CHECK(contrast_level_ok(512, 256, 7) == ContrastLevelStatus::ok);                 // two rows
    CHECK(contrast_level_ok(514, 256, 2) == ContrastLevelStatus::not_divisible);      // the width
    CHECK(contrast_level_ok(512, 258, 2) == ContrastLevelStatus::not_divisible);      // the height
    CHECK(contrast_level_ok(514, 258, 1) == ContrastLevelStatus::ok);
    CHECK(contrast_level_ok(24, 12, 2) == ContrastLevelStatus::ok && contrast_level_ok(24, 12, 3) == ContrastLevelStatus::not_divisible);
    CHECK(contrast_level_ok(16, 4, 2) == ContrastLevelStatus::too_few_rows);          // divisible, one row
}

static bool same(const ContrastVotes& a, const ContrastVotes& b) { return !std::memcmp(&a, &b, sizeof a); }

static void print_vote(double x, double y, int W, int H, int level)
{
    const ContrastVotes v = contrast_vote_level(x, y, contrast_level_grid(W, H, level));
    std::printf("LVOTE %.17g %.17g %d %d %d |", x, y, W, H, level);
    for (int k = 0; k < 4; ++k) std::printf(" %d", v.cell[k]);
    const double* rows[3] = {v.w, v.dwx, v.dwy};
    for (const double* r : rows) {
        std::printf(" |");
        for (int k = 0; k < 4; ++k) std::printf(" %.17g", r[k]);
    }
    std::printf("\n");
}

static void test_scaled_votes()
{
    const int W = 512, H = 256;
    for (int i = 0; i < 4000; ++i) {
        const double x = -3.0 + (W + 6.0) * ((i * 7919) % 4000) / 4000.0 + 1e-3, y = -3.0 + (H + 6.0) * ((i * 104729) % 4000) / 4000.0 + 2e-3;
        // level 0 is the rule itself, bit for bit
        CHECK(same(contrast_vote_level(x, y, contrast_level_grid(W, H, 0)), contrast_vote(x, y, W, H)));
        for (int l = 1; l <= 4; ++l) {
            const ContrastLevel g = contrast_level_grid(W, H, l);
            const ContrastVotes v = contrast_vote_level(x, y, g);
            CHECK(same(v, contrast_vote(x / (1 << l), y / (1 << l), W >> l, H >> l)));      // (a division by a power of two is the same exact scaling)
            for (int k = 0; k < 4; ++k) CHECK(v.cell[k] >= -1 && v.cell[k] < g.W * g.H && v.w[k] >= 0 && v.w[k] <= 1);
            CHECK(std::fabs(((v.w[0] + v.w[1]) + (v.w[2] + v.w[3])) - 1.0) < 1e-15);
        }
    }
    // level 3 of 512 x 256: 64 x 32 cells of 8 px.  pm = (508, 100) -> pm_l = (63.5, 12.5): columns 63 and 0 (the wrap modulo W_l), rows 12 and 13
    ContrastVotes v = contrast_vote_level(508.0, 100.0, contrast_level_grid(W, H, 3));
    CHECK(v.cell[0] == 12 * 64 + 63 && v.cell[1] == 12 * 64 + 0 && v.cell[2] == 13 * 64 + 63 && v.cell[3] == 13 * 64 + 0);
    CHECK(v.w[0] == 0.25 && v.w[1] == 0.25 && v.w[2] == 0.25 && v.w[3] == 0.25 && v.dwx[1] == 0.5 && v.dwy[2] == 0.5);
    // the last row of the level: pm_y = 252 -> 31.5: row 32 = H_l has no cell, its weights stay for the caller to count
    v = contrast_vote_level(16.0, 252.0, contrast_level_grid(W, H, 3));
    CHECK(v.cell[0] == 31 * 64 + 2 && v.cell[2] == -1 && v.cell[3] == -1 && v.w[0] == 0.5 && v.w[2] == 0.5 && v.w[1] == 0 && v.w[3] == 0);
    // rows above the first
    v = contrast_vote_level(16.0, -4.0, contrast_level_grid(W, H, 3));
    CHECK(v.cell[0] == -1 && v.cell[1] == -1 && v.cell[2] == 2 && v.w[0] == 0.5 && v.w[2] == 0.5);
    // not finite: nowhere
    const double bad[3] = {std::numeric_limits<double>::quiet_NaN(), std::numeric_limits<double>::infinity(), -std::numeric_limits<double>::infinity()};
    for (double b : bad) {
        v = contrast_vote_level(b, 5.0, contrast_level_grid(W, H, 2));
        for (int k = 0; k < 4; ++k) CHECK(v.cell[k] == -1 && v.w[k] == 0 && v.dwx[k] == 0 && v.dwy[k] == 0);
    }
    print_vote(508.0, 100.0, W, H, 3);
    print_vote(16.0, 252.0, W, H, 3);
    print_vote(-0.75, 17.3, W, H, 1);
    print_vote(511.99, 255.99, W, H, 4);
    print_vote(123.456, 78.9, W, H, 2);
    print_vote(123.456, 78.9, W, H, 0);
}

static void test_vote_plan()
{
    CHECK(kContrastLdsCells * (int)sizeof(double) <= 64 * 1024);      // what a workgroup may declare as a static array
    // exactly the budget, one cell more (the boundary), and the shapes DESIGN.md §14 names
    CHECK(contrast_vote_plan(128, 64, -1) == ContrastVotePath::lds && 128 * 64 == kContrastLdsCells);
    CHECK(contrast_vote_plan(kContrastLdsCells, 1, -1) == ContrastVotePath::lds);
    CHECK(contrast_vote_plan(kContrastLdsCells + 1, 1, -1) == ContrastVotePath::hbm);
    CHECK(contrast_vote_plan(129, 64, -1) == ContrastVotePath::hbm && contrast_vote_plan(128, 65, -1) == ContrastVotePath::hbm);
    CHECK(contrast_vote_plan(2048 >> 4, 1024 >> 4, -1) == ContrastVotePath::lds && contrast_vote_plan(2048 >> 3, 1024 >> 3, -1) == ContrastVotePath::hbm);
    CHECK(contrast_vote_plan(1024 >> 3, 512 >> 3, -1) == ContrastVotePath::lds && contrast_vote_plan(1024 >> 2, 512 >> 2, -1) == ContrastVotePath::hbm);
    CHECK(contrast_vote_plan(1 << 20, 1 << 19, -1) == ContrastVotePath::hbm);      // (no 32-bit overflow of the product)
    // forced: HBM always; LDS only where the image fits
    CHECK(contrast_vote_plan(64, 32, 0) == ContrastVotePath::hbm && contrast_vote_plan(64, 32, 1) == ContrastVotePath::lds);
    CHECK(contrast_vote_plan(256, 128, 1) == ContrastVotePath::hbm && contrast_vote_plan(kContrastLdsCells + 1, 1, 1) == ContrastVotePath::hbm);
    CHECK(contrast_lds_grid(256) == 256 && contrast_lds_grid(0) == 1 && contrast_lds_grid(-3) == 1);
}

static void test_shares()
{
    const long sizes[] = {0, 1, 100, 1023, 1024, 1025, 2900, 262144, 262145, 999900, 1000000, 50000000};
    const int grids[] = {1, 2, 7, 256, 304};
    for (long nn : sizes)
        for (int blocks : grids) {
            long at = 0, busy = 0;
            for (int b = 0; b < blocks; ++b) {
                const ContrastShare s = contrast_share(nn, blocks, b);
                CHECK(s.beg == at && s.end >= s.beg && s.end <= nn);      // contiguous, in order, inside the range
                if (s.end > s.beg) ++busy;
                at = s.end;
            }
            CHECK(at == nn);                                              // every event once
            CHECK(busy <= (nn + kContrastLdsThreads - 1) / kContrastLdsThreads);      // no workgroup is started for less than one round of its lanes
        }
    // 100 events on 256 workgroups: the first takes them all, the others nothing
    CHECK(contrast_share(100, 256, 0).beg == 0 && contrast_share(100, 256, 0).end == 100);
    for (int b = 1; b < 256; ++b) CHECK(contrast_share(100, 256, b).beg == 100 && contrast_share(100, 256, b).end == 100);
    // a share that is no multiple of anything
    CHECK(contrast_share(1000000, 256, 0).end == 3907 && contrast_share(1000000, 256, 255).end == 1000000);
}

int main()
{
    test_grids_and_refusals();
    test_scaled_votes();
    test_vote_plan();
    test_shares();
    if (g_fail) { std::printf("%d checks failed\n", g_fail); return 1; }
    std::printf("OK contrast_level_rule\n");
    return 0;
}
