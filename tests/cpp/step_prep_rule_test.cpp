// tests/cpp/step_prep_rule_test.cpp — the rules of emba_amd/csrc/step_rule.h that decide when the texels are packed again and when the launch in front of
// the warp kernel is dropped (plain C++17, no HIP), on hand-computed cases.  Built and run by tests/test_step_prep_rule_cpu.py.
#include <cstdio>

#include "../../emba_amd/csrc/step_rule.h"

using namespace emba;

static int g_fail = 0;
#define CHECK(x) do { if (!(x)) { std::printf("FAIL %s:%d  %s\n", __FILE__, __LINE__, #x); ++g_fail; } } while (0)

int main()
{
    // ---- rect_contained: boxes {xmin, ymin, xmax, ymax}, inclusive
    const int E0 = 0x7FFFFFFF, E1 = -1;      // the empty box as the context initialises it
    CHECK(rect_contained(E0, E0, E1, E1, E0, E0, E1, E1, 12));       // nothing touched: nothing to pack, whatever is packed
    CHECK(rect_contained(E0, E0, E1, E1, 10, 10, 20, 20, 12));
    CHECK(!rect_contained(10, 10, 20, 20, E0, E0, E1, E1, 12));      // a first footprint: nothing is packed yet
    CHECK(rect_contained(10, 10, 20, 20, 10, 10, 20, 20, 0));        // the same box, no slack
    CHECK(rect_contained(10, 10, 20, 20, 22, 22, 30, 30, 12));       // exactly the slack on the low side ...
    CHECK(!rect_contained(9, 10, 20, 20, 22, 22, 30, 30, 12));       // ... one pixel more in x
    CHECK(!rect_contained(10, 9, 20, 20, 22, 22, 30, 30, 12));       // ... in y
    CHECK(rect_contained(30, 30, 42, 42, 22, 22, 30, 30, 12));       // exactly the slack on the high side
    CHECK(!rect_contained(30, 30, 43, 42, 22, 22, 30, 30, 12));
    CHECK(!rect_contained(30, 30, 42, 43, 22, 22, 30, 30, 12));
    CHECK(rect_contained(0, 0, 5, 5, 3, 3, 4, 4, 12));               // the grown box may reach past the panorama's edge: only the new box is real
    CHECK(!rect_contained(100, 100, 101, 101, 10, 10, 20, 20, 12));  // disjoint
    for (int s = 0; s <= kRectMargin; ++s)                            // a larger slack never turns fresh into stale
        for (int d = -30; d <= 30; ++d)
            if (rect_contained(50 + d, 50, 60 + d, 60, 50, 50, 60, 60, s)) CHECK(rect_contained(50 + d, 50, 60 + d, 60, 50, 50, 60, 60, s + 1));
    // whatever is fresh has its texels: the slack never exceeds the margin the pack grows its box by
    CHECK(kRectFreshSlack >= 0 && kRectFreshSlack <= kRectMargin);

    // ---- texels_stale(map_owned, map_version, packed_version, verdict_seq, step_seq)
    CHECK(texels_stale(true, 1, 0, 0, 0));        // a new context: never packed, no step yet
    CHECK(texels_stale(true, 1, 1, 0, 0));        // packed, but no step has reduced a box yet
    CHECK(!texels_stale(true, 1, 1, 7, 7));       // same map, step 7's box inside the packed one
    CHECK(texels_stale(true, 2, 1, 7, 7));        // the map changed since the pack
    CHECK(texels_stale(true, 1, 1, 0, 7));        // step 7's box left the packed one
    CHECK(texels_stale(true, 1, 1, 6, 7));        // step 7's verdict has not arrived: step 6's says nothing about it
    CHECK(texels_stale(false, 1, 1, 7, 7));       // a bound map is the caller's memory
    CHECK(texels_stale(true, 0u, 0xFFFFFFFFu, 7, 7));   // versions only compare equal or not: a wrapped counter is still another map

    // ---- texel_blocks(hessian_src, stale)
    CHECK(texel_blocks(3, true) == 1024 && texel_blocks(3, false) == 0);
    CHECK(texel_blocks(0, true) == 0 && texel_blocks(1, true) == 0 && texel_blocks(0, false) == 0 && texel_blocks(1, false) == 0);

    // ---- prep_inside_warp(step_prep, tile_order, segpose, K, inline_knots, n_sorted, n_prep_blk, n_tex_blk, hessian_src)
    const int IK = 104;
    CHECK(prep_inside_warp(1, false, true, 21, IK, 1000000, 0, 0, 3));     // the steady step of the benchmark
    CHECK(prep_inside_warp(1, false, true, 2, IK, 1, 0, 0, 0));            // one record, one entry, the stencil
    CHECK(prep_inside_warp(1, false, true, IK, IK, 1000, 0, 0, 3));        // the last K whose poses travel in the arguments
    CHECK(!prep_inside_warp(1, false, true, IK + 1, IK, 1000, 0, 0, 3));   // the first that is staged
    CHECK(!prep_inside_warp(0, false, true, 21, IK, 1000000, 0, 0, 3));    // option step_prep = 0
    CHECK(!prep_inside_warp(1, true, true, 21, IK, 1000000, 0, 0, 3));     // tile order
    CHECK(!prep_inside_warp(1, false, false, 21, IK, 1000000, 0, 0, 3));   // the per-batch pose table (segpose = 1)
    CHECK(!prep_inside_warp(1, false, true, 21, IK, 0, 0, 0, 3));          // an empty window launches no warp kernel
    CHECK(!prep_inside_warp(1, false, true, 21, IK, 1000000, 2048, 0, 3)); // unclean lines
    CHECK(!prep_inside_warp(1, false, true, 21, IK, 1000000, 0, 1024, 3)); // stale texels
    CHECK(!prep_inside_warp(1, false, true, 21, IK, 1000000, 0, 0, 1));    // the full pack is a launch of its own behind the first one
    // with the rules it is fed from: an empty window on clean lines has no prep blocks either, and still keeps the launch
    CHECK(prep_blocks(true, 0, 2097152) == 2048 && !prep_inside_warp(1, false, true, 21, IK, 0, prep_blocks(true, 0, 2097152), 0, 3));
    CHECK(prep_inside_warp(1, false, segpose_in_pixel_order(false, 0), 21, IK, 1000000, prep_blocks(true, 1000000, 2097152), texel_blocks(hessian_source(0, 1000000, 2097152), false),
                           hessian_source(0, 1000000, 2097152)));

    if (g_fail) { std::printf("%d checks failed\n", g_fail); return 1; }
    std::printf("OK step_prep_rule\n");
    return 0;
}
