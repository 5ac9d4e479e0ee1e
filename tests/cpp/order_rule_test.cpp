// The host arithmetic of the device order (emba_amd/csrc/order_rule.h) on a CPU: the cutting of occupied tiles into chunks over a few hundred deterministic
// start tables, and the order rule on cases computed by hand from the numbers in its comments.  Prints "OK ..." and returns 0, or names what failed.
#include "../../emba_amd/csrc/order_rule.h"

#include <cstdio>
#include <cstdlib>
#include <map>

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

struct Lcg {
    uint64_t s;
    uint32_t next() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(s >> 33); }
    uint32_t below(uint32_t n) { return next() % n; }
};

#ifndef TILE_ROUND
#define TILE_ROUND 504      // kWarpNew x kTileWaves of kernels.h (tests/test_cpp_host.py passes the current value)
#endif
constexpr size_t kRound = TILE_ROUND;
// the four 1152-pixel shapes of kernels.h, as the geometry cases below assume them; the chunk tables only need some shapes
constexpr TileShape kShapes[4] = {{48, 24, 32, 8, 16, 4}, {72, 16, 48, 4, 24, 4}, {96, 12, 64, 4, 32, 2}, {36, 32, 24, 8, 12, 8}};
size_t ceil_div(size_t a, size_t b) { return (a + b - 1) / b; }

// the chunk size as include/emba_hip.h and prepare_order's comments state it, restated: ~8 rounds of the chip's 2 n_cu workgroup slots, at least 8 groups per
// wave (5 from 8 M entries), at most 16; option tile_chunk overrides
size_t chunk_spec(size_t nd, int n_cu, int opt)
{
    if (opt > 0) return (size_t)opt;
    const size_t lo = kRound * (nd < 8000000 ? 8 : 5), hi = kRound * 16;
    return std::min(std::max(ceil_div(nd, (size_t)n_cu * 2 * 8), lo), hi);
}

struct Seen { bool nch1 = false, nch2 = false, nch_more = false, skipped_empty = false, ties = false; size_t tables = 0, tiles = 0, chunks = 0; };

// one start table: `fill` percent of the tiles occupied, sizes drawn so that whole multiples of the chunk, one entry more and one entry less all occur
void check_table(Lcg& rng, int shape, bool fine, int reserve, int fill, uint32_t max_cnt, int n_cu, int opt_chunk, Seen* seen)
{
    const BinGeom g = tile_geometry(384, 96, kShapes[shape], fine, reserve);
    const size_t nbins = (size_t)g.nbx * g.nby + 1;
    std::vector<uint32_t> start(nbins + 1, 0xFFFFFFFFu), cnt(nbins, 0);
    for (size_t b = 0; b < nbins; ++b) {
        if ((int)rng.below(100) >= fill) continue;
        switch (rng.below(4)) {
        case 0: cnt[b] = 1 + rng.below(max_cnt); break;
        case 1: cnt[b] = (uint32_t)kRound * (1 + rng.below(max_cnt / (uint32_t)kRound + 1)); break;
        case 2: cnt[b] = (uint32_t)kRound * (1 + rng.below(max_cnt / (uint32_t)kRound + 1)) + 1; break;
        default: cnt[b] = 1 + rng.below(40); break;
        }
    }
    size_t nd = 0;
    for (size_t b = 0; b < nbins; ++b) if (cnt[b]) { start[b] = (uint32_t)nd; nd += cnt[b]; }
    const size_t chunk = chunk_spec(nd, n_cu, opt_chunk);
    CHECK(chunk_target(kRound, nd, n_cu, opt_chunk) == chunk, "nd %zu n_cu %d opt %d: %zu vs %zu", nd, n_cu, opt_chunk, chunk_target(kRound, nd, n_cu, opt_chunk), chunk);

    const std::vector<ChunkDesc> in_bin_order = cut_chunks(kRound, start.data(), nbins, nd, g, n_cu, opt_chunk, false);
    const std::vector<ChunkDesc> lpt = cut_chunks(kRound, start.data(), nbins, nd, g, n_cu, opt_chunk, true);

    // bin order: the pieces of a tile follow each other, tiles in the order of their entries
    size_t k = 0, expect_chunks = 0;
    for (size_t b = 0; b < nbins; ++b) {
        if (!cnt[b]) continue;
        const size_t b0 = start[b], b1 = b0 + cnt[b];
        const size_t nch = ceil_div(cnt[b], chunk), per = ceil_div(ceil_div(cnt[b], nch), kRound) * kRound;      // whole rounds per piece
        const size_t pieces = ceil_div(cnt[b], per);      // (== nch unless rounding up to whole rounds left the trailing pieces empty: those are skipped)
        seen->nch1 |= nch == 1; seen->nch2 |= nch == 2; seen->nch_more |= nch > 2; seen->skipped_empty |= pieces < nch;
        expect_chunks += pieces; ++seen->tiles;
        size_t at = b0, n_here = 0;
        while (k < in_bin_order.size() && in_bin_order[k].begin < b1) {
            const ChunkDesc& d = in_bin_order[k];
            CHECK(d.begin == at, "tile %zu: piece %zu begins at %u, the tile is covered up to %zu", b, n_here, d.begin, at);
            CHECK(d.end > d.begin, "tile %zu: empty piece at %u", b, d.begin);
            CHECK(d.end <= b1, "tile %zu [%zu, %zu): piece ends at %u", b, b0, b1, d.end);
            if (d.end < b1) CHECK((d.end - d.begin) % kRound == 0, "tile %zu: inner piece of %u entries is not whole rounds", b, d.end - d.begin);
            CHECK(d.x0 == (int)(b % (size_t)g.nbx) * g.bw - g.r && d.y0 == (int)(b / (size_t)g.nbx) * g.bh - g.r, "tile %zu: origin (%d, %d)", b, d.x0, d.y0);
            at = d.end; ++n_here; ++k;
            if (d.end <= d.begin) break;
        }
        CHECK(at == b1, "tile %zu [%zu, %zu): covered up to %zu only (nch %zu)", b, b0, b1, at, nch);
        CHECK(n_here == pieces, "tile %zu: %zu pieces, expected %zu (cnt %u chunk %zu)", b, n_here, pieces, cnt[b], chunk);
    }
    CHECK(k == in_bin_order.size() && in_bin_order.size() == expect_chunks, "%zu chunks, %zu walked, %zu expected", in_bin_order.size(), k, expect_chunks);

    // longest first: the same pieces, lengths non-increasing, equal lengths in their bin order (stable)
    CHECK(lpt.size() == in_bin_order.size(), "longest-first has %zu chunks, bin order %zu", lpt.size(), in_bin_order.size());
    std::map<uint32_t, const ChunkDesc*> by_begin;
    for (const ChunkDesc& d : in_bin_order) by_begin[d.begin] = &d;
    for (size_t i = 0; i < lpt.size(); ++i) {
        const ChunkDesc& d = lpt[i];
        auto it = by_begin.find(d.begin);
        CHECK(it != by_begin.end() && it->second->end == d.end && it->second->x0 == d.x0 && it->second->y0 == d.y0, "longest-first chunk %zu is not one of the bin order's", i);
        if (it != by_begin.end()) by_begin.erase(it);      // (each once)
        if (!i) continue;
        const uint32_t len = d.end - d.begin, prev = lpt[i - 1].end - lpt[i - 1].begin;
        CHECK(len <= prev, "longest-first: chunk %zu has %u entries after one of %u", i, len, prev);
        if (len == prev) { seen->ties = true; CHECK(d.begin > lpt[i - 1].begin, "longest-first: equal chunks %zu and %zu swapped", i - 1, i); }
    }
    ++seen->tables; seen->chunks += in_bin_order.size();
}

void check_chunks()
{
    Lcg rng{20240611};
    Seen seen;
    const int opts[3] = {0, 100, 504};
    const int fills[3] = {4, 40, 95};                 // sparse ... dense occupancy
    const uint32_t sizes[3] = {900, 6000, 30000};     // the default chunk is 4032 entries at these totals: nch 1 ... 8
    for (int rep = 0; rep < 4; ++rep)
        for (int oi = 0; oi < 3; ++oi)
            for (int fi = 0; fi < 3; ++fi)
                for (int si = 0; si < 3; ++si)
                    for (int shape = 0; shape < 4; ++shape)
                        check_table(rng, shape, (rep & 1) != 0, rep == 3 ? 5 : 2, fills[fi], sizes[si], rep == 2 ? 64 : 256, opts[oi], &seen);
    // a window large enough for the first rule (8 rounds of the chip) and the cap of 16 groups per wave to decide
    check_table(rng, 3, false, 2, 95, 400000, 256, 0, &seen);
    CHECK(seen.tables >= 300, "%zu tables", seen.tables);
    CHECK(seen.nch1 && seen.nch2 && seen.nch_more && seen.skipped_empty && seen.ties, "coverage of the cases: nch 1 %d, 2 %d, > 2 %d, skipped empty pieces %d, ties %d",
          seen.nch1, seen.nch2, seen.nch_more, seen.skipped_empty, seen.ties);
    std::printf("chunks: %zu tables, %zu occupied tiles, %zu chunks\n", seen.tables, seen.tiles, seen.chunks);
}

void check_rule()
{
    // (the numbers below are computed for a round of 63 x 8 = 504 entries)
    // the chunk size: 3 M entries on 256 CUs — 733 per slot-round is below 8 groups per wave (4032); 10 M — 2442 below 5 groups (2520); 100 M — capped at 16 (8064)
    CHECK(chunk_target(504, 3000000, 256, 0) == 4032 && chunk_target(504, 10000000, 256, 0) == 2520 && chunk_target(504, 100000000, 256, 0) == 8064 && chunk_target(504, 100000000, 256, 100) == 100, "chunk_target");

    // geometry: reserve 5 leaves a 2-px pitch in y on the 96 x 12 tile; the fine grid of the 48 x 24 tile is 16 x 4
    BinGeom g = tile_geometry(1024, 512, kShapes[2], false, 5);
    CHECK(g.tw == 96 && g.th == 12 && g.bw == 64 && g.bh == 2 && g.nbx == 16 && g.nby == 256 && g.r == 5, "geometry 96 x 12, reserve 5");
    g = tile_geometry(1000, 500, kShapes[0], true, 2);
    CHECK(g.bw == 16 && g.bh == 4 && g.nbx == 63 && g.nby == 125 && g.W == 1000 && g.H == 500, "geometry 48 x 24 fine");
    CHECK(clamp_tile_reserve(-3) == 0 && clamp_tile_reserve(9) == 5 && clamp_tile_reserve(2) == 2, "reserve clamp");

    // cost in entries: 3 M events + 300 k lead-ins on 1000 tiles = 3.3 M + 256 x max(1000, 3.3 M / 4032 = 818.5)
    CHECK(candidate_cost(504, 3000000, 300000, 1000) == 3556000.0, "%f", candidate_cost(504, 3000000, 300000, 1000));
    CHECK(candidate_cost(504, 3000000, 300000, 500) == 3300000.0 + 256.0 * (3300000.0 / 4032.0), "few tiles: the chunk count comes from the entries");
    // a later candidate must beat the first by 2 %: 3 526 000 is 0.8 % cheaper — no; 3 456 000 < 0.98 x 3 556 000 = 3 484 880 — yes
    TileChoice t{504};
    CHECK(t.shape < 0 && !t.wants_fine(1, 1000), "nothing offered");
    t.offer(3, 3000000, 300000, 1000);
    t.offer(0, 3000000, 270000, 1000);
    CHECK(t.shape == 3 && t.cost == 3556000.0, "0.8 %% cheaper must not win");
    t.offer(1, 3000000, 200000, 1000);
    CHECK(t.shape == 1 && !t.fine && t.cost == 3456000.0 && t.breaks == 200000 && t.used == 1000, "2.8 %% cheaper wins");
    // the fine grid: from 2 x 4032 events per occupied tile, below 16 M events; option tile_fine 0 / 1 forces
    CHECK(!t.wants_fine(-1, 3000000), "3000 events per tile");
    t.used = 300;
    CHECK(t.wants_fine(-1, 3000000) && !t.wants_fine(0, 3000000) && !t.wants_fine(-1, 16000000) && t.wants_fine(1, 16000000), "fine grid clause");
    t.offer_fine(-1, 3000000, 200000, 2000);      // dearer (more chunks): refused
    CHECK(!t.fine && t.used == 300, "a dearer fine grid");
    t.offer_fine(1, 3000000, 200000, 2000);       // ... unless forced
    CHECK(t.fine && t.used == 2000, "forced fine grid");

    // the order: 83 f > 41 + 31 lead
    CHECK(order_hopeless(0, 0.49) && !order_hopeless(0, 0.5) && !order_hopeless(2, 0.0), "83 f <= 41 under order = 0 is pixel order without a search");
    CHECK(!tile_order_wins(0, 5000000, 1650000, 50.0, 0.49, 0.0), "f = 0.49");
    CHECK(tile_order_wins(0, 5000000, 1650000, 50.0, 0.5, 0.0) && !tile_order_wins(0, 5000000, 1650000, 50.0, 0.5, 0.35), "f = 0.5: 41.5 > 41, but not > 51.85");
    CHECK(!tile_order_wins(0, 10000000, 1650000, 50.0, 0.34, 0.1) && order_hopeless(0, 0.34), "the 34 %%-inlier stream stays in pixel order");
    CHECK(tile_order_wins(0, 3000000, 1650000, 8.0, 0.9, 0.2) && !tile_order_wins(0, 3000000, 1650000, 7.9, 0.9, 0.2), "at least 8 events per panorama pixel");
    CHECK(!tile_order_wins(0, 1649999, 1650000, 50.0, 1.0, 0.0) && tile_order_wins(0, 1650000, 1650000, 50.0, 1.0, 0.0), "tile_min_events");
    CHECK(tile_order_wins(2, 10, 1650000, 0.0, 0.0, 1.0), "order = 2 forces the tile order");
    CHECK(order_considers_tiles(2, 10, 1650000) && !order_considers_tiles(1, 100000000, 0) && !order_considers_tiles(0, 1649999, 1650000) && order_considers_tiles(0, 1650000, 1650000), "who searches");
    // what the decision sees: 3 M events on 1000 occupied 32 x 8 cells = 11.7 per pixel; 300 k lead-ins = 10 %
    g = tile_geometry(1024, 512, kShapes[0], false, 2);
    CHECK(events_per_pano_px(3000000, 1000, g) == 3000000.0 / 256000.0 && events_per_pano_px(5, 0, g) == 0.0, "events per pixel");
    CHECK(lead_in_fraction(3000000, 300000) == 0.1 && lead_in_fraction(0, 0) == 1.0, "lead-in fraction");
}

}  // namespace

int main()
{
    check_chunks();
    check_rule();
    if (g_fail) { std::printf("%d checks failed\n", g_fail); return 1; }
    std::printf("OK order_rule\n");
    return 0;
}
