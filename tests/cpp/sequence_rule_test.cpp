// The host arithmetic of the resident event sequence (emba_amd/csrc/sequence_rule.h) on a CPU: the event window behind the probe kernel against a loop
// restatement of getEventSubset (emba.cpp:473-510) on a few thousand random sequences and on hand cases, the ranks' batches (printed as "RANK ..." lines, which
// tests/test_cpp_host.py compares with emba_amd.sharded.window_shard_ranges), the layouts of a halo and of an upload chunk, the shard check, the hot-pixel
// threshold against values computed in Python in the operation order of emba_amd.io.filter_events, and the plan of a filter call against the expressions
// emba_seq_filter held before they moved there.
// Prints "OK ..." and returns 0, or names what failed.
#include "../../emba_amd/csrc/sequence_rule.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
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

// sequence_kernels.h: kSeqProbe (tests/test_cpp_host.py passes the current value)
#ifndef SEQ_PROBE
#define SEQ_PROBE 100
#endif
constexpr size_t kProbe = SEQ_PROBE;

// ---- seq_window ----
// getEventSubset as written: both cursors move `probe` events at a time, the tail from the head; `end -= 100` at the tail's FIRST probe leaves a range
// that is reversed or has underflowed (stops_at_first_probe); a head behind the last event leaves end = n < beg (begins_behind_last).
SeqWindow event_subset(const std::vector<int64_t>& t, int64_t t_beg, int64_t t_end)
{
    const size_t n = t.size();
    const int64_t a = t_beg + 1000000, b = t_end - 1000000;
    size_t beg, end;
    for (beg = 0; beg < n; beg += kProbe)
        if (t[beg] > a) break;
    for (end = beg; end < n; end += kProbe)
        if (t[end] > b) {
            if (end == beg) return {SeqWindowStatus::stops_at_first_probe, beg, beg};
            end -= kProbe;
            break;
        }
    if (end > n) end = n;
    if (end < beg) return {SeqWindowStatus::begins_behind_last, beg, end};
    return {SeqWindowStatus::ok, beg, end};
}

// what emba_seq_window_kernel leaves: the smallest j with t[probe j] > cursor over the probes probe j < n
uint32_t first_probe_past(const std::vector<int64_t>& t, int64_t cursor)
{
    for (size_t j = 0; kProbe * j < t.size(); ++j)
        if (t[kProbe * j] > cursor) return (uint32_t)j;
    return kNoProbe;
}

void check_seq_window_sweep()
{
    std::mt19937_64 rng(20240607);
    const size_t lengths[] = {0, 1, 2, 99, 100, 101, 199, 200, 201, 250, 299, 300, 301, 999, 1000, 1001, 1099, 1100, 1101, 2500, 3000};
    const int64_t ms = 1000000, steps[] = {1, 1000, 20000, 300000, 5 * ms};
    int n_case = 0, n_ok = 0, n_stop = 0, n_behind = 0, n_reversed = 0, n_off = 0;
    for (int rep = 0; rep < 12; ++rep)
        for (size_t n : lengths) {
            // sorted timestamps, a few microseconds to a few milliseconds apart, with ties
            std::vector<int64_t> t(n);
            const int64_t step = steps[rng() % 5];
            int64_t now = (int64_t)(rng() % 1000) * ms;
            for (size_t i = 0; i < n; ++i) { if (rng() % 4) now += (int64_t)(rng() % (2 * step + 1)); t[i] = now; }
            const int64_t lo = (n ? t.front() : 0) - 20 * ms, hi = (n ? t.back() : 0) + 20 * ms;
            for (int k = 0; k < 16; ++k) {
                int64_t tb = lo + (int64_t)(rng() % (uint64_t)(hi - lo + 1)), te = lo + (int64_t)(rng() % (uint64_t)(hi - lo + 1));
                if (k % 4 && te < tb) std::swap(tb, te);          // (every fourth pair stays as drawn: t_end < t_beg included)
                if (k == 14) { tb = lo - 100 * ms; te = hi + 100 * ms; }      // both bounds outside the data ...
                if (k == 15) { tb = hi + 50 * ms; te = hi + 100 * ms; }       // ... and behind it
                const SeqCursors cur = seq_window_cursors(tb, te);
                const SeqWindow got = seq_window(n, first_probe_past(t, cur.a), first_probe_past(t, cur.b), kProbe), want = event_subset(t, tb, te);
                ++n_case;
                n_reversed += te < tb; n_off += tb < (n ? t.front() : 0) || te > (n ? t.back() : 0);
                n_ok += want.status == SeqWindowStatus::ok; n_stop += want.status == SeqWindowStatus::stops_at_first_probe; n_behind += want.status == SeqWindowStatus::begins_behind_last;
                CHECK(got.status == want.status && got.beg == want.beg && (got.status != SeqWindowStatus::ok || got.end == want.end),
                      "n = %zu, window (%lld, %lld): status %d [%zu, %zu), the loops give %d [%zu, %zu)", n, (long long)tb, (long long)te, (int)got.status, got.beg, got.end,
                      (int)want.status, want.beg, want.end);
                if (got.status == SeqWindowStatus::ok) CHECK(got.beg <= got.end && got.end <= n && got.beg % kProbe == 0, "n = %zu: [%zu, %zu) is no range on the probe grid", n, got.beg, got.end);
            }
        }
    CHECK(n_case >= 4000 && n_ok > 500 && n_stop > 100 && n_behind > 100 && n_reversed > 100 && n_off > 500, "the sweep is meant to meet every case: %d cases, %d ok, %d stop, %d behind, %d reversed, %d outside",
          n_case, n_ok, n_stop, n_behind, n_reversed, n_off);
    std::printf("seq_window: %d cases (%d windows, %d stop at the first probe, %d begin behind the last event)\n", n_case, n_ok, n_stop, n_behind);
}

void check_seq_window_by_hand()
{
    const SeqCursors cur = seq_window_cursors(5000000, 9000000);
    CHECK(cur.a == 6000000 && cur.b == 8000000, "t_epsilon is 1 ms");
    if (kProbe != 100) return;      // (the answers below are written for probes every 100 events)
    auto is = [](const SeqWindow& w, SeqWindowStatus s, size_t beg, size_t end) { return w.status == s && w.beg == beg && (s != SeqWindowStatus::ok || w.end == end); };
    CHECK(is(seq_window(0, kNoProbe, kNoProbe, 100), SeqWindowStatus::ok, 0, 0), "no events: the empty window");
    CHECK(seq_window(250, kNoProbe, kNoProbe, 100).status == SeqWindowStatus::begins_behind_last, "250 events, no probe past a: begins behind the last event");
    CHECK(seq_window(250, kNoProbe, 1, 100).status == SeqWindowStatus::begins_behind_last, "... whatever the tail probe says");
    CHECK(is(seq_window(250, 1, kNoProbe, 100), SeqWindowStatus::ok, 100, 250), "250 events, probes (1, none): [100, 250)");
    CHECK(is(seq_window(250, 1, 2, 100), SeqWindowStatus::ok, 100, 100), "250 events, probes (1, 2): [100, 100)");
    CHECK(is(seq_window(250, 1, 1, 100), SeqWindowStatus::stops_at_first_probe, 100, 0), "250 events, probes (1, 1): the tail search stops at its first probe");
    CHECK(is(seq_window(250, 1, 0, 100), SeqWindowStatus::stops_at_first_probe, 100, 0), "250 events, probes (1, 0): clamped to the head, the tail search stops at its first probe");
    CHECK(is(seq_window(250, 0, 2, 100), SeqWindowStatus::ok, 0, 100), "250 events, probes (0, 2): [0, 100)");
    CHECK(is(seq_window(300, kNoProbe, kNoProbe, 100), SeqWindowStatus::ok, 300, 300), "300 events, no probe past a: the empty window at the end");
}

// ---- rank_batches ----
void check_rank_batches()
{
    // WINDOWS of tests/test_sequence_sharded_cpu.py (test_cpp_host.py checks that these are the same windows)
    const size_t windows[][2] = {{0, 20000}, {137, 30187}, {1300, 31400}, {500, 800}, {700, 700}, {42, 99}};
    bool seen_uneven = false, seen_fewer = false;
    for (const auto& w : windows)
        for (int world : {1, 2, 3, 8}) {
            const size_t n = w[1] - w[0], nb = n / kBatch;
            size_t at = 0;
            for (int r = 0; r < world; ++r) {
                const EventRange b = rank_batches(n, world, r);
                std::printf("RANK %zu %zu %d %d %zu %zu\n", w[0], w[1], world, r, b.lo, b.hi);
                CHECK(b.lo == at && b.hi >= b.lo, "window of %zu events, world %d, rank %d: [%zu, %zu) does not follow %zu", n, world, r, b.lo, b.hi, at);
                CHECK(b.lo % kBatch == 0 && b.hi % kBatch == 0, "window of %zu events, world %d, rank %d: off the batch grid", n, world, r);
                const size_t cnt = (b.hi - b.lo) / kBatch;
                CHECK(cnt == nb / world + ((size_t)r < nb % world ? 1 : 0), "window of %zu events, world %d, rank %d: %zu batches (the remainder goes to the first ranks)", n, world, r, cnt);
                at = b.hi;
            }
            CHECK(at == nb * kBatch, "window of %zu events, world %d: the ranks cover %zu events, not the %zu whole batches", n, world, at, nb);
            seen_uneven |= nb % world != 0; seen_fewer |= nb > 0 && nb < (size_t)world;
        }
    CHECK(seen_uneven && seen_fewer, "the windows are meant to include a remainder and fewer batches than ranks");
    CHECK(rank_batches(799, 8, 0).hi == 100 && rank_batches(799, 8, 6).hi == 700 && rank_batches(799, 8, 7).lo == 700 && rank_batches(799, 8, 7).hi == 700, "7 batches on 8 ranks: the last rank gets none");
}

// ---- the layouts ----
void check_layouts()
{
    for (size_t n : {(size_t)0, (size_t)1, (size_t)2, (size_t)3, (size_t)1000}) {
        const HaloLayout h(n);
        CHECK(h.hbt == 0 && h.hx == h.hbt + 8 * n && h.hy == h.hx + 2 * n, "halo of %zu: [hbt (8 B) | hx (2 B) | hy (2 B)] in this order, end to end", n);
        CHECK(h.hy + 2 * n == (n ? h.bytes : 0) && h.bytes == (n ? n : 1) * 12, "halo of %zu: the parts end at %zu of %zu bytes", n, h.hy + 2 * n, h.bytes);
        CHECK(h.hbt % 8 == 0 && h.hx % 2 == 0 && h.hy % 2 == 0, "halo of %zu: alignment", n);
        alignas(8) static unsigned char buf[12 * 1000];
        CHECK((unsigned char*)h.hbt_in(buf) == buf + h.hbt && (unsigned char*)h.hx_in(buf) == buf + h.hx && (unsigned char*)h.hy_in(buf) == buf + h.hy, "halo of %zu: the pointers are the offsets", n);
    }
    CHECK(HaloLayout(0).bytes == 12, "an empty halo still reserves one entry");
    for (size_t chunk : {(size_t)1, (size_t)3, (size_t)1 << 19}) {
        const SeqChunkLayout r(chunk);
        CHECK(r.t == 0 && r.x == r.t + 8 * chunk && r.y == r.x + 2 * chunk && r.pol == r.y + 2 * chunk && r.bytes == r.pol + chunk, "chunk of %zu: [t | x | y | pol] end to end", chunk);
        CHECK(r.bytes == 13 * chunk && r.x % 2 == 0 && r.y % 2 == 0, "chunk of %zu: 13 bytes per event", chunk);
    }
    static_assert(SeqChunkLayout((size_t)1 << 19).bytes == 6815744, "6.5 MB per upload chunk");
}

void check_counts_and_shards()
{
    for (size_t n : {(size_t)0, (size_t)1, (size_t)7, (size_t)1000}) {
        for (int32_t rate : {-3, 0, 1}) CHECK(sampling_stride(rate) == 1 && sampled_count(n, rate) == n, "rate %d keeps every event", rate);
        for (int32_t rate : {2, 3, 7, 1001}) CHECK(sampling_stride(rate) == (size_t)rate && sampled_count(n, rate) == n / (size_t)rate, "rate %d keeps every %d-th event", rate, rate);
    }
    CHECK(seq_shard_ok(100, 300, 450, 450) == SeqShardStatus::ok && seq_shard_ok(100, 100, 100, 100) == SeqShardStatus::ok && seq_shard_ok(0, 0, 0, 0) == SeqShardStatus::ok, "shards on the window's grid");
    CHECK(seq_shard_ok(137, 237, 300, 1000) == SeqShardStatus::ok, "the WINDOW's grid, not the sequence's");
    CHECK(seq_shard_ok(300, 200, 400, 1000) == SeqShardStatus::not_a_range && seq_shard_ok(0, 400, 300, 1000) == SeqShardStatus::not_a_range &&
          seq_shard_ok(0, 100, 1001, 1000) == SeqShardStatus::not_a_range, "a shard in front of its window, reversed, or past the sequence");
    CHECK(seq_shard_ok(0, 150, 300, 1000) == SeqShardStatus::off_grid && seq_shard_ok(137, 200, 300, 1000) == SeqShardStatus::off_grid, "a shard off the window's batch grid");
    CHECK(seq_shard_ok(300, 250, 1001, 1000) == SeqShardStatus::not_a_range, "not a range is reported first");
    static_assert(kBatch == 100, "quirk Q1");
}

// ---- hot_threshold: computed in Python (floats: every operation rounded on its own) in the order of emba_amd.io.hot_pixel_threshold, printed with float.hex() ----
void check_hot_threshold()
{
    const struct { uint64_t s1, m, s2; double sigma, want; } cases[] = {
        {110ull, 5ull, 10030ull, 0x1.8000000000000p+1, 0x1.1613b0670619ep+7},      // counts 1 2 3 4 100
        {91ull, 13ull, 637ull, 0x1.4000000000000p+1, 0x1.c000000000000p+2},        // thirteen pixels of 7 events: no spread
        {1ull, 1ull, 1ull, 0x1.0000000000000p+0, 0x1.0000000000000p+0},
        {13ull, 4ull, 43ull, 0x0.0p+0, 0x1.a000000000000p+1},                      // sigma = 0: the mean
        {219ull, 7ull, 40113ull, 0x1.0000000000000p-1, 0x1.0701ccd37e40ep+6},
        {541780751ull, 7ull, 41932340307732001ull, 0x1.8000000000000p+1, 0x1.273f408924925p+26},      // var < 0 by rounding (six pixels of c events, one of c + 1): the mean
        {562402891ull, 7ull, 45185287400736841ull, 0x1.8000000000000p+1, 0x1.327c398924925p+26},      // "
        {616847297ull, 13ull, 29269275985862017ull, 0x1.8000000000000p+1, 0x1.6a036009d89d9p+25},     // "
    };
    for (const auto& k : cases) {
        const double got = hot_threshold(k.s1, k.m, k.s2, k.sigma);
        CHECK(std::memcmp(&got, &k.want, sizeof got) == 0, "hot_threshold(%llu, %llu, %llu, %a) = %a, Python gives %a", (unsigned long long)k.s1, (unsigned long long)k.m,
              (unsigned long long)k.s2, k.sigma, got, k.want);
    }
}

// ---- FilterPlan against the expressions at the top of emba_seq_filter before they moved (verbatim) ----
void check_filter_plan()
{
    const size_t S = 64 * 48;
    for (double hot_sigma : {0.0, 3.0})
        for (int64_t refractory_ns : {(int64_t)0, (int64_t)1000})
            for (int64_t support_ns : {(int64_t)0, (int64_t)5000})
                for (int32_t sampling_rate : {0, 1, 2, 3})
                    for (size_t n : {(size_t)0, (size_t)1, (size_t)5}) {
                        const bool hot_on = hot_sigma > 0.0, filters_on = hot_on || refractory_ns > 0 || support_ns > 0;
                        const size_t rate = sampling_rate >= 2 ? (size_t)sampling_rate : 1;
                        const bool sorts = filters_on && n, rewrites = filters_on || rate > 1;      // (neither: the sequence stays exactly as it is)
                        const size_t n_fresh = std::max<size_t>(n / rate, 1);
                        const FilterPlan p(n, S, hot_sigma, refractory_ns, support_ns, sampling_rate);
                        CHECK(p.n == n && p.S == S && p.hot_on == hot_on && p.filters_on == filters_on && p.rate == rate && p.sorts == sorts && p.rewrites == rewrites && p.n_fresh == n_fresh,
                              "sigma %g refractory %lld support %lld rate %d n %zu", hot_sigma, (long long)refractory_ns, (long long)support_ns, sampling_rate, n);
                        CHECK(p.n_fresh >= 1, "the fresh arrays are never empty");
                    }
    CHECK(!FilterPlan(5, S, -1.0, -5, -5, 1).filters_on && !FilterPlan(5, S, -1.0, -5, -5, 1).rewrites, "negative settings switch a filter off");
}

}  // namespace

int main()
{
    check_seq_window_sweep();
    check_seq_window_by_hand();
    check_rank_batches();
    check_layouts();
    check_counts_and_shards();
    check_hot_threshold();
    check_filter_plan();
    if (g_fail) { std::printf("%d checks failed\n", g_fail); return 1; }
    std::printf("OK sequence_rule\n");
    return 0;
}
