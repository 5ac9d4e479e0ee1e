// emba_amd/csrc/sequence_rule.h — the host arithmetic of the resident event sequence (sequence_host.h) and of the time shards cut from it (group.h), as
// functions of plain values: the batch length, the down-sampled count, the layouts of an upload chunk and of a halo, the event window behind the probe
// kernel, which shard of a window is acceptable, which batches a rank gets, the hot-pixel threshold and what a filter call has to do.
//
// No HIP in here: plain C++17, so that tests/cpp/sequence_rule_test.cpp checks it on a CPU in milliseconds.  The kernels' sizes come in as values (`probe`:
// kSeqProbe of sequence_kernels.h).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <cmath>

namespace emba {

// Events per batch: a window's events are handled in groups of 100 with one pose each, a tail of n % 100 is dropped (quirk Q1, model.cpp:79).
// (kSeqProbe of sequence_kernels.h, the stride of getEventSubset's probes, is another 100 that happens to be equal.)
constexpr size_t kBatch = 100;

// emba.cpp:281-304: of every `rate` events the last one is kept; a rate below 2 keeps every event.
inline size_t sampling_stride(int32_t sampling_rate) { return sampling_rate >= 2 ? (size_t)sampling_rate : 1; }      // emba.cpp:282
inline size_t sampled_count(size_t n, int32_t sampling_rate) { return n / sampling_stride(sampling_rate); }

// One upload chunk of `chunk` raw events, 8 B + 2 B + 2 B + 1 B each, laid out [t | x | y | pol]: byte offsets of the parts, and the size of the whole.
struct SeqChunkLayout {
    size_t t, x, y, pol, bytes;
    constexpr explicit SeqChunkLayout(size_t chunk) : t(0), x(chunk * 8), y(x + chunk * 2), pol(y + chunk * 2), bytes(pol + chunk) {}
};

// The halo of a time shard as emba_set_events stages it in one buffer: [hbt (8 B) | hx (2 B) | hy (2 B)] x n — byte offsets of the parts, and the size to
// reserve (an empty halo still reserves one entry).  Nobody else knows this layout: the host takes its pointers from here.
struct HaloLayout {
    size_t hbt, hx, hy, bytes;
    explicit HaloLayout(size_t n) : hbt(0), hx(n * 8), hy(hx + n * 2), bytes(std::max<size_t>(n, 1) * 12) {}
    int64_t* hbt_in(void* base) const { return reinterpret_cast<int64_t*>(static_cast<uint8_t*>(base) + hbt); }
    uint16_t* hx_in(void* base) const { return reinterpret_cast<uint16_t*>(static_cast<uint8_t*>(base) + hx); }
    uint16_t* hy_in(void* base) const { return reinterpret_cast<uint16_t*>(static_cast<uint8_t*>(base) + hy); }
};

// ---- getEventSubset (emba.cpp:473-510) behind the probe kernel ----
// the cursors the probes are compared with: t_epsilon = ros::Duration(1e-3), emba.cpp:476-478
struct SeqCursors { int64_t a, b; };
inline SeqCursors seq_window_cursors(int64_t t_beg_ns, int64_t t_end_ns) { return {t_beg_ns + 1000000, t_end_ns - 1000000}; }

constexpr uint32_t kNoProbe = 0xFFFFFFFFu;   // what the probe kernel leaves where no probe lies past a cursor
enum class SeqWindowStatus {
    ok,
    stops_at_first_probe,   // the tail search stops at its first probe, event `beg` (the reference's `-= 100` underflows)
    begins_behind_last,     // the window begins behind the last event
};
struct SeqWindow { SeqWindowStatus status; size_t beg, end; };
// n events probed at every `probe`-th; first_past_a / first_past_b: the smallest j with t[probe j] > a / > b, or kNoProbe
inline SeqWindow seq_window(size_t n, uint32_t first_past_a, uint32_t first_past_b, size_t probe)
{
    const size_t m = (n + probe - 1) / probe;
    // head: the first probe past a, or the first multiple of 100 >= n (emba.cpp:483-491)
    const size_t jb = first_past_a != kNoProbe ? first_past_a : m, beg = probe * jb;
    size_t end = n;                                                      // no probe past b: the loop runs off the sequence, :504-505
    if (jb < m && first_past_b != kNoProbe) {
        // tail: the first probe >= beg past b (every probe from beg on is past a; where b < a the search stops at beg itself)
        const size_t je = std::max<size_t>(first_past_b, jb);
        if (je == jb) return {SeqWindowStatus::stops_at_first_probe, beg, beg};
        end = probe * je - probe;                                        // :500
    }
    if (beg > end) return {SeqWindowStatus::begins_behind_last, beg, end};
    return {SeqWindowStatus::ok, beg, end};
}

// The shard [lo, hi) of the window that begins at win_beg, of a sequence of n events: a range of the sequence, and beginning on the WINDOW's batch grid
enum class SeqShardStatus { ok, not_a_range, off_grid };
inline SeqShardStatus seq_shard_ok(size_t win_beg, size_t lo, size_t hi, size_t n)
{
    if (win_beg > lo || lo > hi || hi > n) return SeqShardStatus::not_a_range;
    if ((lo - win_beg) % kBatch) return SeqShardStatus::off_grid;
    return SeqShardStatus::ok;
}

// Time shards of a window of n_events: rank r of `world` gets whole batches, nb / world each and the remainder on the first ranks — [lo, hi) relative to
// the window's first event.  (The n_events % kBatch tail is nobody's: the callers hand it to the last rank, which ignores it as every window does.)
struct EventRange { size_t lo, hi; };
inline EventRange rank_batches(size_t n_events, int world, int r)
{
    const size_t nb = n_events / kBatch, base = nb / (size_t)world, rem = nb % (size_t)world;
    const size_t first = (size_t)r * base + std::min<size_t>((size_t)r, rem), cnt = base + ((size_t)r < rem ? 1 : 0);
    return {first * kBatch, (first + cnt) * kBatch};
}

// thr = mean + sigma sqrt(var) over the pixels with events, from the exact integer sums: every operation rounded on its own (no contraction), so that
// the host form (emba_amd.io.filter_events) and the loop reference of the tests get the same bits.
inline double hot_threshold(uint64_t s1, uint64_t m, uint64_t s2, double sigma)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double mean = (double)s1 / (double)m;
    const double msq = (double)s2 / (double)m;
    const double mean2 = mean * mean;
    double var = msq - mean2;
    if (var < 0.0) var = 0.0;
    const double sd = std::sqrt(var);
    const double spread = sigma * sd;
    return mean + spread;
}

// What one emba_seq_filter call does to a sequence of n events on a sensor of S pixels
struct FilterPlan {
    size_t n, S;
    bool hot_on, filters_on;
    size_t rate;
    bool sorts, rewrites;      // (neither: the sequence stays exactly as it is)
    size_t n_fresh;            // the fresh arrays at their upper bound n / rate
    FilterPlan(size_t n_, size_t S_, double hot_sigma, int64_t refractory_ns, int64_t support_ns, int32_t sampling_rate)
        : n(n_), S(S_), hot_on(hot_sigma > 0.0), filters_on(hot_on || refractory_ns > 0 || support_ns > 0), rate(sampling_stride(sampling_rate)),
          sorts(filters_on && n), rewrites(filters_on || rate > 1), n_fresh(std::max<size_t>(n / rate, 1))
    {
    }
};

}  // namespace emba
