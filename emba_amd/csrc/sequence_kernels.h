// emba_amd/csrc/sequence_kernels.h — the whole event sequence resident in HBM, and the 3x3 median blur of the initial map (gfx950, wave64).
//
// What EMBA::EMBA / EMBA::Run do to their inputs before and between time windows (reference src/emba/emba.cpp):
//   * emba_seq_ingest_kernel   validation of a chunk of the raw sequence + the down-sampling of emba.cpp:281-304 as a strided gather
//   * emba_seq_window_kernel   getEventSubset (emba.cpp:473-510): both cursors as min-reductions over every 100th timestamp
//   * emba_median3_kernel      cv::medianBlur(., ., 3) on a float32 copy of a plane (emba.cpp:357-364)
//   * emba_halo_*_kernel       the per-pixel halo of a time shard of a window: for every sensor pixel the last event in front of the
//                              rank's range, in three passes — last event per pixel (atomicMax), flags + scan (order_kernels.h), gather
//   * emba_filter_*_kernel     hot-pixel, refractory and neighbour-support filters on the raw sequence (no counterpart in the reference): one stable
//                              sort by sensor pixel (order_kernels.h), per-pixel starts, keep-flags per event, scan, gather into fresh arrays
// All of it is bandwidth-bound, once-per-run or once-per-window work: one thread per element, coalesced loads, no tuning.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "order_kernels.h"   // batch_mid_ns_dev

namespace emba {

constexpr int kSeqProbe = 100;   // getEventSubset probes every 100th event (emba.cpp:485, 496)

// One chunk of the raw sequence (n_chunk events, the first of them has the original index k0; t_prev: the timestamp in front of the chunk).
// err[0] = smallest original index of an event outside the sensor, err[1] = smallest original index of an event earlier than its predecessor
// (0xFFFFFFFF each when clean) — every raw event is checked, kept or not.  rate <= 1: every event is kept; otherwise the events with original
// index rate-1, 2 rate-1, ... (sampling_count reaches the rate at the rate-th event, emba.cpp:287-298) go to slot (index + 1) / rate - 1.
__global__ void emba_seq_ingest_kernel(const int64_t* __restrict__ t, const uint16_t* __restrict__ x, const uint16_t* __restrict__ y, const uint8_t* __restrict__ pol,
                                       long n_chunk, long k0, int64_t t_prev, int sw, int sh, long rate, long n_kept,
                                       uint16_t* __restrict__ ox, uint16_t* __restrict__ oy, uint8_t* __restrict__ opol, int64_t* __restrict__ ot, uint32_t* __restrict__ err)
{
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_chunk) return;
    const long g = k0 + i;
    const uint16_t xi = x[i], yi = y[i];
    const int64_t ti = t[i];
    if (xi >= sw || yi >= sh) atomicMin(err + 0, (uint32_t)g);
    if (g > 0 && ti < (i > 0 ? t[i - 1] : t_prev)) atomicMin(err + 1, (uint32_t)g);
    long dst = g;
    if (rate > 1) {
        if ((g + 1) % rate) return;
        dst = (g + 1) / rate - 1;
    }
    if (dst >= n_kept) return;
    ox[dst] = xi; oy[dst] = yi; opol[dst] = pol[i]; ot[dst] = ti;
}

// res[0] = smallest j with t[100 j] > a, res[1] = smallest j with t[100 j] > b, over the probes 100 j < n (0xFFFFFFFF each: none).  The
// timestamps are sorted, so the first probe past a cursor IS the smallest one: a min-reduction, one atomic per wave that found any.
__global__ __launch_bounds__(256) void emba_seq_window_kernel(const int64_t* __restrict__ t, long n, int64_t a, int64_t b, uint32_t* __restrict__ res)
{
    const long m = (n + kSeqProbe - 1) / kSeqProbe;
    uint32_t ja = 0xFFFFFFFFu, jb = 0xFFFFFFFFu;
    for (long j = (long)blockIdx.x * blockDim.x + threadIdx.x; j < m; j += (long)gridDim.x * blockDim.x) {
        const int64_t tj = t[kSeqProbe * j];
        if (tj > a) ja = min(ja, (uint32_t)j);
        if (tj > b) jb = min(jb, (uint32_t)j);
    }
    for (int o = 32; o; o >>= 1) { ja = min(ja, (uint32_t)__shfl_xor((int)ja, o)); jb = min(jb, (uint32_t)__shfl_xor((int)jb, o)); }
    if ((threadIdx.x & 63) == 0) {
        if (ja != 0xFFFFFFFFu) atomicMin(res + 0, ja);
        if (jb != 0xFFFFFFFFu) atomicMin(res + 1, jb);
    }
}

// ---- the halo of a time shard: the events [0, m) handed in are [win_beg, lo) of the sequence, m a multiple of 100 (the WINDOW's batch grid) ----
// Pass 1: last[p] = the largest i with pixel(i) == p (last preset to -1: "none", below offset 0).  One 32-bit atomic per event on a table of sensor size.
__global__ void emba_halo_last_kernel(const uint16_t* __restrict__ x, const uint16_t* __restrict__ y, long m, int sw, int32_t* __restrict__ last)
{
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < m) atomicMax(last + ((size_t)y[i] * sw + x[i]), (int32_t)i);
}

// Pass 2: flag[i] = 1 iff event i is its pixel's last one; the exclusive scan of the flags (dev_scan) then numbers the halo entries in index = time order.
__global__ void emba_halo_flag_kernel(const uint16_t* __restrict__ x, const uint16_t* __restrict__ y, long m, int sw, const int32_t* __restrict__ last,
                                      uint32_t* __restrict__ flag)
{
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < m) flag[i] = last[(size_t)y[i] * sw + x[i]] == (int32_t)i;
}

// Pass 3: entry pos[i] of the halo = (x, y, midpoint of the window batch i / 100) of every flagged event; t: the window's timestamps (t[0] is win_beg's).
__global__ void emba_halo_gather_kernel(const uint16_t* __restrict__ x, const uint16_t* __restrict__ y, const int64_t* __restrict__ t, long m,
                                        const uint32_t* __restrict__ flag, const uint32_t* __restrict__ pos, uint16_t* __restrict__ hx, uint16_t* __restrict__ hy,
                                        int64_t* __restrict__ hbt)
{
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m || !flag[i]) return;
    const long b = i / 100;
    const uint32_t j = pos[i];
    hx[j] = x[i]; hy[j] = y[i];
    hbt[j] = batch_mid_ns_dev(t[100 * b], t[100 * b + 99]);
}

// ---- sensor-noise filters on the raw resident sequence (emba_seq_filter; the rule: include/emba_hip.h) -------------------------------
// The sequence is sorted by (sensor pixel, index) with the radix sort of order_kernels.h (keys p = y sw + x, values k); everything below works on that
// order.  Every event is judged from the RAW sequence, so the three tests are independent of each other and of the order in which they run.

// start[p], p in [0, S]: the first sorted entry of pixel p (start[S] = n); c[p] = start[p + 1] - start[p].  One coalesced pass over the n >= 1 sorted keys:
// the head of a pixel's chain (entry i whose predecessor has a smaller key) writes i to every pixel in (keys[i - 1], keys[i]] — the pixels without events in
// between begin where the next chain begins — and the last entry writes n to every pixel behind its own.  Every p in [0, S] is written exactly once.
__global__ void emba_filter_starts_kernel(const uint32_t* __restrict__ keys, long n, long S, uint32_t* __restrict__ start)
{
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const long key = keys[i], prev = i > 0 ? (long)keys[i - 1] : -1L;
    for (long p = prev + 1; p <= key && p <= S; ++p) start[p] = (uint32_t)i;
    if (i == n - 1)
        for (long p = key + 1; p <= S; ++p) start[p] = (uint32_t)n;
}

__device__ __forceinline__ unsigned long long wave_sum_u64(unsigned long long v)
{
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// sums[0] += pixels with c > 0, sums[1] += sum of c^2 (exact: c < 2^32, the sum <= n^2 < 2^64).  One atomic pair per wave.
__global__ __launch_bounds__(256) void emba_filter_pixel_sums_kernel(const uint32_t* __restrict__ start, long S, unsigned long long* __restrict__ sums)
{
    unsigned long long m = 0, s2 = 0;
    for (long p = (long)blockIdx.x * 256 + threadIdx.x; p < S; p += (long)gridDim.x * 256) {
        const unsigned long long c = start[p + 1] - start[p];
        m += c ? 1ull : 0ull;
        s2 += c * c;
    }
    m = wave_sum_u64(m); s2 = wave_sum_u64(s2);
    if ((threadIdx.x & 63) == 0) { atomicAdd(sums + 0, m); atomicAdd(sums + 1, s2); }
}

// hot[p] = double(c[p]) > thr (thr: computed by the host from the exact sums, one rounding per operation); sums[2] += hot pixels, sums[3] += their events.
__global__ __launch_bounds__(256) void emba_filter_hot_kernel(const uint32_t* __restrict__ start, long S, double thr, uint8_t* __restrict__ hot,
                                                              unsigned long long* __restrict__ sums)
{
    unsigned long long np = 0, ne = 0;
    for (long p = (long)blockIdx.x * 256 + threadIdx.x; p < S; p += (long)gridDim.x * 256) {
        const uint32_t c = start[p + 1] - start[p];
        const bool h = (double)c > thr;
        hot[p] = h ? 1 : 0;
        if (h) { np += 1; ne += c; }
    }
    np = wave_sum_u64(np); ne = wave_sum_u64(ne);
    if ((threadIdx.x & 63) == 0 && np) { atomicAdd(sums + 2, np); atomicAdd(sums + 3, ne); }
}

// One thread per SORTED entry r (pixel p = keys[r], event k = vals[r]; a pixel's entries are its events in index order, the sort is stable).
//   hot         hot[p]
//   refractory  entry r - 1 is prev(k) when it has the same pixel: fails iff t[k] - t[prev] < refr_ns                     (refr_ns <= 0: off)
//   support     per neighbouring pixel q inside the sensor and not hot: the largest entry of q's chain with index < k (binary search in vals over
//               [start[q], start[q + 1])), passes iff t[k] - t[that] <= supp_ns for some q                                     (supp_ns <= 0: off)
// Neighbouring lanes hold neighbouring entries of one chain: they search the same ranges, so the probes hit the same cache lines.
// keep[k] (the event's ORIGINAL index) = 1 iff it fails none; sums[4] += events failing refractory, sums[5] += events failing support (one atomic per wave).
__global__ __launch_bounds__(256) void emba_filter_flags_kernel(const uint32_t* __restrict__ keys, const uint32_t* __restrict__ vals, const int64_t* __restrict__ t,
                                                                long n, int sw, int sh, const uint32_t* __restrict__ start, const uint8_t* __restrict__ hot,
                                                                int64_t refr_ns, int64_t supp_ns, uint32_t* __restrict__ keep, unsigned long long* __restrict__ sums)
{
    const long r = (long)blockIdx.x * 256 + threadIdx.x;
    bool f_ref = false, f_sup = false;
    if (r < n) {
        const uint32_t p = keys[r], k = vals[r];
        const int64_t tk = t[k];
        if (refr_ns > 0 && r > 0 && keys[r - 1] == p) f_ref = tk - t[vals[r - 1]] < refr_ns;
        if (supp_ns > 0) {
            const int px = (int)(p % (uint32_t)sw), py = (int)(p / (uint32_t)sw);
            bool ok = false;
            for (int dy = -1; dy <= 1; ++dy)
                for (int dx = -1; dx <= 1; ++dx) {
                    const int qx = px + dx, qy = py + dy;
                    if (ok || (!dx && !dy) || qx < 0 || qx >= sw || qy < 0 || qy >= sh) continue;
                    const size_t q = (size_t)qy * sw + qx;
                    if (hot[q]) continue;
                    const uint32_t base = start[q];
                    uint32_t lo = base, hi = start[q + 1];
                    while (lo < hi) {
                        const uint32_t mid = lo + ((hi - lo) >> 1);
                        if (vals[mid] < k) lo = mid + 1; else hi = mid;
                    }
                    if (lo > base && tk - t[vals[lo - 1]] <= supp_ns) ok = true;
                }
            f_sup = !ok;
        }
        keep[k] = (hot[p] || f_ref || f_sup) ? 0u : 1u;
    }
    const unsigned long long b_ref = __ballot(f_ref), b_sup = __ballot(f_sup);
    if ((threadIdx.x & 63) == 0) {
        if (b_ref) atomicAdd(sums + 4, (unsigned long long)__popcll(b_ref));
        if (b_sup) atomicAdd(sums + 5, (unsigned long long)__popcll(b_sup));
    }
}

// The survivors (keep == nullptr: every event), in their order, into FRESH arrays: survivor of rank r = pos[k] (the exclusive scan of keep) goes to slot r, or,
// with rate > 1, to slot (r + 1) / rate - 1 iff (r + 1) % rate == 0 — the counting loop of emba.cpp:281-304 over the survivors.  cap: slots of the fresh arrays.
__global__ void emba_filter_gather_kernel(const uint16_t* __restrict__ x, const uint16_t* __restrict__ y, const uint8_t* __restrict__ pol, const int64_t* __restrict__ t,
                                          long n, const uint32_t* __restrict__ keep, const uint32_t* __restrict__ pos, long rate, long cap,
                                          uint16_t* __restrict__ ox, uint16_t* __restrict__ oy, uint8_t* __restrict__ opol, int64_t* __restrict__ ot)
{
    const long k = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    long r = k;
    if (keep) { if (!keep[k]) return; r = pos[k]; }
    long dst = r;
    if (rate > 1) {
        if ((r + 1) % rate) return;
        dst = (r + 1) / rate - 1;
    }
    if (dst >= cap) return;
    ox[dst] = x[k]; oy[dst] = y[k]; opol[dst] = pol[k]; ot[dst] = t[k];
}

// a <- min, b <- max: one exchange of the median network (no branch on data)
__device__ __forceinline__ void med_exchange(float& a, float& b)
{
    const float lo = fminf(a, b), hi = fmaxf(a, b);
    a = lo; b = hi;
}

// dst = f64(median3x3(f32(src))) with replicated borders (cv::BORDER_REPLICATE: SURVEY Appendix A), h x w row-major; dst must not be src.
// convertTo(CV_32F) rounds to nearest even, which is what the conversion below does; the median SELECTS one of the nine floats (19 exchanges:
// the classic minimum-exchange network for nine values), so the result is exact.  NaN input is undefined, as in OpenCV.
__global__ __launch_bounds__(256) void emba_median3_kernel(const double* __restrict__ src, int h, int w, double* __restrict__ dst)
{
    const int x = blockIdx.x * 64 + (threadIdx.x & 63);
    const int y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= w || y >= h) return;
    const int xm = max(x - 1, 0), xp = min(x + 1, w - 1);
    const size_t r0 = (size_t)max(y - 1, 0) * w, r1 = (size_t)y * w, r2 = (size_t)min(y + 1, h - 1) * w;
    float p0 = (float)src[r0 + xm], p1 = (float)src[r0 + x], p2 = (float)src[r0 + xp];
    float p3 = (float)src[r1 + xm], p4 = (float)src[r1 + x], p5 = (float)src[r1 + xp];
    float p6 = (float)src[r2 + xm], p7 = (float)src[r2 + x], p8 = (float)src[r2 + xp];
    med_exchange(p1, p2); med_exchange(p4, p5); med_exchange(p7, p8);
    med_exchange(p0, p1); med_exchange(p3, p4); med_exchange(p6, p7);
    med_exchange(p1, p2); med_exchange(p4, p5); med_exchange(p7, p8);
    med_exchange(p0, p3); med_exchange(p5, p8); med_exchange(p4, p7);
    med_exchange(p3, p6); med_exchange(p1, p4); med_exchange(p2, p5);
    med_exchange(p4, p7); med_exchange(p4, p2); med_exchange(p6, p4);
    med_exchange(p4, p2);
    dst[r1 + x] = (double)p4;
}

}  // namespace emba
