// emba_amd/csrc/render_kernels.h — the reference's record_data map images (EMBA::saveEvoData / saveOptData, src/emba/solver.cpp:370-479) rendered
// on the device: Gx and Gy robust-normalised (image_util::normalizeRobust, src/utils/image_utils.cpp:14-38), the HSV image of the gradient (hue =
// orientation, value = magnitude) and the robust-normalised Poisson intensity.  Only the finished 8-bit images cross PCIe.
//
// Robust order statistics, exact: a radix select of the two ranks i_min, i_max of an f64 plane on the order-preserving 64-bit key (sign bit flipped
// for non-negative values, all bits for negative ones).  Launches per set of planes (1 or 2 planes, both ranks of each):
//     emba_rsel_stats_kernel     histogram of the top 12 key bits (LDS per workgroup, merged with global atomics); the workgroup with the last
//                                ticket picks each rank's bucket and residual rank.  With hsv: also min / max of 0.5*angle and of the magnitude.
//     emba_rsel_compact_kernel   the keys of the chosen buckets into a candidate buffer (these two launches are the plane's two full reads)
//     emba_rsel_round_kernel x4  13 more key bits per round over the candidates, the last workgroup of each rank picks (12 + 4 x 13 = 64 bits)
// Nothing returns to the host between the launches: the render / normalise kernels read rmin / rmax (and the min / max) from RenderState.
//
// Arithmetic (emba_amd/io.normalize_robust; the numpy restatement in tests/test_record_cpu.py pins it):
//     u8 = sat(rint(scale * (v - rmin))), scale = 255 / (rmax - rmin), or 1 when rmax == rmin
//     angle = atan2(Gy, Gx) in degrees, + 360 where negative;  mag = sqrt(Gx*Gx + Gy*Gy)
//     H = sat(rint(0.5*angle*s + t)), s = 179 * (1 / (max - min)) when max - min > DBL_EPSILON else 0, t = 0 - min*s (min, max over 0.5*angle)
//     V: the same over mag with 255;  S = 255;  RGB: OpenCV's 8-bit HSV -> RGB with hue range 180, in float32 (hsv_to_rgb below)
// OpenCV's cartToPolar uses an approximate arctangent and its MatExpr evaluation of scale*(src - rmin) may round differently, so G_hsv and
// last-level rounding are NOT pinned against the reference; the rules above are this project's definition.  Contraction into FMA is switched off
// in every function that states one of these rules, so that the device rounds each operation as numpy does.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace emba {

constexpr int kRselBits0 = 12, kRselBins0 = 1 << kRselBits0;     // first pass: the top 12 key bits (16 KiB of LDS per plane)
constexpr int kRselBits = 13, kRselBins = 1 << kRselBits;        // rounds 1-4: 13 bits each (32 KiB of LDS)
constexpr int kRselRounds = 4;
constexpr int kRselThreads = 512;
constexpr int kRselSlots = 4;                                    // slot 2*plane + r: rank r (0: i_min, 1: i_max) of plane 0 / 1

struct RselSlot {
    unsigned long long prefix;   // key bits resolved so far (the bits below the current digit are zero)
    unsigned int rank;           // residual rank among the candidates that share the prefix
    unsigned int cand_off;       // this slot's candidates in its plane's candidate buffer: [cand_off, cand_off + cand_n)
    unsigned int cand_n;
    unsigned int ticket;         // workgroups of the running round that are done (the last one picks and puts it back to 0)
    double value;                // the order statistic, once all 64 bits are resolved
};

struct RenderState {
    RselSlot slot[kRselSlots];
    unsigned int cand_cnt[kRselSlots];   // write cursors of emba_rsel_compact_kernel
    unsigned int ticket0;                // workgroups of emba_rsel_stats_kernel that are done
    unsigned int pad;
    unsigned long long mm[4];            // keys: min / max of 0.5*angle, min / max of mag (reset to ~0 / 0 by the last workgroup)
    double mmv[4];                       // ... their values
};

struct RselParams {
    const double* src[2];        // the planes (n values each)
    unsigned int n;
    int nplanes;
    unsigned int k[2];           // the two ranks, the same for every plane
    int hsv;                     // 1: src = (Gx, Gy) and the min / max of 0.5*angle and mag are wanted too
    unsigned int* hist;          // [kRselSlots][kRselBins], zero between uses
    unsigned long long* cand;    // [nplanes][n]
    RenderState* st;
};

__device__ __forceinline__ unsigned long long rsel_key(double v)
{
    const unsigned long long b = (unsigned long long)__double_as_longlong(v);
    return b ^ ((b >> 63) ? ~0ull : 0x8000000000000000ull);
}
__device__ __forceinline__ double rsel_unkey(unsigned long long k)
{
    return __longlong_as_double((long long)((k >> 63) ? (k ^ 0x8000000000000000ull) : ~k));
}

// 0.5 * angle in degrees [0, 180) and the magnitude of one gradient
__device__ __forceinline__ void polar_half(double gx, double gy, double& half, double& mag)
{
#pragma clang fp contract(off)
    double a = atan2(gy, gx) * (180.0 / M_PI);
    if (a < 0.0) a = a + 360.0;
    half = 0.5 * a;
    mag = sqrt(gx * gx + gy * gy);
}

__device__ __forceinline__ unsigned char sat_u8(double x)      // x already rounded
{
    return (unsigned char)fmin(fmax(x, 0.0), 255.0);
}
__device__ __forceinline__ unsigned char sat_u8f(float x)
{
    return (unsigned char)fminf(fmaxf(x, 0.0f), 255.0f);
}

__device__ __forceinline__ unsigned char robust_u8(double v, double rmin, double scale)
{
#pragma clang fp contract(off)
    return sat_u8(rint(scale * (v - rmin)));
}
__device__ __forceinline__ double robust_scale(double rmin, double rmax)
{
    return (rmax != rmin) ? 255.0 / (rmax - rmin) : 1.0;
}
// cv::normalize(src, dst, 0, a, NORM_MINMAX, CV_8U): dst = sat(rint(src*s + t))
__device__ __forceinline__ void minmax_coef(double mn, double mx, double a, double& s, double& t)
{
#pragma clang fp contract(off)
    const double d = mx - mn;
    s = (d > 2.220446049250313e-16) ? a * (1.0 / d) : 0.0;
    t = 0.0 - mn * s;
}
__device__ __forceinline__ unsigned char minmax_u8(double v, double s, double t)
{
#pragma clang fp contract(off)
    return sat_u8(rint(v * s + t));
}

// OpenCV's 8-bit HSV -> RGB (hue range 180) in float32; out = (r, g, b)
__device__ __forceinline__ void hsv_to_rgb(unsigned char H, unsigned char S, unsigned char V, unsigned char out[3])
{
#pragma clang fp contract(off)
    float h = (float)H * (6.f / 180.f), s = (float)S * (1.f / 255.f), v = (float)V * (1.f / 255.f);
    float fs = floorf(h);
    int sector = (int)fs;
    h = h - fs;
    if (sector < 0 || sector >= 6) { sector = 0; h = 0.f; }
    const float t0 = v, t1 = v * (1.f - s), t2 = v * (1.f - s * h), t3 = v * (1.f - s * (1.f - h));
    float b, g, r;      // (b, g, r) = tab[{1,3,0},{1,0,2},{3,0,1},{0,2,1},{0,1,3},{2,1,0}][sector], tab = {t0, t1, t2, t3}
    switch (sector) {
    case 0: b = t1; g = t3; r = t0; break;
    case 1: b = t1; g = t0; r = t2; break;
    case 2: b = t3; g = t0; r = t1; break;
    case 3: b = t0; g = t2; r = t1; break;
    case 4: b = t0; g = t1; r = t3; break;
    default: b = t2; g = t1; r = t0; break;
    }
    out[0] = sat_u8f(rintf(r * 255.f)); out[1] = sat_u8f(rintf(g * 255.f)); out[2] = sat_u8f(rintf(b * 255.f));
}

// The last workgroup's pick: hist (nb bins, read and zeroed at the point of coherence) into LDS, an exclusive scan, and for each rank in k[0 .. nk)
// the bin that holds it, the count below that bin and the bin's count.  nb / blockDim.x bins per thread.
template <int NB>
__device__ void rsel_pick(unsigned int* __restrict__ hist, unsigned int* lds, unsigned int* scan, const unsigned int* k, int nk,
                          unsigned int* bin_out, unsigned int* below_out, unsigned int* cnt_out)
{
    constexpr int per = NB / kRselThreads;
    const int t = threadIdx.x;
    if (t < nk) { bin_out[t] = 0u; below_out[t] = 0u; cnt_out[t] = 0u; }   // (a rank outside the histogram cannot happen; if it did, no candidates)
    unsigned int sum = 0;
    for (int j = 0; j < per; ++j) { const unsigned int v = atomicExch(&hist[t * per + j], 0u); lds[t * per + j] = v; sum += v; }
    scan[t] = sum;
    __syncthreads();
    for (int off = 1; off < kRselThreads; off <<= 1) {          // inclusive scan of the per-thread sums
        const unsigned int add = t >= off ? scan[t - off] : 0u;
        __syncthreads();
        scan[t] += add;
        __syncthreads();
    }
    unsigned int base = scan[t] - sum;
    for (int r = 0; r < nk; ++r) {
        if (k[r] >= base && k[r] < base + sum) {
            unsigned int b = base;
            for (int j = 0; j < per; ++j) {
                const unsigned int v = lds[t * per + j];
                if (k[r] < b + v) { bin_out[r] = (unsigned int)(t * per + j); below_out[r] = b; cnt_out[r] = v; break; }
                b += v;
            }
        }
    }
    __syncthreads();
}

__device__ __forceinline__ bool rsel_last_block(unsigned int* ticket, unsigned int nblk)
{
    __shared__ int s_last;
    __threadfence();
    __syncthreads();
    if (threadIdx.x == 0) s_last = (atomicAdd(ticket, 1u) == nblk - 1u) ? 1 : 0;
    __syncthreads();
    if (s_last) __threadfence();
    return s_last != 0;
}

// Pass 1 over the planes: top-12-bit histograms (+ the HSV min / max); the last workgroup picks both ranks' buckets for every plane.
__global__ void __launch_bounds__(kRselThreads) emba_rsel_stats_kernel(RselParams p)
{
    __shared__ unsigned int h[2][kRselBins0];
    __shared__ unsigned int scan[kRselThreads];
    __shared__ unsigned long long smm[4];
    __shared__ unsigned int pk_bin[2], pk_below[2], pk_cnt[2];
    const int t = threadIdx.x;
    for (int j = t; j < 2 * kRselBins0; j += kRselThreads) (&h[0][0])[j] = 0u;
    if (t < 4) smm[t] = (t & 1) ? 0ull : ~0ull;
    __syncthreads();
    unsigned long long mm[4] = {~0ull, 0ull, ~0ull, 0ull};
    const long n = p.n;
    for (long i = (long)blockIdx.x * kRselThreads + t; i < n; i += (long)gridDim.x * kRselThreads) {
        const double a = p.src[0][i];
        atomicAdd(&h[0][rsel_key(a) >> (64 - kRselBits0)], 1u);
        if (p.nplanes > 1) {
            const double b = p.src[1][i];
            atomicAdd(&h[1][rsel_key(b) >> (64 - kRselBits0)], 1u);
            if (p.hsv) {
                double half, mag;
                polar_half(a, b, half, mag);
                const unsigned long long kh = rsel_key(half), km = rsel_key(mag);
                mm[0] = kh < mm[0] ? kh : mm[0]; mm[1] = kh > mm[1] ? kh : mm[1];
                mm[2] = km < mm[2] ? km : mm[2]; mm[3] = km > mm[3] ? km : mm[3];
            }
        }
    }
    if (p.hsv) { atomicMin(&smm[0], mm[0]); atomicMax(&smm[1], mm[1]); atomicMin(&smm[2], mm[2]); atomicMax(&smm[3], mm[3]); }
    __syncthreads();
    for (int pl = 0; pl < p.nplanes; ++pl)
        for (int j = t; j < kRselBins0; j += kRselThreads)
            if (h[pl][j]) atomicAdd(&p.hist[(size_t)(2 * pl) * kRselBins + j], h[pl][j]);
    if (p.hsv && t == 0) { atomicMin(&p.st->mm[0], smm[0]); atomicMax(&p.st->mm[1], smm[1]); atomicMin(&p.st->mm[2], smm[2]); atomicMax(&p.st->mm[3], smm[3]); }
    if (!rsel_last_block(&p.st->ticket0, gridDim.x)) return;
    RenderState* st = p.st;
    const unsigned int kk[2] = {p.k[0], p.k[1]};
    for (int pl = 0; pl < p.nplanes; ++pl) {
        rsel_pick<kRselBins0>(p.hist + (size_t)(2 * pl) * kRselBins, h[0], scan, kk, 2, pk_bin, pk_below, pk_cnt);
        if (t < 2) {
            RselSlot& s = st->slot[2 * pl + t];
            s.prefix = (unsigned long long)pk_bin[t] << (64 - kRselBits0);
            s.rank = kk[t] - pk_below[t];
            s.cand_n = pk_cnt[t];
            s.cand_off = (t == 1 && pk_bin[1] != pk_bin[0]) ? pk_cnt[0] : 0u;     // both ranks in one bucket: one set of candidates
            s.value = 0.0;
            st->cand_cnt[2 * pl + t] = 0u;
        }
        __syncthreads();
    }
    if (t == 0) {
        if (p.hsv) {
            const unsigned long long init[4] = {~0ull, 0ull, ~0ull, 0ull};
            for (int j = 0; j < 4; ++j) st->mmv[j] = rsel_unkey(atomicExch(&st->mm[j], init[j]));
        }
        st->ticket0 = 0u;
    }
}

// Pass 2 over the planes: the keys of the two chosen buckets into the candidate buffer.
__global__ void __launch_bounds__(256) emba_rsel_compact_kernel(RselParams p)
{
    RenderState* st = p.st;
    const long n = p.n;
    for (int pl = 0; pl < p.nplanes; ++pl) {
        const unsigned long long b0 = st->slot[2 * pl].prefix >> (64 - kRselBits0), b1 = st->slot[2 * pl + 1].prefix >> (64 - kRselBits0);
        const unsigned int o0 = st->slot[2 * pl].cand_off, n0 = st->slot[2 * pl].cand_n, o1 = st->slot[2 * pl + 1].cand_off, n1 = st->slot[2 * pl + 1].cand_n;
        unsigned long long* cand = p.cand + (size_t)pl * p.n;
        for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
            const unsigned long long key = rsel_key(p.src[pl][i]), d = key >> (64 - kRselBits0);
            if (d == b0) { const unsigned int pos = atomicAdd(&st->cand_cnt[2 * pl], 1u); if (pos < n0) cand[o0 + pos] = key; }
            else if (d == b1) { const unsigned int pos = atomicAdd(&st->cand_cnt[2 * pl + 1], 1u); if (pos < n1) cand[o1 + pos] = key; }
        }
    }
}

// Round r = 1 .. 4: the next 13 key bits of the candidates that share the slot's prefix (blockIdx.y = slot); the slot's last workgroup picks.
__global__ void __launch_bounds__(kRselThreads) emba_rsel_round_kernel(RselParams p, int round)
{
    __shared__ unsigned int h[kRselBins];
    __shared__ unsigned int scan[kRselThreads];
    __shared__ unsigned int pk_bin[1], pk_below[1], pk_cnt[1];
    const int t = threadIdx.x, slot = blockIdx.y, pl = slot >> 1;
    const int shift = 64 - kRselBits0 - kRselBits * round, hi = shift + kRselBits;
    RselSlot* s = &p.st->slot[slot];
    const unsigned long long want = s->prefix >> hi;
    const unsigned int off = s->cand_off, cnt = s->cand_n;
    for (int j = t; j < kRselBins; j += kRselThreads) h[j] = 0u;
    __syncthreads();
    const unsigned long long* cand = p.cand + (size_t)pl * p.n + off;
    for (unsigned int i = blockIdx.x * kRselThreads + t; i < cnt; i += gridDim.x * kRselThreads) {
        const unsigned long long key = cand[i];
        if ((key >> hi) == want) atomicAdd(&h[(key >> shift) & (kRselBins - 1)], 1u);
    }
    __syncthreads();
    unsigned int* gh = p.hist + (size_t)slot * kRselBins;
    for (int j = t; j < kRselBins; j += kRselThreads)
        if (h[j]) atomicAdd(&gh[j], h[j]);
    if (!rsel_last_block(&s->ticket, gridDim.x)) return;
    const unsigned int k = s->rank;
    rsel_pick<kRselBins>(gh, h, scan, &k, 1, pk_bin, pk_below, pk_cnt);
    if (t == 0) {
        const unsigned long long prefix = s->prefix | ((unsigned long long)pk_bin[0] << shift);
        s->prefix = prefix;
        s->rank = k - pk_below[0];
        if (round == kRselRounds) s->value = rsel_unkey(prefix);
        s->ticket = 0u;
    }
}

// robust normalisation of one plane with the order statistics of slots (2*plane, 2*plane + 1)
__global__ void __launch_bounds__(256) emba_robust_u8_kernel(const double* __restrict__ src, unsigned int n, const RenderState* __restrict__ st, int plane,
                                                             unsigned char* __restrict__ out)
{
    const double rmin = st->slot[2 * plane].value, rmax = st->slot[2 * plane + 1].value, scale = robust_scale(rmin, rmax);
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < (long)n; i += (long)gridDim.x * blockDim.x)
        out[i] = robust_u8(src[i], rmin, scale);
}

// The fused render pass: Gx and Gy read once; Gx_u8, Gy_u8 and the interleaved RGB image (PNG channel order) written.  4 pixels per thread.
__global__ void __launch_bounds__(256) emba_render_kernel(const double* __restrict__ gx, const double* __restrict__ gy, unsigned int n,
                                                          const RenderState* __restrict__ st, unsigned char* __restrict__ gx_u8,
                                                          unsigned char* __restrict__ gy_u8, unsigned char* __restrict__ rgb, int vec)
{
    const double xmin = st->slot[0].value, xmax = st->slot[1].value, ymin = st->slot[2].value, ymax = st->slot[3].value;
    const double xs = robust_scale(xmin, xmax), ys = robust_scale(ymin, ymax);
    double hs, ht, vs, vt;
    minmax_coef(st->mmv[0], st->mmv[1], 179.0, hs, ht);
    minmax_coef(st->mmv[2], st->mmv[3], 255.0, vs, vt);
    const long q = (long)blockIdx.x * blockDim.x + threadIdx.x, i0 = 4 * q;
    if (i0 >= (long)n) return;
    const int m = (int)(((long)n - i0) < 4 ? ((long)n - i0) : 4);
    double a[4], b[4];
    if (m == 4 && vec) {
        const double2* pa = reinterpret_cast<const double2*>(gx + i0);
        const double2* pb = reinterpret_cast<const double2*>(gy + i0);
        const double2 a0 = pa[0], a1 = pa[1], b0 = pb[0], b1 = pb[1];
        a[0] = a0.x; a[1] = a0.y; a[2] = a1.x; a[3] = a1.y; b[0] = b0.x; b[1] = b0.y; b[2] = b1.x; b[3] = b1.y;
    } else {
        for (int j = 0; j < 4; ++j) { a[j] = j < m ? gx[i0 + j] : 0.0; b[j] = j < m ? gy[i0 + j] : 0.0; }
    }
    unsigned char ox[4], oy[4], oc[12];
    for (int j = 0; j < 4; ++j) {
        ox[j] = robust_u8(a[j], xmin, xs);
        oy[j] = robust_u8(b[j], ymin, ys);
        double half, mag;
        polar_half(a[j], b[j], half, mag);
        hsv_to_rgb(minmax_u8(half, hs, ht), 255, minmax_u8(mag, vs, vt), oc + 3 * j);
    }
    if (m == 4) {
        if (gx_u8) *reinterpret_cast<uchar4*>(gx_u8 + i0) = make_uchar4(ox[0], ox[1], ox[2], ox[3]);
        if (gy_u8) *reinterpret_cast<uchar4*>(gy_u8 + i0) = make_uchar4(oy[0], oy[1], oy[2], oy[3]);
        if (rgb) {
            unsigned int w[3];
            for (int j = 0; j < 3; ++j) w[j] = (unsigned int)oc[4 * j] | ((unsigned int)oc[4 * j + 1] << 8) | ((unsigned int)oc[4 * j + 2] << 16) | ((unsigned int)oc[4 * j + 3] << 24);
            *reinterpret_cast<uint3*>(rgb + 3 * i0) = make_uint3(w[0], w[1], w[2]);
        }
    } else {
        for (int j = 0; j < m; ++j) {
            if (gx_u8) gx_u8[i0 + j] = ox[j];
            if (gy_u8) gy_u8[i0 + j] = oy[j];
            if (rgb) for (int c = 0; c < 3; ++c) rgb[3 * (i0 + j) + c] = oc[3 * j + c];
        }
    }
}

}  // namespace emba
