// emba_amd/csrc/sim_kernels.h — the event simulator (gfx950, wave64): from the samples a sensor pixel sees at consecutive step times to the events it reports.
// The rule: sim_rule.h, include/emba_hip.h (emba_simulate_events), DESIGN.md §18.
//   * samples                    emba_view_kernel (view_kernels.h) as it is, over (frame, pixel) of a chunk of steps, outside pixels marked by its fill
//   * emba_sim_count_kernel      one lane per sensor pixel walks the chunk's frames: sim_frame per step, the number of events per (step, pixel) cell as a
//                                word for dev_scan, the pixel's state behind the chunk, and the wave's sums of positive events, capped and outside cells
//   * emba_sim_emit_kernel       the same walk from the same state in front of the chunk, writing every event at its cell's offset + k: its time, its
//                                (pixel, polarity) word, the low word of its sort key and its own index as the sort's value
//   * emba_sim_hikey_kernel      for chunks longer than 2^32 ns: the high word of the key of the event at every sorted position
//   * emba_sim_gather_kernel     the events in sorted order into the recording: x, y, polarity, t
// The walk is sequential in the frame and, at a few hundred waves, far from filling the chip: what it waits for is the load of the next sample.  Its loop
// therefore takes kSimUnroll frames at a time and issues their loads — coalesced across the pixels of a wave, independent of each other and of the state —
// before the first of them is used; the step times sit at wave-uniform addresses.  64-thread workgroups spread the waves over the compute units.  No LDS,
// no scratch.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sim_rule.h"

namespace emba {

constexpr int kSimThreads = 64;
constexpr int kSimUnroll = 4;

struct SimParams {
    const double* frames;         // [ns + 1, S]: slot 0 is the frame at the chunk's first step time, slot j + 1 the one that ends step j
    const int64_t* step_t;        // the chunk's ns + 1 step times
    int S, ns;
    int first;                    // slot 0 is frame 0 of the recording: every pixel starts unarmed and meets it (else: the state of ref_in / armed_in)
    double c_on, c_off;
    int max_per_step;
    const double* ref_in; const uint8_t* armed_in;      // [S] the pixels' state in front of the chunk
    double* ref_out; uint8_t* armed_out;                // [S] ... and behind it (count)
    uint32_t* cells;              // [ns, S] count: events per cell, out; emit: their exclusive scan, in
    unsigned long long* sums;     // count: [0] positive events [1] capped cells [2] outside cells
    // emit
    int64_t t_base;               // the chunk's first step time
    uint32_t n_total;             // events of the chunk (the scan's total): no write at or behind it
    uint32_t* key; uint32_t* val; // [n_total] low word of t - t_base; the event's index
    int64_t* t; uint32_t* sp;     // [n_total] time; pixel << 1 | polarity
};

// Compiled without contraction, like the rule it runs.
#pragma clang fp contract(off)
template <bool kEmit>
__device__ __forceinline__ void sim_walk(const SimParams& p)
{
    const int s_raw = (int)blockIdx.x * kSimThreads + (int)threadIdx.x;
    const bool live = s_raw < p.S;
    const size_t s = live ? s_raw : p.S - 1, S = p.S;      // (a lane past the sensor walks the last pixel and stores nothing)
    unsigned int n_pos = 0, n_cap = 0, n_out = 0;
    auto emit = [&](int k, bool up, int64_t t, uint32_t at) {
        if constexpr (kEmit) {
            const uint32_t i = at + (uint32_t)k;
            if (live && i < p.n_total) { p.t[i] = t; p.sp[i] = (uint32_t)s << 1 | (up ? 1u : 0u); p.key[i] = (uint32_t)(uint64_t)(t - p.t_base); p.val[i] = i; }
        } else n_pos += up ? 1u : 0u;
    };
    double prev = p.frames[s];
    SimPixel px{0.0, false};
    if (p.first) {
        const bool inside = !sim_marked_outside(prev);
        n_out += inside ? 0u : 1u;
        (void)sim_frame(&px, inside, prev, prev, 0, 1, p.c_on, p.c_off, p.max_per_step, [](int, bool, int64_t) {});
    } else { px.ref = p.ref_in[s]; px.armed = p.armed_in[s] != 0; }
    for (int j0 = 0; j0 < p.ns; j0 += kSimUnroll) {
        double v[kSimUnroll];
        uint32_t at[kSimUnroll];
#pragma unroll
        for (int u = 0; u < kSimUnroll; ++u) {      // the loads of kSimUnroll frames, before any of them is used
            const size_t j = (size_t)min(j0 + u, p.ns - 1);
            v[u] = p.frames[(j + 1) * S + s];
            at[u] = kEmit ? p.cells[j * S + s] : 0u;
        }
#pragma unroll
        for (int u = 0; u < kSimUnroll; ++u) {
            const int j = j0 + u;
            if (j < p.ns) {      // (uniform over the launch)
                const int64_t t_prev = p.step_t[j], d = p.step_t[j + 1] - t_prev;
                const bool inside = !sim_marked_outside(v[u]);
                const uint32_t a = at[u];
                const SimStep r = sim_frame(&px, inside, prev, v[u], t_prev, d, p.c_on, p.c_off, p.max_per_step, [&](int k, bool up, int64_t t) { emit(k, up, t, a); });
                if constexpr (!kEmit) {
                    n_out += inside ? 0u : 1u;
                    n_cap += r.capped ? 1u : 0u;
                    if (live) p.cells[(size_t)j * S + s] = (uint32_t)r.n;
                }
                prev = v[u];
            }
        }
    }
    if constexpr (!kEmit) {
        if (live) { p.ref_out[s] = px.ref; p.armed_out[s] = px.armed ? 1 : 0; }
        if (!live) n_pos = n_cap = n_out = 0;
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) { n_pos += __shfl_xor(n_pos, o); n_cap += __shfl_xor(n_cap, o); n_out += __shfl_xor(n_out, o); }
        if ((threadIdx.x & 63) == 0) {
            if (n_pos) atomicAdd(p.sums, (unsigned long long)n_pos);
            if (n_cap) atomicAdd(p.sums + 1, (unsigned long long)n_cap);
            if (n_out) atomicAdd(p.sums + 2, (unsigned long long)n_out);
        }
    }
}

__global__ __launch_bounds__(kSimThreads) void emba_sim_count_kernel(SimParams p) { sim_walk<false>(p); }
__global__ __launch_bounds__(kSimThreads) void emba_sim_emit_kernel(SimParams p) { sim_walk<true>(p); }
#pragma clang fp contract(fast)

// key[i] = the high word of t[val[i]] - t_base: the second sort's keys, in the order the first one left
__global__ __launch_bounds__(256) void emba_sim_hikey_kernel(const uint32_t* __restrict__ val, const int64_t* __restrict__ t, int64_t t_base, long n, uint32_t* __restrict__ key)
{
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) key[i] = (uint32_t)((uint64_t)(t[val[i]] - t_base) >> 32);
}

// the recording's next n events: position i takes the chunk's event val[i]
__global__ __launch_bounds__(256) void emba_sim_gather_kernel(const uint32_t* __restrict__ val, const int64_t* __restrict__ t, const uint32_t* __restrict__ sp, long n, int sw,
                                                              uint16_t* __restrict__ ox, uint16_t* __restrict__ oy, uint8_t* __restrict__ opol, int64_t* __restrict__ ot)
{
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const uint32_t j = val[i], w = sp[j], pix = w >> 1;
    ox[i] = (uint16_t)(pix % (uint32_t)sw); oy[i] = (uint16_t)(pix / (uint32_t)sw); opol[i] = (uint8_t)(w & 1u); ot[i] = t[j];
}

}  // namespace emba
