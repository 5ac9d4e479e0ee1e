// emba_amd/csrc/sim_rule.h — the event simulator (sim_host.h, sim_kernels.h), as functions of plain values: what one sensor pixel does with the sample of one
// more step time — disarm, arm, or emit the events of the brightness change since its reference — and the cut of F steps into chunks.
// emba_amd.io.simulate_events is the same rule in numpy; include/emba_hip.h (emba_simulate_events) states it in words; DESIGN.md §18.
//
// No HIP in here: plain C++17, so that tests/cpp/sim_rule_test.cpp checks it on a CPU in milliseconds.  sim_step, sim_frame and sim_marked_outside are
// compiled for the host and for the device: the kernels and the CPU test run the same functions.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <cmath>

#include "view_rule.h"      // EMBA_RULE_HD; the chunks are cut by view_chunk_count / view_chunk, over steps

namespace emba {

constexpr uint64_t kSimMaxEvents = 0xFFFFFFFEull;          // the limit of the 32-bit scan and sort: what max_events = 0 stands for
constexpr int64_t kSimMaxSpan = (int64_t)1 << 52;          // step_t[F] - step_t[0] stays below it: every step length d is exact as a double
constexpr int kSimMaxPerStep = 255;

// ---- chunks: the device holds the samples of one chunk of steps at a time, plus the frame in front of it — at most 32 MiB of fp64 samples and 65 534 steps
// (the frame is the view kernel's grid y index, and the first chunk renders one frame more than it has steps), but always one step.  Step j (0 <= j < F) is the interval [step_t[j], step_t[j + 1]); consecutive chunks
// share the frame between them.  At 32 MiB a chunk has at most 2^22 (step, pixel) cells of at most 255 events: their offsets fit 32 bits; a sensor larger
// than that has one step per chunk and sim_sensor_fits says whether its S * 255 events still do.
constexpr size_t kSimChunkMaxBytes = (size_t)32 << 20;
constexpr size_t kSimChunkMaxSteps = 65534;
inline size_t sim_chunk_steps(size_t S)      // steps per chunk for frames of S fp64 samples
{
    const size_t frame = S * sizeof(double), fit = frame ? kSimChunkMaxBytes / frame : kSimChunkMaxSteps;
    return fit < 1 ? 1 : (fit > kSimChunkMaxSteps ? kSimChunkMaxSteps : fit);
}
inline bool sim_sensor_fits(size_t S) { return (uint64_t)S * kSimMaxPerStep <= kSimMaxEvents; }

// F + 1 step times, strictly increasing, spanning less than 2^52 ns
inline bool sim_steps_ok(const int64_t* step_t, size_t F)
{
    if (!view_edges_ok(step_t, F)) return false;
    return (uint64_t)step_t[F] - (uint64_t)step_t[0] < (uint64_t)kSimMaxSpan;
}
inline bool sim_threshold_ok(double c) { return std::isfinite(c) && c > 0.0; }

// ---- the mark of an outside sample.  The simulator renders its samples with emba_view_kernel as it is, whose only word on a pixel without a sample is the
// caller's `fill`: it passes this quiet NaN and knows the pixel by its bits.  (Arithmetic on the plane never makes this payload: a sample is outside here
// exactly where emba_render_views counts it, unless the plane itself holds these 64 bits.)
constexpr uint64_t kSimOutsideBits = 0x7FF8000053494D31ull;
EMBA_RULE_HD inline double sim_outside_mark() { double v; const uint64_t u = kSimOutsideBits; __builtin_memcpy(&v, &u, 8); return v; }
EMBA_RULE_HD inline bool sim_marked_outside(double v) { uint64_t u; __builtin_memcpy(&u, &v, 8); return u == kSimOutsideBits; }

struct SimPixel { double ref; bool armed; };      // what a pixel carries from step to step (and from chunk to chunk)
struct SimStep { int n; bool capped; };           // events emitted in this step; the cap ended the loop (the condition still held after max_per_step events)

// ---- one step of an armed pixel whose samples at both ends are inside: prev = V_{f-1}, cur = V_f, the step is [t_prev, t_prev + d).  While
// fabs(cur - ref) >= C (C = c_on, sgn = +1 where cur - ref > 0, else C = c_off, sgn = -1), at most max_per_step times: ref = ref + sgn C;
// frac = (ref - prev) / (cur - prev), 0 where it is not >= 0 (a NaN too), 1 where it is > 1; off = (int64)(frac * (double)d), at most d - 1; the event
// (sgn > 0, t_prev + off) goes to emit(k, positive, t) with k the number of events before it.  Every operation in fp64, in this order, without contraction.
template <class Emit>
EMBA_RULE_HD inline SimStep sim_step(double* ref, double prev, double cur, int64_t t_prev, int64_t d, double c_on, double c_off, int max_per_step, Emit&& emit)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double dd = (double)d, span = cur - prev;
    for (int n = 0;; ++n) {
        const double diff = cur - *ref;
        const bool up = diff > 0.0;
        const double C = up ? c_on : c_off;
        if (!(fabs(diff) >= C)) return SimStep{n, false};
        if (n == max_per_step) return SimStep{n, true};
        *ref = up ? *ref + C : *ref - C;
        double frac = (*ref - prev) / span;
        if (!(frac >= 0.0)) frac = 0.0;
        else if (frac > 1.0) frac = 1.0;
        int64_t off = (int64_t)(frac * dd);
        if (off > d - 1) off = d - 1;
        emit(n, up, t_prev + off);
    }
}

// ---- one more sample of a pixel: outside disarms it; inside and not armed takes the sample as the reference and emits nothing; inside and armed (so the
// sample before was inside as well) is sim_step.  For f = 0 there is no step: the caller passes any prev, t_prev and d, and an unarmed pixel.
template <class Emit>
EMBA_RULE_HD inline SimStep sim_frame(SimPixel* px, bool inside, double prev, double cur, int64_t t_prev, int64_t d, double c_on, double c_off, int max_per_step,
                                      Emit&& emit)
{
    if (!inside) { px->armed = false; return SimStep{0, false}; }
    if (!px->armed) { px->ref = cur; px->armed = true; return SimStep{0, false}; }
    return sim_step(&px->ref, prev, cur, t_prev, d, c_on, c_off, max_per_step, emit);
}

// ---- the sort of a chunk's events by time: keys are t minus the chunk's first step time, below `span` = the chunk's length in ns.  One pass of the 32-bit
// stable sort on that many bits where span <= 2^32, else the low 32 bits first and the high ones after.
struct SimSortPlan { int lo_bits, hi_bits; };      // hi_bits 0: one sort
inline SimSortPlan sim_sort_plan(uint64_t span)
{
    auto bits = [](uint64_t n_values) { int b = 1; while (b < 64 && ((uint64_t)1 << b) < n_values) ++b; return b; };
    if (span <= ((uint64_t)1 << 32)) return SimSortPlan{bits(span), 0};
    return SimSortPlan{32, bits(((span - 1) >> 32) + 1)};
}

}  // namespace emba
