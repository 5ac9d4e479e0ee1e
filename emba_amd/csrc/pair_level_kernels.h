// emba_amd/csrc/pair_level_kernels.h — the pair alignment coarse to fine, with the pair's exposure estimated (gfx950, wave64): the pyramid of the sensor
// frames and, per pair and level, the normal equations of the 5-parameter photometric alignment (rotation, gain, bias) of frame i's level pixels to frame j's.
// The rules: pair_level_rule.h, pair_rule.h, exposure_rule.h, include/emba_hip.h (emba_frames_pair_level_eval, emba_frames_pair_align_levels), DESIGN.md §27.
//   * emba_frames_pair_reduce_kernel         the resident sequence [F, S] into the bytes of every level of a mask, one workgroup per 128 x 128 tile of a frame:
//                                            every frame byte is read once, into the box sums of level 1 in LDS; each level above is the sum of four boxes of
//                                            the level below (integers: sums of sums are exact), ping-pong between two LDS arrays; a level of the mask is
//                                            rounded from its own sum and stored.  "The box holds a zero byte" rides in bit 31 of a box.  32 KB of LDS.
//   * emba_pair_level_lut_kernel             one lane per level pixel: pair_level_bearing of the context's table
//   * emba_frames_pair_exposure_eval_kernel  emba_frames_pair_eval_kernel's shape — one lane per level pixel, the pair in blockIdx.y, kFrameThreads lanes per
//                                            workgroup, wave-uniform pair loads, a pair whose status is final leaves — with pair_exposure_term and
//                                            frame_sum_tail<21>: the workgroup writes partial[pair][workgroup][23].  That record is the exposure stage's, so
//                                            emba_frames_exposure_reduce_kernel and emba_frames_exposure_step_kernel (exposure_kernels.h) run behind it as
//                                            they are.  The target level is gathered through the caches, as the 10-sum kernel gathers the frame.
//   * emba_pair_level_handover_kernel        one lane per pair, behind the loop of a level: a pair that is still in the schedule records the level's status and
//                                            iterations, takes the level's accepted state as its result, and starts the next level from it; a pair whose
//                                            level ended degenerate leaves the schedule: its flag gates the first evaluation of every later level, and its
//                                            evaluation is zeroed, so the unchanged step kernel ends it there at once and it costs no evaluation
// No floating-point atomic and no grid-wide synchronisation: the same inputs give the same bits.  No scratch.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "exposure_rule.h"
#include "frame_kernels.h"
#include "pair_level_rule.h"

namespace emba {

constexpr int kPairTile = 1 << kPairMaxLevel;      // 128: a multiple of every level's box

struct PairReduceParams {
    const uint8_t* frames;        // [F, S]
    uint8_t* out[kPairMaxLevel + 1];      // out[l]: [F, S_l] for the levels of the mask, l >= 1
    long f0, nf;                  // the frames of this launch
    int sw, sh, tiles_x, tiles;   // tiles = tiles_x * tiles_y
    int top;                      // the highest level of the mask
    unsigned mask;                // bit l: level l is stored
    int skip_zero;
};

__global__ __launch_bounds__(kFrameThreads) void emba_frames_pair_reduce_kernel(PairReduceParams p)
{
    __shared__ uint32_t bx[2][(kPairTile / 2) * (kPairTile / 2)];      // (the odd levels in [1], the even ones in [0])
    const long f = p.f0 + (long)(blockIdx.x / (unsigned)p.tiles);
    const int tile = (int)(blockIdx.x % (unsigned)p.tiles);
    const int tx = tile % p.tiles_x, ty = tile / p.tiles_x;
    const size_t S = (size_t)p.sw * (size_t)p.sh;
    const uint8_t* fr = p.frames + (size_t)f * S;
    for (int l = 1; l <= p.top; ++l) {
        const int side = kPairTile >> l;                      // the tile's boxes of level l per row
        const int wl = p.sw >> l, hl = p.sh >> l;
        uint32_t* cur = bx[l & 1];
        const uint32_t* below = bx[(l - 1) & 1];
        for (int i = (int)threadIdx.x; i < side * side; i += kFrameThreads) {
            const int bxl = i % side, byl = i / side;
            const int X = tx * side + bxl, Y = ty * side + byl;
            if (X >= wl || Y >= hl) continue;               // (a box of level l that exists has its four boxes of level l - 1: 2 X + 1 < 2 wl <= sw >> (l - 1))
            uint32_t box;
            if (l == 1) {
                const uint8_t* r0 = fr + (size_t)(2 * Y) * (size_t)p.sw + (size_t)(2 * X);
                const uint8_t* r1 = r0 + p.sw;
                box = pair_box_join(pair_box_of_byte(r0[0]), pair_box_of_byte(r0[1]), pair_box_of_byte(r1[0]), pair_box_of_byte(r1[1]));
            } else {
                const uint32_t* q0 = below + (2 * byl) * (2 * side) + 2 * bxl;
                box = pair_box_join(q0[0], q0[1], q0[2 * side], q0[2 * side + 1]);
            }
            cur[i] = box;
            if (p.mask >> l & 1u) p.out[l][(size_t)f * ((size_t)wl * (size_t)hl) + (size_t)Y * (size_t)wl + (size_t)X] = (uint8_t)pair_box_byte(box, l, p.skip_zero != 0);
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(kFrameThreads) void emba_pair_level_lut_kernel(const double* lut, int sw, int l, int wl, int Sl, double* out)
{
    const int s = (int)blockIdx.x * kFrameThreads + (int)threadIdx.x;
    if (s >= Sl) return;
    double b[3];
    pair_level_bearing(lut, sw, s % wl, s / wl, l, b);
    out[3 * (size_t)s] = b[0]; out[3 * (size_t)s + 1] = b[1]; out[3 * (size_t)s + 2] = b[2];
}

struct PairLevelEvalParams {
    const double* lut;            // the level's bearing per level pixel [S, 3]
    const uint8_t* frames;        // the level's bytes of the whole sequence [F, S]
    const int32_t* pairs;         // the chunk's (i, j) [np, 2]: source frame, target frame; both below F (pair_args_ok)
    const double* q;              // the rotation each pair is evaluated at [np, 4]
    const double* gain;           // ... and its relative gain and bias [np]
    const double* bias;
    const int32_t* status;        // [np] or nullptr: a pair whose status is not EMBA_ALIGN_RUNNING is left out
    int S, sw, sh;                // the level's
    PairCamera cam;               // the level's
    double huber_k;
    int skip_zero;
    double* partial;              // [np, gridDim.x, frame_partial(kExposureSums)]
    double* uv;                   // [np, S, 2] or nullptr
    double* resid;                // [np, S] or nullptr
};

#pragma clang fp contract(off)
__global__ __launch_bounds__(kFrameThreads) void emba_frames_pair_exposure_eval_kernel(PairLevelEvalParams p)
{
    constexpr int N = kExposureSums;
    const size_t pr = blockIdx.y;
    if (p.status && p.status[pr] != EMBA_ALIGN_RUNNING) return;      // (the whole workgroup: the pair is blockIdx.y)
    const size_t fi = (size_t)p.pairs[2 * pr], fj = (size_t)p.pairs[2 * pr + 1];
    const double Q[4] = {p.q[4 * pr], p.q[4 * pr + 1], p.q[4 * pr + 2], p.q[4 * pr + 3]};
    const double a = p.gain[pr], b = p.bias[pr];
    const int s = (int)blockIdx.x * kFrameThreads + (int)threadIdx.x;
    double acc[N];
    unsigned int cnt[4] = {0, 0, 0, 0};
#pragma unroll
    for (int k = 0; k < N; ++k) acc[k] = 0.0;
    if (s < p.S) {
        const unsigned int v = p.frames[fi * (size_t)p.S + (size_t)s];
        const size_t o = pr * (size_t)p.S + (size_t)s;
        double uv[2];
        ExposureTerm t;
        const int cls = pair_exposure_term(p.lut, s, Q, p.cam, p.frames + fj * (size_t)p.S, p.sw, p.sh, v, a, b, p.skip_zero != 0, p.huber_k, uv, &t);
        if (p.uv) { p.uv[2 * o] = uv[0]; p.uv[2 * o + 1] = uv[1]; }
        if (p.resid) p.resid[o] = t.r;
        if (cls == kAlignUsed) exposure_accumulate(t, acc);
#pragma unroll
        for (int k = 0; k < 4; ++k) cnt[k] = cls == k ? 1u : 0u;
    }
    frame_sum_tail<N>(acc, cnt, p.partial, pr);
}
#pragma clang fp contract(fast)

// The result of a chunk's pairs over the schedule, one array per member; the loop's state of the level that has just ended is `q` ... `n0`.
struct PairHandoverParams {
    long np;
    int k, n;                     // the entry of the schedule that has ended, of n
    const double *q, *gain, *bias, *sums, *cost0;
    const unsigned long long *counts, *n0;
    const int32_t *status, *iters;
    double *q_trial, *gain_trial, *bias_trial;      // where the next level starts
    int32_t* out_of;              // [np]: not 0 once a level of the pair has ended degenerate (zeroed in front of the first level)
    double* esums;                // the evaluation the next level's first step reads, [np, 21] and [np, 4]: zeroed for a pair that leaves the schedule
    unsigned long long* ecounts;
    double *r_q, *r_gain, *r_bias, *r_sums, *r_cost0;
    unsigned long long *r_counts, *r_n0;
    int32_t *r_status, *r_iters, *r_level_status, *r_level_iters;      // r_iters: summed over the levels; the last two [np, n], zeroed in front of the first level
};

__global__ __launch_bounds__(64) void emba_pair_level_handover_kernel(PairHandoverParams p)
{
    const long f = (long)blockIdx.x * 64 + threadIdx.x;
    if (f >= p.np || p.out_of[f]) return;
    const int32_t st = p.status[f], it = p.iters[f];
#pragma unroll
    for (int i = 0; i < 4; ++i) { p.r_q[4 * f + i] = p.q[4 * f + i]; p.r_counts[4 * f + i] = p.counts[4 * f + i]; p.q_trial[4 * f + i] = p.q[4 * f + i]; }
#pragma unroll
    for (int i = 0; i < kExposureSums; ++i) p.r_sums[(size_t)kExposureSums * f + i] = p.sums[(size_t)kExposureSums * f + i];
    p.r_gain[f] = p.gain_trial[f] = p.gain[f];
    p.r_bias[f] = p.bias_trial[f] = p.bias[f];
    p.r_status[f] = st;
    p.r_iters[f] = (p.k ? p.r_iters[f] : 0) + it;
    p.r_level_status[(size_t)p.n * f + p.k] = st;
    p.r_level_iters[(size_t)p.n * f + p.k] = it;
    if (!p.k) { p.r_cost0[f] = p.cost0[f]; p.r_n0[f] = p.n0[f]; }
    if (pair_level_hands_on(st)) return;
    // the pair leaves the schedule: out_of gates the first evaluation and its reduction at every later level, so the step kernel there makes the pair's state
    // from this evaluation of no pixels and ends it at once (n < min_pixels); it is never evaluated again
    p.out_of[f] = 1;
#pragma unroll
    for (int i = 0; i < kExposureSums; ++i) p.esums[(size_t)kExposureSums * f + i] = 0.0;
#pragma unroll
    for (int i = 0; i < 4; ++i) p.ecounts[4 * f + i] = 0;
}

}  // namespace emba
