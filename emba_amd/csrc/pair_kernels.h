// emba_amd/csrc/pair_kernels.h — one intensity frame aligned to another (gfx950, wave64): per pair of frames the normal equations of a 3-DoF photometric
// alignment of frame i's pixels to frame j's bytes.
// The rules: pair_rule.h, align_rule.h, include/emba_hip.h (emba_frames_pair_eval, emba_frames_pair_align), DESIGN.md §26.
//   * emba_frames_pair_eval_kernel   one lane per source pixel, the pair in blockIdx.y, kFrameThreads lanes per workgroup.  The pair's frames, rotation and
//                                    exposure are wave-uniform loads; a pair whose status is final lets the whole workgroup leave; then the source byte,
//                                    pair_term (the turned bearing projected through the plumb_bob model, four byte gathers from frame j, the term), and
//                                    frame_sum_tail<10> (frame_kernels.h): the workgroup writes partial[pair][workgroup][12]
// That record is the alignment's, so emba_frames_align_reduce_kernel and emba_frames_align_step_kernel (align_kernels.h) run behind it as they are.
// The target frame is gathered through the caches, not staged in LDS: a pixel reads five bytes and spends some 150 fp64 operations, a whole 240 x 180
// frame is 43 KB — it stays in the 4 MB L2 of the XCD its workgroups run on, and a workgroup's patch of it (256 pixels, a few rows) in the 32 KB L1 — while a
// staged patch would need the workgroup's bounding box first: a second projection pass, a min / max reduction and a barrier, for a box that a roll about
// the optical axis makes as large as the frame.  DESIGN.md §26 has the register and LDS figures that go with this form.
// 384 B of LDS, no scratch.  No floating-point atomic: the same inputs give the same bits.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "align_rule.h"
#include "frame_kernels.h"
#include "pair_rule.h"

namespace emba {

struct PairEvalParams {
    const double* lut;            // bearing vector per sensor pixel [S, 3]
    const uint8_t* frames;        // the whole sequence [F, S]
    const int32_t* pairs;         // the chunk's (i, j) [np, 2]: source frame, target frame; both below F (pair_args_ok)
    const double* q;              // the rotation each pair is evaluated at [np, 4]
    const double* gain;           // [np] or nullptr (1)
    const double* bias;           // [np] or nullptr (0)
    const int32_t* status;        // [np] or nullptr: a pair whose status is not EMBA_ALIGN_RUNNING is left out
    int S, sw, sh;
    PairCamera cam;
    double huber_k;
    int skip_zero;
    double* partial;              // [np, gridDim.x, frame_partial(kAlignSums)]
    double* uv;                   // [np, S, 2] or nullptr
    double* resid;                // [np, S] or nullptr
};

#pragma clang fp contract(off)
__global__ __launch_bounds__(kFrameThreads) void emba_frames_pair_eval_kernel(PairEvalParams p)
{
    constexpr int N = kAlignSums;
    const size_t pr = blockIdx.y;
    if (p.status && p.status[pr] != EMBA_ALIGN_RUNNING) return;      // (the whole workgroup: the pair is blockIdx.y)
    const size_t fi = (size_t)p.pairs[2 * pr], fj = (size_t)p.pairs[2 * pr + 1];
    const double Q[4] = {p.q[4 * pr], p.q[4 * pr + 1], p.q[4 * pr + 2], p.q[4 * pr + 3]};
    const double a = p.gain ? p.gain[pr] : 1.0, b = p.bias ? p.bias[pr] : 0.0;
    const int s = (int)blockIdx.x * kFrameThreads + (int)threadIdx.x;
    double acc[N];
    unsigned int cnt[4] = {0, 0, 0, 0};
#pragma unroll
    for (int k = 0; k < N; ++k) acc[k] = 0.0;
    if (s < p.S) {
        const unsigned int v = p.frames[fi * (size_t)p.S + (size_t)s];
        const size_t o = pr * (size_t)p.S + (size_t)s;
        double uv[2];
        AlignTerm t;
        const int cls = pair_term(p.lut, s, Q, p.cam, p.frames + fj * (size_t)p.S, p.sw, p.sh, v, a, b, p.skip_zero != 0, p.huber_k, uv, &t);
        if (p.uv) { p.uv[2 * o] = uv[0]; p.uv[2 * o + 1] = uv[1]; }
        if (p.resid) p.resid[o] = t.r;
        if (cls == kAlignUsed) align_accumulate(t, acc);
#pragma unroll
        for (int k = 0; k < 4; ++k) cnt[k] = cls == k ? 1u : 0u;
    }
    frame_sum_tail<N>(acc, cnt, p.partial, pr);
}
#pragma clang fp contract(fast)

}  // namespace emba
