// emba_amd/csrc/mosaic_rule.h — the mosaic of intensity frames on the panorama and the gradient map made from it (mosaic_host.h, mosaic_kernels.h), as
// functions of plain values: the argument checks, the bound that keeps the integer sums exact, the weighted mean of a cell, the log-intensity of a mean
// (the inverse of view_u8's tone) and the backward differences of a plane with holes.  The vote itself is pano_vote of panorama_rule.h, as it is; the chunks
// are view_chunk_frames(S, 1) of view_rule.h.
// emba_amd.io.mosaic_votes / mosaic_mean / mosaic_log / gradient_from_plane are the same rules in numpy; include/emba_hip.h (emba_mosaic_frames,
// emba_mosaic_get, emba_mosaic_map) states them in words.
//
// No HIP in here: plain C++17, so that tests/cpp/mosaic_rule_test.cpp checks it on a CPU in milliseconds.  mosaic_mean, mosaic_log and mosaic_gradient are
// compiled for the host and for the device: the kernels and the CPU test run the same functions.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <cmath>

#include "panorama_rule.h"
#include "view_rule.h"

namespace emba {

// ---- exactness: a frame pixel votes 256 units of weight and at most 255 * 256 = 65 280 units of value.  With fewer than 2^36 votes accumulated,
// sum_v <= 65 280 * votes < 2^53 (and sum_w <= 256 * votes < 2^44): both convert to double exactly, and the mean is one IEEE division.
constexpr uint64_t kMosaicMaxVotes = (uint64_t)1 << 36;
// the votes after F frames of S pixels more on top of `have`, or kMosaicMaxVotes where that would reach the bound (also where F * S does not fit 64 bits)
inline uint64_t mosaic_votes_after(uint64_t have, uint64_t F, uint64_t S)
{
    if (have >= kMosaicMaxVotes) return kMosaicMaxVotes;
    if (F && S && F > (kMosaicMaxVotes - 1) / S) return kMosaicMaxVotes;
    const uint64_t add = F * S;
    return add >= kMosaicMaxVotes - have ? kMosaicMaxVotes : have + add;
}

// ---- argument checks (the order the C ABI reports them in)
enum class MosaicArgStatus { ok, frames_null, times_null, knots_null, too_few_knots, bad_dt, too_many_frames, too_many_votes };
inline MosaicArgStatus mosaic_args_ok(bool have_frames, bool have_times, bool have_knots, size_t F, size_t S, uint64_t votes_have, int K, int64_t dt_ns)
{
    if (F && !have_frames) return MosaicArgStatus::frames_null;
    if (F && !have_times) return MosaicArgStatus::times_null;
    if (F && !have_knots) return MosaicArgStatus::knots_null;
    if (K < 2) return MosaicArgStatus::too_few_knots;
    if (dt_ns <= 0) return MosaicArgStatus::bad_dt;
    if (F > 0x7FFFFFFFull) return MosaicArgStatus::too_many_frames;
    if (mosaic_votes_after(votes_have, F, S) >= kMosaicMaxVotes) return MosaicArgStatus::too_many_votes;
    return MosaicArgStatus::ok;
}
enum class MosaicToneStatus { ok, bad_min_weight, not_finite, hi_not_above_lo };
inline MosaicToneStatus mosaic_get_args_ok(uint64_t min_weight, double fill)
{
    if (min_weight < 1) return MosaicToneStatus::bad_min_weight;
    if (!std::isfinite(fill)) return MosaicToneStatus::not_finite;
    return MosaicToneStatus::ok;
}
inline MosaicToneStatus mosaic_map_args_ok(uint64_t min_weight, double lo, double hi, double eps)
{
    if (min_weight < 1) return MosaicToneStatus::bad_min_weight;
    if (!(std::isfinite(lo) && std::isfinite(hi) && std::isfinite(eps))) return MosaicToneStatus::not_finite;
    if (!(hi > lo)) return MosaicToneStatus::hi_not_above_lo;
    return MosaicToneStatus::ok;
}

// ---- the mean of a cell: covered where sum_w >= min_weight (min_weight >= 1; 256 is one whole pixel's worth); there sum_v / sum_w, both converted
// exactly, one division; elsewhere `fill`.
EMBA_RULE_HD inline bool mosaic_covered(uint64_t sum_w, uint64_t min_weight) { return sum_w >= min_weight; }
EMBA_RULE_HD inline double mosaic_mean(uint64_t sum_w, uint64_t sum_v, uint64_t min_weight, double fill)
{
    return mosaic_covered(sum_w, min_weight) ? (double)sum_v / (double)sum_w : fill;
}

// ---- the log-intensity of a covered cell's mean: I = lo + mean (hi - lo) / 255 — the inverse of view_u8's tone, in this order and without contraction —
// and L = I (take_log == 0: the bytes were log intensity already) or L = log(I + eps).  false: the cell is not covered, or I + eps is not positive (a NaN
// too), and *L is left alone.
EMBA_RULE_HD inline bool mosaic_log(double mean, bool covered, double lo, double hi, double eps, int take_log, double* L)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    if (!covered) return false;
    const double I = lo + mean * (hi - lo) / 255.0;
    if (!take_log) { *L = I; return true; }
    const double a = I + eps;
    if (!(a > 0.0)) return false;
    *L = log(a);
    return true;
}

// ---- the gradient map of a plane with holes: backward differences, the field whose divergence (poisson_rule.h) is the 5-point operator.
//     Gx[i][j] = L[i][j] - L[i][(j - 1) mod W]   where both cells are covered, else 0
//     Gy[i][j] = L[i][j] - L[i - 1][j]           where both are covered and i >= 1, else 0
EMBA_RULE_HD inline void mosaic_gradient(const double* L, const uint8_t* covered, int W, int i, int j, double* gx, double* gy)
{
    const size_t c = (size_t)i * (size_t)W + (size_t)j, left = (size_t)i * (size_t)W + (size_t)(j ? j - 1 : W - 1);
    *gx = *gy = 0.0;
    if (!covered[c]) return;
    if (covered[left]) *gx = L[c] - L[left];
    if (i >= 1 && covered[c - (size_t)W]) *gy = L[c] - L[c - (size_t)W];
}

}  // namespace emba
