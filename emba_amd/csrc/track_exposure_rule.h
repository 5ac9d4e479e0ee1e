// emba_amd/csrc/track_exposure_rule.h — the frame tracker with a per-frame exposure (track_exposure_host.h, track_exposure_kernels.h), as functions of plain
// values: a tracked frame carries (q_f, a_f, b_f); gain and bias are estimated with the rotation at every level of the schedule, and a tracked frame votes its
// compensated bytes.  Here are the argument checks behind track_rule.h's, one pixel of a frame against a level's two integer sums under the frame's gain and
// bias, and the start of a frame's gain and bias.  The cell, the mask, the four means, the sample with its gradient and the classes are track_rule.h's and
// align_rule.h's; the term, its 21 sums, the step and the compensated byte are exposure_rule.h's; the prediction of the rotation, the overlap and the verdict
// are track_rule.h's: they are called here, not restated.
// emba_amd.io.track_exposure_terms / track_votes_exposure / track_frames_exposure are the same rules in numpy; include/emba_hip.h
// (emba_frames_track_exposure, emba_track_exposure_eval) states them in words.
//
// No HIP in here: plain C++17, so that tests/cpp/track_exposure_rule_test.cpp checks it on a CPU in milliseconds.  Everything below the argument checks is
// compiled for the host and for the device: the kernels and the CPU test run the same functions.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/emba_hip.h"      // emba_track_exposure_settings
#include "align_rule.h"
#include "exposure_rule.h"
#include "mosaic_rule.h"
#include "track_rule.h"

namespace emba {

// ---- argument checks behind track_args_ok, in the order the C ABI reports them in
enum class TrackExposureArgStatus { ok, bad_bounds, bad_estimate };
inline TrackExposureArgStatus track_exposure_args_ok(const emba_track_exposure_settings& s)
{
    if (!exposure_bounds_ok(s.gain_min, s.gain_max)) return TrackExposureArgStatus::bad_bounds;
    if (!exposure_estimate_ok(s.estimate)) return TrackExposureArgStatus::bad_estimate;
    return TrackExposureArgStatus::ok;
}

// ---- one pixel of a frame against a level under the frame's gain and bias: track_pixel up to the sample, expression for expression; then I0 = v (the
// plane is in byte units), r = val - (a * I0 + b) (multiply, then add, without contraction), its weight and cost, and g from the level's J23.  With a = 1,
// b = 0 every member is track_pixel's.
EMBA_RULE_HD inline int track_exposure_pixel(const uint64_t* sum_w, const uint64_t* sum_v, int W, int H, double pm_x, double pm_y, const double* J23, unsigned v,
                                             uint64_t min_weight, double gain, double bias, bool skip_zero, double huber_k, ExposureTerm* t)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    t->r = 0.0;
    AlignCell c;
    if (!align_cell(W, H, pm_x, pm_y, &c)) return kAlignOutside;
    const size_t i00 = c.row0 + (size_t)c.c0, i01 = c.row0 + (size_t)c.c1, i10 = i00 + (size_t)W, i11 = i01 + (size_t)W;
    const uint64_t w00 = sum_w[i00], w01 = sum_w[i01], w10 = sum_w[i10], w11 = sum_w[i11];
    if (!(mosaic_covered(w00, min_weight) && mosaic_covered(w01, min_weight) && mosaic_covered(w10, min_weight) && mosaic_covered(w11, min_weight))) return kAlignMasked;
    if (skip_zero && v == 0) return kAlignSkipped;
    const double P[4] = {mosaic_mean(w00, sum_v[i00], min_weight, 0.0), mosaic_mean(w01, sum_v[i01], min_weight, 0.0), mosaic_mean(w10, sum_v[i10], min_weight, 0.0),
                         mosaic_mean(w11, sum_v[i11], min_weight, 0.0)};
    const AlignCell local{0, 0, 1, c.ax, c.ay};      // the four means as a plane of 2 x 2
    double val, gx, gy;
    align_sample_cell(P, 2, local, &val, &gx, &gy);
    t->I0 = (double)v;
    const double scaled = gain * t->I0;
    t->r = val - (scaled + bias);
    align_huber(t->r, huber_k, &t->w, &t->rho);
    for (int j = 0; j < 3; ++j) t->g[j] = gx * J23[j] + gy * J23[3 + j];
    return kAlignUsed;
}

// ---- the start of a frame's gain and bias: those of the last tracked frame in front of its batch (the anchor counts, with a = 1, b = 0), whether the
// rotation is predicted or not; exposure is not extrapolated.  status [f0], gain [f0], bias [f0]: the frames in front of the batch.  false (a = 1, b = 0):
// none of them is tracked.
EMBA_RULE_HD inline bool track_exposure_start(const int32_t* status, const double* gain, const double* bias, long f0, double* a, double* b)
{
    long k = f0 - 1;
    while (k >= 0 && !track_votes(status[k])) --k;
    if (k < 0) { *a = 1.0; *b = 0.0; return false; }
    *a = gain[k]; *b = bias[k];
    return true;
}

}  // namespace emba
