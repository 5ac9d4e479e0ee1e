// emba_amd/csrc/refit_rule.h — tracked frames refitted against the mosaic of the other frames (refit_host.h, refit_kernels.h), as functions of plain values:
// the argument checks behind the trackers', the value a vote is taken out with, the order a sweep visits its batches in, the start of a frame (its own
// values, or an interpolation across lost frames), the code a frame ends a sweep with, and the rotation change a sweep is measured by.  The batches, the
// prediction formula, the pixel, the step, the compensated byte, the overlap and the verdict are track_rule.h's, track_exposure_rule.h's and
// exposure_rule.h's: they are called here, not restated.  emba_amd.io.refit_frames is the same rule in numpy; include/emba_hip.h (emba_frames_refit) states
// it in words.
//
// No HIP in here: plain C++17, so that tests/cpp/refit_rule_test.cpp checks it on a CPU in milliseconds.  Everything below the argument checks is compiled
// for the host and for the device: the kernels and the CPU test run the same functions.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <cmath>

#include "../../include/emba_hip.h"      // emba_refit_settings, EMBA_REFIT_*
#include "track_exposure_rule.h"

namespace emba {

// ---- argument checks behind track_args_ok and track_exposure_args_ok, in the order the C ABI reports them in
enum class RefitArgStatus { ok, q_null, gain_null, bias_null, status_null, bad_sweeps, bad_sweep_tol, bad_status, no_voting_frame, bad_q, bad_gain, bad_bias };
inline bool refit_status_ok(int32_t s) { return s == EMBA_TRACK_ANCHOR || s == EMBA_TRACK_TRACKED || s == EMBA_TRACK_LOST; }
// *where: the frame that was refused (bad_status, bad_q, bad_gain, bad_bias)
inline RefitArgStatus refit_args_ok(const double* q, const double* gain, const double* bias, const int32_t* status, size_t F, const emba_refit_settings& s, size_t* where)
{
    if (where) *where = 0;
    if (F && !q) return RefitArgStatus::q_null;
    if (F && !gain) return RefitArgStatus::gain_null;
    if (F && !bias) return RefitArgStatus::bias_null;
    if (F && !status) return RefitArgStatus::status_null;
    if (s.sweeps < 0) return RefitArgStatus::bad_sweeps;
    if (!(s.sweep_tol >= 0.0)) return RefitArgStatus::bad_sweep_tol;      // (a NaN is refused)
    size_t voting = 0;
    for (size_t f = 0; f < F; ++f) {
        if (!refit_status_ok(status[f])) { if (where) *where = f; return RefitArgStatus::bad_status; }
        voting += track_votes(status[f]);
    }
    if (!voting) return RefitArgStatus::no_voting_frame;
    for (size_t f = 0; f < F; ++f) {
        if (where) *where = f;
        if (!align_q_ok(q + 4 * f)) return RefitArgStatus::bad_q;
        if (!(std::isfinite(gain[f]) && gain[f] >= s.track.gain_min && gain[f] <= s.track.gain_max)) return RefitArgStatus::bad_gain;
        if (!std::isfinite(bias[f])) return RefitArgStatus::bad_bias;
    }
    if (where) *where = 0;
    return RefitArgStatus::ok;
}

// ---- the un-vote: a frame's votes leave a sum by the two's complement of what was added, modulo 2^64.  refit_signed(x, true) + x == 0 for every x, so a sum
// that wrapped on the way up is back where it was.
EMBA_RULE_HD inline uint64_t refit_signed(uint64_t x, bool negate) { return negate ? (uint64_t)0 - x : x; }

// ---- which frames a vote launch serves: every voting frame (the build), or the voting frames that may move — the tracked ones; anchors are never taken
// out of the planes, so they are never voted back either
enum RefitSelect { kRefitSelectVoting = 0, kRefitSelectMovable = 1 };
EMBA_RULE_HD inline bool refit_movable(int status) { return status == EMBA_TRACK_TRACKED; }
EMBA_RULE_HD inline bool refit_selected(int select, int status) { return select == kRefitSelectMovable ? refit_movable(status) : track_votes(status); }
// the frames a sweep aligns: the movable ones, and with `recover` the lost ones
EMBA_RULE_HD inline bool refit_active(int status, bool recover) { return refit_movable(status) || (recover && status == EMBA_TRACK_LOST); }

// a batch the sweep has something to do in: one with an active frame.  `status`: the call's input — a status only ever changes from lost to tracked, and only
// with `recover`, under which a lost frame is active already
inline bool refit_batch_active(const int32_t* status, size_t f0, size_t nf, bool recover)
{
    for (size_t f = f0; f < f0 + nf; ++f) if (refit_active(status[f], recover)) return true;
    return false;
}

// ---- the order of a sweep: batch k of n in the order the tracker cuts them; with `alternate` the odd sweeps run from the last batch to the first
EMBA_RULE_HD inline size_t refit_batch_index(int sweep, size_t k, size_t n, bool alternate) { return alternate && (sweep & 1) ? n - 1 - k : k; }

// ---- the start of frame f among F.  A voting frame starts at its own (q, a, b).  A lost frame starts from the nearest voting frames a < f < b by index: with
// both, track_predict's formula at t_f — its factor (t_f - t_b) / (t_b - t_a) lies in (-1, 0), an interpolation — and gain and bias linear in the same
// factor; with one, that frame's values.  false (q, a, b untouched): no frame votes.
EMBA_RULE_HD inline bool refit_start(const int32_t* status, const long long* t, const double* q_all, const double* gain_all, const double* bias_all, long F, long f, double* q,
                                     double* gain, double* bias)
{
    if (track_votes(status[f])) {
        for (int k = 0; k < 4; ++k) q[k] = q_all[4 * f + k];
        *gain = gain_all[f]; *bias = bias_all[f];
        return true;
    }
    long a = f - 1, b = f + 1;
    while (a >= 0 && !track_votes(status[a])) --a;
    while (b < F && !track_votes(status[b])) ++b;
    if (a < 0 && b >= F) return false;
    if (a < 0 || b >= F) {
        const long o = a < 0 ? b : a;
        for (int k = 0; k < 4; ++k) q[k] = q_all[4 * o + k];
        *gain = gain_all[o]; *bias = bias_all[o];
        return true;
    }
    track_predict(2, q_all + 4 * a, t[a], q_all + 4 * b, t[b], t[f], true, q);
    const double u = (double)(t[f] - t[b]) / (double)(t[b] - t[a]);
    *gain = gain_all[b] + (gain_all[b] - gain_all[a]) * u;
    *bias = bias_all[b] + (bias_all[b] - bias_all[a]) * u;
    return true;
}

// ---- the code of a frame behind its verdict: `status` as the frame entered the batch, `passed`: track_verdict gave EMBA_TRACK_TRACKED
EMBA_RULE_HD inline int refit_code(int status, bool passed)
{
    if (status == EMBA_TRACK_ANCHOR) return EMBA_REFIT_ANCHOR;
    if (status == EMBA_TRACK_TRACKED) return passed ? EMBA_REFIT_MOVED : EMBA_REFIT_KEPT;
    return passed ? EMBA_REFIT_RECOVERED : EMBA_REFIT_LOST;
}

// ---- the rotation change of a sweep: the largest angle (rad) between a frame's rotation before and behind it
inline double refit_rotation_change(const double* q_before, const double* q_after, size_t F)
{
    double worst = 0.0;
    for (size_t f = 0; f < F; ++f) {
        double w[3];
        track_log_between(q_before + 4 * f, q_after + 4 * f, w);
        const double a = sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
        if (a > worst) worst = a;
    }
    return worst;
}
// the call ends behind a sweep whose change is below sweep_tol; 0 never ends it
inline bool refit_converged(double change, double sweep_tol) { return change < sweep_tol; }

}  // namespace emba
