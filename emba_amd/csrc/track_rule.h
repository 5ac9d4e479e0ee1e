// emba_amd/csrc/track_rule.h — intensity frames tracked against their own growing mosaic (track_host.h, track_kernels.h), as functions of plain values: the
// argument checks, the geometry of a level, the batches of a call, the start of a frame predicted from the last two tracked frames, one pixel of a frame
// against a level's two integer sums, and the verdict on a frame.  The vote is pano_vote of panorama_rule.h on the level's grid, the mean of a cell is
// mosaic_mean of mosaic_rule.h, the sample with its gradient, the weight, the sums and the Levenberg-Marquardt step are align_rule.h's, as they are.
// emba_amd.io.track_level_pm / track_votes / track_terms / track_predict / track_frames are the same rules in numpy; include/emba_hip.h (emba_frames_track,
// emba_track_eval, emba_track_level_get) states them in words.
//
// No HIP in here: plain C++17, so that tests/cpp/track_rule_test.cpp checks it on a CPU in milliseconds.  Everything below the argument checks is compiled
// for the host and for the device: the kernels and the CPU test run the same functions.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <cmath>

#include "../../include/emba_hip.h"      // emba_track_settings, EMBA_TRACK_*
#include "align_rule.h"
#include "mosaic_rule.h"

namespace emba {

constexpr int kTrackMaxLevel = 7;          // levels 0 ... 7
constexpr int kTrackMaxSchedule = 8;       // a schedule names 1 ... 8 levels
constexpr int kTrackMaxPlanes = 9;         // the planes a frame votes into: the schedule's, and level 0 where the schedule does not name it

// ---- level l: the panorama with cells 2^l pixels wide.  W_l = W >> l, H_l = H >> l, pm_l = pm * 2^-l, J23_l = J23 * 2^-l (a power of two: exact).
enum class TrackLevelStatus { ok, out_of_range, not_divisible, too_few_rows };
struct TrackLevel { int W, H; double scale; };
EMBA_RULE_HD inline TrackLevelStatus track_level(int W, int H, int l, TrackLevel* out)
{
    if (l < 0 || l > kTrackMaxLevel) return TrackLevelStatus::out_of_range;
    const int m = (1 << l) - 1;
    if ((W & m) || (H & m)) return TrackLevelStatus::not_divisible;
    if ((H >> l) < 2) return TrackLevelStatus::too_few_rows;
    if (out) { out->W = W >> l; out->H = H >> l; out->scale = 1.0 / (double)(1 << l); }
    return TrackLevelStatus::ok;
}

// ---- argument checks (the order the C ABI reports them in)
enum class TrackArgStatus {
    ok, frames_null, times_null, q0_null, settings_null, too_many_frames, schedule_length, level_range, level_not_divisible, level_too_few_rows, bad_batch,
    bad_min_overlap, bad_min_weight, times_not_increasing, bad_q0, bad_align_settings, too_many_votes
};
// *where: the index of the schedule entry (level_*) or of the frame time (times_not_increasing) that was refused
inline TrackArgStatus track_args_ok(bool have_frames, bool have_times, const double* q0, const emba_track_settings* s, const int64_t* t_ns, size_t F, size_t S, int W,
                                    int H, size_t* where)
{
    if (where) *where = 0;
    if (F && !have_frames) return TrackArgStatus::frames_null;
    if (F && !have_times) return TrackArgStatus::times_null;
    if (!q0) return TrackArgStatus::q0_null;
    if (!s) return TrackArgStatus::settings_null;
    if (F > 0x7FFFFFFFull) return TrackArgStatus::too_many_frames;
    if (s->n_levels < 1 || s->n_levels > kTrackMaxSchedule) return TrackArgStatus::schedule_length;
    for (int i = 0; i < s->n_levels; ++i) {
        if (where) *where = (size_t)i;
        switch (track_level(W, H, s->levels[i], nullptr)) {
        case TrackLevelStatus::ok: break;
        case TrackLevelStatus::out_of_range: return TrackArgStatus::level_range;
        case TrackLevelStatus::not_divisible: return TrackArgStatus::level_not_divisible;
        case TrackLevelStatus::too_few_rows: return TrackArgStatus::level_too_few_rows;
        }
    }
    if (where) *where = 0;
    if (s->batch < 1) return TrackArgStatus::bad_batch;
    if (!(s->min_overlap >= 0.0 && s->min_overlap <= 1.0)) return TrackArgStatus::bad_min_overlap;      // (a NaN is refused)
    if (s->min_weight < 1) return TrackArgStatus::bad_min_weight;
    for (size_t f = 1; f < F; ++f)
        if (!(t_ns[f] > t_ns[f - 1])) { if (where) *where = f; return TrackArgStatus::times_not_increasing; }
    if (!align_q_ok(q0)) return TrackArgStatus::bad_q0;
    if (align_settings_ok(&s->align) != AlignSetStatus::ok || std::isnan(s->align.huber_k)) return TrackArgStatus::bad_align_settings;
    if (mosaic_votes_after(0, F, S) >= kMosaicMaxVotes) return TrackArgStatus::too_many_votes;
    return TrackArgStatus::ok;
}

// ---- the planes a tracked frame votes into: the schedule's levels in their order, each once, then level 0 where the schedule does not name it
inline int track_vote_levels(const emba_track_settings& s, int* levels /* [kTrackMaxPlanes] */)
{
    int n = 0;
    bool zero = false;
    for (int i = 0; i < s.n_levels; ++i) {
        bool seen = false;
        for (int k = 0; k < n; ++k) seen = seen || levels[k] == s.levels[i];
        if (!seen) levels[n++] = s.levels[i];
        zero = zero || s.levels[i] == 0;
    }
    if (!zero) levels[n++] = 0;
    return n;
}

// ---- the batches: frame 0 is the anchor and a batch of its own; behind it the frames [f0, f0 + batch) are aligned at once, cut at the end of the call and at
// the end of f0's chunk of `per` frames (a chunk's bytes are on the device together).  Returns the number of frames of the batch that starts at f0 < F.
inline size_t track_batch_frames(size_t f0, size_t F, size_t per, size_t batch)
{
    if (f0 == 0) return 1;
    const size_t chunk_end = (f0 / per + 1) * per;
    size_t n = batch;
    if (n > F - f0) n = F - f0;
    if (n > chunk_end - f0) n = chunk_end - f0;
    return n;
}

// ---- quaternions xyzw
EMBA_RULE_HD inline void track_normalise(const double* q, double* out)
{
    const double n = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    out[0] = q[0] / n; out[1] = q[1] / n; out[2] = q[2] / n; out[3] = q[3] / n;
}
// omega = log(qb (x) qa^-1): the rotation vector that turns qa into qb, the short way round
EMBA_RULE_HD inline void track_log_between(const double* qa, const double* qb, double* omega)
{
    const double ax = -qa[0], ay = -qa[1], az = -qa[2], aw = qa[3];      // qa^-1 of a unit quaternion
    const double bx = qb[0], by = qb[1], bz = qb[2], bw = qb[3];
    double x = bw * ax + bx * aw + by * az - bz * ay, y = bw * ay + by * aw + bz * ax - bx * az;
    double z = bw * az + bz * aw + bx * ay - by * ax, w = bw * aw - bx * ax - by * ay - bz * az;
    if (w < 0.0) { x = -x; y = -y; z = -z; w = -w; }
    const double n2 = x * x + y * y + z * z;
    double f;
    if (n2 < 1e-20) f = 2.0 / w;
    else { const double n = sqrt(n2); f = 2.0 * atan2(n, w) / n; }
    omega[0] = f * x; omega[1] = f * y; omega[2] = f * z;
}
// ---- the start of the frame at time t.  a < b are the last two tracked frames (n_tracked of them are there: 0, 1 or 2; with 1 only b).  With predict and both:
// normalise(exp(omega (t - t_b) / (t_b - t_a)) (x) q_b), omega = log(q_b (x) q_a^-1) — a constant angular velocity.  Otherwise q_b.  With none: q unchanged, false.
EMBA_RULE_HD inline bool track_predict(int n_tracked, const double* qa, int64_t ta, const double* qb, int64_t tb, int64_t t, bool predict, double* q)
{
    if (n_tracked < 1) return false;
    if (!predict || n_tracked < 2) { for (int k = 0; k < 4; ++k) q[k] = qb[k]; return true; }
    double omega[3];
    track_log_between(qa, qb, omega);
    const double u = (double)(t - tb) / (double)(tb - ta);
    const double d[3] = {omega[0] * u, omega[1] * u, omega[2] * u};
    align_apply(d, qb, q);
    return true;
}

// ---- one pixel of a frame against a level: the cell is align_cell on the level's grid at the level's pm; masked when any of its four cells has
// sum_w < min_weight; the four means are mosaic_mean's, formed here and sampled by align_sample_cell; the frame's byte is in the plane's units (I = v);
// J23 is the level's.  Classes and precedence are align_pixel's.
EMBA_RULE_HD inline int track_pixel(const uint64_t* sum_w, const uint64_t* sum_v, int W, int H, double pm_x, double pm_y, const double* J23, unsigned v,
                                    uint64_t min_weight, bool skip_zero, double huber_k, AlignTerm* t)
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
    t->r = val - (double)v;
    align_huber(t->r, huber_k, &t->w, &t->rho);
    for (int j = 0; j < 3; ++j) t->g[j] = gx * J23[j] + gy * J23[3 + j];
    return kAlignUsed;
}

// ---- the verdict: overlap = used / (S - skipped) at q_out (0 where every pixel was skipped); tracked when the last level did not end degenerate and
// overlap >= min_overlap, else lost
EMBA_RULE_HD inline double track_overlap(uint64_t used, uint64_t skipped, uint64_t S)
{
    return S > skipped ? (double)used / (double)(S - skipped) : 0.0;
}
EMBA_RULE_HD inline int track_verdict(int last_level_status, double overlap, double min_overlap)
{
    return last_level_status != EMBA_ALIGN_DEGENERATE && overlap >= min_overlap ? EMBA_TRACK_TRACKED : EMBA_TRACK_LOST;
}
EMBA_RULE_HD inline bool track_votes(int status) { return status == EMBA_TRACK_ANCHOR || status == EMBA_TRACK_TRACKED; }

}  // namespace emba
