// emba_amd/csrc/graph_rule.h — a rotation graph over tracked frames (emba_rotation_graph_solve): one rotation per frame, the anchors held exactly, an edge
// per aligned pair of frames (pair_rule.h) with the pair's relative rotation and its information.  Sequential host code: a few thousand 3 x 3 blocks.
//   unknowns   q_f (camera to world, xyzw) of every frame whose status is not EMBA_TRACK_ANCHOR and that an edge reaches; anchors are constants, and a frame
//              without an edge keeps its input
//   edge       (i, j, Q_ij, Lambda_ij): e = log(Q_ij (x) q_i^-1 (x) q_j), in camera j's coordinates, where Lambda_ij lives; the cost is sum e^T Lambda e
//   Jacobian   with q <- exp(delta) q on both ends, e' ~ e + Jr^-1(e) R_j^T (delta_j - delta_i)
//   solver     damped Gauss-Newton: (A + lambda diag A) delta = -g by conjugate gradients with the 3 x 3 block-Jacobi preconditioner, matrix-free over the
//              edges in edge order: deterministic.  A trial is accepted when its cost is below the cost (lambda down, and the solve has converged when
//              |delta|_inf < tol), else rejected (lambda up, stalled when lambda > lambda_max): align_step's decisions on the total cost
// emba_amd.io.rotation_graph_solve is the same rule in numpy; include/emba_hip.h states it in words.
//
// No HIP in here: plain C++17; tests/cpp/graph_rule_test.cpp checks it on a CPU.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <cmath>
#include <vector>

#include "../../include/emba_hip.h"      // emba_graph_settings, EMBA_GRAPH_*, EMBA_TRACK_ANCHOR

namespace emba {

// ---- small SO(3) on quaternions xyzw and 3-vectors
inline void graph_qmul(const double* a, const double* b, double* out)      // normalised a (x) b
{
    const double ax = a[0], ay = a[1], az = a[2], aw = a[3], bx = b[0], by = b[1], bz = b[2], bw = b[3];
    const double x = aw * bx + ax * bw + ay * bz - az * by, y = aw * by + ay * bw + az * bx - ax * bz;
    const double z = aw * bz + az * bw + ax * by - ay * bx, w = aw * bw - ax * bx - ay * by - az * bz;
    const double n = sqrt(x * x + y * y + z * z + w * w);
    out[0] = x / n; out[1] = y / n; out[2] = z / n; out[3] = w / n;
}
inline void graph_qexp(const double* d, double* q)
{
    const double th2 = d[0] * d[0] + d[1] * d[1] + d[2] * d[2];
    double imag, real;
    if (th2 < 1e-20) { imag = 0.5 - th2 / 48.0; real = 1.0 - th2 / 8.0; }
    else { const double th = sqrt(th2); imag = sin(0.5 * th) / th; real = cos(0.5 * th); }
    q[0] = imag * d[0]; q[1] = imag * d[1]; q[2] = imag * d[2]; q[3] = real;
}
inline void graph_qlog(const double* q, double* e)      // the rotation vector of the shorter way round (|e| <= pi)
{
    const double s = q[3] < 0.0 ? -1.0 : 1.0;
    const double x = s * q[0], y = s * q[1], z = s * q[2], w = s * q[3];
    const double n2 = x * x + y * y + z * z;
    double f;
    if (n2 < 1e-20) f = 2.0 / w - (2.0 / 3.0) * n2 / (w * w * w);
    else { const double n = sqrt(n2); f = 2.0 * atan2(n, w) / n; }
    e[0] = f * x; e[1] = f * y; e[2] = f * z;
}
inline void graph_qmatrix(const double* q, double* R)      // row-major
{
    const double x = q[0], y = q[1], z = q[2], w = q[3];
    R[0] = 1 - 2 * (y * y + z * z); R[1] = 2 * (x * y - z * w); R[2] = 2 * (x * z + y * w);
    R[3] = 2 * (x * y + z * w); R[4] = 1 - 2 * (x * x + z * z); R[5] = 2 * (y * z - x * w);
    R[6] = 2 * (x * z - y * w); R[7] = 2 * (y * z + x * w); R[8] = 1 - 2 * (x * x + y * y);
}
// Jr^-1(e) = I + 1/2 [e]x + c [e]x^2, c = (1 - (th / 2) cot(th / 2)) / th^2 (1 / 12 at th -> 0); good up to th = pi, where cot(th / 2) = 0
inline void graph_jr_inv(const double* e, double* J)
{
    const double th2 = e[0] * e[0] + e[1] * e[1] + e[2] * e[2];
    double c;
    if (th2 < 1e-8) c = 1.0 / 12.0 + th2 / 720.0;
    else { const double th = sqrt(th2), h = 0.5 * th; c = (1.0 - h * cos(h) / sin(h)) / th2; }
    const double x = e[0], y = e[1], z = e[2];
    // [e]x^2 = e e^T - th2 I
    J[0] = 1.0 + c * (x * x - th2); J[1] = -0.5 * z + c * x * y;       J[2] = 0.5 * y + c * x * z;
    J[3] = 0.5 * z + c * x * y;     J[4] = 1.0 + c * (y * y - th2);   J[5] = -0.5 * x + c * y * z;
    J[6] = -0.5 * y + c * x * z;    J[7] = 0.5 * x + c * y * z;       J[8] = 1.0 + c * (z * z - th2);
}
// the residual of an edge at (q_i, q_j)
inline void graph_residual(const double* Qij, const double* qi, const double* qj, double* e)
{
    const double qi_inv[4] = {-qi[0], -qi[1], -qi[2], qi[3]};
    double t[4], E[4];
    graph_qmul(Qij, qi_inv, t);
    graph_qmul(t, qj, E);
    graph_qlog(E, e);
}
inline double graph_quad(const double* L, const double* e)      // e^T Lambda e, Lambda as 00 01 02 11 12 22
{
    return e[0] * (L[0] * e[0] + L[1] * e[1] + L[2] * e[2]) + e[1] * (L[1] * e[0] + L[3] * e[1] + L[4] * e[2]) + e[2] * (L[2] * e[0] + L[4] * e[1] + L[5] * e[2]);
}

// ---- argument checks (the order the C ABI reports them in); *at: the edge or the frame that is refused
enum class GraphArgStatus { ok, q_null, status_null, edges_null, settings, bad_q, no_anchor, edge_out_of_range, bad_edge_q, info_not_finite, unreachable };
inline bool graph_settings_ok(const emba_graph_settings* s)
{
    return s && s->max_iters >= 0 && s->cg_max_iters >= 1 && s->lambda0 > 0.0 && std::isfinite(s->lambda0) && s->lambda_up > 1.0 && s->lambda_down > 1.0 &&
           std::isfinite(s->lambda_up) && std::isfinite(s->lambda_down) && s->lambda_min >= 0.0 && s->lambda_max > 0.0 && s->lambda_min <= s->lambda_max &&
           s->tol >= 0.0 && s->cg_tol >= 0.0;
}
// reached[f]: frame f is an anchor or an edge path leads from an anchor to it
inline void graph_reach(const int32_t* status, size_t F, const int32_t* edges, size_t E, std::vector<uint8_t>* reached)
{
    reached->assign(F, 0);
    for (size_t f = 0; f < F; ++f) (*reached)[f] = status[f] == EMBA_TRACK_ANCHOR;
    for (bool grew = true; grew;) {      // (a sweep over the edges per round: a few thousand edges, a few rounds)
        grew = false;
        for (size_t k = 0; k < E; ++k) {
            const size_t i = (size_t)edges[2 * k], j = (size_t)edges[2 * k + 1];
            if ((*reached)[i] != (*reached)[j]) { (*reached)[i] = (*reached)[j] = 1; grew = true; }
        }
    }
}
inline GraphArgStatus graph_args_ok(const double* q, const int32_t* status, size_t F, const int32_t* edges, const double* Qe, const double* info, size_t E,
                                    const emba_graph_settings* set, size_t* at)
{
    if (F && !q) return GraphArgStatus::q_null;
    if (F && !status) return GraphArgStatus::status_null;
    if (E && !(edges && Qe && info)) return GraphArgStatus::edges_null;
    if (!graph_settings_ok(set)) return GraphArgStatus::settings;
    bool anchor = false;
    for (size_t f = 0; f < F; ++f) {
        *at = f;
        const double n2 = q[4 * f] * q[4 * f] + q[4 * f + 1] * q[4 * f + 1] + q[4 * f + 2] * q[4 * f + 2] + q[4 * f + 3] * q[4 * f + 3];
        if (!(std::isfinite(n2) && n2 > 0.0)) return GraphArgStatus::bad_q;
        anchor = anchor || status[f] == EMBA_TRACK_ANCHOR;
    }
    if (!anchor) return GraphArgStatus::no_anchor;
    for (size_t k = 0; k < E; ++k) {
        *at = k;
        if (edges[2 * k] < 0 || edges[2 * k + 1] < 0 || (size_t)edges[2 * k] >= F || (size_t)edges[2 * k + 1] >= F) return GraphArgStatus::edge_out_of_range;
    }
    for (size_t k = 0; k < E; ++k) {
        *at = k;
        const double* Q = Qe + 4 * k;
        const double n2 = Q[0] * Q[0] + Q[1] * Q[1] + Q[2] * Q[2] + Q[3] * Q[3];
        if (!(std::isfinite(n2) && n2 > 0.0)) return GraphArgStatus::bad_edge_q;
    }
    for (size_t k = 0; k < E; ++k) {
        *at = k;
        for (int m = 0; m < 6; ++m) if (!std::isfinite(info[6 * k + m])) return GraphArgStatus::info_not_finite;
    }
    std::vector<uint8_t> reached;
    graph_reach(status, F, edges, E, &reached);
    std::vector<uint8_t> touched(F, 0);
    for (size_t k = 0; k < E; ++k) touched[(size_t)edges[2 * k]] = touched[(size_t)edges[2 * k + 1]] = 1;
    for (size_t f = 0; f < F; ++f)
        if (touched[f] && !reached[f]) { *at = f; return GraphArgStatus::unreachable; }
    return GraphArgStatus::ok;
}

// ---- the solve
struct GraphResult { double cost0, cost; int32_t iters, cg_iters, end; };

namespace graph_detail {
struct Lin { std::vector<double> W, D, g; };      // per edge W = M^T Lambda M [9]; per frame the diagonal block D [9] and the gradient g [3]
inline void mat3_mul(const double* A, const double* B, double* C)
{
    for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) C[3 * r + c] = A[3 * r] * B[c] + A[3 * r + 1] * B[3 + c] + A[3 * r + 2] * B[6 + c];
}
inline void mat3_vec(const double* A, const double* x, double* y)
{
    for (int r = 0; r < 3; ++r) y[r] = A[3 * r] * x[0] + A[3 * r + 1] * x[1] + A[3 * r + 2] * x[2];
}
// x = B^-1 r for a symmetric positive definite 3 x 3 B; false where it is not
inline bool spd3_solve(const double* B, const double* r, double* x)
{
    if (!(B[0] > 0.0)) return false;
    const double l00 = sqrt(B[0]), l10 = B[3] / l00, l20 = B[6] / l00;
    const double d1 = B[4] - l10 * l10;
    if (!(d1 > 0.0)) return false;
    const double l11 = sqrt(d1), l21 = (B[7] - l20 * l10) / l11;
    const double d2 = B[8] - l20 * l20 - l21 * l21;
    if (!(d2 > 0.0)) return false;
    const double l22 = sqrt(d2);
    const double y0 = r[0] / l00, y1 = (r[1] - l10 * y0) / l11, y2 = (r[2] - l20 * y0 - l21 * y1) / l22;
    x[2] = y2 / l22; x[1] = (y1 - l21 * x[2]) / l11; x[0] = (y0 - l10 * x[1] - l20 * x[2]) / l00;
    return true;
}
}  // namespace graph_detail

inline double graph_cost(const double* q, const int32_t* edges, const double* Qe, const double* info, size_t E)
{
    double cost = 0.0;
    for (size_t k = 0; k < E; ++k) {
        double e[3];
        graph_residual(Qe + 4 * k, q + 4 * (size_t)edges[2 * k], q + 4 * (size_t)edges[2 * k + 1], e);
        cost += graph_quad(info + 6 * k, e);
    }
    return cost;
}

// The arguments are good (graph_args_ok).  q_out [F, 4]: anchors and frames without an edge are copies of the input, bit for bit.
inline GraphResult graph_solve(const double* q_in, const int32_t* status, size_t F, const int32_t* edges, const double* Qe, const double* info, size_t E,
                               const emba_graph_settings& set, double* q_out)
{
    using namespace graph_detail;
    std::vector<double> q(q_in, q_in + 4 * F), trial(4 * F);
    std::vector<uint8_t> free_(F, 0);
    for (size_t k = 0; k < E; ++k) free_[(size_t)edges[2 * k]] = free_[(size_t)edges[2 * k + 1]] = 1;
    size_t n_free = 0;
    for (size_t f = 0; f < F; ++f) { if (status[f] == EMBA_TRACK_ANCHOR) free_[f] = 0; n_free += free_[f]; }
    GraphResult res{graph_cost(q.data(), edges, Qe, info, E), 0.0, 0, 0, EMBA_GRAPH_CONVERGED};
    res.cost = res.cost0;
    if (!n_free) { for (size_t k = 0; k < 4 * F; ++k) q_out[k] = q_in[k]; return res; }

    Lin L;
    L.W.resize(9 * E); L.D.resize(9 * F); L.g.resize(3 * F);
    std::vector<double> x(3 * F), r(3 * F), z(3 * F), p(3 * F), Ap(3 * F), B(9 * F);
    double lambda = set.lambda0;
    bool relinearise = true;
    res.end = EMBA_GRAPH_ITERATIONS;
    while (res.iters < set.max_iters) {
        if (relinearise) {
            std::fill(L.D.begin(), L.D.end(), 0.0);
            std::fill(L.g.begin(), L.g.end(), 0.0);
            for (size_t k = 0; k < E; ++k) {
                const size_t i = (size_t)edges[2 * k], j = (size_t)edges[2 * k + 1];
                double e[3], Jr[9], Rj[9], RjT[9], M[9], LM[9], MT[9], Le[3], Ge[3];
                graph_residual(Qe + 4 * k, &q[4 * i], &q[4 * j], e);
                graph_jr_inv(e, Jr);
                graph_qmatrix(&q[4 * j], Rj);
                for (int a = 0; a < 3; ++a) for (int b = 0; b < 3; ++b) RjT[3 * a + b] = Rj[3 * b + a];
                mat3_mul(Jr, RjT, M);
                const double* I6 = info + 6 * k;
                const double Lm[9] = {I6[0], I6[1], I6[2], I6[1], I6[3], I6[4], I6[2], I6[4], I6[5]};
                for (int a = 0; a < 3; ++a) for (int b = 0; b < 3; ++b) MT[3 * a + b] = M[3 * b + a];
                mat3_mul(Lm, M, LM);
                mat3_mul(MT, LM, &L.W[9 * k]);
                mat3_vec(Lm, e, Le);
                mat3_vec(MT, Le, Ge);      // the gradient with respect to delta_j; minus it with respect to delta_i
                if (i == j) { for (int a = 0; a < 9; ++a) L.W[9 * k + a] = 0.0; continue; }      // (both ends move together: the edge says nothing)
                for (int a = 0; a < 9; ++a) { L.D[9 * i + a] += L.W[9 * k + a]; L.D[9 * j + a] += L.W[9 * k + a]; }
                for (int a = 0; a < 3; ++a) { L.g[3 * j + a] += Ge[a]; L.g[3 * i + a] -= Ge[a]; }
            }
            relinearise = false;
        }
        // the damped blocks of the preconditioner
        for (size_t f = 0; f < F; ++f) {
            for (int a = 0; a < 9; ++a) B[9 * f + a] = L.D[9 * f + a];
            for (int a = 0; a < 3; ++a) B[9 * f + 4 * a] += lambda * L.D[9 * f + 4 * a];
        }
        auto apply = [&](const std::vector<double>& v, std::vector<double>& out) {      // out = (A + lambda diag A) v over the free frames
            std::fill(out.begin(), out.end(), 0.0);
            for (size_t k = 0; k < E; ++k) {
                const size_t i = (size_t)edges[2 * k], j = (size_t)edges[2 * k + 1];
                if (i == j) continue;
                double d[3], t[3];
                for (int a = 0; a < 3; ++a) d[a] = (free_[j] ? v[3 * j + a] : 0.0) - (free_[i] ? v[3 * i + a] : 0.0);
                mat3_vec(&L.W[9 * k], d, t);
                for (int a = 0; a < 3; ++a) { out[3 * j + a] += t[a]; out[3 * i + a] -= t[a]; }
            }
            for (size_t f = 0; f < F; ++f)
                for (int a = 0; a < 3; ++a) out[3 * f + a] = free_[f] ? out[3 * f + a] + lambda * L.D[9 * f + 4 * a] * v[3 * f + a] : 0.0;
        };
        auto precondition = [&](const std::vector<double>& v, std::vector<double>& out) {
            bool ok = true;
            for (size_t f = 0; f < F; ++f) {
                if (!free_[f]) { out[3 * f] = out[3 * f + 1] = out[3 * f + 2] = 0.0; continue; }
                ok = spd3_solve(&B[9 * f], &v[3 * f], &out[3 * f]) && ok;
            }
            return ok;
        };
        auto dot = [&](const std::vector<double>& a, const std::vector<double>& b) { double s = 0.0; for (size_t k = 0; k < 3 * F; ++k) s += a[k] * b[k]; return s; };
        // conjugate gradients on (A + lambda diag A) x = -g
        std::fill(x.begin(), x.end(), 0.0);
        for (size_t f = 0; f < F; ++f) for (int a = 0; a < 3; ++a) r[3 * f + a] = free_[f] ? -L.g[3 * f + a] : 0.0;
        const double r0 = sqrt(dot(r, r));
        bool solved = precondition(r, z);
        if (solved && r0 > 0.0) {
            p = z;
            double rz = dot(r, z);
            for (int it = 0; it < set.cg_max_iters; ++it) {
                apply(p, Ap);
                const double pAp = dot(p, Ap);
                if (!(pAp > 0.0)) break;
                const double alpha = rz / pAp;
                for (size_t k = 0; k < 3 * F; ++k) { x[k] += alpha * p[k]; r[k] -= alpha * Ap[k]; }
                ++res.cg_iters;
                if (sqrt(dot(r, r)) <= set.cg_tol * r0) break;
                precondition(r, z);
                const double rz1 = dot(r, z), beta = rz1 / rz;
                rz = rz1;
                for (size_t k = 0; k < 3 * F; ++k) p[k] = z[k] + beta * p[k];
            }
        }
        if (!solved) { res.end = EMBA_GRAPH_DEGENERATE; break; }
        // the trial
        double dmax = 0.0;
        trial = q;
        for (size_t f = 0; f < F; ++f) {
            if (!free_[f]) continue;
            double ex[4];
            graph_qexp(&x[3 * f], ex);
            graph_qmul(ex, &q[4 * f], &trial[4 * f]);
            for (int a = 0; a < 3; ++a) dmax = fabs(x[3 * f + a]) > dmax ? fabs(x[3 * f + a]) : dmax;
        }
        const double cost1 = graph_cost(trial.data(), edges, Qe, info, E);
        ++res.iters;
        if (cost1 < res.cost) {
            q.swap(trial);
            res.cost = cost1;
            const double down = lambda / set.lambda_down;
            lambda = down > set.lambda_min ? down : set.lambda_min;
            relinearise = true;
            if (dmax < set.tol) { res.end = EMBA_GRAPH_CONVERGED; break; }
        } else {
            if (dmax < set.tol) { res.end = EMBA_GRAPH_CONVERGED; break; }      // (a step below the tolerance that no longer lowers the cost: the minimum)
            lambda *= set.lambda_up;
            if (lambda > set.lambda_max) { res.end = EMBA_GRAPH_STALLED; break; }
        }
    }
    for (size_t f = 0; f < F; ++f)
        for (int a = 0; a < 4; ++a) q_out[4 * f + a] = free_[f] ? q[4 * f + a] : q_in[4 * f + a];
    return res;
}

}  // namespace emba
