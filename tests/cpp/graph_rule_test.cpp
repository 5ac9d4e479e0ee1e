// tests/cpp/graph_rule_test.cpp — emba_amd/csrc/graph_rule.h on a CPU (plain C++17, no HIP; tests/test_graph_rule_cpu.py builds and runs it, also under the
// address and undefined-behaviour sanitizers): the refusals in the order the C ABI reports them, Jr^-1 against central differences of log(E exp(x)) at small,
// moderate and near-pi angles, and the solve: exact edges from a perturbed start recover the truth, anchors and frames without an edge keep their bits, an
// unreachable free frame and a graph without an anchor are refused, and a permuted edge list gives the same rotations within the spread it prints.
#include "../../emba_amd/csrc/graph_rule.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

using namespace emba;

static int g_fail = 0;
#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #cond); ++g_fail; } \
    } while (0)

static emba_graph_settings settings()
{
    emba_graph_settings s;
    s.max_iters = 50; s.cg_max_iters = 200;
    s.lambda0 = 1e-4; s.lambda_up = 10.0; s.lambda_down = 10.0; s.lambda_min = 1e-12; s.lambda_max = 1e8; s.tol = 1e-10; s.cg_tol = 1e-10;
    return s;
}

static double angle_between(const double* a, const double* b)
{
    const double ai[4] = {-a[0], -a[1], -a[2], a[3]};
    double d[4], e[3];
    graph_qmul(b, ai, d);
    graph_qlog(d, e);
    return std::sqrt(e[0] * e[0] + e[1] * e[1] + e[2] * e[2]);
}

// a small deterministic generator (no <random>: the same numbers on every library)
static uint64_t g_state = 0x9E3779B97F4A7C15ull;
static double uniform() { g_state = g_state * 6364136223846793005ull + 1442695040888963407ull; return (double)(g_state >> 11) / 9007199254740992.0 - 0.5; }

struct Graph {
    std::vector<double> truth, start, Qe, info;
    std::vector<int32_t> status, edges;
    size_t F, E;
};
// F frames on a sweep out and back, frame 0 the anchor; edges between neighbours and across the loop, exact: Q = q_j^-1 q_i of the truth
static Graph make_graph(size_t F, double perturb)
{
    Graph g;
    g.F = F;
    g.truth.resize(4 * F); g.start.resize(4 * F); g.status.assign(F, EMBA_TRACK_TRACKED);
    g.status[0] = EMBA_TRACK_ANCHOR;
    for (size_t f = 0; f < F; ++f) {
        const double u = (double)f / (double)(F - 1), pan = 0.6 * (u < 0.5 ? 2 * u : 2 - 2 * u), tilt = 0.1 * std::sin(6.28 * u);
        const double d[3] = {tilt, pan, 0.05 * u}, I4[4] = {0, 0, 0, 1};
        double ex[4];
        graph_qexp(d, ex);
        graph_qmul(ex, I4, &g.truth[4 * f]);
        const double p[3] = {perturb * uniform(), perturb * uniform(), perturb * uniform()};
        graph_qexp(p, ex);
        graph_qmul(ex, &g.truth[4 * f], &g.start[4 * f]);
    }
    for (int k = 0; k < 4; ++k) g.start[k] = g.truth[k];      // the anchor is where it is
    auto add = [&](size_t i, size_t j) {
        const double qj_inv[4] = {-g.truth[4 * j], -g.truth[4 * j + 1], -g.truth[4 * j + 2], g.truth[4 * j + 3]};
        double Q[4];
        graph_qmul(qj_inv, &g.truth[4 * i], Q);
        g.edges.push_back((int32_t)i); g.edges.push_back((int32_t)j);
        for (int k = 0; k < 4; ++k) g.Qe.push_back(Q[k]);
        const double L[6] = {900.0 + 10.0 * (double)i, 30.0, -20.0, 700.0, 15.0, 400.0 + 5.0 * (double)j};
        for (int k = 0; k < 6; ++k) g.info.push_back(L[k]);
    };
    for (size_t f = 0; f + 1 < F; ++f) add(f, f + 1);
    for (size_t f = 0; f + 2 < F; ++f) add(f, f + 2);
    for (size_t f = 0; f < F / 2; ++f) add(f, F - 1 - f);      // the way back sees the way out
    g.E = g.edges.size() / 2;
    return g;
}

static void test_jr_inv()
{
    const double angles[] = {1e-7, 1e-3, 0.4, 1.7, 3.0, 3.14};
    for (double th : angles) {
        const double axis[3] = {0.36, -0.48, 0.8};
        const double e[3] = {th * axis[0], th * axis[1], th * axis[2]};
        double J[9], E[4];
        graph_jr_inv(e, J);
        graph_qexp(e, E);
        for (int c = 0; c < 3; ++c) {
            const double h = 1e-6;
            double lo[3], hi[3];
            for (int sgn = 0; sgn < 2; ++sgn) {
                double x[3] = {0, 0, 0}, ex[4], Ex[4];
                x[c] = sgn ? h : -h;
                graph_qexp(x, ex);
                graph_qmul(E, ex, Ex);
                graph_qlog(Ex, sgn ? hi : lo);
            }
            for (int r = 0; r < 3; ++r) CHECK(std::fabs((hi[r] - lo[r]) / (2 * h) - J[3 * r + c]) < 2e-6 * (1.0 + std::fabs(J[3 * r + c])));
        }
    }
    // the log takes the shorter way round, and undoes the exponential
    const double e[3] = {0.3, -0.2, 0.5};
    double q[4], back[3];
    graph_qexp(e, q);
    graph_qlog(q, back);
    for (int k = 0; k < 3; ++k) CHECK(std::fabs(back[k] - e[k]) < 1e-15);
    const double neg[4] = {-q[0], -q[1], -q[2], -q[3]};
    graph_qlog(neg, back);
    for (int k = 0; k < 3; ++k) CHECK(std::fabs(back[k] - e[k]) < 1e-15);
}

static void test_refusals()
{
    using A = GraphArgStatus;
    static_assert((int)A::ok == 0 && (int)A::q_null == 1 && (int)A::status_null == 2 && (int)A::edges_null == 3 && (int)A::settings == 4 && (int)A::bad_q == 5 &&
                  (int)A::no_anchor == 6 && (int)A::edge_out_of_range == 7 && (int)A::bad_edge_q == 8 && (int)A::info_not_finite == 9 && (int)A::unreachable == 10,
                  "the order the C ABI reports them in");
    const double nan = std::numeric_limits<double>::quiet_NaN();
    Graph g = make_graph(6, 0.01);
    const emba_graph_settings s = settings();
    size_t at = 99;
    CHECK(graph_args_ok(g.start.data(), g.status.data(), g.F, g.edges.data(), g.Qe.data(), g.info.data(), g.E, &s, &at) == A::ok);
    CHECK(graph_args_ok(nullptr, nullptr, g.F, nullptr, nullptr, nullptr, g.E, nullptr, &at) == A::q_null);
    CHECK(graph_args_ok(g.start.data(), nullptr, g.F, nullptr, nullptr, nullptr, g.E, nullptr, &at) == A::status_null);
    CHECK(graph_args_ok(g.start.data(), g.status.data(), g.F, g.edges.data(), nullptr, g.info.data(), g.E, nullptr, &at) == A::edges_null);
    CHECK(graph_args_ok(g.start.data(), g.status.data(), g.F, g.edges.data(), g.Qe.data(), g.info.data(), g.E, nullptr, &at) == A::settings);
    { emba_graph_settings b = s; b.lambda_up = 1.0; CHECK(graph_args_ok(g.start.data(), g.status.data(), g.F, g.edges.data(), g.Qe.data(), g.info.data(), g.E, &b, &at) == A::settings); }
    { emba_graph_settings b = s; b.tol = nan; CHECK(graph_args_ok(g.start.data(), g.status.data(), g.F, g.edges.data(), g.Qe.data(), g.info.data(), g.E, &b, &at) == A::settings); }
    { emba_graph_settings b = s; b.cg_max_iters = 0; CHECK(graph_args_ok(g.start.data(), g.status.data(), g.F, g.edges.data(), g.Qe.data(), g.info.data(), g.E, &b, &at) == A::settings); }
    { Graph b = g; b.start[4 * 3] = nan; b.status[0] = EMBA_TRACK_TRACKED; CHECK(graph_args_ok(b.start.data(), b.status.data(), b.F, b.edges.data(), b.Qe.data(), b.info.data(), b.E, &s, &at) == A::bad_q && at == 3); }
    { Graph b = g; b.status[0] = EMBA_TRACK_TRACKED; b.edges[2] = 77; CHECK(graph_args_ok(b.start.data(), b.status.data(), b.F, b.edges.data(), b.Qe.data(), b.info.data(), b.E, &s, &at) == A::no_anchor); }
    { Graph b = g; b.edges[2 * 4 + 1] = (int32_t)b.F; b.info[0] = nan; CHECK(graph_args_ok(b.start.data(), b.status.data(), b.F, b.edges.data(), b.Qe.data(), b.info.data(), b.E, &s, &at) == A::edge_out_of_range && at == 4); }
    { Graph b = g; b.edges[2 * 4 + 1] = (int32_t)b.F; CHECK(graph_args_ok(b.start.data(), b.status.data(), b.F, b.edges.data(), b.Qe.data(), b.info.data(), b.E, &s, &at) == A::edge_out_of_range && at == 4); }
    { Graph b = g; b.edges[0] = -1; CHECK(graph_args_ok(b.start.data(), b.status.data(), b.F, b.edges.data(), b.Qe.data(), b.info.data(), b.E, &s, &at) == A::edge_out_of_range && at == 0); }
    { Graph b = g; for (int k = 0; k < 4; ++k) b.Qe[4 * 2 + k] = 0.0; CHECK(graph_args_ok(b.start.data(), b.status.data(), b.F, b.edges.data(), b.Qe.data(), b.info.data(), b.E, &s, &at) == A::bad_edge_q && at == 2); }
    { Graph b = g; b.info[6 * 5 + 3] = nan; CHECK(graph_args_ok(b.start.data(), b.status.data(), b.F, b.edges.data(), b.Qe.data(), b.info.data(), b.E, &s, &at) == A::info_not_finite && at == 5); }
    {   // two more frames with an edge between them alone: the first of them is named
        Graph b = g;
        b.F = g.F + 3;
        b.start.resize(4 * b.F, 0.0); b.status.resize(b.F, EMBA_TRACK_TRACKED);
        for (size_t f = g.F; f < b.F; ++f) b.start[4 * f + 3] = 1.0;
        b.edges.push_back((int32_t)g.F + 2); b.edges.push_back((int32_t)g.F + 1);
        for (int k = 0; k < 4; ++k) b.Qe.push_back(k == 3 ? 1.0 : 0.0);
        for (int k = 0; k < 6; ++k) b.info.push_back(k == 0 || k == 3 || k == 5 ? 1.0 : 0.0);
        b.E = g.E + 1;
        CHECK(graph_args_ok(b.start.data(), b.status.data(), b.F, b.edges.data(), b.Qe.data(), b.info.data(), b.E, &s, &at) == A::unreachable && at == g.F + 1);
        b.status[g.F + 2] = EMBA_TRACK_ANCHOR;      // a second anchor reaches them; frame F, which no edge names, is no obstacle
        CHECK(graph_args_ok(b.start.data(), b.status.data(), b.F, b.edges.data(), b.Qe.data(), b.info.data(), b.E, &s, &at) == A::ok);
    }
    // a reversed chain is reached in one call whatever the order of its edges
    { const int32_t st[4] = {EMBA_TRACK_TRACKED, EMBA_TRACK_TRACKED, EMBA_TRACK_TRACKED, EMBA_TRACK_ANCHOR}; const int32_t ed[6] = {0, 1, 1, 2, 2, 3};
      std::vector<uint8_t> r; graph_reach(st, 4, ed, 3, &r); CHECK(r[0] && r[1] && r[2] && r[3]); }
}

static void test_solve()
{
    const emba_graph_settings s = settings();
    Graph g = make_graph(12, 0.05);
    // a frame that no edge names keeps its input
    g.F += 1;
    g.truth.insert(g.truth.end(), {0.5, 0.5, 0.5, 0.5});
    g.start.insert(g.start.end(), {0.1, 0.2, 0.3, 0.9});
    g.status.push_back(EMBA_TRACK_LOST);
    std::vector<double> out(4 * g.F);
    double worst0 = 0.0;
    for (size_t f = 0; f + 1 < g.F; ++f) worst0 = std::max(worst0, angle_between(&g.truth[4 * f], &g.start[4 * f]));
    const GraphResult r = graph_solve(g.start.data(), g.status.data(), g.F, g.edges.data(), g.Qe.data(), g.info.data(), g.E, s, out.data());
    double worst = 0.0;
    for (size_t f = 0; f + 1 < g.F; ++f) worst = std::max(worst, angle_between(&g.truth[4 * f], &out[4 * f]));
    std::printf("exact edges: worst angle %.3e -> %.3e rad, cost %.3e -> %.3e, %d trials, %d cg iterations, end %d\n", worst0, worst, r.cost0, r.cost, (int)r.iters,
                (int)r.cg_iters, (int)r.end);
    CHECK(worst0 > 0.01 && worst < 1e-9 && r.cost < 1e-15 * r.cost0 && r.end == EMBA_GRAPH_CONVERGED && r.iters >= 2 && r.cg_iters >= r.iters);
    CHECK(std::memcmp(&out[0], &g.start[0], 4 * sizeof(double)) == 0);                                  // the anchor keeps its bits
    CHECK(std::memcmp(&out[4 * (g.F - 1)], &g.start[4 * (g.F - 1)], 4 * sizeof(double)) == 0);          // and so does the frame without an edge

    // a second anchor in the middle, displaced: it is held, and the others settle around both
    Graph h = make_graph(12, 0.02);
    h.status[6] = EMBA_TRACK_ANCHOR;
    std::vector<double> out2(4 * h.F);
    const GraphResult r2 = graph_solve(h.start.data(), h.status.data(), h.F, h.edges.data(), h.Qe.data(), h.info.data(), h.E, s, out2.data());
    CHECK(std::memcmp(&out2[4 * 6], &h.start[4 * 6], 4 * sizeof(double)) == 0 && r2.cost < r2.cost0 && r2.cost > 0.0);

    // nothing free: converged at once, the cost is reported
    std::vector<int32_t> all(g.F, EMBA_TRACK_ANCHOR);
    const GraphResult r3 = graph_solve(g.start.data(), all.data(), g.F, g.edges.data(), g.Qe.data(), g.info.data(), g.E, s, out.data());
    CHECK(r3.iters == 0 && r3.end == EMBA_GRAPH_CONVERGED && r3.cost == r3.cost0 && r3.cost0 > 0.0 && std::memcmp(out.data(), g.start.data(), 4 * g.F * sizeof(double)) == 0);

    // noisy edges (no exact solution): the edge list permuted gives the same rotations within a spread that is printed
    Graph n = make_graph(12, 0.03);
    for (size_t k = 0; k < n.E; ++k) {
        const double p[3] = {2e-3 * uniform(), 2e-3 * uniform(), 2e-3 * uniform()};
        double ex[4], Q[4];
        graph_qexp(p, ex);
        graph_qmul(ex, &n.Qe[4 * k], Q);
        for (int m = 0; m < 4; ++m) n.Qe[4 * k + m] = Q[m];
    }
    std::vector<double> a(4 * n.F), b(4 * n.F);
    const GraphResult ra = graph_solve(n.start.data(), n.status.data(), n.F, n.edges.data(), n.Qe.data(), n.info.data(), n.E, s, a.data());
    Graph p = n;
    for (size_t k = 0; k < n.E; ++k) {
        const size_t src = (k * 7 + 3) % n.E;      // 7 and E = 27 are coprime: a permutation
        for (int m = 0; m < 2; ++m) p.edges[2 * k + m] = n.edges[2 * src + m];
        for (int m = 0; m < 4; ++m) p.Qe[4 * k + m] = n.Qe[4 * src + m];
        for (int m = 0; m < 6; ++m) p.info[6 * k + m] = n.info[6 * src + m];
    }
    const GraphResult rb = graph_solve(p.start.data(), p.status.data(), p.F, p.edges.data(), p.Qe.data(), p.info.data(), p.E, s, b.data());
    double spread = 0.0;
    for (size_t f = 0; f < n.F; ++f) spread = std::max(spread, angle_between(&a[4 * f], &b[4 * f]));
    std::printf("permuted edges: spread %.3e rad, cost %.9e and %.9e, ends %d %d\n", spread, ra.cost, rb.cost, (int)ra.end, (int)rb.end);
    CHECK(n.E == 27 && spread < 1e-8 && ra.cost > 0.0 && std::fabs(ra.cost - rb.cost) < 1e-9 * ra.cost);
    // the same call twice gives the same bits
    const GraphResult rc = graph_solve(n.start.data(), n.status.data(), n.F, n.edges.data(), n.Qe.data(), n.info.data(), n.E, s, b.data());
    CHECK(std::memcmp(a.data(), b.data(), a.size() * sizeof(double)) == 0 && rc.cost == ra.cost && rc.cg_iters == ra.cg_iters);
}

int main()
{
    test_jr_inv();
    test_refusals();
    test_solve();
    if (g_fail) { std::printf("%d checks failed\n", g_fail); return 1; }
    std::printf("OK graph_rule\n");
    return 0;
}
