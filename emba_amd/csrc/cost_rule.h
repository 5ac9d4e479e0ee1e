// emba_amd/csrc/cost_rule.h — the two cost terms of a trial point (solver.cpp:88-91, 265-268) as functions of plain values: the summand of one residual
// under the quadratic, Huber and Cauchy cost, the summand of one map pixel, the factors behind the sums, and the grid of the launch that sums them
// (cost_kernels.h: emba_costs_kernel; cost_host.h: the five entry points).
//
//     dataCost = cost_scale(irls, eta) * sum over inliers of cost_term(e, irls, eta)          regCost = reg_scale(alpha) * sum over pixels of reg_term(Gx, Gy)
//
// No HIP in here: plain C++17, so that tests/cpp/cost_rule_test.cpp checks it on a CPU in milliseconds.  cost_term and reg_term are compiled for the host
// and for the device, without contraction: the kernel and the CPU test run the same functions.
#pragma once
#include <stddef.h>

#include <algorithm>
#include <cmath>

#if !defined(EMBA_RULE_HD)
#if defined(__HIPCC__)
#define EMBA_RULE_HD __host__ __device__
#else
#define EMBA_RULE_HD
#endif
#endif

namespace emba {

// irls — 0 quadratic: e^2 (0.5*ep.dot(ep), solver.cpp:88); 2 Cauchy: log1p(eta e^2) (model.cpp:283-290); otherwise Huber: 0.5 e^2 below eta,
// eta |e| - 0.5 eta^2 from there on (model.cpp:294-312; the two branches meet at |e| = eta)
EMBA_RULE_HD inline double cost_term(double e, int irls, double eta)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    if (irls == 0) return e * e;
    if (irls == 2) return log1p(eta * (e * e));
    const double a = fabs(e);
    return (a < eta) ? 0.5 * a * a : eta * a - 0.5 * eta * eta;
}
inline double cost_scale(int irls, double eta) { return irls == 0 ? 0.5 : irls == 2 ? 0.5 / eta : 1.0; }

// evaluateRegError, model.cpp:260-277
EMBA_RULE_HD inline double reg_term(double gx, double gy)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    return gx * gx + gy * gy;
}
inline double reg_scale(double alpha) { return 0.5 * alpha; }

// The launch: blocks [0, nb_data) sum the data term over the n_pm entries of the window, the nb_reg blocks behind them the regulariser over the npix map
// pixels, kCostBlock entries per block and round.
// (a few hundred blocks: every block ends with two same-address atomics — its sum and its ticket —, and 4096 of them on one word serialise for longer than the sums take)
// A term that is not asked for, and a data term over nothing, gets no block; the regulariser that is asked for always has one; a launch has at least one
// block, because the last block is what publishes the sums.
constexpr int kCostBlock = 256;
struct CostGrid { int nb_data, nb_reg; };
inline CostGrid cost_grid(size_t n_pm, size_t npix, int n_cu, bool want_data, bool want_reg)
{
    const size_t cu = (size_t)std::max(n_cu, 1);
    auto blocks = [](size_t n) { return n / kCostBlock + (n % kCostBlock ? 1 : 0); };
    CostGrid g{};
    g.nb_data = want_data ? (int)std::min(blocks(n_pm), cu) : 0;
    g.nb_reg = want_reg ? (int)std::max<size_t>(1, std::min(blocks(npix), 2 * cu)) : 0;
    if (g.nb_data + g.nb_reg == 0) g.nb_data = 1;
    return g;
}

}  // namespace emba
