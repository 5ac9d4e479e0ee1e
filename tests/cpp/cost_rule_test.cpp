// tests/cpp/cost_rule_test.cpp — emba_amd/csrc/cost_rule.h (plain C++17, no HIP): the summand of one residual under the three costs against closed forms
// and around Huber's threshold, the factors behind the sums, and the grid of the cost launch at every size where its arithmetic can go wrong.
// Built and run by tests/test_cost_rule_cpu.py, which also compares the TERM lines printed here with the oracle.
#include <cmath>
#include <cstdio>

#include "../../emba_amd/csrc/cost_rule.h"

using namespace emba;

static int g_fail = 0;
#define CHECK(x) do { if (!(x)) { std::printf("FAIL %s:%d  %s\n", __FILE__, __LINE__, #x); ++g_fail; } } while (0)

static bool close(double a, double b, double rel = 1e-15) { return std::fabs(a - b) <= rel * std::fmax(std::fabs(a), std::fabs(b)); }

int main()
{
    // ---- cost_term at e = 0: nothing, under every cost
    for (int irls = 0; irls <= 2; ++irls)
        for (double eta : {0.1, 1.0, 5.0, 1e9}) CHECK(cost_term(0.0, irls, eta) == 0.0 && cost_term(-0.0, irls, eta) == 0.0);

    // ---- closed forms, both signs
    for (double e : {1e-9, 0.003, 0.25, 1.0, 7.5, 1e4})
        for (double s : {1.0, -1.0}) {
            CHECK(cost_term(s * e, 0, 0.0) == e * e);
            for (double eta : {0.1, 1.0, 5.0}) {
                const double x = eta * e * e;
                if (x >= 1e-3) CHECK(close(cost_term(s * e, 2, eta), std::log(1.0 + x), 1e-12));      // (below that log(1 + x) loses what log1p keeps)
                else CHECK(close(cost_term(s * e, 2, eta), x - 0.5 * x * x, 1e-8));                    // the series, to its third term's size
                CHECK(close(cost_term(s * e, 2, eta), std::log1p(x), 4e-15));
                const double huber = e < eta ? 0.5 * e * e : eta * (e - 0.5 * eta);
                CHECK(close(cost_term(s * e, 1, eta), huber, 1e-14));
            }
            CHECK(cost_term(s * e, 1, 1e9) == 0.5 * e * e);                                                             // a threshold nothing reaches: half the square
        }
    CHECK(close(cost_term(1e-9, 2, 0.1), 0.1 * 1e-18, 1e-12));      // Cauchy of a small residual: eta e^2

    // ---- Huber just below, at and just above eta: the branches meet there (value eta^2 / 2), the quadratic one below, the linear one from eta on
    for (double eta : {0.1, 1.0, 5.0}) {
        const double lo = std::nextafter(eta, 0.0), hi = std::nextafter(eta, 2.0 * eta), mid = 0.5 * eta * eta;
        CHECK(cost_term(lo, 1, eta) == 0.5 * lo * lo);
        CHECK(cost_term(eta, 1, eta) == eta * eta - 0.5 * eta * eta);
        CHECK(cost_term(hi, 1, eta) == eta * hi - 0.5 * eta * eta);
        CHECK(close(cost_term(lo, 1, eta), mid, 4e-15) && close(cost_term(eta, 1, eta), mid, 4e-15) && close(cost_term(hi, 1, eta), mid, 4e-15));      // no step across the seam
        CHECK(cost_term(-eta, 1, eta) == cost_term(eta, 1, eta) && cost_term(-hi, 1, eta) == cost_term(hi, 1, eta));
    }

    // ---- the factors behind the sums
    CHECK(cost_scale(0, 0.0) == 0.5 && cost_scale(0, 3.0) == 0.5);
    CHECK(cost_scale(1, 0.1) == 1.0 && cost_scale(1, 1e9) == 1.0);
    CHECK(cost_scale(2, 0.1) == 0.5 / 0.1 && cost_scale(2, 5.0) == 0.1);
    CHECK(reg_scale(0.0) == 0.0 && reg_scale(5.0) == 2.5 && reg_scale(0.4) == 0.2);
    CHECK(reg_term(0.0, 0.0) == 0.0 && reg_term(3.0, -4.0) == 25.0 && reg_term(-0.5, 0.0) == 0.25);

    // ---- the grid
    const size_t sizes[] = {0, 1, 255, 256, 257, (size_t)1 << 31};
    for (int n_cu : {1, 8, 256, 304})
        for (size_t n_pm : sizes)
            for (size_t npix : sizes)
                for (int want = 1; want < 4; ++want) {
                    const bool wd = want & 1, wr = want & 2;
                    const CostGrid g = cost_grid(n_pm, npix, n_cu, wd, wr);
                    CHECK(g.nb_data >= 0 && g.nb_data <= n_cu);
                    CHECK(g.nb_reg >= 0 && g.nb_reg <= 2 * n_cu);
                    CHECK((g.nb_reg == 0) == !wr);
                    CHECK(g.nb_data + g.nb_reg >= 1);
                    // every block has work in its first round, or it is the one block a launch or an asked-for regulariser always has
                    if (g.nb_data) CHECK((size_t)(g.nb_data - 1) * kCostBlock < n_pm || (g.nb_data == 1 && g.nb_reg == 0));
                    if (g.nb_reg) CHECK((size_t)(g.nb_reg - 1) * kCostBlock < npix || g.nb_reg == 1);
                    if (!wd) CHECK(g.nb_data == 0);      // (want >= 1: then the regulariser is asked for and has its block)
                    // below the cap: one block per kCostBlock entries
                    if (wd && n_pm && n_pm <= (size_t)n_cu * kCostBlock) CHECK((size_t)g.nb_data == (n_pm + kCostBlock - 1) / kCostBlock);
                    if (wr && npix && npix <= (size_t)2 * n_cu * kCostBlock) CHECK((size_t)g.nb_reg == (npix + kCostBlock - 1) / kCostBlock);
                    if (wd && n_pm > (size_t)n_cu * kCostBlock) CHECK(g.nb_data == n_cu);
                    if (wr && npix > (size_t)2 * n_cu * kCostBlock) CHECK(g.nb_reg == 2 * n_cu);
                }
    {   // hand-computed
        CostGrid g = cost_grid(1000000, 1024 * 512, 256, true, true);   CHECK(g.nb_data == 256 && g.nb_reg == 512);
        g = cost_grid(257, 300, 256, true, true);                       CHECK(g.nb_data == 2 && g.nb_reg == 2);
        g = cost_grid(0, 300, 256, true, true);                         CHECK(g.nb_data == 0 && g.nb_reg == 2);      // no inliers to sum: the regulariser's blocks alone
        g = cost_grid(0, 0, 256, true, false);                          CHECK(g.nb_data == 1 && g.nb_reg == 0);      // the one block that publishes a zero
        g = cost_grid(5000, 300, 256, false, true);                     CHECK(g.nb_data == 0 && g.nb_reg == 2);      // regCost alone
    }

    // ---- single residuals for the comparison with the oracle: TERM irls eta e cost_scale*cost_term (17 significant digits)
    for (int irls = 0; irls <= 2; ++irls)
        for (double eta : {0.1, 5.0})
            for (double e : {0.0, 1e-6, -0.03, 0.0999999, 0.1, 0.1000001, -0.7, 4.9999, 5.0, 5.0001, 123.456})
                std::printf("TERM %d %.17g %.17g %.17g\n", irls, eta, e, cost_scale(irls, eta) * cost_term(e, irls, eta));

    if (g_fail) { std::printf("%d checks failed\n", g_fail); return 1; }
    std::printf("OK cost_rule\n");
    return 0;
}
