// tests/cpp/contrast_prior_rule_test.cpp — the prior additions of emba_amd/csrc/contrast_rule.h on a CPU (plain C++17, no HIP;
// tests/test_contrast_prior_cpu.py builds and runs it, once plain and once with -fsanitize=address,undefined): the level mask of
// emba_seq_contrast_prior_add — what is refused and which level is named —, the order its levels are voted in, the weight of a call, and the cell the image
// starts from; then the rule itself on a small grid: with a prior the image is prior_weight P plus the votes, J its sum of squares, and an event's
// gradient the existing contrast_event_grad on that image.
#include "../../emba_amd/csrc/contrast_rule.h"

#include <cstdio>
#include <limits>
#include <vector>

using namespace emba;

static int g_fail = 0;
#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #cond); ++g_fail; } \
    } while (0)

static void test_mask()
{
    static_assert(kContrastLevels == 9, "levels 0 ... 8");
    int bad = -7;
    CHECK(contrast_prior_mask_ok(512, 256, 0, &bad) == ContrastMaskStatus::empty && bad == -7);
    CHECK(contrast_prior_mask_ok(512, 256, 1u << 9, &bad) == ContrastMaskStatus::bad_bit && bad == -7);
    CHECK(contrast_prior_mask_ok(512, 256, 0x80000001u, &bad) == ContrastMaskStatus::bad_bit);
    CHECK(contrast_prior_mask_ok(512, 256, 0xFFFFFFFFu) == ContrastMaskStatus::bad_bit);
    CHECK(contrast_prior_mask_ok(1 << 20, 1 << 19, 0x1FF, &bad) == ContrastMaskStatus::ok && bad == -7);      // every level
    CHECK(contrast_prior_mask_ok(512, 256, 0x0FF) == ContrastMaskStatus::ok);                                 // 0 ... 7: two rows left at 7
    CHECK(contrast_prior_mask_ok(512, 256, 0x1FF, &bad) == ContrastMaskStatus::bad_level && bad == 8);        // one row left at 8
    bad = -7;
    CHECK(contrast_prior_mask_ok(516, 260, 0x0F, &bad) == ContrastMaskStatus::bad_level && bad == 3);         // 516 = 4 x 129
    CHECK(contrast_prior_mask_ok(516, 260, 0x07) == ContrastMaskStatus::ok);
    CHECK(contrast_prior_mask_ok(516, 260, 0x18, &bad) == ContrastMaskStatus::bad_level && bad == 3);         // the lowest refused level
    CHECK(contrast_prior_mask_ok(516, 260, 0x18) == ContrastMaskStatus::bad_level);                           // (no pointer given)
    for (int l = 0; l < kContrastLevels; ++l)
        CHECK((contrast_prior_mask_ok(1024, 512, 1u << l) == ContrastMaskStatus::ok) == (contrast_level_ok(1024, 512, l) == ContrastLevelStatus::ok));
}

static void test_levels_of_a_mask()
{
    int lv[kContrastLevels];
    CHECK(contrast_prior_levels(0, lv) == 0);
    CHECK(contrast_prior_levels(0x0F, lv) == 4 && lv[0] == 0 && lv[1] == 1 && lv[2] == 2 && lv[3] == 3);
    CHECK(contrast_prior_levels(0x104, lv) == 2 && lv[0] == 2 && lv[1] == 8);
    CHECK(contrast_prior_levels(0x1FF, lv) == kContrastLevels && lv[8] == 8);
    CHECK(contrast_prior_levels(0xFFFFFFFFu, lv) == kContrastLevels);      // (bits a checked mask cannot have: never past the array)
}

static void test_weight_and_cell()
{
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    CHECK(contrast_prior_weight_ok(0.0) && contrast_prior_weight_ok(-0.0) && contrast_prior_weight_ok(0.25) && contrast_prior_weight_ok(1.0));
    CHECK(contrast_prior_weight_ok(std::numeric_limits<double>::max()) && contrast_prior_weight_ok(std::numeric_limits<double>::denorm_min()));
    CHECK(!contrast_prior_weight_ok(-1.0) && !contrast_prior_weight_ok(-1e-300) && !contrast_prior_weight_ok(inf) && !contrast_prior_weight_ok(-inf) && !contrast_prior_weight_ok(nan));
    CHECK(contrast_prior_cell(1.0, -3.5) == -3.5 && contrast_prior_cell(0.25, 8.0) == 2.0 && contrast_prior_cell(0.0, 5.0) == 0.0 && contrast_prior_cell(2.0, 0.0) == 0.0);
}

// The rule on a 8 x 4 grid, two events: the image with a prior is weight * P + votes; an event's ge is contrast_event_grad on that image, which is the
// ge of the votes alone plus the ge of the prior alone (the gradient is linear in the image it gathers).
static void test_the_rule_on_a_small_grid()
{
    const int W = 8, H = 4;
    const double weight = 0.25;
    std::vector<double> P(W * H), votes(W * H, 0.0), I(W * H);
    for (int i = 0; i < W * H; ++i) P[i] = (i % 5) - 2.0;      // negative cells included
    const double pm[2][2] = {{7.25, 1.5}, {2.75, 2.125}};      // the first wraps over the column seam
    ContrastVotes v[2];
    for (int k = 0; k < 2; ++k) {
        v[k] = contrast_vote(pm[k][0], pm[k][1], W, H);
        for (int i = 0; i < 4; ++i) { CHECK(v[k].cell[i] >= 0 && v[k].cell[i] < W * H); votes[v[k].cell[i]] += v[k].w[i]; }
    }
    double J = 0.0, J_votes = 0.0, J_prior = 0.0, cross = 0.0;
    for (int i = 0; i < W * H; ++i) {
        I[i] = contrast_prior_cell(weight, P[i]) + votes[i];
        J += I[i] * I[i];
        J_votes += votes[i] * votes[i];
        J_prior += weight * P[i] * weight * P[i];
        cross += weight * P[i] * votes[i];
    }
    CHECK(std::fabs(J - (J_votes + 2.0 * cross + J_prior)) <= 1e-12 * J);      // own contrast + twice the correlation + a constant
    const double D[12] = {1, 0.5, -0.25, 2, 0, 1, -1, 0.75, 0.5, 0, 3, -2};
    for (int k = 0; k < 2; ++k) {
        double a[4], b[4], c[4], ga[6], gb[6], gc[6];
        for (int i = 0; i < 4; ++i) { a[i] = I[v[k].cell[i]]; b[i] = votes[v[k].cell[i]]; c[i] = contrast_prior_cell(weight, P[v[k].cell[i]]); }
        contrast_event_grad(v[k], a, D, 1.0, ga);
        contrast_event_grad(v[k], b, D, 1.0, gb);
        contrast_event_grad(v[k], c, D, 1.0, gc);
        for (int j = 0; j < 6; ++j) CHECK(std::fabs(ga[j] - (gb[j] + gc[j])) <= 1e-12 * (std::fabs(gb[j]) + std::fabs(gc[j]) + 1.0));
    }
}

int main()
{
    test_mask();
    test_levels_of_a_mask();
    test_weight_and_cell();
    test_the_rule_on_a_small_grid();
    if (g_fail) { std::printf("%d checks failed\n", g_fail); return 1; }
    std::printf("OK contrast_prior_rule\n");
    return 0;
}
