// tests/cpp/sim_rule_test.cpp — emba_amd/csrc/sim_rule.h on a CPU (plain C++17, no HIP; tests/test_sim_rule_cpu.py builds and runs it, also under the
// address and undefined-behaviour sanitizers): one step of one pixel at, below and above its threshold in both directions, the cap and what it carries, a
// step without a brightness change, the last nanosecond of a step, a step of one nanosecond, disarming and arming around an outside sample, the mark of an
// outside sample, the cut of F steps into chunks and the passes of the sort.
#include "../../emba_amd/csrc/sim_rule.h"

#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

using namespace emba;

static int g_fail = 0;
#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #cond); ++g_fail; } \
    } while (0)

struct Ev { int k; bool up; int64_t t; };
struct Run { SimStep r; double ref; std::vector<Ev> ev; };

static const double C_ON = 0.25, C_OFF = 0.375;      // binary fractions: the sums below are exact
static const int64_t T0 = 1000000000, D = 1000;

static Run step(double ref, double prev, double cur, int cap = 255, int64_t d = D)
{
    Run o{{0, false}, ref, {}};
    o.r = sim_step(&o.ref, prev, cur, T0, d, C_ON, C_OFF, cap, [&](int k, bool up, int64_t t) { o.ev.push_back(Ev{k, up, t}); });
    return o;
}

static void test_thresholds()
{
    const double below = std::nextafter(C_ON, 0.0), below_off = std::nextafter(C_OFF, 0.0);
    // rising: just below c_on nothing, at c_on one event at the step's last nanosecond, above it one event inside the step
    Run a = step(0.0, 0.0, below);
    CHECK(a.r.n == 0 && !a.r.capped && a.ev.empty() && a.ref == 0.0);
    a = step(0.0, 0.0, C_ON);
    CHECK(a.r.n == 1 && !a.r.capped && a.ev.size() == 1 && a.ev[0].k == 0 && a.ev[0].up && a.ref == C_ON);
    CHECK(a.ev[0].t == T0 + D - 1);      // frac == 1: off = d clamped to d - 1
    a = step(0.0, 0.0, 0.5);
    CHECK(a.r.n == 2 && a.ev[0].t == T0 + 500 && a.ev[1].t == T0 + D - 1 && a.ev[0].up && a.ev[1].up && a.ev[1].k == 1 && a.ref == 0.5);
    a = step(0.0, 0.0, 0.4);
    CHECK(a.r.n == 1 && a.ref == C_ON && a.ev[0].t == T0 + (int64_t)((0.25 / 0.4) * 1000.0));
    // falling: the other threshold
    a = step(0.0, 0.0, -below_off);
    CHECK(a.r.n == 0 && a.ev.empty());
    a = step(0.0, 0.0, -C_ON);      // c_on is not the falling threshold
    CHECK(a.r.n == 0);
    a = step(0.0, 0.0, -C_OFF);
    CHECK(a.r.n == 1 && !a.ev[0].up && a.ev[0].t == T0 + D - 1 && a.ref == -C_OFF);
    a = step(0.0, 0.0, -1.0);
    CHECK(a.r.n == 2 && !a.r.capped && a.ref == -0.75 && !a.ev[0].up && a.ev[0].t == T0 + 375 && a.ev[1].t == T0 + 750);
    // cur - ref == 0: not > 0, so the falling branch, and 0 >= c_off is false
    a = step(0.5, 0.25, 0.5);
    CHECK(a.r.n == 0 && !a.r.capped);
    // a sample that is not a number emits nothing and leaves the reference
    a = step(0.5, 0.25, std::numeric_limits<double>::quiet_NaN());
    CHECK(a.r.n == 0 && a.ref == 0.5);
}

static void test_cap_and_carry()
{
    // four thresholds of rise, the cap at 1: one event, three carried
    Run a = step(0.0, 0.0, 1.0, 1);
    CHECK(a.r.n == 1 && a.r.capped && a.ref == 0.25 && a.ev.size() == 1 && a.ev[0].t == T0 + 250);
    // the next step, no further change (cur == prev): frac = (ref - prev) / 0 — -inf becomes 0, every carried event lands on the step's first nanosecond
    Run b = step(a.ref, 1.0, 1.0, 2);
    CHECK(b.r.n == 2 && b.r.capped && b.ref == 0.75 && b.ev[0].t == T0 && b.ev[1].t == T0 && b.ev[0].up && b.ev[1].k == 1);
    Run c = step(b.ref, 1.0, 1.0, 2);
    CHECK(c.r.n == 1 && !c.r.capped && c.ref == 1.0 && c.ev[0].t == T0);      // ref == prev: 0 / 0 = NaN becomes 0
    // exactly as many events as the cap allows: the cap did not end the loop
    a = step(0.0, 0.0, 0.5, 2);
    CHECK(a.r.n == 2 && !a.r.capped);
    // cur == prev with a carried difference the other way round: +inf becomes 1
    a = step(1.0, 0.0, 0.0, 255);      // falling from a reference above: ref - prev > 0, divided by +0
    CHECK(a.r.n == 2 && !a.ev[0].up && a.ev[0].t == T0 + D - 1 && a.ev[1].t == T0 + D - 1 && a.ref == 0.25);
    // a carried reference behind prev while the brightness goes on rising: frac < 0 becomes 0, then the step's own events
    a = step(0.0, 0.5, 1.0, 255);
    CHECK(a.r.n == 4 && a.ev[0].t == T0 && a.ev[1].t == T0 && a.ev[2].t == T0 + 500 && a.ev[3].t == T0 + D - 1);
    // the cap at its largest
    a = step(0.0, 0.0, 100.0, 255);
    CHECK(a.r.n == 255 && a.r.capped && a.ref == 63.75 && a.ev.size() == 255);
}

static void test_short_and_long_steps()
{
    // d == 1: every event on the step's only nanosecond
    Run a = step(0.0, 0.0, 1.0, 255, 1);
    CHECK(a.r.n == 4);
    for (const Ev& e : a.ev) CHECK(e.t == T0);
    // the longest step: d = 2^52 - 1 is exact as a double, and frac == 1 stays inside the step
    const int64_t dmax = kSimMaxSpan - 1;
    a = step(0.0, 0.0, C_ON, 255, dmax);
    CHECK(a.r.n == 1 && a.ev[0].t == T0 + dmax - 1);
    a = step(0.0, 0.0, 0.5, 255, dmax);
    CHECK(a.ev[0].t == T0 + (int64_t)(0.5 * (double)dmax) && a.ev[1].t == T0 + dmax - 1);
}

static void test_frames()
{
    std::vector<Ev> ev;
    auto emit = [&](int k, bool up, int64_t t) { ev.push_back(Ev{k, up, t}); };
    SimPixel px{123.0, false};
    // f = 0 inside: armed on it, no event
    SimStep r = sim_frame(&px, true, 0.0, 1.0, T0, D, C_ON, C_OFF, 255, emit);
    CHECK(r.n == 0 && px.armed && px.ref == 1.0 && ev.empty());
    // a step of two thresholds
    r = sim_frame(&px, true, 1.0, 1.5, T0, D, C_ON, C_OFF, 255, emit);
    CHECK(r.n == 2 && px.armed && px.ref == 1.5 && ev.size() == 2);
    // outside: disarmed, whatever the sample holds; the reference is not read again
    r = sim_frame(&px, false, 1.5, 99.0, T0, D, C_ON, C_OFF, 255, emit);
    CHECK(r.n == 0 && !px.armed && ev.size() == 2);
    r = sim_frame(&px, false, 99.0, 99.0, T0, D, C_ON, C_OFF, 255, emit);
    CHECK(r.n == 0 && !px.armed);
    // inside again: the reference is the new sample, however far from the old one, and the step that ends here has no event
    r = sim_frame(&px, true, 99.0, -4.0, T0, D, C_ON, C_OFF, 255, emit);
    CHECK(r.n == 0 && px.armed && px.ref == -4.0 && ev.size() == 2);
    r = sim_frame(&px, true, -4.0, -4.375, T0, D, C_ON, C_OFF, 255, emit);
    CHECK(r.n == 1 && !ev.back().up && px.ref == -4.375);
    // the mark of an outside sample is known by its bits alone
    const double mark = sim_outside_mark();
    CHECK(mark != mark && sim_marked_outside(mark));
    CHECK(!sim_marked_outside(std::numeric_limits<double>::quiet_NaN()) && !sim_marked_outside(-std::numeric_limits<double>::quiet_NaN()));
    CHECK(!sim_marked_outside(0.0) && !sim_marked_outside(std::numeric_limits<double>::infinity()));
}

static void test_checks()
{
    const int64_t ok[3] = {5, 6, 8}, rep[3] = {5, 5, 8}, back[3] = {5, 8, 6}, wide[2] = {-1, kSimMaxSpan - 1}, widest[2] = {-1, kSimMaxSpan - 2};
    const int64_t ends[2] = {std::numeric_limits<int64_t>::min(), std::numeric_limits<int64_t>::max()};
    CHECK(sim_steps_ok(ok, 2) && !sim_steps_ok(rep, 2) && !sim_steps_ok(back, 2) && !sim_steps_ok(wide, 1) && sim_steps_ok(widest, 1) && !sim_steps_ok(ends, 1));
    CHECK(sim_threshold_ok(0.25) && !sim_threshold_ok(0.0) && !sim_threshold_ok(-1.0) && !sim_threshold_ok(std::numeric_limits<double>::infinity()));
    CHECK(!sim_threshold_ok(std::numeric_limits<double>::quiet_NaN()));
    CHECK(sim_sensor_fits(240 * 180) && sim_sensor_fits(16843009 - 1) && !sim_sensor_fits(16843009));      // (2^32 - 2) / 255 = 16 843 009.4: S * 255 <= 2^32 - 2
}

static void test_chunks()
{
    // 260 pixels: 32 MiB / (260 * 8 B) = 16 131 steps per chunk
    const size_t S = 260, per = sim_chunk_steps(S);
    CHECK(per == (kSimChunkMaxBytes / (S * 8)) && per == 16131);
    // F = 1; one chunk exactly; one chunk and one step
    CHECK(view_chunk_count(1, per) == 1 && view_chunk(1, per, 0).f0 == 0 && view_chunk(1, per, 0).nf == 1);
    CHECK(view_chunk_count(per, per) == 1 && view_chunk(per, per, 0).nf == per);
    CHECK(view_chunk_count(per + 1, per) == 2 && view_chunk(per + 1, per, 0).nf == per && view_chunk(per + 1, per, 1).f0 == per && view_chunk(per + 1, per, 1).nf == 1);
    // a tiny sensor stops at the grid's limit, a huge one keeps one step; a chunk's cells times 255 fit 32 bits
    CHECK(sim_chunk_steps(35) == kSimChunkMaxSteps && sim_chunk_steps(1) == kSimChunkMaxSteps && sim_chunk_steps((size_t)1 << 24) == 1);
    CHECK(sim_chunk_steps(240 * 180) == 97);
    for (size_t s : {(size_t)1, (size_t)35, (size_t)260, (size_t)43200, (size_t)1 << 22, ((size_t)1 << 22) + 1})
        CHECK((uint64_t)sim_chunk_steps(s) * s * kSimMaxPerStep <= kSimMaxEvents || sim_chunk_steps(s) == 1);
}

static void test_sort_plan()
{
    SimSortPlan p = sim_sort_plan(1);
    CHECK(p.lo_bits == 1 && p.hi_bits == 0);
    p = sim_sort_plan(30000000);      // 30 ms: keys below 2^25
    CHECK(p.lo_bits == 25 && p.hi_bits == 0);
    p = sim_sort_plan((uint64_t)1 << 32);      // keys 0 ... 2^32 - 1: still one sort
    CHECK(p.lo_bits == 32 && p.hi_bits == 0);
    p = sim_sort_plan(((uint64_t)1 << 32) + 1);      // the key 2^32 has a high word of 1
    CHECK(p.lo_bits == 32 && p.hi_bits == 1);
    p = sim_sort_plan(6000000000ull);
    CHECK(p.lo_bits == 32 && p.hi_bits == 1);
    p = sim_sort_plan(3 * ((uint64_t)1 << 32));      // high words 0, 1, 2
    CHECK(p.lo_bits == 32 && p.hi_bits == 2);
    p = sim_sort_plan((uint64_t)kSimMaxSpan);
    CHECK(p.lo_bits == 32 && p.hi_bits == 20);
}

int main()
{
    test_thresholds();
    test_cap_and_carry();
    test_short_and_long_steps();
    test_frames();
    test_checks();
    test_chunks();
    test_sort_plan();
    if (g_fail) { std::printf("%d FAILED\n", g_fail); return 1; }
    std::printf("OK sim_rule\n");
    return 0;
}
