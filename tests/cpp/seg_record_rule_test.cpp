// tests/cpp/seg_record_rule_test.cpp — emba_amd/csrc/seg_record_rule.h compiled for the host (plain C++17, no HIP): the segment records the host forms for a
// steady step (option step_prep = 2).  Built and run by tests/test_seg_record_rule_cpu.py, which feeds it the control-pose pairs of the reference's golden spline
// cases (tests/golden/so3_spline_n2.npz: general, tiny, identical, on_knot, near_pi) and compares what it writes with the oracle's restatement.
//
//   seg_record_rule_test IN OUT     IN: int32 n, then n x 8 doubles {p0 xyzw, p1 xyzw};  OUT: n x 12 doubles, the records
//   seg_record_rule_test            the hand-computed cases below only
//
// Bounds — MEASURED, not chosen: tests/golden/seg_records_device_gfx950.npz holds the records the device's launch in front of the warp kernel (step_prep = 0)
// formed for the same golden pairs on gfx950 (tests/test_gpu_step_prep_host.py checks that it still forms exactly these).  Their largest differences from the oracle:
//   delta 2.22e-16 (2^-52)   r1 1.11e-16 (2^-53)   k 2.22e-16 (2^-52)   Jl^-1 = I + r1 A + r2 A^2 (r2) 7.77e-16 (7 x 2^-53), the largest of all   spline value q 1.11e-16 (2^-53)
// and the bound on each quantity is 4 x its own figure (none above 4 x 7.77e-16 = 3.11e-15): 8.9e-16, 4.4e-16, 8.9e-16, 3.1e-15, 4.4e-16, absolute; p0 is copied: identical.
// The host's records measured the same way (g++ and hipcc's host compiler, glibc): 2.22e-16, 1.11e-16, 2.22e-16, 3.33e-16 ... 7.77e-16, 0 ... 1.11e-16; host against device
// word by word: at most 2.22e-16 (delta, k), 1.11e-16 (r1), 7.77e-16 (r2).  The Python side recomputes the device figures from the fixture and holds every form to the bounds.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../emba_amd/csrc/seg_record_rule.h"
#include "../../emba_amd/csrc/step_rule.h"

using namespace emba;

static int g_fail = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); ++g_fail; } } while (0)

static const double kTolDelta = 4 * 0x1p-52, kTolR1 = 4 * 0x1p-53, kTolK = 4 * 0x1p-52, kTolR2 = 4 * 7 * 0x1p-53;      // (header)

static void axis_angle(double x, double y, double z, double ang, double* q)
{
    const double n = std::sqrt(x * x + y * y + z * z), s = std::sin(0.5 * ang) / n;
    q[0] = s * x; q[1] = s * y; q[2] = s * z; q[3] = std::cos(0.5 * ang);
}

static void hand_cases()
{
    const double id[4] = {0, 0, 0, 1};
    double seg[kSegRecordDoubles], q[4];
    // identical poses: the small-angle branch of the logarithm, theta = 0, no axis
    segment_consts(id, id, seg);
    for (int i = 0; i < 4; ++i) CHECK(seg[i] == id[i]);
    for (int i = 4; i < 12; ++i) CHECK(seg[i] == 0.0);
    // a quarter turn about z from the identity: delta = (0, 0, pi/2), k = z, r1 = -pi/4, r2 = 1 - (pi/2)(1 + 0)/2
    axis_angle(0, 0, 1, 0.5 * kPi, q);
    segment_consts(id, q, seg);
    CHECK(std::fabs(seg[4]) <= kTolDelta && std::fabs(seg[5]) <= kTolDelta && std::fabs(seg[6] - 0.5 * kPi) <= kTolDelta);
    CHECK(std::fabs(seg[7] + 0.25 * kPi) <= kTolR1);
    CHECK(std::fabs(seg[8]) <= kTolK && std::fabs(seg[9]) <= kTolK && std::fabs(seg[10] - 1.0) <= kTolK);
    CHECK(std::fabs(seg[11] - (1.0 - 0.25 * kPi)) <= kTolR2);
    // a tiny relative rotation (|delta|^2 below the Taylor switch of Jl^-1): r2 = theta^2 / 12
    axis_angle(1, 2, -1, 1e-6, q);
    segment_consts(id, q, seg);
    const double th = std::sqrt(seg[4] * seg[4] + seg[5] * seg[5] + seg[6] * seg[6]);
    CHECK(std::fabs(th - 1e-6) <= 1e-6 * 1e-9 && seg[11] == (seg[4] * seg[4] + seg[5] * seg[5] + seg[6] * seg[6]) / 12.0 && seg[7] == -0.5 * th);
    // past pi - sqrt(eps): the near-pi branch, r2 = theta^2 / pi^2
    axis_angle(0, 1, 0, kPi - 1e-7, q);
    segment_consts(id, q, seg);
    CHECK(std::fabs(seg[5] - (kPi - 1e-7)) <= kTolDelta && std::fabs(seg[11] - (kPi - 1e-7) * (kPi - 1e-7) / (kPi * kPi)) <= kTolR2);
    // K poses give K - 1 records, record s from poses s and s + 1, and nothing is written behind them
    double knots[12], out[3 * kSegRecordDoubles];
    std::memcpy(knots, id, sizeof id); axis_angle(1, 0, 0, 0.3, knots + 4); axis_angle(1, 1, 0, 0.5, knots + 8);
    for (double& v : out) v = -7.0;
    segment_records(knots, 3, out);
    double one[kSegRecordDoubles];
    segment_consts(knots + 4, knots + 8, one);
    CHECK(std::memcmp(out + kSegRecordDoubles, one, sizeof one) == 0);
    for (int i = 2 * kSegRecordDoubles; i < 3 * kSegRecordDoubles; ++i) CHECK(out[i] == -7.0);
    segment_records(knots, 1, out + 2 * kSegRecordDoubles);      // one pose: no record
    CHECK(out[2 * kSegRecordDoubles] == -7.0);
}

// step_rule.h: which steady steps the host forms the records for (prep_on_host), beside the in-kernel producer's rule (prep_inside_warp).
// arguments: step_prep, tile_order, segpose, K, carrier (records / knots), n_sorted, clearing blocks, texel blocks, Hessian source
static void rule_cases()
{
    const int cap = 35;
    CHECK(prep_on_host(2, false, true, 21, cap, 1000, 0, 0, 3));                  // the steady step
    CHECK(prep_on_host(2, false, true, 21, cap, 1000, 0, 0, 0));                  // ... with the stencil as the Hessian source too
    CHECK(!prep_on_host(2, false, true, 21, cap, 1000, 0, 0, 1));                 // every texel packed: the launch packs them
    CHECK(!prep_on_host(0, false, true, 21, cap, 1000, 0, 0, 3));                 // the option's other values
    CHECK(!prep_on_host(1, false, true, 21, cap, 1000, 0, 0, 3));
    CHECK(!prep_on_host(3, false, true, 21, cap, 1000, 0, 0, 3));
    CHECK(!prep_on_host(2, true, true, 21, cap, 1000, 0, 0, 3));                  // tile order
    CHECK(!prep_on_host(2, false, false, 21, cap, 1000, 0, 0, 3));                // the per-batch pose table
    CHECK(!prep_on_host(2, false, true, 21, cap, 0, 0, 0, 3));                    // an empty window launches no warp kernel
    CHECK(!prep_on_host(2, false, true, 21, cap, 1000, 1, 0, 3));                 // lines to clear
    CHECK(!prep_on_host(2, false, true, 21, cap, 1000, 0, 1024, 3));              // stale texels
    CHECK(prep_on_host(2, false, true, cap, cap, 1000, 0, 0, 3));                 // K - 1 == cap - 1
    CHECK(prep_on_host(2, false, true, cap + 1, cap, 1000, 0, 0, 3));             // K - 1 == cap: the last that fits
    CHECK(!prep_on_host(2, false, true, cap + 2, cap, 1000, 0, 0, 3));            // K - 1 == cap + 1: the launch
    CHECK(prep_on_host(2, false, true, 2, cap, 1000, 0, 0, 3));                   // one record
    CHECK(!prep_on_host(2, false, true, 1, cap, 1000, 0, 0, 3));                  // K < 2: no record to form
    CHECK(!prep_on_host(2, false, true, 0, cap, 1000, 0, 0, 3));
    // the two rules never both hold: step_prep = 2 is not the in-kernel producer, step_prep = 1 not the host
    CHECK(prep_inside_warp(1, false, true, 21, 32, 1000, 0, 0, 3));
    CHECK(!prep_inside_warp(2, false, true, 21, 32, 1000, 0, 0, 3));
    CHECK(!prep_inside_warp(0, false, true, 21, 32, 1000, 0, 0, 3));
    for (int sp = 0; sp <= 3; ++sp)
        for (int K = 0; K <= cap + 3; ++K)
            CHECK(!(prep_on_host(sp, false, true, K, cap, 1000, 0, 0, 3) && prep_inside_warp(sp, false, true, K, 32, 1000, 0, 0, 3)));
}

int main(int argc, char** argv)
{
    hand_cases();
    rule_cases();
    if (argc == 3) {
        std::FILE* f = std::fopen(argv[1], "rb");
        int32_t n = 0;
        if (!f || std::fread(&n, sizeof n, 1, f) != 1 || n < 0) { std::printf("FAIL cannot read %s\n", argv[1]); return 2; }
        std::vector<double> in((size_t)8 * n), out((size_t)kSegRecordDoubles * n);
        if (std::fread(in.data(), sizeof(double), in.size(), f) != in.size()) { std::printf("FAIL short read\n"); return 2; }
        std::fclose(f);
        for (int32_t i = 0; i < n; ++i) segment_consts(&in[(size_t)8 * i], &in[(size_t)8 * i + 4], &out[(size_t)kSegRecordDoubles * i]);
        f = std::fopen(argv[2], "wb");
        if (!f || std::fwrite(out.data(), sizeof(double), out.size(), f) != out.size()) { std::printf("FAIL cannot write %s\n", argv[2]); return 2; }
        std::fclose(f);
    }
    if (g_fail) return 1;
    std::printf("OK seg_record_rule\n");
    return 0;
}
