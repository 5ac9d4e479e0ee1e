// What the host knows about the map planes (emba_amd/csrc/map_rule.h: MapState) on a CPU, against a second, deliberately naive model: the loose fields
// emba_ctx held before MapState, with the assignments of the handlers that used to write them, transcribed line for line (device buffers and the caller's
// tensors are numbers here: 0 is "not allocated", every allocation and every bound tensor gets a new one).  Every sequence of the transitions up to length 6,
// from the created state and from an uploaded one; after every step every query, both versions and the verdict of texels_stale (step_rule.h) must agree.
// Plain C++17, no HIP.  Built and run by tests/test_cpp_host.py.
#include <cstdint>
#include <cstdio>
#include <utility>

#include "../../emba_amd/csrc/map_rule.h"
#include "../../emba_amd/csrc/step_rule.h"

using namespace emba;

static long g_fail = 0;
#define CHECK(x) do { if (!(x)) { if (g_fail < 20) std::printf("FAIL %s:%d  %s\n", __FILE__, __LINE__, #x); ++g_fail; } } while (0)

// ---- the old model: emba_ctx's map fields and what each entry point did with them ----
struct Old {
    int d_Gx_own = 0, d_Gy_own = 0;
    int d_Gx = 0, d_Gy = 0;
    int d_Gx_cur = 0, d_Gy_cur = 0;
    int d_Gx_trial = 0, d_Gy_trial = 0; bool map_is_trial = false;
    bool map_bound = false;
    uint32_t map_version = 1, packed_version = 0;
    bool have_map = false;
    int next_buf = 1, next_tensor = 1000;
    void ensure(int& b) { if (!b) b = next_buf++; }      // DevBuf::ensure at one size: allocates once
    void map_changed() { ++map_version; }

    bool upload_map()
    {
        ensure(d_Gx_own); ensure(d_Gy_own);
        d_Gx = d_Gx_cur = d_Gx_own; d_Gy = d_Gy_cur = d_Gy_own;
        map_is_trial = false; map_bound = false;
        have_map = true;
        map_changed();
        return true;
    }
    bool bind_map_dev()
    {
        const int Gx_dev = next_tensor++, Gy_dev = next_tensor++;
        d_Gx = d_Gx_cur = Gx_dev; d_Gy = d_Gy_cur = Gy_dev;
        map_is_trial = false; map_bound = true;
        have_map = true;
        map_changed();
        return true;
    }
    bool update_map()
    {
        if (!have_map) return false;
        ensure(d_Gx_trial); ensure(d_Gy_trial);
        d_Gx = d_Gx_trial; d_Gy = d_Gy_trial;
        map_is_trial = true;
        map_changed();
        return true;
    }
    bool map_accept()
    {
        if (!map_is_trial) return false;
        std::swap(d_Gx_own, d_Gx_trial); std::swap(d_Gy_own, d_Gy_trial);
        d_Gx_cur = d_Gx = d_Gx_own; d_Gy_cur = d_Gy = d_Gy_own;
        map_is_trial = false; map_bound = false;
        map_changed();
        return true;
    }
    bool map_reject()
    {
        if (d_Gx != d_Gx_cur || d_Gy != d_Gy_cur) map_changed();
        d_Gx = d_Gx_cur; d_Gy = d_Gy_cur;
        map_is_trial = false;
        return true;
    }
    bool median_blur3_map()
    {
        if (!have_map) return false;
        if (map_is_trial) return false;
        const bool own = d_Gx_cur == d_Gx_own && d_Gy_cur == d_Gy_own;
        if (!own) { ensure(d_Gx_own); ensure(d_Gy_own); }
        const int dst[2] = {d_Gx_own, d_Gy_own};
        d_Gx = d_Gx_cur = dst[0]; d_Gy = d_Gy_cur = dst[1];
        map_bound = false;
        map_changed();
        return true;
    }
    bool pack_texels()      // launch_prep_pose_texel with texel blocks (an evaluation: it needs a map)
    {
        if (!have_map) return false;
        packed_version = map_version;
        return true;
    }
    // the expressions the call sites derived
    bool map_owned() const { return map_is_trial || !map_bound; }                              // step_host.h
    bool cur_own() const { return d_Gx_cur == d_Gx_own && d_Gy_cur == d_Gy_own; }              // the blur
    bool trial_pending_by_pointer() const { return d_Gx != d_Gx_cur || d_Gy != d_Gy_cur; }     // the reject
};

enum Transition { kUpload, kBind, kUpdate, kAccept, kReject, kBlur, kPacked, kNumTransitions };

// the new side, with the preconditions map_host.h / step_host.h ask of the state before they call the transition
static bool apply_new(MapState& m, int t)
{
    switch (t) {
    case kUpload: m.uploaded(); return true;
    case kBind: m.bound(); return true;
    case kUpdate: if (!m.resident()) return false; m.trial_built(); return true;
    case kAccept: if (!m.trial_pending()) return false; m.accepted(); return true;
    case kReject: m.rejected(); return true;
    case kBlur: if (!m.resident() || m.trial_pending()) return false; m.blurred(); return true;
    default: if (!m.resident()) return false; m.texels_packed(); return true;
    }
}
static bool apply_old(Old& o, int t)
{
    switch (t) {
    case kUpload: return o.upload_map();
    case kBind: return o.bind_map_dev();
    case kUpdate: return o.update_map();
    case kAccept: return o.map_accept();
    case kReject: return o.map_reject();
    case kBlur: return o.median_blur3_map();
    default: return o.pack_texels();
    }
}

// verdict word and step number: no step yet, a fresh verdict, the last step's verdict, "the box left the packed one"
static const int kSeqs[4][2] = {{0, 0}, {7, 7}, {6, 7}, {0, 7}};
static bool g_clause_seen[4][2];      // every clause of texels_stale, false and true
static long g_stale_seen[2], g_steps = 0, g_refused = 0;

static void compare(const MapState& m, const Old& o)
{
    CHECK(m.resident() == o.have_map);
    CHECK(m.trial_pending() == o.map_is_trial);
    CHECK(m.trial_pending() == o.trial_pending_by_pointer());
    CHECK(m.reads_own_memory() == o.map_owned());
    CHECK(m.current_is_own() == o.cur_own());
    CHECK(m.version() == o.map_version);
    CHECK(m.packed_version() == o.packed_version);
    for (const auto& q : kSeqs) {
        const bool a = texels_stale(m.reads_own_memory(), m.version(), m.packed_version(), q[0], q[1]);
        const bool b = texels_stale(o.map_owned(), o.map_version, o.packed_version, q[0], q[1]);
        CHECK(a == b);
        g_stale_seen[b] += 1;
        g_clause_seen[0][!o.map_owned()] = true;
        g_clause_seen[1][o.map_version != o.packed_version] = true;
        g_clause_seen[2][q[1] == 0] = true;
        g_clause_seen[3][q[0] != q[1]] = true;
    }
}

static void walk(const MapState& m, const Old& o, int depth)
{
    if (depth == 6) return;
    for (int t = 0; t < kNumTransitions; ++t) {
        MapState m2 = m; Old o2 = o;
        const bool did_new = apply_new(m2, t), did_old = apply_old(o2, t);
        CHECK(did_new == did_old);      // the state refuses what the old handlers refused: accept without a trial, blur with one, update / blur / evaluation without a map
        if (!did_new || !did_old) { ++g_refused; continue; }
        ++g_steps;
        compare(m2, o2);
        // the version never decreases; it stays only across a reject without a pending trial and across "packed"
        CHECK(m2.version() >= m.version());
        const bool may_stay = t == kPacked || (t == kReject && !m.trial_pending());
        CHECK((m2.version() == m.version()) == may_stay);
        walk(m2, o2, depth + 1);
    }
}

int main()
{
    MapState m; Old o;
    CHECK(m.version() == 1 && m.packed_version() == 0 && !m.resident() && !m.trial_pending());      // emba_create
    compare(m, o);
    walk(m, o, 0);
    m.uploaded(); o.upload_map();
    compare(m, o);
    walk(m, o, 0);
    for (int k = 0; k < 4; ++k) CHECK(g_clause_seen[k][0] && g_clause_seen[k][1]);
    CHECK(g_stale_seen[0] > 0 && g_stale_seen[1] > 0);
    CHECK(g_steps > 0 && g_refused > 0);
    if (g_fail) { std::printf("%ld checks failed\n", g_fail); return 1; }
    std::printf("%ld steps, %ld refused\nOK map_rule\n", g_steps, g_refused);
    return 0;
}
