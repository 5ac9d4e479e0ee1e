// emba_amd/csrc/map_rule.h — what the host knows about the map planes (context.h: MapPlanes holds the buffers and pointers, map_host.h the calls), as a
// value with named transitions.  Plain C++17, no HIP: tests/cpp/map_rule_test.cpp walks every sequence of the transitions against the loose fields and
// hand-written assignments this replaced.
#pragma once

#include <cstdint>

namespace emba {

// Whether a map is resident, whose memory its current (accepted) planes are, whether a trial map is pending, and the count of the calls that changed or
// rebound the planes next to the count the last texel pack read (step_rule.h: texels_stale).  The members change through the transitions only: every
// transition that changes or rebinds the planes counts itself, so that no call site can forget to.
struct MapState {
    bool resident() const { return resident_; }               // a map has been uploaded or bound
    bool trial_pending() const { return trial_; }             // emba_update_map built a trial map: the next evaluation reads it, not the current planes
    bool current_is_own() const { return !bound_; }           // the current planes are the context's own buffers, not memory the caller bound
    bool reads_own_memory() const { return trial_ || !bound_; }   // the planes the next evaluation reads are the context's own memory: they change through a
                                                                  // call only (the trial map is always the context's own; a bound map is the caller's)
    uint32_t version() const { return version_; }             // counts the calls that change or rebind the planes
    uint32_t packed_version() const { return packed_; }       // the count the last texel pack read

    void uploaded() { resident_ = true; trial_ = false; bound_ = false; ++version_; }   // emba_upload_map (a pending trial is dropped)
    void bound() { resident_ = true; trial_ = false; bound_ = true; ++version_; }       // emba_bind_map_dev (a pending trial is dropped)
    void trial_built() { trial_ = true; ++version_; }                                   // emba_update_map[_dev]: also a second one before an accept
    // emba_map_accept: the same values at the same addresses as the trial map's; counted all the same: every rebinding is
    void accepted() { trial_ = false; bound_ = false; ++version_; }
    // emba_map_reject: counted only when a trial was pending (none: a step that moved the poses only was rejected, the planes stay)
    void rejected() { if (trial_) ++version_; trial_ = false; }
    void blurred() { bound_ = false; ++version_; }            // emba_median_blur3_map: the blurred planes are the context's own
    void texels_packed() { packed_ = version_; }              // the launch in front of the warp kernel carried texel blocks: they describe this count's planes

private:
    bool resident_ = false, bound_ = false, trial_ = false;
    uint32_t version_ = 1, packed_ = 0;
};

}  // namespace emba
