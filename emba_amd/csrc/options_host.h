// emba_amd/csrc/options_host.h — tuning and A/B switches (documented, versioned by EMBA_ABI_VERSION; not environment variables): the one table
// of what emba_set_option sets, and the read-only names emba_get_option answers besides.  tests/option_matrix.py reads kOptions from this file: every name in
// it has a GPU parity test for each value that selects a branch, or a stated exemption (tests/test_option_matrix_cpu.py).
// Part of emba_hip.hip's translation unit.
#pragma once
#include "context.h"

using namespace emba;

namespace {

// reorders: a change invalidates the device order, which is rebuilt at the next evaluation
struct OptionRef { const char* name; int emba_ctx::*field; int lo, hi; bool reorders; };
const OptionRef kOptions[] = {
    {"step_ep", &emba_ctx::step_ep, 0, 2, false},
    {"step_fast", &emba_ctx::step_fast, 0, 1, false},
    {"step_gather", &emba_ctx::step_gather, 0, 3, false},
    {"step_one_set", &emba_ctx::step_one_set, 0, 1, false},
    {"gram_tags", &emba_ctx::use_tags, 0, 1, false},
    {"segpose", &emba_ctx::segpose_mode, 0, 2, false},
    {"order", &emba_ctx::order_mode, 0, 2, true},
    {"texel", &emba_ctx::texel_mode, 0, 3, false},
    {"solve_perm", &emba_ctx::solve_perm_mode, -1, 1, false},
    {"gather_waves", &emba_ctx::opt_gather_waves, 0, 4, false},
    {"chunk_order_bin", &emba_ctx::opt_chunk_order_bin, 0, 1, true},
    {"poison", &emba_ctx::opt_poison, 0, 1, false},
    {"tile_reserve", &emba_ctx::opt_tile_reserve, 0, 5, true},
    {"tile_shape", &emba_ctx::opt_tile_shape, -1, kNumTileShapes - 1, true},
    {"tile_fine", &emba_ctx::opt_tile_fine, -1, 1, true},
    {"tile_min_events", &emba_ctx::opt_tile_min_events, 0, 2000000000, true},
    {"tile_chunk", &emba_ctx::opt_tile_chunk, 0, 1 << 20, true},
    {"solve_counts", &emba_ctx::opt_solve_counts, -1, 2, false},
    {"syrk_dense", &emba_ctx::opt_syrk_dense, 0, 1, false},
    {"syrk_lists", &emba_ctx::opt_syrk_lists, 0, 2, false},
    {"gram_sparse", &emba_ctx::opt_gram_sparse, -1, 1, false},
    {"gram_sparse_chunk", &emba_ctx::opt_gram_sparse_chunk, 1, 8, false},
    {"syrk_min_cols", &emba_ctx::opt_syrk_min_cols, 64, 4096, false},
    {"syrk_item_cap", &emba_ctx::opt_syrk_item_cap, 1, 65536, false},
    {"solve_debug", &emba_ctx::opt_solve_debug, 0, 1, false},
    {"poisson", &emba_ctx::opt_poisson, 0, 2, false},
    {"gemm64", &emba_ctx::opt_gemm64, 0, 1, false},
    // who forms the steady step's segment records: the launch in front of the warp kernel, workgroup 0 of the warp launch, the host (step_rule.h: prep_inside_warp, prep_on_host)
    {"step_prep", &emba_ctx::step_prep, 0, 2, false},
    {"step_prep_polls", &emba_ctx::step_prep_polls, 0, 1 << 16, false},
    // the vote kernel of emba_seq_contrast_gradient_level (contrast_rule.h: contrast_vote_plan)
    {"contrast_vote", &emba_ctx::opt_contrast_vote, -1, 1, false},
    // the form of the dense pixel-order Gram launch (step_rule.h: gram_paired)
    {"gram_multikey", &emba_ctx::opt_gram_multikey, 0, 1, false},
};

// waves that formed their segment records themselves, over all evaluations of the context: a device counter (drains the stream)
emba_status read_step_prep_fallbacks(emba_ctx* c, int32_t* value)
{
    unsigned n = 0;
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    c->spun = false; c->knots_in_flight = false;
    HIP_TRY(c, hipMemcpy(&n, c->d_seg_flag.as<unsigned>() + 32, sizeof n, hipMemcpyDeviceToHost));
    *value = (int32_t)std::min<unsigned>(n, 0x7FFFFFFFu);
    return EMBA_OK;
}

// read-only names: what the last call of its kind did
struct ReadOnlyRef { const char* name; emba_status (*read)(emba_ctx*, int32_t*); };
const ReadOnlyRef kReadOnly[] = {
    {"prep_on_host", [](emba_ctx* c, int32_t* v) { *v = c->ev.prep_on_host ? 1 : 0; return EMBA_OK; }},          // the last evaluation: no launch in front of its warp kernel, the host formed its segment records
    {"seg_by_value", [](emba_ctx*, int32_t* v) { *v = kSegByValue; return EMBA_OK; }},                            // segment records the warp kernel's arguments carry: step_prep = 2 up to K = seg_by_value + 1
    {"prep_in_warp", [](emba_ctx* c, int32_t* v) { *v = c->ev.prep_in_warp ? 1 : 0; return EMBA_OK; }},          // the last evaluation: no launch in front of its warp kernel
    {"texels_packed", [](emba_ctx* c, int32_t* v) { *v = c->ev.texels_packed ? 1 : 0; return EMBA_OK; }},        // the last evaluation: its first launch carried texel blocks
    {"step_prep_fallbacks", read_step_prep_fallbacks},
    {"ep_valid", [](emba_ctx* c, int32_t* v) { *v = c->ev.ep_valid ? 1 : 0; return EMBA_OK; }},                  // the device holds the last evaluation's ep (a step produced it, or a compaction)
    {"contrast_vote_path", [](emba_ctx* c, int32_t* v) { *v = c->contrast_vote_path; return EMBA_OK; }},         // the vote kernel of the last contrast call — 0 HBM, 1 LDS, -1 none yet
    {"gram_paired", [](emba_ctx* c, int32_t* v) { *v = c->last_gram_paired ? 1 : 0; return EMBA_OK; }},          // the last Gram launch took the pair-aligned form
};

}  // namespace

extern "C" {

emba_status emba_set_option(emba_ctx* c, const char* name, int32_t value)
{
    if (!c || !name) return EMBA_ERR_INVALID_ARG;
    for (const OptionRef& o : kOptions)
        if (!strcmp(o.name, name)) {
            if (value < o.lo || value > o.hi) return fail(c, EMBA_ERR_INVALID_ARG, "option %s: %d outside [%d, %d]", name, (int)value, o.lo, o.hi);
            c->*(o.field) = (int)value;
            if (o.reorders) c->order.keys_ready = false;
            return EMBA_OK;
        }
    return fail(c, EMBA_ERR_INVALID_ARG, "unknown option '%s'", name);
}

emba_status emba_get_option(emba_ctx* c, const char* name, int32_t* value)
{
    if (!c || !name || !value) return EMBA_ERR_INVALID_ARG;
    for (const ReadOnlyRef& r : kReadOnly)
        if (!strcmp(r.name, name)) return r.read(c, value);
    for (const OptionRef& o : kOptions)
        if (!strcmp(o.name, name)) { *value = c->*(o.field); return EMBA_OK; }
    return fail(c, EMBA_ERR_INVALID_ARG, "unknown option '%s'", name);
}

}  // extern "C"
