"""What the GPU suite runs under each emba_set_option value (not a test module).

include/emba_hip.h promises that every option changes speed or the internal form only.  That promise is kept by tests: COVERED names, per
option, the values the GPU tests set and the tests that set them; EXEMPT gives the reason an option needs no parity test of its own.
REQUIRED lists, per covered option, the non-default values that a kernel or a host branch switches on: tests/test_option_matrix_cpu.py
checks that the table in the source, COVERED, EXEMPT and REQUIRED agree, so a new option cannot land without a test or a stated exemption.
"""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPTIONS_SRC = os.path.join(ROOT, "emba_amd", "csrc", "options_host.h")
KERNELS_H = os.path.join(ROOT, "emba_amd", "csrc", "kernels.h")

_V = "test_gpu_variants.py::"
_P = "test_gpu_parity.py::"
_S = "test_gpu_step_prep.py::"
_C = "test_gpu_contrast_pyramid.py::"
_G = "test_gpu_gram_paired.py::"

# option -> (values the GPU tests set, tests that set them)
COVERED = {
    "order": ((0, 1, 2), (_V + "test_auto_order_rule_at_small_sizes", _V + "test_pixel_order_segpose", _V + "test_every_tile_instantiation")),
    "tile_shape": ((0, 1, 2, 3), (_V + "test_every_tile_instantiation", _V + "test_tile_reserve_extremes", _V + "test_tile_order_after_drift_per_shape")),
    "tile_fine": ((0, 1), (_V + "test_every_tile_instantiation", _V + "test_tile_order_event_state")),
    "tile_reserve": ((0, 2, 5), (_V + "test_tile_reserve_extremes", _V + "test_every_tile_instantiation")),
    "tile_chunk": ((100, 504), (_V + "test_tile_chunking",)),
    "chunk_order_bin": ((0, 1), (_V + "test_tile_chunking",)),
    "tile_min_events": ((0,), (_V + "test_auto_order_rule_at_small_sizes",)),
    "segpose": ((1, 2), (_V + "test_pixel_order_segpose",)),
    "gram_tags": ((0,), (_V + "test_pixel_order_gram_forms",)),
    "gather_waves": ((1, 2, 4), (_V + "test_pixel_order_gram_forms",)),
    "gram_sparse": ((0, 1), (_V + "test_pixel_order_gram_forms", _P + "test_gram_sums_from_a_sparse_slot_stream")),
    "gram_sparse_chunk": ((1, 8), (_V + "test_pixel_order_gram_forms",)),
    "step_gather": ((0, 1, 2, 3), (_P + "test_resident_step_sequences", _V + "test_pixel_order_gram_forms")),
    "step_one_set": ((0,), (_V + "test_step_alternating_record_sets",)),
    "step_fast": ((0, 1), (_P + "test_resident_step_sequences",)),
    "step_ep": ((0, 1, 2), (_P + "test_resident_step_returns_ep_in_reference_order",)),
    "solve_counts": ((0, 2), (_V + "test_pixel_order_segpose", _V + "test_every_tile_instantiation", _V + "test_tile_order_after_drift_per_shape")),
    "poisson": ((1, 2), (_V + "test_poisson_forms", _P + "test_poisson_reconstruction_matches_oracle")),
    "gemm64": ((1,), (_V + "test_poisson_forms",)),
    "texel": ((1, 2, 3), (_P + "test_hessian_sources_agree",)),
    "solve_perm": ((0, 1), (_P + "test_schur_solve_with_the_columns_of_U_in_panorama_column_order", _P + "test_schur_solve_under_every_form_of_the_syrk")),
    "syrk_dense": ((1,), (_P + "test_schur_solve_under_every_form_of_the_syrk",)),
    "syrk_lists": ((1, 2), (_P + "test_schur_solve_under_every_form_of_the_syrk",)),
    "syrk_min_cols": ((64,), (_P + "test_schur_solve_under_every_form_of_the_syrk",)),
    "syrk_item_cap": ((8,), (_P + "test_schur_solve_under_every_form_of_the_syrk",)),
    "step_prep": ((0, 1), (_S + "test_consecutive_steps_never_read_stale_records", _S + "test_both_forms_against_the_oracle")),
    "step_prep_polls": ((0,), (_S + "test_waves_that_give_up_waiting_form_the_same_records",)),
    "contrast_vote": ((-1, 0, 1), (_C + "test_forced_vote_kernel", _C + "test_wrap_and_pole_at_a_coarse_level")),
    "gram_multikey": ((0, 1), (_G + "test_gram_forms_on_windows_that_stress_the_plan", _G + "test_window_without_candidates")),
}

# covered option -> the non-default values that select another kernel instantiation or host branch (read from the code that switches on them)
REQUIRED = {
    "order": (0, 1, 2),                    # the pricing rule (at a size it runs: tile_min_events 0), both forced orders
    "tile_shape": (0, 1, 2, 3),            # emba_warp_tiled_kernel<tw, th>: one instantiation per shape
    "tile_fine": (0, 1),                   # coarse and fine grid of tile origins
    "tile_reserve": (0, 5),                # no reserve; the largest, which leaves a 2-px pitch on the 96 x 12 tile
    "tile_chunk": (100, 504),              # below one round of the workgroup's waves (empty pieces skipped); exactly one round (tile_round())
    "chunk_order_bin": (1,),               # chunks in bin order instead of longest first
    "tile_min_events": (0,),               # the auto rule at test sizes
    "segpose": (1, 2),                     # per-batch pose table; per-event pose from the segment records
    "gram_tags": (0,),                     # Gram kernel without the tag stream
    "gather_waves": (1, 2, 4),
    "gram_sparse": (0, 1),
    "gram_sparse_chunk": (1, 8),
    "step_gather": (0, 1, 3),
    "step_one_set": (0,),
    "step_fast": (0,),
    "step_ep": (0, 2),
    "solve_counts": (0, 2),                # CSR counts from the records; from both, compared
    "poisson": (1, 2),
    "gemm64": (1,),
    "texel": (1, 2, 3),
    "solve_perm": (0, 1),
    "syrk_dense": (1,),
    "syrk_lists": (1, 2),
    "syrk_min_cols": (64,),
    "syrk_item_cap": (8,),
    "step_prep": (1,),                     # the segment records formed inside the warp launch (step_rule.h: prep_inside_warp); the library's default is 0
    "step_prep_polls": (0,),               # nobody waits: the bounded wait's exit
    "contrast_vote": (0, 1),               # the HBM vote forced where the image fits LDS; the LDS vote asked for where it does not (contrast_rule.h: contrast_vote_plan)
    "gram_multikey": (1,),                 # the multi-key form of the dense pixel-order Gram launch instead of the pair-aligned one (step_rule.h: gram_paired)
}

EXEMPT = {
    "poison": "test aid, not a variant: fills new device allocations with 0xFF so a read of unwritten workspace shows (used in test_gpu_sharded.py)",
    "solve_debug": "prints band statistics of a solve and computes nothing else",
}


def _block(text, head):
    i = text.index(head)
    return text[i:text.index("};", i)]


def _eval_int(expr, consts):
    e = expr.strip()
    for k, v in consts.items():
        e = re.sub(r"\b%s\b" % k, str(v), e)
    if not re.fullmatch(r"[0-9\s+\-*()<>]+", e):
        raise ValueError(f"cannot evaluate the bound {expr!r}")
    return int(eval(e, {"__builtins__": {}}))      # (digits and + - * << >> only)


def parse_constants(path=KERNELS_H):
    """constexpr int NAME = <integer or macro>; of kernels.h, a macro taken at the default its #define gives (kTileWaves = TILE_WAVES)."""
    with open(path) as f:
        text = f.read()
    defines = {m.group(1): int(m.group(2)) for m in re.finditer(r"^\s*#define\s+(\w+)\s+(\d+)\s*$", text, re.M)}
    out = {}
    for m in re.finditer(r"constexpr\s+int\s+(\w+)\s*=\s*(\w+)\s*;", text):
        v = m.group(2)
        if v.isdigit():
            out[m.group(1)] = int(v)
        elif v in defines:
            out[m.group(1)] = defines[v]
    return out


def tile_round(consts=None):
    """Entries one round of the tiled kernel's waves takes (kWarpNew groups per wave x kTileWaves waves): its pieces of a tile are whole rounds."""
    consts = parse_constants() if consts is None else consts
    return consts["kWarpNew"] * consts["kTileWaves"]


def parse_options(path=OPTIONS_SRC, consts=None):
    """The kOptions table of options_host.h: [{"name", "field", "lo", "hi", "reorders"}] in source order."""
    consts = parse_constants() if consts is None else consts
    with open(path) as f:
        block = _block(f.read(), "kOptions[] = {")
    out = []
    for m in re.finditer(r'\{\s*"(\w+)"\s*,\s*&emba_ctx::(\w+)\s*,\s*([^,{}]+?)\s*,\s*([^,{}]+?)\s*,\s*(true|false)\s*\}', block):
        out.append(dict(name=m.group(1), field=m.group(2), lo=_eval_int(m.group(3), consts), hi=_eval_int(m.group(4), consts), reorders=m.group(5) == "true"))
    return out


def parse_tile_shapes(path=KERNELS_H):
    """kTileShapes of kernels.h: [{"tw", "th", "pw", "ph", "fine_pw", "fine_ph"}]."""
    with open(path) as f:
        block = _block(f.read(), "kTileShapes[kNumTileShapes] = {")
    keys = ("tw", "th", "pw", "ph", "fine_pw", "fine_ph")
    return [dict(zip(keys, map(int, m.groups()))) for m in re.finditer(r"\{\s*" + r"\s*,\s*".join([r"(\d+)"] * 6) + r"\s*\}", block)]


def tile_geometry(shape, fine, reserve, shapes=None):
    """What emba_last_tile_geometry (LEGM.setup_info()["tile"]) reports for a tile-order window of this shape, grid and reserve."""
    s = (shapes or parse_tile_shapes())[shape]
    return dict(w=s["tw"], h=s["th"], pitch_x=min(s["fine_pw"] if fine else s["pw"], s["tw"] - 2 * reserve),
                pitch_y=min(s["fine_ph"] if fine else s["ph"], s["th"] - 2 * reserve), reserve=reserve)
