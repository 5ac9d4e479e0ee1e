// emba_amd/csrc/cmax_host.h — contrast maximisation on the resident event sequence, as host code over the kernels of cmax_kernels.h: the angular velocity of
// every slice (emba_seq_cmax) and the objective of given candidates over one event range, the seam the tests pin (emba_seq_cmax_objective).  What is plain
// arithmetic — the vote grid, the pinhole fitted to the bearing LUT (emba_create keeps it: emba_ctx::cmax_pin), the slices, the search's schedule, the
// argument checks — is decided in cmax_rule.h; here are the buffers (emba_ctx::cmax), the launches and the C ABI.
// Part of emba_hip.hip's translation unit, included by it below sequence_host.h (SEQ_TRY; the sequence itself: emba_ctx::evseq) and transfer_host.h
// (d2h_pageable).
#pragma once
#include "cmax_kernels.h"
#include "cmax_rule.h"
#include "context.h"

using namespace emba;

namespace {

// the kernels' view of the resident sequence and of the image plane
emba_status cmax_params(emba_ctx* c, CmaxParams* P, CmaxGrid* grid)
{
    if (!c->cmax_pin.ok) return fail(c, EMBA_ERR_STATE, "the bearing LUT has no pinhole fit (no centre row or column with b.z > 0 and a positive slope)");
    *grid = cmax_grid(c->sw, c->sh);
    *P = CmaxParams{c->evseq.x.as<uint16_t>(), c->evseq.y.as<uint16_t>(), c->evseq.t.as<int64_t>(), c->d_lut.as<double>(), c->sw, grid->w, grid->h, grid->shift,
                    c->cmax_pin.f, c->cmax_pin.cu, c->cmax_pin.cv};
    return EMBA_OK;
}

}  // namespace

extern "C" emba_status emba_seq_cmax(emba_ctx* c, int64_t slice_events, double omega_max, double* omega_out, int64_t* t_ref_ns_out, uint64_t* j0_out, uint64_t* j_out,
                                     int32_t* evals_out, size_t cap_slices, size_t* n_slices_out)
{
    if (!c) return EMBA_ERR_INVALID_ARG;
    if (!c->evseq.have) return fail(c, EMBA_ERR_STATE, "no resident sequence (emba_seq_upload first)");
    switch (cmax_args_ok(slice_events, omega_max)) {
    case CmaxArgStatus::bad_slice: return fail(c, EMBA_ERR_INVALID_ARG, "slice_events = %lld: a slice has at least one event", (long long)slice_events);
    case CmaxArgStatus::bad_omega_max: return fail(c, EMBA_ERR_INVALID_ARG, "omega_max must be finite and positive");
    case CmaxArgStatus::slice_too_long:
        return fail(c, EMBA_ERR_INVALID_ARG, "slice_events = %lld: the 32-bit cells of the image count at most %zu events exactly", (long long)slice_events, kCmaxMaxRange);
    case CmaxArgStatus::ok: break;
    }
    const size_t ns = cmax_slice_count(c->evseq.n, slice_events);
    if (n_slices_out) *n_slices_out = ns;
    if (!ns) return EMBA_OK;
    const bool wants = omega_out || t_ref_ns_out || j0_out || j_out || evals_out;
    if (!wants) return EMBA_OK;      // (the count alone)
    if (cap_slices < ns) return fail(c, EMBA_ERR_CAPACITY, "%zu slices, the arrays hold %zu", ns, cap_slices);
    if (ns > 0x7FFFFFFFull) return fail(c, EMBA_ERR_INVALID_ARG, "%zu slices are too many for one launch", ns);
    CmaxParams P;
    CmaxGrid grid;
    SEQ_TRY(cmax_params(c, &P, &grid));
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t s = c->stream;
    SEQ_TRY(ensure<double>(c, c->cmax.omega, 3 * ns));
    SEQ_TRY(ensure<int64_t>(c, c->cmax.t_ref, ns + 1));
    SEQ_TRY(ensure<uint64_t>(c, c->cmax.j0, ns));
    SEQ_TRY(ensure<uint64_t>(c, c->cmax.j, ns));
    SEQ_TRY(ensure<int32_t>(c, c->cmax.evals, ns));
    hipLaunchKernelGGL(emba_cmax_search_kernel, dim3((unsigned)ns), dim3(kCmaxThreads), 0, s, P, (long)ns, (long)slice_events, omega_max, c->cmax.omega.as<double>(),
                       c->cmax.t_ref.as<int64_t>(), c->cmax.j0.as<unsigned long long>(), c->cmax.j.as<unsigned long long>(), c->cmax.evals.as<int32_t>());
    HIP_TRY(c, hipGetLastError());
    // behind the slices' t_ref: the timestamp of the last estimated event, where the integration ends
    HIP_TRY(c, hipMemcpyAsync(c->cmax.t_ref.as<int64_t>() + ns, c->evseq.t.as<int64_t>() + ns * (size_t)slice_events - 1, 8, hipMemcpyDeviceToDevice, s));
    HIP_TRY(c, hipStreamSynchronize(s));
    if (omega_out) SEQ_TRY(d2h_pageable(c, omega_out, c->cmax.omega.p, ns * 24));
    if (t_ref_ns_out) SEQ_TRY(d2h_pageable(c, t_ref_ns_out, c->cmax.t_ref.p, (ns + 1) * 8));
    if (j0_out) SEQ_TRY(d2h_pageable(c, j0_out, c->cmax.j0.p, ns * 8));
    if (j_out) SEQ_TRY(d2h_pageable(c, j_out, c->cmax.j.p, ns * 8));
    if (evals_out) SEQ_TRY(d2h_pageable(c, evals_out, c->cmax.evals.p, ns * 4));
    return EMBA_OK;
}

extern "C" emba_status emba_seq_cmax_objective(emba_ctx* c, size_t beg, size_t end, const double* omega, size_t M, uint64_t* j_out, uint32_t* iwe_out, int32_t* grid_w,
                                               int32_t* grid_h, int32_t* shift)
{
    if (!c) return EMBA_ERR_INVALID_ARG;
    const CmaxGrid grid = cmax_grid(c->sw, c->sh);
    if (grid_w) *grid_w = grid.w;
    if (grid_h) *grid_h = grid.h;
    if (shift) *shift = grid.shift;
    if (!M || (!j_out && !iwe_out)) return EMBA_OK;      // (the grid alone)
    if (!omega) return fail(c, EMBA_ERR_INVALID_ARG, "omega NULL");
    if (!c->evseq.have) return fail(c, EMBA_ERR_STATE, "no resident sequence (emba_seq_upload first)");
    switch (cmax_range_ok(beg, end, c->evseq.n)) {
    case CmaxRangeStatus::not_a_range: return fail(c, EMBA_ERR_INVALID_ARG, "[%zu, %zu) is not a range of the resident sequence of %zu events", beg, end, c->evseq.n);
    case CmaxRangeStatus::too_long: return fail(c, EMBA_ERR_INVALID_ARG, "[%zu, %zu): the 32-bit cells of the image count at most %zu events exactly", beg, end, kCmaxMaxRange);
    case CmaxRangeStatus::ok: break;
    }
    const size_t cells = grid.cells();
    if (M > 0x7FFFFFFFull / cells) return fail(c, EMBA_ERR_INVALID_ARG, "%zu candidates are too many for one call", M);
    for (size_t i = 0; i < 3 * M; ++i)
        if (!std::isfinite(omega[i])) return fail(c, EMBA_ERR_INVALID_ARG, "omega[%zu] is not finite", i);
    CmaxParams P;
    CmaxGrid g2;
    SEQ_TRY(cmax_params(c, &P, &g2));
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t s = c->stream;
    SEQ_TRY(ensure<double>(c, c->cmax.cand, 3 * M));
    SEQ_TRY(ensure<uint64_t>(c, c->cmax.cand_j, M));
    if (iwe_out) SEQ_TRY(ensure<uint32_t>(c, c->cmax.cand_iwe, M * cells));
    HIP_TRY(c, hipStreamSynchronize(s));
    if (beg == end) {      // no event votes: J = 0, an empty image
        HIP_TRY(c, hipMemsetAsync(c->cmax.cand_j.p, 0, M * 8, s));
        if (iwe_out) HIP_TRY(c, hipMemsetAsync(c->cmax.cand_iwe.p, 0, M * cells * 4, s));
    } else {
        HIP_TRY(c, hipMemcpyAsync(c->cmax.cand.p, omega, M * 24, hipMemcpyHostToDevice, s));
        hipLaunchKernelGGL(emba_cmax_objective_kernel, dim3((unsigned)M), dim3(kCmaxThreads), 0, s, P, (long)beg, (long)end, (const double*)c->cmax.cand.as<double>(), (long)M,
                           c->cmax.cand_j.as<unsigned long long>(), iwe_out ? c->cmax.cand_iwe.as<uint32_t>() : (uint32_t*)nullptr);
        HIP_TRY(c, hipGetLastError());
    }
    HIP_TRY(c, hipStreamSynchronize(s));
    if (j_out) SEQ_TRY(d2h_pageable(c, j_out, c->cmax.cand_j.p, M * 8));
    if (iwe_out) SEQ_TRY(d2h_pageable(c, iwe_out, c->cmax.cand_iwe.p, M * cells * 4));
    return EMBA_OK;
}
