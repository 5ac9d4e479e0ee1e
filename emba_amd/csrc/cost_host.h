// emba_amd/csrc/cost_host.h — the cost terms of a trial point (solver.cpp:88-91, 265-268) as host code over emba_costs_kernel (cost_kernels.h): one enqueue, one
// wait, and the five entry points over them.  The launch sums the data term, the regulariser or both; its last block writes the two sums, the step's status word
// and a sequence number to pinned host memory, and the host spins on the number — no memset, no copies, no stream synchronise (round 5: 159 -> 130 us per LM
// iteration at the BASELINE shape, most of it the evaluation it waits for).  What is plain arithmetic — the summands, the factors, the grid — is cost_rule.h.
// Part of emba_hip.hip's translation unit, included below step_host.h (resolve_pending) and map_host.h.
#pragma once
#include "context.h"
#include "cost_kernels.h"
#include "cost_rule.h"

using namespace emba;

namespace {

// the launch behind whatever the stream holds; the sums come back with costs_wait
emba_status costs_enqueue(emba_ctx* c, int irls, double eta, bool want_data, bool want_reg)
{
    if (!c->h_cost) {
        HIP_TRY(c, hipHostMalloc((void**)&c->h_cost, 4 * sizeof(double), hipHostMallocDefault));
        memset(c->h_cost, 0, 4 * sizeof(double));
        HIP_TRY(c, hipHostGetDevicePointer((void**)&c->h_cost_dev, c->h_cost, 0));
        if (emba_status st = ensure<double>(c, c->d_cost_acc, 4)) return st;
        HIP_TRY(c, hipMemsetAsync(c->d_cost_acc.as<double>(), 0, 4 * sizeof(double), c->stream));      // (on the kernels' stream: a hipMemset on the default stream is not ordered in front of them)
    }
    CostsParams p{};
    p.e_sorted = c->d_e_sorted.as<double>(); p.flag = c->d_flag.as<uint8_t>(); p.n_pm = (want_data && c->win.n_sorted) ? (long)c->win.n_pm : 0L; p.irls = irls; p.eta = eta;
    p.Gx = c->map.Gx(); p.Gy = c->map.Gy(); p.npix = want_reg ? (long)c->npix : 0L;
    const CostGrid g = cost_grid((size_t)p.n_pm, (size_t)p.npix, c->n_cu, want_data, want_reg);
    p.nb_data = g.nb_data; p.nb_reg = g.nb_reg;
    p.acc = c->d_cost_acc.as<double>(); p.ticket = reinterpret_cast<unsigned int*>(c->d_cost_acc.as<double>() + 2); p.err_dev = c->d_err;
    p.host_out = c->h_cost_dev; p.seq = ++c->cost_seq;
    hipLaunchKernelGGL(emba_costs_kernel, dim3((unsigned)(p.nb_data + p.nb_reg)), dim3(kCostBlock), 0, c->stream, p);
    HIP_TRY(c, hipGetLastError());
    return EMBA_OK;
}

// the kernel's last block publishes the sequence number behind the sums: spin on it (a stream synchronise costs tens of microseconds); bounded — a faulted
// kernel never publishes — with the stream as the fallback.  Then c->h_cost holds {data sum, reg sum, status word}.
emba_status costs_wait(emba_ctx* c)
{
    volatile int* w = reinterpret_cast<volatile int*>(c->h_cost + 3);
    bool polled = false;
    for (long spin = 0; spin < 50000000L; ++spin) { if (w[0] == c->cost_seq) { polled = true; break; } __builtin_ia32_pause(); }
    if (polled) { std::atomic_thread_fence(std::memory_order_acquire); c->spun = true; }
    else { HIP_TRY(c, hipStreamSynchronize(c->stream)); c->spun = false; }
    return EMBA_OK;
}

}  // namespace

extern "C" {

emba_status emba_data_cost(emba_ctx* c, int32_t irls, double eta, double* cost)
{
    if (!c || !cost) return EMBA_ERR_INVALID_ARG;
    if (!c->ev.readable()) return fail(c, EMBA_ERR_STATE, "no residuals yet");
    HIP_TRY(c, hipSetDevice(c->device));
    { emba_status st0 = resolve_pending(c); if (st0) return st0; }
    emba_status st;
    if ((st = costs_enqueue(c, (int)irls, eta, true, false)) || (st = costs_wait(c))) return st;
    *cost = cost_scale((int)irls, eta) * c->h_cost[0];
    return EMBA_OK;
}

// (needs the map and nothing of an evaluation: the status word the kernel carries along is not looked at)
emba_status emba_reg_cost(emba_ctx* c, double alpha, double* cost)
{
    if (!c || !cost) return EMBA_ERR_INVALID_ARG;
    if (!c->map.state().resident()) return fail(c, EMBA_ERR_STATE, "no map");
    HIP_TRY(c, hipSetDevice(c->device));
    emba_status st;
    if ((st = costs_enqueue(c, 0, 0.0, false, true)) || (st = costs_wait(c))) return st;
    *cost = reg_scale(alpha) * c->h_cost[1];
    return EMBA_OK;
}

// emba_costs_launch / _finish split emba_costs so that a group can enqueue every rank before it waits for any.
emba_status emba_costs_launch(emba_ctx* c, int32_t irls, double eta, int32_t with_reg)
{
    if (!c) return EMBA_ERR_INVALID_ARG;
    if (!c->ev.readable()) return fail(c, EMBA_ERR_STATE, "no residuals yet");
    if (with_reg && !c->map.state().resident()) return fail(c, EMBA_ERR_STATE, "no map");
    HIP_TRY(c, hipSetDevice(c->device));
    // An evaluation that has only been launched stays that way: the reductions read the per-event residuals and flags the warp kernel wrote,
    // not the compacted vector — so the formNormalEq that follows an accepted trial still finds the post-warp work fused (emba_form_active), and
    // a rejected trial never pays for a residual vector nobody asks for.  The step's status word comes back with the sums (emba_costs_finish).
    if (!c->ev.ep_deferred) { emba_status st0 = resolve_pending(c); if (st0) return st0; }
    return costs_enqueue(c, (int)irls, eta, true, with_reg != 0);
}

emba_status emba_costs_finish(emba_ctx* c, int32_t irls, double eta, double alpha, double* data_cost, double* reg_cost)
{
    if (!c || !c->h_cost) return EMBA_ERR_INVALID_ARG;
    HIP_TRY(c, hipSetDevice(c->device));
    if (emba_status st = costs_wait(c)) return st;
    { int w = 0; memcpy(&w, c->h_cost + 2, sizeof(int)); if (w & 1) return fail(c, EMBA_ERR_TIME_RANGE, "a batch midpoint lies outside the spline's knots"); }
    if (data_cost) *data_cost = cost_scale((int)irls, eta) * c->h_cost[0];
    if (reg_cost) *reg_cost = reg_scale(alpha) * c->h_cost[1];
    return EMBA_OK;
}

emba_status emba_costs(emba_ctx* c, int32_t irls, double eta, double alpha, double* data_cost, double* reg_cost)
{
    emba_status st = emba_costs_launch(c, irls, eta, reg_cost ? 1 : 0);
    if (st) return st;
    return emba_costs_finish(c, irls, eta, alpha, data_cost, reg_cost);
}

}  // extern "C"
