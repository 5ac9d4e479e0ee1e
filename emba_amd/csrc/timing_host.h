// emba_amd/csrc/timing_host.h — the measurement aids of the C ABI: the context's event timers, the kernel timing of a step (slots of events recorded by
// step_host.h), what an event bracket around nothing reads (emba_bracket_overhead_us), the shader clock under load (emba_clock_probe) and the device's PCI
// bus id.  None of it touches the product's data.
// Part of emba_hip.hip's translation unit.
#pragma once
#include "context.h"

using namespace emba;

extern "C" {

emba_status emba_timer_start(emba_ctx* c, int32_t slot)
{
    if (!c || slot < 0 || slot >= 8) return EMBA_ERR_INVALID_ARG;
    HIP_TRY(c, hipEventRecord(c->ev_start[slot], c->stream));
    return EMBA_OK;
}

emba_status emba_timer_stop(emba_ctx* c, int32_t slot)
{
    if (!c || slot < 0 || slot >= 8) return EMBA_ERR_INVALID_ARG;
    HIP_TRY(c, hipEventRecord(c->ev_stop[slot], c->stream));
    return EMBA_OK;
}

emba_status emba_timer_elapsed_ms(emba_ctx* c, int32_t slot, float* ms)
{
    if (!c || !ms || slot < 0 || slot >= 8) return EMBA_ERR_INVALID_ARG;
    HIP_TRY(c, hipEventSynchronize(c->ev_stop[slot]));
    HIP_TRY(c, hipEventElapsedTime(ms, c->ev_start[slot], c->ev_stop[slot]));
    return EMBA_OK;
}

emba_status emba_enable_kernel_timing(emba_ctx* c, int32_t on)
{
    if (!c || on < 0 || on > 16) return EMBA_ERR_INVALID_ARG;
    c->kernel_timing = on != 0;
    if (on) {       // on = 1 + slot: the next evaluation / form record their events in that slot, to be read later (emba_kernel_ms_slot)
        const int slot = on - 1;
        for (int i = 0; i < 5; ++i) if (!c->kt_sets[slot][i]) HIP_TRY(c, hipEventCreate(&c->kt_sets[slot][i]));
        c->kt = c->kt_sets[slot]; c->kt_slot = slot;
        c->kt_valid[slot][0] = c->kt_valid[slot][1] = c->kt_valid[slot][2] = false;
    }
    c->kt_warp_valid = c->kt_accum_valid = false;
    return EMBA_OK;
}

emba_status emba_kernel_ms_slot(emba_ctx* c, int32_t slot, float* warp_ms, float* accum_ms)
{
    if (!c || slot < 0 || slot >= 16) return EMBA_ERR_INVALID_ARG;
    hipEvent_t* k = c->kt_sets[slot];
    if (warp_ms) {
        *warp_ms = -1.f;
        if (c->kt_valid[slot][0]) { HIP_TRY(c, hipEventSynchronize(k[1])); HIP_TRY(c, hipEventElapsedTime(warp_ms, k[0], k[1])); }
    }
    if (accum_ms) {
        *accum_ms = -1.f;
        if (c->kt_valid[slot][1]) { HIP_TRY(c, hipEventSynchronize(k[3])); HIP_TRY(c, hipEventElapsedTime(accum_ms, k[2], k[3])); }
    }
    return EMBA_OK;
}

emba_status emba_last_kernel_ms(emba_ctx* c, float* warp_ms, float* accum_ms)
{
    if (!c) return EMBA_ERR_INVALID_ARG;
    return emba_kernel_ms_slot(c, c->kt_slot, warp_ms, accum_ms);
}

emba_status emba_kernel_timing_all(emba_ctx* c, int32_t on)
{
    if (!c) return EMBA_ERR_INVALID_ARG;
    c->kt_all = on != 0;
    return EMBA_OK;
}

emba_status emba_kernel_ms_all(emba_ctx* c, int32_t slot, float* ms4)
{
    if (!c || !ms4 || slot < 0 || slot >= 16) return EMBA_ERR_INVALID_ARG;
    hipEvent_t* k = c->kt_sets[slot];
    for (int i = 0; i < 4; ++i) ms4[i] = -1.f;
    if (!(c->kt_valid[slot][0] && c->kt_valid[slot][1] && c->kt_valid[slot][2])) return EMBA_OK;
    HIP_TRY(c, hipEventSynchronize(k[3]));
    HIP_TRY(c, hipEventElapsedTime(ms4 + 0, k[4], k[0]));     // prep || pose || texel (+ the full texel pack where it is used)
    HIP_TRY(c, hipEventElapsedTime(ms4 + 1, k[0], k[1]));     // warp kernel
    HIP_TRY(c, hipEventElapsedTime(ms4 + 2, k[1], k[2]));     // launch A (+ the sweeping active write where it is a launch of its own)
    HIP_TRY(c, hipEventElapsedTime(ms4 + 3, k[2], k[3]));     // Gram kernel (with the gather inside)
    return EMBA_OK;
}

emba_status emba_bracket_overhead_us(emba_ctx* c, int32_t reps, float* us)
{
    if (!c || !us || reps < 1 || reps > 1000) return EMBA_ERR_INVALID_ARG;
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t s = c->stream;
    double sum = 0.0;
    for (int r = 0; r < reps; ++r) {
        // the bracket sits BEHIND queued work, like the brackets of a step: a busy kernel first, then event | empty kernel | event
        hipLaunchKernelGGL(emba_clock_probe_kernel, dim3(1), dim3(64), 0, s, c->d_probe.as<unsigned long long>() + 4, 256);
        HIP_TRY(c, hipEventRecord(c->cal_ev[0], s));
        hipLaunchKernelGGL(emba_empty_kernel, dim3(1), dim3(64), 0, s);
        HIP_TRY(c, hipEventRecord(c->cal_ev[1], s));
        HIP_TRY(c, hipEventSynchronize(c->cal_ev[1]));
        float ms = 0.f;
        HIP_TRY(c, hipEventElapsedTime(&ms, c->cal_ev[0], c->cal_ev[1]));
        sum += ms;
    }
    HIP_TRY(c, hipGetLastError());
    *us = (float)(sum / reps * 1e3);
    return EMBA_OK;
}

emba_status emba_clock_probe(emba_ctx* c, double* sclk_mhz_est, double* probe_us, double* memtime_per_realtime, int32_t* clock_rate_khz,
                             int32_t* mem_clock_rate_khz, int32_t* wall_clock_rate_khz)
{
    if (!c) return EMBA_ERR_INVALID_ARG;
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t s = c->stream;
    int v = 0;
    if (clock_rate_khz) { *clock_rate_khz = 0; if (hipDeviceGetAttribute(&v, hipDeviceAttributeClockRate, c->device) == hipSuccess) *clock_rate_khz = v; }
    if (mem_clock_rate_khz) { *mem_clock_rate_khz = 0; if (hipDeviceGetAttribute(&v, hipDeviceAttributeMemoryClockRate, c->device) == hipSuccess) *mem_clock_rate_khz = v; }
    int wall_khz = 100000;
    if (hipDeviceGetAttribute(&v, hipDeviceAttributeWallClockRate, c->device) == hipSuccess && v > 0) wall_khz = v;
    if (wall_clock_rate_khz) *wall_clock_rate_khz = wall_khz;
    // every SIMD of the chip busy with one wave's dependent chain of kClockProbeOps fp32 adds (4 cycles each on a 16-lane SIMD, issued back to back)
    const int loops = 1024;
    HIP_TRY(c, hipEventRecord(c->cal_ev[0], s));
    hipLaunchKernelGGL(emba_clock_probe_kernel, dim3((unsigned)c->n_cu), dim3(256), 0, s, c->d_probe.as<unsigned long long>(), loops);
    HIP_TRY(c, hipEventRecord(c->cal_ev[1], s));
    HIP_TRY(c, hipGetLastError());
    unsigned long long h[4] = {0, 0, 0, 0};
    HIP_TRY(c, hipMemcpyAsync(h, c->d_probe.as<unsigned long long>(), sizeof h, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipStreamSynchronize(s));
    c->spun = false;
    float ms = 0.f;
    HIP_TRY(c, hipEventElapsedTime(&ms, c->cal_ev[0], c->cal_ev[1]));
    const double wall_s = (double)h[1] / ((double)wall_khz * 1e3);      // the wave's own constant-rate clock around its chain
    if (probe_us) *probe_us = wall_s * 1e6;
    // s_memtime counts shader cycles (measured, round 5: 8.08 ticks per dependent v_add_f32 of the chain, the pipeline's 8-cycle dependent-issue
    // cadence; its ratio to the 100-MHz counter moves with the power state), so ticks(s_memtime) / seconds(s_memrealtime) IS the shader clock
    if (sclk_mhz_est) *sclk_mhz_est = wall_s > 0 ? (double)h[0] / wall_s * 1e-6 : 0.0;
    if (memtime_per_realtime) *memtime_per_realtime = h[1] ? (double)h[0] / ((double)kClockProbeUnroll * loops) : 0.0;
    (void)ms;
    return EMBA_OK;
}

emba_status emba_device_pci_bus_id(emba_ctx* c, char* buf, size_t len)
{
    if (!c || !buf || len < 16) return EMBA_ERR_INVALID_ARG;
    HIP_TRY(c, hipDeviceGetPCIBusId(buf, (int)len, c->device));
    return EMBA_OK;
}

}  // extern "C"
