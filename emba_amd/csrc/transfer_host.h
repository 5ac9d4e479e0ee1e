// emba_amd/csrc/transfer_host.h — device -> host copies into memory the CALLER owns (pageable: an Eigen vector, a cv::Mat, a numpy array): the
// process-wide pool of helper threads for the CPU half of a large copy, the population of the destination's pages, the context's two pinned staging
// buffers and the pipelined chunks through them.  The step, solve, sequence and image code call d2h_pageable / d2h_chunks / ensure_stage.
// Part of emba_hip.hip's translation unit, included by it first: nothing here needs another host header.
#pragma once
#include "context.h"

#include <pthread.h>
#include <sys/mman.h>

#include <condition_variable>
#include <cstring>
#include <functional>
#include <mutex>
#include <thread>

namespace {

// Device -> host into memory the CALLER owns (pageable: an Eigen vector, a cv::Mat, a numpy array).  hipMemcpy stages such a copy through the runtime's own bounce
// buffers one chunk after the other; here the DMA of chunk i + 1 into one pinned buffer runs while the CPU copies chunk i out of the other — the two halves of the
// drop-in's largest transfer (ep: 56 MB per evaluateDataError at 10 M events) overlap instead of adding up.  The stream must have been drained up to `src`'s producer.
// A few helper threads for the CPU half of a large device -> pageable copy (round 6): memcpy into FRESH pages is bound by the page faults of the one thread that touches
// them (ep into the vector evaluateDataError returns, 60 MB at config 2's shape: 8.8 ms = 6.8 GB/s).  The pool is process-wide, created at the first large copy and never
// torn down (its threads sleep on a condition variable; a caller that arrives while another copy runs copies alone).
struct CopyPool {
    static constexpr int kHelpers = 3;
    std::mutex m, use; std::condition_variable go, done;
    uint64_t gen = 0; int pending = 0; bool started = false;
    const std::function<void(int)>* job = nullptr;      // job(h), h = 0 (the caller) .. kHelpers
    static void piece(int h, size_t n, size_t& lo, size_t& hi)
    {
        const size_t per = ((n / (kHelpers + 1)) + 4095) & ~(size_t)4095;      // whole pages to every thread
        lo = std::min(n, per * (size_t)h); hi = (h == kHelpers) ? n : std::min(n, per * (size_t)(h + 1));
    }
    void worker(int h)
    {
        uint64_t seen = 0;
        for (;;) {
            const std::function<void(int)>* f;
            { std::unique_lock<std::mutex> l(m); go.wait(l, [&] { return gen != seen; }); seen = gen; f = job; }
            (*f)(h + 1);
            { std::lock_guard<std::mutex> l(m); if (--pending == 0) done.notify_one(); }
        }
    }
    // f(0) on the caller, f(1 .. kHelpers) on the helpers; alone (f(0 .. kHelpers) in turn) when another caller holds the pool
    void run(const std::function<void(int)>& f)
    {
        std::unique_lock<std::mutex> u(use, std::try_to_lock);
        if (!u.owns_lock()) { for (int h = 0; h <= kHelpers; ++h) f(h); return; }
        if (!started) { for (int h = 0; h < kHelpers; ++h) std::thread([this, h] { worker(h); }).detach(); started = true; }
        { std::lock_guard<std::mutex> l(m); job = &f; pending = kHelpers; ++gen; }
        go.notify_all();
        f(0);
        { std::unique_lock<std::mutex> l(m); done.wait(l, [&] { return pending == 0; }); }
    }
    void copy(void* d, const void* sp, size_t nn)
    {
        if (nn < ((size_t)1 << 20)) { std::memcpy(d, sp, nn); return; }
        run([&](int h) { size_t lo, hi; piece(h, nn, lo, hi); if (hi > lo) std::memcpy((char*)d + lo, (const char*)sp + lo, hi - lo); });
    }
};
CopyPool* copy_pool()      // (never destroyed: its detached threads may outlive every context)
{
    static CopyPool* p = [] {
        CopyPool* q = new CopyPool;
        // a fork()ed child has none of the helper threads and possibly a mutex that a thread of the parent held: it starts from a fresh pool
        static CopyPool* self = q;
        (void)pthread_atfork(nullptr, nullptr, [] { new (self) CopyPool; });
        return q;
    }();
    return p;
}

// Have the pages of [p, p + bytes) mapped before they are written: memory a caller has just allocated (the vector evaluateDataError returns) has no pages yet, and
// a first write per page is a trap each (60 MB: 15 k of them on the copying thread).  One MADV_POPULATE_WRITE per piece does the same inside the kernel, without
// changing what the pages hold; where the kernel does not know it (< 5.14) the pages are simply faulted in by the copy that follows.
void populate_pages(void* p, size_t bytes)
{
#ifndef MADV_POPULATE_WRITE
#define MADV_POPULATE_WRITE 23
#endif
    const uintptr_t lo = ((uintptr_t)p + 4095) & ~(uintptr_t)4095, hi = ((uintptr_t)p + bytes) & ~(uintptr_t)4095;
    if (hi > lo) (void)madvise((void*)lo, hi - lo, MADV_POPULATE_WRITE);
}
void populate_pages_parallel(void* p, size_t bytes)
{
    if (bytes < ((size_t)4 << 20)) return;
    copy_pool()->run([&](int h) { size_t lo, hi; CopyPool::piece(h, bytes, lo, hi); if (hi > lo) populate_pages((char*)p + lo, hi - lo); });
}

// the context's two pinned staging buffers (8 MB each) and the events that say when a transfer through one of them has completed
constexpr size_t kStageBytes = (size_t)8 << 20;
emba_status ensure_stage(emba_ctx* c)
{
    for (int k = 0; k < 2; ++k)
        if (!c->h_stage[k]) { HIP_TRY(c, hipHostMalloc(&c->h_stage[k], kStageBytes, hipHostMallocDefault)); HIP_TRY(c, hipEventCreateWithFlags(&c->stage_ev[k], hipEventDisableTiming)); }
    return EMBA_OK;
}

// device -> host in pipelined chunks through the context's two pinned buffers: the DMA of chunk i + 1 runs while `consume(chunk, byte offset, bytes)` works on chunk i.
// The stream must have been drained up to `src`'s producer.
emba_status d2h_chunks(emba_ctx* c, const void* src, size_t bytes, const std::function<void(const void*, size_t, size_t)>& consume,
                       const std::function<void()>& while_first_chunk_travels = nullptr)
{
    if (!bytes) return EMBA_OK;
    constexpr size_t kChunk = kStageBytes;
    if (emba_status st = ensure_stage(c)) return st;
    hipStream_t s = c->stream;
    const size_t n = (bytes + kChunk - 1) / kChunk;
    auto len = [&](size_t i) { return std::min(kChunk, bytes - i * kChunk); };
    HIP_TRY(c, hipMemcpyAsync(c->h_stage[0], src, len(0), hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipEventRecord(c->stage_ev[0], s));
    if (while_first_chunk_travels) while_first_chunk_travels();
    for (size_t i = 0; i < n; ++i) {
        if (i + 1 < n) {
            HIP_TRY(c, hipMemcpyAsync(c->h_stage[(i + 1) & 1], (const char*)src + (i + 1) * kChunk, len(i + 1), hipMemcpyDeviceToHost, s));
            HIP_TRY(c, hipEventRecord(c->stage_ev[(i + 1) & 1], s));
        }
        HIP_TRY(c, hipEventSynchronize(c->stage_ev[i & 1]));
        consume(c->h_stage[i & 1], i * kChunk, len(i));
    }
    return EMBA_OK;
}

emba_status d2h_pageable(emba_ctx* c, void* dst, const void* src, size_t bytes)
{
    if (!bytes) return EMBA_OK;
    if (bytes <= ((size_t)1 << 20)) { HIP_TRY(c, hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost)); return EMBA_OK; }
    // (the first chunk's DMA is queued before the destination's pages are populated: the two run side by side)
    bool populated = false;
    return d2h_chunks(c, src, bytes, [&](const void* chunk, size_t off, size_t len) { copy_pool()->copy((char*)dst + off, chunk, len); },
                      [&]() { if (!populated) { populate_pages_parallel(dst, bytes); populated = true; } });
}

}  // namespace
