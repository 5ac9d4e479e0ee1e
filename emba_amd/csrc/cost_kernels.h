// emba_amd/csrc/cost_kernels.h — a12: the cost reductions (gfx950, wave64).  One kernel sums the data term, the regulariser or both (cost_rule.h: the
// summands and the grid; cost_host.h: the entry points).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cost_rule.h"
#include "kernels.h"      // wave_sum (also solve_kernels.h's)

namespace emba {

// the sum of x over the four waves of a block, the same value in every thread; s_w: four doubles of LDS
__device__ __forceinline__ double cost_block_sum(double x, double* s_w)
{
    x = wave_sum(x);
    if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = x;
    __syncthreads();
    return (s_w[0] + s_w[1]) + (s_w[2] + s_w[3]);
}

// Both cost terms of a trial point in ONE launch, results straight to pinned host memory (round 5): blocks [0, nb_data) reduce the data term, the blocks behind them
// the regulariser (either number may be 0, not both); every block adds its sum to acc[0 / 1] and takes a ticket; the block with the last ticket reads the two totals,
// writes {data, reg, error word} and then the sequence number to the host (system-scope release: the host spins on it, as it does for a step's counts) and puts
// acc / ticket back to zero for the next call.
struct CostsParams {
    const double* e_sorted; const uint8_t* flag; long n_pm; int irls; double eta;
    const double* Gx; const double* Gy; long npix; int nb_data, nb_reg;
    double* acc; unsigned int* ticket; const int* err_dev;
    double* host_out; int seq;       // host_out (pinned): [0] data sum, [1] reg sum, [2] error word (int), [3] sequence number (int)
};
static_assert(kCostBlock == 256, "emba_costs_kernel: four waves per block");
__global__ __launch_bounds__(256) void emba_costs_kernel(CostsParams p)
{
    __shared__ double s_w[4];
    __shared__ int s_last;
    const bool reg = (int)blockIdx.x >= p.nb_data;
    double acc = 0;
    if (!reg) {
        for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < p.n_pm; i += (long)p.nb_data * 256) {
            if (!p.flag[i]) continue;
            acc += cost_term(p.e_sorted[i], p.irls, p.eta);
        }
    } else {
        for (long i = (long)((int)blockIdx.x - p.nb_data) * 256 + threadIdx.x; i < p.npix; i += (long)p.nb_reg * 256)
            acc += reg_term(p.Gx[i], p.Gy[i]);
    }
    acc = cost_block_sum(acc, s_w);
    if (threadIdx.x == 0) {
        atomicAdd(p.acc + (reg ? 1 : 0), acc);
        __threadfence();
        s_last = (atomicAdd(p.ticket, 1u) == gridDim.x - 1u) ? 1 : 0;
        if (s_last) {
            __threadfence();
            const double d = atomicAdd(p.acc, 0.0), r = atomicAdd(p.acc + 1, 0.0);      // (read at the point of coherence: every other block's add precedes its ticket)
            p.acc[0] = 0.0; p.acc[1] = 0.0; *p.ticket = 0u;                              // (the next call is ordered behind this kernel on the stream)
            p.host_out[0] = d; p.host_out[1] = r;
            reinterpret_cast<int*>(p.host_out + 2)[0] = p.err_dev[0];
            __threadfence_system();
            __hip_atomic_store(reinterpret_cast<int*>(p.host_out + 3), p.seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
        }
    }
}

}  // namespace emba
