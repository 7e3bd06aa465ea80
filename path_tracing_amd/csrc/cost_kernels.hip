// Tree cost (include/hpt.h, "tree cost"): the ten integer sums and the root's extent over the quantised binary tree the
// first trace launch walks, to the bytes of tree_cost_sums_host (scene_build.cpp), which is the definition.  Everything is
// exact 64-bit integer arithmetic, so the result depends on neither the grid's shape nor the order of the adds.
#include "refit_kernels.h"

#include <algorithm>

namespace hpt {
namespace {

constexpr uint32_t kLeaf = 0x80000000u, kEmpty = 0xFFFFFFFFu;
constexpr int kCostWaves = kRefitBlock / 64;

// sum over the wave in lane 0: the two 32-bit halves travel separately
__device__ __forceinline__ uint64_t wave_sum(uint64_t v){
#pragma unroll
    for(int off = 32; off > 0; off >>= 1){
        const uint32_t lo = __shfl_down((uint32_t) v, off, 64), hi = __shfl_down((uint32_t) (v >> 32), off, 64);
        v += ((uint64_t) hi << 32) | lo;
    }
    return v;
}

// One lane per node and trip, both children per lane; the node's two halves are fetched as the trace kernel fetches them
// (two dwordx4).  acc: inner, leaf, empty children, leaf slots, inner xy yz zx, leaf xy yz zx -- the order of hpt_tree_cost
// and of result[0 .. 9].  The lane that meets node 0 stores the root's extent in the three 32-bit words behind them.
__global__ __launch_bounds__(kRefitBlock) void k_tree_cost(const uint4 *__restrict__ qnodes, uint32_t num_nodes,
                                                            unsigned long long *__restrict__ result){
    __shared__ uint64_t red[kCostWaves][kCostCounters];
    uint64_t acc[kCostCounters];
#pragma unroll
    for(int k = 0; k < kCostCounters; ++k) acc[k] = 0u;
    const uint32_t stride = gridDim.x * (uint32_t) kRefitBlock;
    for(uint32_t i = blockIdx.x * (uint32_t) kRefitBlock + threadIdx.x; i < num_nodes; i += stride){
        const uint4 a = qnodes[(size_t) i * 2], b = qnodes[(size_t) i * 2 + 1];
        const uint32_t w[6] = { a.x, a.y, a.z, a.w, b.x, b.y };
        const uint32_t code[2] = { b.z, b.w };
        uint32_t rlo[3] = { 0xFFFFu, 0xFFFFu, 0xFFFFu }, rhi[3] = { 0u, 0u, 0u };
        bool any = false;
#pragma unroll
        for(int c = 0; c < 2; ++c){
            if(code[c] == kEmpty){ acc[2] += 1u; continue; }
            uint64_t d[3];
#pragma unroll
            for(int ax = 0; ax < 3; ++ax){
                const uint32_t lo = c ? w[2 * ax] >> 16 : w[2 * ax] & 0xFFFFu, hi = c ? w[2 * ax + 1] >> 16 : w[2 * ax + 1] & 0xFFFFu;
                d[ax] = hi >= lo ? hi - lo : 0u;
                rlo[ax] = lo < rlo[ax] ? lo : rlo[ax]; rhi[ax] = hi > rhi[ax] ? hi : rhi[ax];
            }
            any = true;
            const uint64_t xy = d[0] * d[1], yz = d[1] * d[2], zx = d[2] * d[0];
            if(code[c] & kLeaf){
                const uint64_t k = (code[c] & 7u) + 1u;
                acc[1] += 1u; acc[3] += k;
                acc[7] += k * xy; acc[8] += k * yz; acc[9] += k * zx;
            } else {
                acc[0] += 1u;
                acc[4] += xy; acc[5] += yz; acc[6] += zx;
            }
        }
        if(i == 0u){
            uint32_t *ext = (uint32_t *) (result + kCostCounters);
#pragma unroll
            for(int ax = 0; ax < 3; ++ax) ext[ax] = any && rhi[ax] >= rlo[ax] ? rhi[ax] - rlo[ax] : 0u;
        }
    }
    const int lane = (int) (threadIdx.x & 63u), wave = (int) (threadIdx.x >> 6);
#pragma unroll
    for(int k = 0; k < kCostCounters; ++k){
        const uint64_t v = wave_sum(acc[k]);
        if(lane == 0) red[wave][k] = v;
    }
    __syncthreads();
    if(threadIdx.x < (uint32_t) kCostCounters){
        uint64_t v = 0u;
#pragma unroll
        for(int q = 0; q < kCostWaves; ++q) v += red[q][threadIdx.x];
        if(v) atomicAdd(result + threadIdx.x, (unsigned long long) v);
    }
}

} // namespace

void launch_tree_cost(hipStream_t s, const uint4 *qnodes, uint32_t num_nodes, unsigned long long *result){
    if(num_nodes == 0) return;
    const dim3 grid(std::min<uint32_t>(refit_blocks(num_nodes), (uint32_t) kCostMaxBlocks));
    hipLaunchKernelGGL(k_tree_cost, grid, dim3(kRefitBlock), 0, s, qnodes, num_nodes, result);
}

} // namespace hpt
