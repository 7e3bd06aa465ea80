// Device builder kernels (lbvh_kernels.h): the topology of a Morton-order linear BVH, to the bytes of lbvh_host_scene
// (scene_build.cpp).  Float expressions are evaluated as written (-ffp-contract=off); the only ones here are the cell of a
// centroid and the half area of a stored box.  Every index read from memory is checked against its array before it is used.
#include "lbvh_kernels.h"

#include <algorithm>
#include <cmath>
#include <rocprim/device/device_radix_sort.hpp>

namespace hpt {
namespace {

constexpr uint32_t kLeaf = 0x80000000u, kEmpty = 0xFFFFFFFFu;
constexpr uint32_t kLeafTris = 2u;        // kMaxLeafTris (hpt_scene.h; asserted in scene_rebuild_device.cpp)

// exclusive prefix sum of v over the block; total = the block's sum (every lane of the block calls this)
__device__ uint32_t block_scan(uint32_t v, uint32_t &total){
    __shared__ uint32_t sh[kLbvhBlock];
    const uint32_t t = threadIdx.x;
    sh[t] = v;
    __syncthreads();
    for(uint32_t off = 1; off < (uint32_t) kLbvhBlock; off <<= 1){
        const uint32_t x = t >= off ? sh[t - off] : 0u;
        __syncthreads();
        sh[t] += x;
        __syncthreads();
    }
    const uint32_t incl = sh[t];
    total = sh[kLbvhBlock - 1];
    __syncthreads();
    return incl - v;
}

__global__ __launch_bounds__(kLbvhBlock) void k_lbvh_identity(float4 *__restrict__ tris, uint32_t *__restrict__ idx, uint32_t num_tris, uint32_t num_rounds){
    const uint32_t stride = gridDim.x * (uint32_t) kLbvhBlock;
    for(uint32_t i = blockIdx.x * (uint32_t) kLbvhBlock + threadIdx.x; i < num_tris; i += stride){
        tris[(size_t) i * 3] = make_float4(0.0f, 0.0f, 0.0f, __uint_as_float(num_rounds + i));
        tris[(size_t) i * 3 + 1] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        tris[(size_t) i * 3 + 2] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        idx[i] = i;
    }
}

// Builder::bin_of's shape (scene_build.cpp): comparisons first, so a NaN goes to cell 0 and nothing out of range is converted
__device__ __forceinline__ uint32_t cell_of(float cen, float lo, float scale){
    const float f = (cen - lo) * scale;
    return f >= 1.0f ? (f < 2097152.0f ? (uint32_t) f : 2097151u) : 0u;
}
// bit k of a 21-bit cell to bit 3 * k
__device__ __forceinline__ unsigned long long spread21(uint32_t v){
    unsigned long long x = v & 0x1FFFFFu;
    x = (x | x << 32) & 0x001F00000000FFFFull;
    x = (x | x << 16) & 0x001F0000FF0000FFull;
    x = (x | x << 8) & 0x100F00F00F00F00Full;
    x = (x | x << 4) & 0x10C30C30C30C30C3ull;
    x = (x | x << 2) & 0x1249249249249249ull;
    return x;
}

__global__ __launch_bounds__(kLbvhBlock) void k_lbvh_keys(const float *__restrict__ box, uint32_t num_tris, LbvhCells c,
                                                          unsigned long long *__restrict__ keys){
    const uint32_t stride = gridDim.x * (uint32_t) kLbvhBlock;
    for(uint32_t i = blockIdx.x * (uint32_t) kLbvhBlock + threadIdx.x; i < num_tris; i += stride){
        const float2 a = ((const float2 *) (box + (size_t) i * 6))[0], b = ((const float2 *) (box + (size_t) i * 6))[1], d = ((const float2 *) (box + (size_t) i * 6))[2];
        const float mn[3] = { a.x, a.y, b.x }, mx[3] = { b.y, d.x, d.y };
        unsigned long long key = ~0ull;                    // dead: above every live key
        if(mn[0] <= mx[0]){
            const uint32_t cx = cell_of(0.5f * (mn[0] + mx[0]), c.lo[0], c.scale[0]);
            const uint32_t cy = cell_of(0.5f * (mn[1] + mx[1]), c.lo[1], c.scale[1]);
            const uint32_t cz = cell_of(0.5f * (mn[2] + mx[2]), c.lo[2], c.scale[2]);
            key = spread21(cx) << 2 | spread21(cy) << 1 | spread21(cz);
        }
        keys[i] = key;
    }
}

__global__ __launch_bounds__(kLbvhBlock) void k_lbvh_rank(const uint32_t *__restrict__ idx_sorted, uint32_t num_tris, uint32_t *__restrict__ rank){
    const uint32_t stride = gridDim.x * (uint32_t) kLbvhBlock;
    for(uint32_t p = blockIdx.x * (uint32_t) kLbvhBlock + threadIdx.x; p < num_tris; p += stride){
        const uint32_t i = idx_sorted[p];
        if(i < num_tris) rank[i] = p;
    }
}

__global__ __launch_bounds__(kLbvhBlock) void k_lbvh_permute(const float4 *__restrict__ old_tris, const uint32_t *__restrict__ rank, uint32_t num_tris,
                                                             uint32_t num_rounds, float4 *__restrict__ new_tris){
    const uint32_t stride = gridDim.x * (uint32_t) kLbvhBlock;
    for(uint32_t s = blockIdx.x * (uint32_t) kLbvhBlock + threadIdx.x; s < num_tris; s += stride){
        const float w0 = old_tris[(size_t) s * 3].w, w1 = old_tris[(size_t) s * 3 + 1].w, w2 = old_tris[(size_t) s * 3 + 2].w;
        const uint32_t i = __float_as_uint(w0) - num_rounds;
        if(i >= num_tris) continue;                        // (a slot's ordinal names an input triangle)
        const uint32_t p = rank[i];
        if(p >= num_tris) continue;
        new_tris[(size_t) p * 3] = make_float4(0.0f, 0.0f, 0.0f, w0);
        new_tris[(size_t) p * 3 + 1] = make_float4(0.0f, 0.0f, 0.0f, w1);
        new_tris[(size_t) p * 3 + 2] = make_float4(0.0f, 0.0f, 0.0f, w2);
    }
}

// common-prefix length of the sorted pairs at positions i and j, -1 when j lies outside
__device__ __forceinline__ int delta(const unsigned long long *__restrict__ keys, long long n, long long i, unsigned long long ki, long long j){
    if(j < 0 || j >= n) return -1;
    const unsigned long long x = ki ^ keys[j];
    if(x) return __clzll((long long) x);
    return 64 + __clz((int) ((uint32_t) i ^ (uint32_t) j));
}

__device__ __forceinline__ uint32_t leaf_code(long long first, long long count){ return kLeaf | ((uint32_t) first << 3) | (uint32_t) (count - 1); }

// Karras 2012, one lane per inner node: the direction of the node's range, its other end by doubling and bisection, the split
// by bisection.  Every loop is bounded by the bit length of num_tris.
__global__ __launch_bounds__(kLbvhBlock) void k_lbvh_radix(const unsigned long long *__restrict__ keys, uint32_t num_tris, uint2 *__restrict__ child){
    const long long n = (long long) num_tris;
    const long long i = (long long) blockIdx.x * kLbvhBlock + threadIdx.x;
    if(i >= n - 1) return;
    const unsigned long long ki = keys[i];
    const long long d = delta(keys, n, i, ki, i + 1) > delta(keys, n, i, ki, i - 1) ? 1 : -1;
    const int dmin = delta(keys, n, i, ki, i - d);
    long long lmax = 2;
    while(lmax < 2 * n && delta(keys, n, i, ki, i + lmax * d) > dmin) lmax *= 2;
    long long l = 0;
    for(long long t = lmax / 2; t >= 1; t /= 2) if(delta(keys, n, i, ki, i + (l + t) * d) > dmin) l += t;
    const long long j = i + l * d;
    const int dnode = delta(keys, n, i, ki, j);
    long long s = 0;
    for(long long t = (l + 1) / 2; ; t = (t + 1) / 2){
        if(delta(keys, n, i, ki, i + (s + t) * d) > dnode) s += t;
        if(t <= 1) break;
    }
    const long long gamma = i + s * d + (d < 0 ? -1 : 0);
    const long long first = i < j ? i : j, last = i < j ? j : i;
    const long long lc = gamma - first + 1, rc = last - gamma;
    child[i] = make_uint2(lc <= (long long) kLeafTris ? leaf_code(first, lc) : (uint32_t) gamma,
                          rc <= (long long) kLeafTris ? leaf_code(gamma + 1, rc) : (uint32_t) (gamma + 1));
}

__device__ __forceinline__ uint32_t is_inner(uint32_t code){ return (code & kLeaf) ? 0u : 1u; }     // (an empty child has the bit too)

__global__ __launch_bounds__(kLbvhBlock) void k_lbvh_level_count(const uint2 *__restrict__ child, uint32_t num_inner, const uint32_t *__restrict__ from,
                                                                 uint32_t first, uint32_t count, uint32_t *__restrict__ cnt, uint32_t *__restrict__ block_sum){
    const uint32_t j = blockIdx.x * (uint32_t) kLbvhBlock + threadIdx.x;
    uint32_t c = 0;
    if(j < count){
        const uint32_t k = from[first + j];
        if(k < num_inner){ const uint2 ch = child[k]; c = is_inner(ch.x) + is_inner(ch.y); }
        cnt[j] = c;
    }
    uint32_t total;
    block_scan(c, total);
    if(threadIdx.x == 0) block_sum[blockIdx.x] = total;
}

__global__ __launch_bounds__(kLbvhBlock) void k_lbvh_scan(uint32_t *__restrict__ block_sum, uint32_t blocks, uint32_t *__restrict__ total_out){
    uint32_t carry = 0;
    for(uint32_t base = 0; base < blocks; base += (uint32_t) kLbvhBlock){
        const uint32_t at = base + threadIdx.x;
        const uint32_t v = at < blocks ? block_sum[at] : 0u;
        uint32_t total;
        const uint32_t ex = block_scan(v, total);
        if(at < blocks) block_sum[at] = carry + ex;
        carry += total;
    }
    if(threadIdx.x == 0) *total_out = carry;
}

__global__ __launch_bounds__(kLbvhBlock) void k_lbvh_level_scatter(const uint2 *__restrict__ child, uint32_t num_inner, uint32_t *__restrict__ from,
                                                                   uint32_t first, uint32_t count, const uint32_t *__restrict__ cnt,
                                                                   const uint32_t *__restrict__ block_sum, float4 *__restrict__ nodes, uint32_t max_nodes){
    const uint32_t j = blockIdx.x * (uint32_t) kLbvhBlock + threadIdx.x;
    const uint32_t c = j < count ? cnt[j] : 0u;
    uint32_t total;
    const uint32_t ex = block_scan(c, total);
    if(j >= count) return;
    const uint32_t node = first + j;
    if(node >= max_nodes) return;
    uint32_t o = first + count + block_sum[blockIdx.x] + ex;
    const uint32_t k = from[node];
    uint2 ch = make_uint2(kEmpty, kEmpty);
    if(k < num_inner) ch = child[k];
    uint32_t code[2] = { ch.x, ch.y };
#pragma unroll
    for(int side = 0; side < 2; ++side){
        if(!is_inner(code[side])) continue;
        if(o < max_nodes){ from[o] = code[side]; code[side] = o; } else code[side] = kEmpty;      // (the host has checked the total: never taken)
        ++o;
    }
    nodes[(size_t) node * 4] = make_float4(INFINITY, INFINITY, INFINITY, __uint_as_float(code[0]));
    nodes[(size_t) node * 4 + 1] = make_float4(-INFINITY, -INFINITY, -INFINITY, __uint_as_float(code[1]));
    nodes[(size_t) node * 4 + 2] = make_float4(INFINITY, INFINITY, INFINITY, 0.0f);
    nodes[(size_t) node * 4 + 3] = make_float4(-INFINITY, -INFINITY, -INFINITY, 0.0f);
}

// ---- bounded builds: the topology top-down, one level per launch pair (lbvh_bounded_host_scene, scene_build.cpp) ----

// the levels a range of count triangles needs: the smallest k >= 1 with 2^k >= (count + 1) / 2
__device__ __forceinline__ int need_of(uint32_t count){
    const uint32_t leaves = (count + 1u) / 2u;
    return leaves <= 2u ? 1 : 32 - __clz((int) (leaves - 1u));
}
// a range a node may have: more than a leaf, inside the sorted positions
__device__ __forceinline__ bool range_ok(uint2 r, uint32_t num_tris){ return r.y > kLeafTris && r.x < num_tris && r.y <= num_tris - r.x; }

// One lane per node of the level, a block per 256 of them, blocks striding.  The lane's split: forced (balanced halves of full
// leaves) when its range needs every level left, else Karras' split by a bisection of at most 32 trips.  The block's scan
// carries the inner children in its low half and the forced nodes in its high half (at most 512 and 256 per block).
__global__ __launch_bounds__(kLbvhBlock) void k_lbvh_bounded_count(const unsigned long long *__restrict__ keys, uint32_t num_tris,
                                                                   const uint2 *__restrict__ range, uint32_t first, uint32_t count, uint32_t max_nodes,
                                                                   int levels_left, uint32_t *__restrict__ split, uint32_t *__restrict__ cnt,
                                                                   uint32_t *__restrict__ block_sum, uint32_t *__restrict__ forced){
    const uint32_t chunks = (count + (uint32_t) kLbvhBlock - 1u) / (uint32_t) kLbvhBlock;
    for(uint32_t chunk = blockIdx.x; chunk < chunks; chunk += gridDim.x){
        const uint32_t j = chunk * (uint32_t) kLbvhBlock + threadIdx.x;
        uint32_t c = 0, f = 0;
        if(j < count){
            const uint32_t node = first + j;
            if(node < max_nodes){
                const uint2 r = range[node];
                uint32_t lc = 0;                               // 0: not a range, the scatter writes nothing for it
                if(range_ok(r, num_tris)){
                    if(need_of(r.y) >= levels_left){
                        const uint32_t leaves = (r.y + 1u) / 2u;
                        lc = 2u * ((leaves + 1u) / 2u);
                        f = 1u;
                    } else {
                        const long long n = (long long) num_tris, a = (long long) r.x, last = a + (long long) r.y - 1;
                        const unsigned long long ka = keys[a];
                        const int dnode = delta(keys, n, a, ka, last);
                        long long lo = a, hi = last;           // delta(a, lo) > dnode >= delta(a, hi)
                        for(int it = 0; it < 32; ++it){
                            if(hi - lo <= 1) break;
                            const long long mid = lo + (hi - lo) / 2;
                            if(delta(keys, n, a, ka, mid) > dnode) lo = mid; else hi = mid;
                        }
                        lc = (uint32_t) (lo - a) + 1u;
                    }
                    c = (lc > kLeafTris ? 1u : 0u) + (r.y - lc > kLeafTris ? 1u : 0u);
                }
                split[node] = lc;
            }
            cnt[j] = c;
        }
        uint32_t total;
        block_scan(c | f << 16, total);
        if(threadIdx.x == 0){
            block_sum[chunk] = total & 0xFFFFu;
            if(total >> 16) atomicAdd(forced, total >> 16);
        }
    }
}

// The record k_lbvh_level_scatter writes, from the node's range and split; the children's ranges go to their new numbers.
__global__ __launch_bounds__(kLbvhBlock) void k_lbvh_bounded_scatter(uint2 *__restrict__ range, const uint32_t *__restrict__ split, uint32_t num_tris,
                                                                     uint32_t first, uint32_t count, const uint32_t *__restrict__ cnt,
                                                                     const uint32_t *__restrict__ block_sum, float4 *__restrict__ nodes, uint32_t max_nodes){
    const uint32_t chunks = (count + (uint32_t) kLbvhBlock - 1u) / (uint32_t) kLbvhBlock;
    for(uint32_t chunk = blockIdx.x; chunk < chunks; chunk += gridDim.x){
        const uint32_t j = chunk * (uint32_t) kLbvhBlock + threadIdx.x;
        const uint32_t c = j < count ? cnt[j] : 0u;
        uint32_t total;
        const uint32_t ex = block_scan(c, total);
        const uint32_t node = first + j;
        if(j >= count || node >= max_nodes) continue;
        const uint2 r = range[node];
        const uint32_t lc = split[node];
        if(!range_ok(r, num_tris) || lc == 0u || lc >= r.y) continue;
        uint32_t o = first + count + block_sum[chunk] + ex;
        const uint32_t cf[2] = { r.x, r.x + lc }, cc[2] = { lc, r.y - lc };
        uint32_t code[2];
#pragma unroll
        for(int side = 0; side < 2; ++side){
            if(cc[side] <= kLeafTris){ code[side] = leaf_code(cf[side], cc[side]); continue; }
            if(o < max_nodes){ range[o] = make_uint2(cf[side], cc[side]); code[side] = o; } else code[side] = kEmpty;     // (the host has checked the total: never taken)
            ++o;
        }
        nodes[(size_t) node * 4] = make_float4(INFINITY, INFINITY, INFINITY, __uint_as_float(code[0]));
        nodes[(size_t) node * 4 + 1] = make_float4(-INFINITY, -INFINITY, -INFINITY, __uint_as_float(code[1]));
        nodes[(size_t) node * 4 + 2] = make_float4(INFINITY, INFINITY, INFINITY, 0.0f);
        nodes[(size_t) node * 4 + 3] = make_float4(-INFINITY, -INFINITY, -INFINITY, 0.0f);
    }
}

// ---- the four-wide collapse ----

struct Kids { uint32_t code[4], src[4]; float area[4]; int n; };

__device__ __forceinline__ void put(Kids &ks, uint32_t code, uint32_t src, float area){
#pragma unroll
    for(int k = 0; k < 4; ++k) if(k == ks.n){ ks.code[k] = code; ks.src[k] = src; ks.area[k] = area; }
    ks.n += 1;
}
// the collapse's half area of a stored box: no clamp (build_host_scene's lambda)
__device__ __forceinline__ float half_area(const float4 &mn, const float4 &mx){
    const float dx = mx.x - mn.x, dy = mx.y - mn.y, dz = mx.z - mn.z;
    return dx * dy + dy * dz + dz * dx;
}
__device__ __forceinline__ void open(Kids &ks, const float4 *__restrict__ nodes, uint32_t num_nodes, uint32_t idx){
    if(idx >= num_nodes || ks.n > 2) return;
    const float4 q0 = nodes[(size_t) idx * 4], q1 = nodes[(size_t) idx * 4 + 1], q2 = nodes[(size_t) idx * 4 + 2], q3 = nodes[(size_t) idx * 4 + 3];
    const uint32_t left = __float_as_uint(q0.w), right = __float_as_uint(q1.w);
    if(left != kEmpty) put(ks, left, idx * 2u, half_area(q0, q1));
    if(right != kEmpty) put(ks, right, idx * 2u + 1u, half_area(q2, q3));
}

__global__ __launch_bounds__(kLbvhBlock) void k_lbvh_wide_collapse(const float4 *__restrict__ nodes, uint32_t num_nodes, const uint32_t *__restrict__ todo,
                                                                   uint32_t first, uint32_t count, uint4 *__restrict__ kid_code,
                                                                   uint4 *__restrict__ wide_src, uint32_t *__restrict__ cnt, uint32_t *__restrict__ block_sum){
    const uint32_t j = blockIdx.x * (uint32_t) kLbvhBlock + threadIdx.x;
    uint32_t c = 0;
    if(j < count){
        Kids ks; ks.n = 0;
#pragma unroll
        for(int k = 0; k < 4; ++k){ ks.code[k] = kEmpty; ks.src[k] = kEmpty; ks.area[k] = 0.0f; }
        open(ks, nodes, num_nodes, todo[first + j]);
        for(int it = 0; it < 2 && ks.n < 4; ++it){         // two openings fill four places
            int best = -1; float ba = -1.0f;
#pragma unroll
            for(int k = 0; k < 4; ++k) if(k < ks.n && !(ks.code[k] & kLeaf) && ks.area[k] > ba){ ba = ks.area[k]; best = k; }
            if(best < 0) break;
            uint32_t cc = kEmpty, lc = kEmpty, ls = kEmpty; float la = 0.0f;
#pragma unroll
            for(int k = 0; k < 4; ++k){ if(k == best) cc = ks.code[k]; if(k == ks.n - 1){ lc = ks.code[k]; ls = ks.src[k]; la = ks.area[k]; } }
            // the opened child's place takes the last child; the last place empties
#pragma unroll
            for(int k = 0; k < 4; ++k){
                if(k == best){ ks.code[k] = lc; ks.src[k] = ls; ks.area[k] = la; }
                if(k == ks.n - 1){ ks.code[k] = kEmpty; ks.src[k] = kEmpty; }
            }
            ks.n -= 1;
            open(ks, nodes, num_nodes, cc);
        }
#pragma unroll
        for(int k = 0; k < 4; ++k) if(k < ks.n && !(ks.code[k] & kLeaf)) ++c;
        kid_code[first + j] = make_uint4(ks.code[0], ks.code[1], ks.code[2], ks.code[3]);
        wide_src[first + j] = make_uint4(ks.src[0], ks.src[1], ks.src[2], ks.src[3]);
        cnt[j] = c;
    }
    uint32_t total;
    block_scan(c, total);
    if(threadIdx.x == 0) block_sum[blockIdx.x] = total;
}

__global__ __launch_bounds__(kLbvhBlock) void k_lbvh_wide_scatter(const uint4 *__restrict__ kid_code, uint32_t *__restrict__ todo, uint32_t first, uint32_t count,
                                                                  const uint32_t *__restrict__ cnt, const uint32_t *__restrict__ block_sum,
                                                                  uint4 *__restrict__ wnodes, uint32_t max_wide){
    const uint32_t j = blockIdx.x * (uint32_t) kLbvhBlock + threadIdx.x;
    const uint32_t c = j < count ? cnt[j] : 0u;
    uint32_t total;
    const uint32_t ex = block_scan(c, total);
    if(j >= count) return;
    const uint32_t w = first + j;
    if(w >= max_wide) return;
    uint32_t o = first + count + block_sum[blockIdx.x] + ex;
    const uint4 kc = kid_code[w];
    uint32_t code[4] = { kc.x, kc.y, kc.z, kc.w };
#pragma unroll
    for(int k = 0; k < 4; ++k){
        if(code[k] & kLeaf) continue;                      // a leaf, or no child
        if(o < max_wide){ todo[o] = code[k]; code[k] = o; } else code[k] = kEmpty;      // (the host has checked the total: never taken)
        ++o;
    }
    wnodes[(size_t) w * 4 + 3] = make_uint4(code[0], code[1], code[2], code[3]);
}

dim3 stride_grid(uint32_t n){ return dim3(std::min<uint32_t>(std::max<uint32_t>(lbvh_blocks(n), 1u), (uint32_t) kLbvhMaxBlocks)); }

} // namespace

void launch_lbvh_identity(hipStream_t s, float4 *tris, uint32_t *idx, uint32_t num_tris, uint32_t num_rounds){
    if(num_tris == 0) return;
    hipLaunchKernelGGL(k_lbvh_identity, stride_grid(num_tris), dim3(kLbvhBlock), 0, s, tris, idx, num_tris, num_rounds);
}

void launch_lbvh_keys(hipStream_t s, const float *box, uint32_t num_tris, LbvhCells cells, unsigned long long *keys){
    if(num_tris == 0) return;
    hipLaunchKernelGGL(k_lbvh_keys, stride_grid(num_tris), dim3(kLbvhBlock), 0, s, box, num_tris, cells, keys);
}

size_t lbvh_sort_tmp_bytes(uint32_t num_tris){
    size_t bytes = 0;
    rocprim::radix_sort_pairs(nullptr, bytes, (unsigned long long *) nullptr, (unsigned long long *) nullptr, (uint32_t *) nullptr, (uint32_t *) nullptr,
                              (size_t) num_tris, 0, 64);
    return bytes;
}

int launch_lbvh_sort(hipStream_t s, void *tmp, size_t tmp_bytes, const unsigned long long *keys, unsigned long long *keys_sorted,
                     const uint32_t *idx, uint32_t *idx_sorted, uint32_t num_tris){
    if(num_tris == 0) return 0;
    // LSD radix sort is stable and its input is in index order: equal keys stay in input order
    size_t bytes = tmp_bytes;
    return (int) rocprim::radix_sort_pairs(tmp, bytes, keys, keys_sorted, idx, idx_sorted, (size_t) num_tris, 0, 64, s);
}

void launch_lbvh_rank(hipStream_t s, const uint32_t *idx_sorted, uint32_t num_tris, uint32_t *rank){
    if(num_tris == 0) return;
    hipLaunchKernelGGL(k_lbvh_rank, stride_grid(num_tris), dim3(kLbvhBlock), 0, s, idx_sorted, num_tris, rank);
}

void launch_lbvh_permute(hipStream_t s, const float4 *old_tris, const uint32_t *rank, uint32_t num_tris, uint32_t num_rounds, float4 *new_tris){
    if(num_tris == 0) return;
    hipLaunchKernelGGL(k_lbvh_permute, stride_grid(num_tris), dim3(kLbvhBlock), 0, s, old_tris, rank, num_tris, num_rounds, new_tris);
}

void launch_lbvh_radix(hipStream_t s, const unsigned long long *keys_sorted, uint32_t num_tris, uint2 *child){
    if(num_tris < 2) return;
    hipLaunchKernelGGL(k_lbvh_radix, dim3(lbvh_blocks(num_tris - 1u)), dim3(kLbvhBlock), 0, s, keys_sorted, num_tris, child);
}

void launch_lbvh_level_count(hipStream_t s, const uint2 *child, uint32_t num_inner, const uint32_t *from, uint32_t first, uint32_t count, uint32_t *cnt,
                             uint32_t *block_sum){
    if(count == 0) return;
    hipLaunchKernelGGL(k_lbvh_level_count, dim3(lbvh_blocks(count)), dim3(kLbvhBlock), 0, s, child, num_inner, from, first, count, cnt, block_sum);
}

void launch_lbvh_scan(hipStream_t s, uint32_t *block_sum, uint32_t blocks, uint32_t *total){
    hipLaunchKernelGGL(k_lbvh_scan, dim3(1), dim3(kLbvhBlock), 0, s, block_sum, blocks, total);
}

void launch_lbvh_level_scatter(hipStream_t s, const uint2 *child, uint32_t num_inner, uint32_t *from, uint32_t first, uint32_t count, const uint32_t *cnt,
                               const uint32_t *block_sum, float4 *nodes, uint32_t max_nodes){
    if(count == 0) return;
    hipLaunchKernelGGL(k_lbvh_level_scatter, dim3(lbvh_blocks(count)), dim3(kLbvhBlock), 0, s, child, num_inner, from, first, count, cnt, block_sum, nodes,
                       max_nodes);
}

void launch_lbvh_bounded_count(hipStream_t s, const unsigned long long *keys_sorted, uint32_t num_tris, const uint2 *range, uint32_t first, uint32_t count,
                               uint32_t max_nodes, int levels_left, uint32_t *split, uint32_t *cnt, uint32_t *block_sum, uint32_t *forced){
    if(count == 0) return;
    hipLaunchKernelGGL(k_lbvh_bounded_count, stride_grid(count), dim3(kLbvhBlock), 0, s, keys_sorted, num_tris, range, first, count, max_nodes, levels_left,
                       split, cnt, block_sum, forced);
}

void launch_lbvh_bounded_scatter(hipStream_t s, uint2 *range, const uint32_t *split, uint32_t num_tris, uint32_t first, uint32_t count, const uint32_t *cnt,
                                 const uint32_t *block_sum, float4 *nodes, uint32_t max_nodes){
    if(count == 0) return;
    hipLaunchKernelGGL(k_lbvh_bounded_scatter, stride_grid(count), dim3(kLbvhBlock), 0, s, range, split, num_tris, first, count, cnt, block_sum, nodes,
                       max_nodes);
}

void launch_lbvh_wide_collapse(hipStream_t s, const float4 *nodes, uint32_t num_nodes, const uint32_t *todo, uint32_t first, uint32_t count,
                               uint4 *kid_code, uint4 *wide_src, uint32_t *cnt, uint32_t *block_sum){
    if(count == 0) return;
    hipLaunchKernelGGL(k_lbvh_wide_collapse, dim3(lbvh_blocks(count)), dim3(kLbvhBlock), 0, s, nodes, num_nodes, todo, first, count, kid_code, wide_src, cnt,
                       block_sum);
}

void launch_lbvh_wide_scatter(hipStream_t s, const uint4 *kid_code, uint32_t *todo, uint32_t first, uint32_t count, const uint32_t *cnt,
                              const uint32_t *block_sum, uint4 *wnodes, uint32_t max_wide){
    if(count == 0) return;
    hipLaunchKernelGGL(k_lbvh_wide_scatter, dim3(lbvh_blocks(count)), dim3(kLbvhBlock), 0, s, kid_code, todo, first, count, cnt, block_sum, wnodes, max_wide);
}

} // namespace hpt
