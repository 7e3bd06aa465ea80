// Refit kernels (refit_kernels.h): the builder's arithmetic on new vertex positions, to the bytes of refit_host_scene
// (scene_build.cpp).  Every float expression is evaluated as written (-ffp-contract=off); min / max are the comparisons of
// std::min / std::max, and the float neighbours are taken on the bit pattern, so nothing depends on a math library.
#include "refit_kernels.h"

#include <algorithm>
#include <cmath>

namespace hpt {
namespace {

constexpr uint32_t kLeaf = 0x80000000u, kEmpty = 0xFFFFFFFFu;

__device__ __forceinline__ float min_f(float a, float b){ return b < a ? b : a; }      // std::min(a, b)
__device__ __forceinline__ float max_f(float a, float b){ return a < b ? b : a; }      // std::max(a, b)

// std::nextafter(x, -INFINITY) and (x, +INFINITY)
__device__ __forceinline__ float next_down(float x){
    if(x != x) return x;
    if(x == 0.0f) return __uint_as_float(0x80000001u);
    const uint32_t u = __float_as_uint(x);
    if(u == 0xFF800000u) return x;
    return __uint_as_float(x > 0.0f ? u - 1u : u + 1u);
}
__device__ __forceinline__ float next_up(float x){
    if(x != x) return x;
    if(x == 0.0f) return __uint_as_float(0x00000001u);
    const uint32_t u = __float_as_uint(x);
    if(u == 0x7F800000u) return x;
    return __uint_as_float(x > 0.0f ? u + 1u : u - 1u);
}

__device__ __forceinline__ bool finite_f(float x){ return (__float_as_uint(x) & 0x7F800000u) != 0x7F800000u; }

// a - b with the host's NaN: the builder's edges are computed by x86 SSE, where a NaN operand comes back quieted (the first
// one when both are) and inf - inf is the negative default NaN; the device's subtraction is an addition of -b and would hand
// out other sign bits.  Only the bytes of dead triangles' records depend on it (no ray hits one: hit_triangle rejects a NaN).
__device__ __forceinline__ float sub_as_host(float a, float b){
    if(a != a) return __uint_as_float(__float_as_uint(a) | 0x00400000u);
    if(b != b) return __uint_as_float(__float_as_uint(b) | 0x00400000u);
    const float r = a - b;
    return r != r ? __uint_as_float(0xFFC00000u) : r;
}

struct DBox { float mn[3], mx[3]; };
__device__ __forceinline__ void reset(DBox &b){ for(int a = 0; a < 3; ++a){ b.mn[a] = INFINITY; b.mx[a] = -INFINITY; } }
__device__ __forceinline__ void grow(DBox &b, const DBox &o){ for(int a = 0; a < 3; ++a){ b.mn[a] = min_f(b.mn[a], o.mn[a]); b.mx[a] = max_f(b.mx[a], o.mx[a]); } }
__device__ __forceinline__ void grow(DBox &b, float x, float y, float z){
    b.mn[0] = min_f(b.mn[0], x); b.mx[0] = max_f(b.mx[0], x);
    b.mn[1] = min_f(b.mn[1], y); b.mx[1] = max_f(b.mx[1], y);
    b.mn[2] = min_f(b.mn[2], z); b.mx[2] = max_f(b.mx[2], z);
}
__device__ __forceinline__ DBox load_box(const float *p){
    const float2 a = ((const float2 *) p)[0], b = ((const float2 *) p)[1], c = ((const float2 *) p)[2];
    DBox r; r.mn[0] = a.x; r.mn[1] = a.y; r.mn[2] = b.x; r.mx[0] = b.y; r.mx[1] = c.x; r.mx[2] = c.y;
    return r;
}
__device__ __forceinline__ void store_box(float *p, const DBox &b){
    ((float2 *) p)[0] = make_float2(b.mn[0], b.mn[1]); ((float2 *) p)[1] = make_float2(b.mn[2], b.mx[0]); ((float2 *) p)[2] = make_float2(b.mx[1], b.mx[2]);
}

// the union of the block's boxes in lane 0's `b` (every lane of the block calls this)
__device__ void block_union(DBox &b){
    __shared__ float red[6][kRefitBlock];
    const int t = (int) threadIdx.x;
    for(int a = 0; a < 3; ++a){ red[a][t] = b.mn[a]; red[3 + a][t] = b.mx[a]; }
    __syncthreads();
    for(int w = kRefitBlock / 2; w > 0; w >>= 1){
        if(t < w) for(int a = 0; a < 3; ++a){ red[a][t] = min_f(red[a][t], red[a][t + w]); red[3 + a][t] = max_f(red[3 + a][t], red[3 + a][t + w]); }
        __syncthreads();
    }
    for(int a = 0; a < 3; ++a){ b.mn[a] = red[a][0]; b.mx[a] = red[3 + a][0]; }
    __syncthreads();
}

__global__ __launch_bounds__(kRefitBlock) void k_refit_tris(const float *__restrict__ verts, float4 *__restrict__ tris, uint32_t num_tris,
                                                             uint32_t num_rounds, float *__restrict__ slot_box, float *__restrict__ partial,
                                                             uint32_t *__restrict__ dead_count){
    const uint32_t s = blockIdx.x * (uint32_t) kRefitBlock + threadIdx.x;
    DBox box; reset(box);
    int dead = 0;
    if(s < num_tris){
        const float4 r0 = tris[(size_t) s * 3], r1 = tris[(size_t) s * 3 + 1], r2 = tris[(size_t) s * 3 + 2];
        const uint32_t idx = __float_as_uint(r0.w) - num_rounds;
        bool live = idx < num_tris;           // (a slot's ordinal names an input triangle: anything else is not read)
        float v[9];
        if(live){
            const float *p = verts + (size_t) idx * 9;
            for(int k = 0; k < 9; ++k) v[k] = p[k];
        } else for(int k = 0; k < 9; ++k) v[k] = NAN;
        float e1[3], e2[3];
        for(int a = 0; a < 3; ++a){ e1[a] = sub_as_host(v[3 + a], v[a]); e2[a] = sub_as_host(v[6 + a], v[a]); }
        for(int a = 0; a < 3; ++a) live = live && finite_f(e1[a]) && finite_f(e2[a]);
        tris[(size_t) s * 3] = make_float4(v[0], v[1], v[2], r0.w);
        tris[(size_t) s * 3 + 1] = make_float4(e1[0], e1[1], e1[2], r1.w);
        tris[(size_t) s * 3 + 2] = make_float4(e2[0], e2[1], e2[2], r2.w);
        if(live){ grow(box, v[0], v[1], v[2]); grow(box, v[3], v[4], v[5]); grow(box, v[6], v[7], v[8]); }
        else dead = 1;
        store_box(slot_box + (size_t) s * 6, box);         // dead: inverted
    }
    const int block_dead = __syncthreads_count(dead);
    block_union(box);
    if(threadIdx.x == 0){
        store_box(partial + (size_t) blockIdx.x * 6, box);
        if(block_dead > 0) atomicAdd(dead_count, (uint32_t) block_dead);
    }
}

__global__ __launch_bounds__(kRefitBlock) void k_refit_reduce(const float *__restrict__ partial, uint32_t blocks, float *__restrict__ out6){
    DBox box; reset(box);
    for(uint32_t i = threadIdx.x; i < blocks; i += (uint32_t) kRefitBlock) grow(box, load_box(partial + (size_t) i * 6));
    block_union(box);
    if(threadIdx.x == 0) store_box(out6, box);
}

__device__ __forceinline__ void padded(const DBox &b, float pad_abs, float4 &mn, float4 &mx){
    float lo[3], hi[3];
    for(int a = 0; a < 3; ++a){
        lo[a] = next_down(next_down(b.mn[a] - pad_abs));
        hi[a] = next_up(next_up(b.mx[a] + pad_abs));
    }
    mn.x = lo[0]; mn.y = lo[1]; mn.z = lo[2]; mx.x = hi[0]; mx.y = hi[1]; mx.z = hi[2];
}

__global__ __launch_bounds__(kRefitBlock) void k_refit_level(float4 *__restrict__ nodes, uint32_t num_nodes, uint32_t first, uint32_t count,
                                                              const float *__restrict__ slot_box, uint32_t num_tris, float *__restrict__ exact,
                                                              float pad_abs, float dead_x, float dead_y, float dead_z){
    const uint32_t k = blockIdx.x * (uint32_t) kRefitBlock + threadIdx.x;
    if(k >= count || first + k >= num_nodes) return;
    const uint32_t i = first + k;
    float4 n[4];
    for(int q = 0; q < 4; ++q) n[q] = nodes[(size_t) i * 4 + q];
    DBox both; reset(both);
    for(int side = 0; side < 2; ++side){
        const uint32_t code = __float_as_uint(side ? n[1].w : n[0].w);
        if(code == kEmpty) continue;                       // keeps its inverted box
        DBox cb;
        if(code & kLeaf){
            reset(cb);
            const uint32_t s0 = (code & ~kLeaf) >> 3, c = (code & 7u) + 1u;
            for(uint32_t s = s0; s < s0 + c && s < num_tris; ++s){
                DBox sb = load_box(slot_box + (size_t) s * 6);
                if(!(sb.mn[0] <= sb.mx[0])){ sb.mn[0] = sb.mx[0] = dead_x; sb.mn[1] = sb.mx[1] = dead_y; sb.mn[2] = sb.mx[2] = dead_z; }
                grow(cb, sb);
            }
        } else {
            if(code >= num_nodes) continue;
            cb = load_box(exact + (size_t) code * 6);
        }
        padded(cb, pad_abs, n[side * 2], n[side * 2 + 1]);
        grow(both, cb);
    }
    for(int q = 0; q < 4; ++q) nodes[(size_t) i * 4 + q] = n[q];
    store_box(exact + (size_t) i * 6, both);
}

// the host's qlo / qhi (scene_build.cpp, grid_lo / grid_hi): the same comparisons, so a NaN lands on 0 here too
__device__ __forceinline__ uint32_t grid_lo(float v, float origin, float scale){
    const double q = floor(((double) v - (double) origin) / (double) scale) - 1.0;
    const double m = 0.0 < q ? q : 0.0;
    return (uint32_t) (m < 65535.0 ? m : 65535.0);
}
__device__ __forceinline__ uint32_t grid_hi(float v, float origin, float scale){
    const double q = ceil(((double) v - (double) origin) / (double) scale) + 1.0;
    const double m = 0.0 < q ? q : 0.0;
    return (uint32_t) (m < 65535.0 ? m : 65535.0);
}

__global__ __launch_bounds__(kRefitBlock) void k_refit_quantise(const float4 *__restrict__ nodes, uint4 *__restrict__ qnodes, uint32_t num_nodes,
                                                                 RefitGrid g){
    const uint32_t i = blockIdx.x * (uint32_t) kRefitBlock + threadIdx.x;
    if(i >= num_nodes) return;
    float4 n[4];
    for(int q = 0; q < 4; ++q) n[q] = nodes[(size_t) i * 4 + q];
    const uint32_t left = __float_as_uint(n[0].w), right = __float_as_uint(n[1].w);
    const float lmin[3] = { n[0].x, n[0].y, n[0].z }, lmax[3] = { n[1].x, n[1].y, n[1].z };
    const float rmin[3] = { n[2].x, n[2].y, n[2].z }, rmax[3] = { n[3].x, n[3].y, n[3].z };
    uint32_t w[6];
    for(int a = 0; a < 3; ++a){
        uint32_t ll = 65535u, lh = 0u, rl = 65535u, rh = 0u;
        if(left != kEmpty){ ll = grid_lo(lmin[a], g.qorigin[a], g.qscale[a]); lh = grid_hi(lmax[a], g.qorigin[a], g.qscale[a]); }
        if(right != kEmpty){ rl = grid_lo(rmin[a], g.qorigin[a], g.qscale[a]); rh = grid_hi(rmax[a], g.qorigin[a], g.qscale[a]); }
        w[2 * a] = ll | (rl << 16); w[2 * a + 1] = lh | (rh << 16);
    }
    qnodes[(size_t) i * 2] = make_uint4(w[0], w[1], w[2], w[3]);
    qnodes[(size_t) i * 2 + 1] = make_uint4(w[4], w[5], left, right);
}

__global__ __launch_bounds__(kRefitBlock) void k_refit_wide(const float4 *__restrict__ nodes, uint32_t num_nodes, uint4 *__restrict__ wnodes,
                                                             const uint4 *__restrict__ wide_src, uint32_t num_wide, RefitGrid g){
    const uint32_t i = blockIdx.x * (uint32_t) kRefitBlock + threadIdx.x;
    if(i >= num_wide) return;
    const uint4 s4 = wide_src[i];
    const uint32_t src[4] = { s4.x, s4.y, s4.z, s4.w };
    uint32_t lo[3][4], hi[3][4];
    for(int k = 0; k < 4; ++k){
        if(src[k] != kEmpty && (src[k] >> 1) < num_nodes){
            const size_t at = (size_t) (src[k] >> 1) * 4 + (size_t) (src[k] & 1u) * 2;
            const float4 mn = nodes[at], mx = nodes[at + 1];
            const float fmn[3] = { mn.x, mn.y, mn.z }, fmx[3] = { mx.x, mx.y, mx.z };
            for(int a = 0; a < 3; ++a){ lo[a][k] = grid_lo(fmn[a], g.qorigin[a], g.qscale[a]); hi[a][k] = grid_hi(fmx[a], g.qorigin[a], g.qscale[a]); }
        } else { for(int a = 0; a < 3; ++a){ lo[a][k] = 65535u; hi[a][k] = 0u; } }
    }
    for(int a = 0; a < 3; ++a)
        wnodes[(size_t) i * 4 + a] = make_uint4(lo[a][0] | (lo[a][1] << 16), lo[a][2] | (lo[a][3] << 16), hi[a][0] | (hi[a][1] << 16), hi[a][2] | (hi[a][3] << 16));
}

// ---- poses (include/hpt.h, "poses") ---------------------------------------------------------------------------------------

// one row of a record applied to a vertex: one operation at a time, left to right
__device__ __forceinline__ float pose_row(float a, float b, float c, float t, float x, float y, float z){
    return ((a * x + b * y) + c * z) + t;
}

// the 48 bytes of the identity's record, +0 throughout
__device__ __forceinline__ bool is_identity(const float4 &r0, const float4 &r1, const float4 &r2){
    constexpr uint32_t one = 0x3F800000u;
    const uint32_t ones = (__float_as_uint(r0.x) ^ one) | (__float_as_uint(r1.y) ^ one) | (__float_as_uint(r2.z) ^ one);
    const uint32_t zeros = __float_as_uint(r0.y) | __float_as_uint(r0.z) | __float_as_uint(r0.w) | __float_as_uint(r1.x) | __float_as_uint(r1.z) |
                           __float_as_uint(r1.w) | __float_as_uint(r2.x) | __float_as_uint(r2.y) | __float_as_uint(r2.w);
    return (ones | zeros) == 0u;
}

// One lane per vertex, a grid-stride loop over the 3 * num_tris vertices: neighbouring lanes read and write neighbouring 12
// bytes, so a wave's loads and stores each cover one contiguous run of 768 bytes.  76 bytes per triangle plus the table,
// which kStaged copies into LDS once per workgroup (num_parts <= kPoseLdsParts) and otherwise reads through the cache.
template <bool kStaged>
__global__ __launch_bounds__(kRefitBlock) void k_pose_verts(const float *__restrict__ rest, const int32_t *__restrict__ tri_part,
                                                             const float4 *__restrict__ xforms, uint32_t num_parts, uint64_t num_verts,
                                                             float *__restrict__ verts){
    __shared__ float4 table[kStaged ? kPoseLdsParts * 3 : 1];
    if(kStaged){
        for(uint32_t i = threadIdx.x; i < num_parts * 3u && i < (uint32_t) kPoseLdsParts * 3u; i += (uint32_t) kRefitBlock) table[i] = xforms[i];
        __syncthreads();
    }
    const uint64_t stride = (uint64_t) gridDim.x * (uint64_t) kRefitBlock;
    for(uint64_t v = (uint64_t) blockIdx.x * (uint64_t) kRefitBlock + threadIdx.x; v < num_verts; v += stride){
        const uint32_t part = (uint32_t) tri_part[v / 3u];
        if(part >= num_parts) continue;                     // (refused on the host: never out of the table)
        const float4 *r = kStaged ? table + (size_t) part * 3 : xforms + (size_t) part * 3;
        const float4 r0 = r[0], r1 = r[1], r2 = r[2];
        const float x = rest[v * 3u], y = rest[v * 3u + 1u], z = rest[v * 3u + 2u];
        float px = x, py = y, pz = z;
        if(!is_identity(r0, r1, r2)){
            px = pose_row(r0.x, r0.y, r0.z, r0.w, x, y, z);
            py = pose_row(r1.x, r1.y, r1.z, r1.w, x, y, z);
            pz = pose_row(r2.x, r2.y, r2.z, r2.w, x, y, z);
            if(!(finite_f(px) && finite_f(py) && finite_f(pz))) px = py = pz = __uint_as_float(0x7FC00000u);
        }
        verts[v * 3u] = px; verts[v * 3u + 1u] = py; verts[v * 3u + 2u] = pz;
    }
}

// ---- skinning (include/hpt.h, "skinning") ----------------------------------------------------------------------------------

// One lane per corner, the pose kernel's shape: a corner reads its four bones as one 8-byte word and its four weights as one
// float4, then 12 bytes of the rest pose, and writes 12 bytes: 148 bytes per triangle plus the table.  The cases of the
// definition (skin_vertex_host, scene_build.cpp), cheapest test first: four zero weights keep the vertex without a look at
// the table; otherwise the active influences are walked in index order, which yields both the blend and whether every
// record met was the identity (keep).  The rigid case needs no branch of its own: with one active weight of 1.0f the walk
// computes 1.0f * p, which has p's bits for every p that is not a NaN, and a NaN leaves as the canonical one either way.
template <bool kStaged>
__global__ __launch_bounds__(kRefitBlock) void k_skin_verts(const float *__restrict__ rest, const uint2 *__restrict__ corner_bone,
                                                             const float4 *__restrict__ corner_weight, const float4 *__restrict__ xforms,
                                                             uint32_t num_bones, uint64_t num_verts, float *__restrict__ verts){
    __shared__ float4 table[kStaged ? kPoseLdsParts * 3 : 1];
    if(kStaged){
        for(uint32_t i = threadIdx.x; i < num_bones * 3u && i < (uint32_t) kPoseLdsParts * 3u; i += (uint32_t) kRefitBlock) table[i] = xforms[i];
        __syncthreads();
    }
    const uint64_t stride = (uint64_t) gridDim.x * (uint64_t) kRefitBlock;
    for(uint64_t v = (uint64_t) blockIdx.x * (uint64_t) kRefitBlock + threadIdx.x; v < num_verts; v += stride){
        const uint2 bw = corner_bone[v];
        const float4 w4 = corner_weight[v];
        const float x = rest[v * 3u], y = rest[v * 3u + 1u], z = rest[v * 3u + 2u];
        const float w[4] = { w4.x, w4.y, w4.z, w4.w };
        const uint32_t b[4] = { bw.x & 0xFFFFu, bw.x >> 16, bw.y & 0xFFFFu, bw.y >> 16 };
        float px = x, py = y, pz = z;
        if((__float_as_uint(w4.x) | __float_as_uint(w4.y) | __float_as_uint(w4.z) | __float_as_uint(w4.w)) != 0u){
            bool keep = true, first = true;
            float ax = 0.0f, ay = 0.0f, az = 0.0f;
#pragma unroll
            for(int j = 0; j < 4; ++j){
                if(__float_as_uint(w[j]) == 0u || b[j] >= num_bones) continue;      // inactive: never evaluated (out of the table: refused on the host)
                const float4 *r = kStaged ? table + (size_t) b[j] * 3 : xforms + (size_t) b[j] * 3;
                const float4 r0 = r[0], r1 = r[1], r2 = r[2];
                keep = keep && is_identity(r0, r1, r2);
                const float mx = w[j] * pose_row(r0.x, r0.y, r0.z, r0.w, x, y, z);
                const float my = w[j] * pose_row(r1.x, r1.y, r1.z, r1.w, x, y, z);
                const float mz = w[j] * pose_row(r2.x, r2.y, r2.z, r2.w, x, y, z);
                ax = first ? mx : ax + mx; ay = first ? my : ay + my; az = first ? mz : az + mz;
                first = false;
            }
            if(!keep){
                px = ax; py = ay; pz = az;
                if(!(finite_f(px) && finite_f(py) && finite_f(pz))) px = py = pz = __uint_as_float(0x7FC00000u);
            }
        }
        verts[v * 3u] = px; verts[v * 3u + 1u] = py; verts[v * 3u + 2u] = pz;
    }
}

// ---- morph targets (include/hpt.h, "morph targets") -----------------------------------------------------------------------

// one entry of a corner's run: acc = acc + w * d if the entry's target is active; says whether it was
__device__ __forceinline__ bool morph_step(const uint4 &m, const float *table, uint32_t num_targets, float &px, float &py, float &pz){
    if(m.x >= num_targets) return false;                    // (refused on the host: never out of the table)
    const float w = table[m.x];
    if((__float_as_uint(w) << 1) == 0u) return false;       // inactive: never evaluated
    const float mx = w * __uint_as_float(m.y), my = w * __uint_as_float(m.z), mz = w * __uint_as_float(m.w);
    px = px + mx; py = py + my; pz = pz + mz;
    return true;
}

// One lane per corner, the skin kernel's shape.  A corner reads the two ends of its run in corner_begin and 12 bytes of the
// rest pose, then its 16-byte entries {target, dx, dy, dz}, four loads at a time; the entries are sorted by corner, then target, so the walk
// is the definition's sum in the definition's order (morph_vertex_host, scene_build.cpp) and neighbouring lanes start on
// neighbouring entries.  The weights, 4 bytes per target, are staged in LDS once per workgroup.  A weight of +0 or -0 skips
// the entry without a look at its delta; a corner on which nothing was active stores the bits it loaded.  The file is
// compiled without contraction, so w * d is rounded before it is added.
__global__ __launch_bounds__(kRefitBlock) void k_morph_verts(const float *__restrict__ rest, const uint32_t *__restrict__ corner_begin,
                                                              const uint4 *__restrict__ entries, const float *__restrict__ weights,
                                                              uint32_t num_targets, uint64_t num_verts, float *__restrict__ verts){
    __shared__ float table[kMorphMaxTargets];
    for(uint32_t i = threadIdx.x; i < num_targets && i < (uint32_t) kMorphMaxTargets; i += (uint32_t) kRefitBlock) table[i] = weights[i];
    __syncthreads();
    const uint64_t stride = (uint64_t) gridDim.x * (uint64_t) kRefitBlock;
    for(uint64_t v = (uint64_t) blockIdx.x * (uint64_t) kRefitBlock + threadIdx.x; v < num_verts; v += stride){
        const uint32_t e0 = corner_begin[v], e1 = corner_begin[v + 1u];
        float px = rest[v * 3u], py = rest[v * 3u + 1u], pz = rest[v * 3u + 2u];
        bool any = false;
        uint32_t e = e0;
        for(; e + 4u <= e1; e += 4u){                       // four loads in flight, then the four steps in order
            const uint4 m0 = entries[e], m1 = entries[e + 1u], m2 = entries[e + 2u], m3 = entries[e + 3u];
            any |= morph_step(m0, table, num_targets, px, py, pz);
            any |= morph_step(m1, table, num_targets, px, py, pz);
            any |= morph_step(m2, table, num_targets, px, py, pz);
            any |= morph_step(m3, table, num_targets, px, py, pz);
        }
        for(; e < e1; ++e) any |= morph_step(entries[e], table, num_targets, px, py, pz);
        if(any && !(finite_f(px) && finite_f(py) && finite_f(pz))) px = py = pz = __uint_as_float(0x7FC00000u);
        verts[v * 3u] = px; verts[v * 3u + 1u] = py; verts[v * 3u + 2u] = pz;
    }
}

} // namespace

void launch_morph_verts(hipStream_t s, const float *rest, const uint32_t *corner_begin, const uint4 *entries, const float *weights,
                        uint32_t num_targets, uint32_t num_tris, float *verts){
    if(num_tris == 0) return;
    const uint64_t num_verts = (uint64_t) num_tris * 3u;
    const uint64_t blocks = (num_verts + (uint64_t) kRefitBlock - 1u) / (uint64_t) kRefitBlock;
    const dim3 grid((uint32_t) std::min<uint64_t>(blocks, (uint64_t) kPoseMaxBlocks));
    hipLaunchKernelGGL(k_morph_verts, grid, dim3(kRefitBlock), 0, s, rest, corner_begin, entries, weights, num_targets, num_verts, verts);
}

void launch_skin_verts(hipStream_t s, const float *rest, const uint2 *corner_bone, const float4 *corner_weight, const float *xforms,
                       uint32_t num_bones, uint32_t num_tris, float *verts){
    if(num_tris == 0) return;
    const uint64_t num_verts = (uint64_t) num_tris * 3u;
    const uint64_t blocks = (num_verts + (uint64_t) kRefitBlock - 1u) / (uint64_t) kRefitBlock;
    const dim3 grid((uint32_t) std::min<uint64_t>(blocks, (uint64_t) kPoseMaxBlocks));
    if(num_bones <= (uint32_t) kPoseLdsParts)
        hipLaunchKernelGGL(k_skin_verts<true>, grid, dim3(kRefitBlock), 0, s, rest, corner_bone, corner_weight, (const float4 *) xforms, num_bones, num_verts, verts);
    else
        hipLaunchKernelGGL(k_skin_verts<false>, grid, dim3(kRefitBlock), 0, s, rest, corner_bone, corner_weight, (const float4 *) xforms, num_bones, num_verts, verts);
}

void launch_pose_verts(hipStream_t s, const float *rest, const int32_t *tri_part, const float *xforms, uint32_t num_parts, uint32_t num_tris,
                       float *verts){
    if(num_tris == 0) return;
    const uint64_t num_verts = (uint64_t) num_tris * 3u;
    const uint64_t blocks = (num_verts + (uint64_t) kRefitBlock - 1u) / (uint64_t) kRefitBlock;
    const dim3 grid((uint32_t) std::min<uint64_t>(blocks, (uint64_t) kPoseMaxBlocks));
    if(num_parts <= (uint32_t) kPoseLdsParts)
        hipLaunchKernelGGL(k_pose_verts<true>, grid, dim3(kRefitBlock), 0, s, rest, tri_part, (const float4 *) xforms, num_parts, num_verts, verts);
    else
        hipLaunchKernelGGL(k_pose_verts<false>, grid, dim3(kRefitBlock), 0, s, rest, tri_part, (const float4 *) xforms, num_parts, num_verts, verts);
}

void launch_refit_tris(hipStream_t s, const float *verts, float4 *tris, uint32_t num_tris, uint32_t num_rounds, float *slot_box,
                       float *partial, uint32_t *dead_count){
    if(num_tris == 0) return;
    hipLaunchKernelGGL(k_refit_tris, dim3(refit_blocks(num_tris)), dim3(kRefitBlock), 0, s, verts, tris, num_tris, num_rounds, slot_box, partial, dead_count);
}

void launch_refit_reduce(hipStream_t s, const float *partial, uint32_t blocks, float *out6){
    hipLaunchKernelGGL(k_refit_reduce, dim3(1), dim3(kRefitBlock), 0, s, partial, blocks, out6);
}

void launch_refit_level(hipStream_t s, float4 *nodes, uint32_t num_nodes, uint32_t first, uint32_t count, const float *slot_box,
                        uint32_t num_tris, float *exact, float pad_abs, float dead_x, float dead_y, float dead_z){
    if(count == 0) return;
    hipLaunchKernelGGL(k_refit_level, dim3(refit_blocks(count)), dim3(kRefitBlock), 0, s, nodes, num_nodes, first, count, slot_box, num_tris, exact,
                       pad_abs, dead_x, dead_y, dead_z);
}

void launch_refit_quantise(hipStream_t s, const float4 *nodes, uint4 *qnodes, uint32_t num_nodes, RefitGrid grid){
    if(num_nodes == 0) return;
    hipLaunchKernelGGL(k_refit_quantise, dim3(refit_blocks(num_nodes)), dim3(kRefitBlock), 0, s, nodes, qnodes, num_nodes, grid);
}

void launch_refit_wide(hipStream_t s, const float4 *nodes, uint32_t num_nodes, uint4 *wnodes, const uint4 *wide_src, uint32_t num_wide,
                       RefitGrid grid){
    if(num_wide == 0) return;
    hipLaunchKernelGGL(k_refit_wide, dim3(refit_blocks(num_wide)), dim3(kRefitBlock), 0, s, nodes, num_nodes, wnodes, wide_src, num_wide, grid);
}

} // namespace hpt
