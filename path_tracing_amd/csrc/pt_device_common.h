// Device helpers shared by the kernel files (pt_*.hip, bdpt_kernels.hip, ppm_kernels.hip): bit casts, the wave64 queue
// push and reductions, the slot -> pixel map with the primary ray built on it, the node step of the plain binary-tree
// walk, and the host-side grid size of the grid-stride kernels.  Included by .hip files only, next to pt_device_math.h.
#pragma once
#include "pt_kernels.h"
#include "pt_device_math.h"

namespace hpt {

HPT_DEV uint32_t f2u(float f){ return __float_as_uint(f); }
HPT_DEV float u2f(uint32_t u){ return __uint_as_float(u); }
HPT_DEV f3 xyz(float4 v){ return mk3(v.x, v.y, v.z); }

// ---- wave64 queue push: ballot, mbcnt prefix, one atomic per wave on the list's counter -- a workgroup-local one in LDS
// in k_shade and the bidirectional kernels (hence the name), the global one in the photon kernels.  Every lane calls it ----
HPT_DEV uint32_t lds_push(bool want, uint32_t *counter){
    unsigned long long mask = __ballot(want);
    if(mask == 0ull) return 0u;
    uint32_t lo = (uint32_t) mask, hi = (uint32_t) (mask >> 32);
    uint32_t prefix = __builtin_amdgcn_mbcnt_hi(hi, __builtin_amdgcn_mbcnt_lo(lo, 0u));
    uint32_t base = 0u;
    int leader = __ffsll((long long) mask) - 1;
    if((int) (threadIdx.x & 63u) == leader) base = atomicAdd(counter, (uint32_t) __popcll(mask));
    base = (uint32_t) __shfl((int) base, leader, 64);
    return base + prefix;
}

// ---- 64-lane reductions ----
HPT_DEV uint32_t wave_max_u32(uint32_t v){
    for(int off = 32; off > 0; off >>= 1){ uint32_t o = (uint32_t) __shfl_xor((int) v, off, 64); v = o > v ? o : v; }
    return v;
}
HPT_DEV unsigned long long wave_sum(unsigned long long v){
    for(int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}

// ---- tiling -----------------------------------------------------------------------------
// local slot p -> global pixel; false when the slot lies outside the image.  This is THE definition of which pixel a
// path slot is; its inverses are k_untile (pt_frame.hip) and path_tracing_amd/tiling.py
HPT_DEV bool tile_to_pixel(const Tiling &tl, uint32_t p, int &x, int &y){
    uint32_t ts2 = (uint32_t) (tl.tile * tl.tile);
    uint32_t lt = p / ts2, q = p % ts2;
    uint32_t gt = lt * (uint32_t) tl.world + (uint32_t) tl.rank;
    if(gt >= (uint32_t) tl.ntiles) return false;
    // tile gt sits in row gt / tiles_x at column (gt % tiles_x + row) % tiles_x: every row is rotated by its
    // index, so the tiles of one rank run down the image diagonally instead of in columns (an object that
    // fills a few tile columns would otherwise load only the ranks owning them)
    uint32_t ty = gt / (uint32_t) tl.tiles_x, tx = (gt % (uint32_t) tl.tiles_x + ty) % (uint32_t) tl.tiles_x;
    uint32_t sub = q >> 6, l = q & 63u;
    uint32_t spr = (uint32_t) tl.tile >> 3;
    uint32_t bx = sub % spr, by = sub / spr;
    x = (int) (tx * (uint32_t) tl.tile + bx * 8u + (l & 7u));
    y = (int) (ty * (uint32_t) tl.tile + by * 8u + (l >> 3));
    return x < tl.W && y < tl.H;
}

// The primary ray of path slot i (reference src/pt_cu.cu:36-46): sample j = i / n_local of local pixel i % n_local,
// jittered with the first two uniforms of the path's stream.  False for a slot outside the image.  k_generate stores
// the result; the PRIMARY variants of k_trace / k_shade recompute it instead, which removes the generate launch and the
// 72 B per path it writes (and iteration 0 reads back) from every pass.
HPT_DEV bool primary_ray(const PrimaryGen &g, uint32_t i, f3 &eye, f3 &dir, uint64_t &rs){
    uint32_t p = i % (uint32_t) g.tl.n_local, j = i / (uint32_t) g.tl.n_local;
    int px, py;
    if(!tile_to_pixel(g.tl, p, px, py)) return false;
    rs = rng_seed(g.seed, (uint32_t) (py * g.tl.W + px), g.first_sample + j);
    float pixel_x = (float) px + rng_next(rs);
    float pixel_y = (float) py + rng_next(rs);
    eye = mk3(g.cam.eye[0], g.cam.eye[1], g.cam.eye[2]);
    f3 pixel_pos = mk3(g.cam.UL[0], g.cam.UL[1], g.cam.UL[2]) + mk3(g.cam.dx[0], g.cam.dx[1], g.cam.dx[2]) * pixel_x
                   + mk3(g.cam.dy[0], g.cam.dy[1], g.cam.dy[2]) * pixel_y;
    dir = normalize3(pixel_pos - eye);
    return true;
}

// ---- traversal: one inner node of the plain binary tree (BvhNode as 4 x float4: the left child's box in n0 / n1, the
// right one's in n2 / n3, the child codes in n0.w / n1.w) against a ray given as ix..oz (t = plane * i - o) and the
// distance `limit` beyond which nothing counts.  hl / hr: the child is there and its box is hit, with 2e-6 of slack (box
// tests only have to be conservative); ln / rn: where the ray enters it.  For walk_bvh (pt_scan.hip) and bd_walk ----
HPT_DEV void bvh2_node_step(float4 n0, float4 n1, float4 n2, float4 n3, float ix, float iy, float iz, float ox, float oy, float oz,
                            float limit, bool &hl, bool &hr, float &ln, float &rn, uint32_t &lc, uint32_t &rc){
    float a0 = fmaf(n0.x, ix, -ox), a1 = fmaf(n1.x, ix, -ox);
    float b0 = fmaf(n0.y, iy, -oy), b1 = fmaf(n1.y, iy, -oy);
    float c0 = fmaf(n0.z, iz, -oz), c1 = fmaf(n1.z, iz, -oz);
    float tln = fmaxf(fmaxf(fminf(a0, a1), fminf(b0, b1)), fmaxf(fminf(c0, c1), 0.0f));
    float lf = fminf(fminf(fmaxf(a0, a1), fmaxf(b0, b1)), fminf(fmaxf(c0, c1), limit));
    a0 = fmaf(n2.x, ix, -ox); a1 = fmaf(n3.x, ix, -ox);
    b0 = fmaf(n2.y, iy, -oy); b1 = fmaf(n3.y, iy, -oy);
    c0 = fmaf(n2.z, iz, -oz); c1 = fmaf(n3.z, iz, -oz);
    float trn = fmaxf(fmaxf(fminf(a0, a1), fminf(b0, b1)), fmaxf(fminf(c0, c1), 0.0f));
    float rf = fminf(fminf(fmaxf(a0, a1), fmaxf(b0, b1)), fminf(fmaxf(c0, c1), limit));
    uint32_t tlc = f2u(n0.w), trc = f2u(n1.w);
    bool thl = (tln <= lf * 1.000002f) && (tlc != kEmptyChild);
    bool thr = (trn <= rf * 1.000002f) && (trc != kEmptyChild);
    // (handed out at the end: computed straight into the references, two s_and_b64 of every caller get their operands swapped)
    hl = thl; hr = thr; ln = tln; rn = trn; lc = tlc; rc = trc;
}

// ---- host: workgroups of a grid-stride kernel over `items`; the bidirectional launches cap at 4096 ----
inline uint32_t grid_for(uint32_t items, uint32_t cap = 2048u){
    uint32_t g = (items + kBlock - 1) / kBlock;
    if(g < 1u) g = 1u;
    return g > cap ? cap : g;           // persistent grid-stride loops above `cap` workgroups
}

} // namespace hpt
