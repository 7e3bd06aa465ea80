// HIP kernels of the guide buffers and the denoiser (include/hpt.h, "guides and denoiser"), written for gfx950 (MI355X).
//
//   guides    hpt_render_guides runs photon mapping's eye pass (ppm_kernels.hip, unchanged) once per sample; after each,
//             k_guides_accumulate adds the hit points' base colour, normal and position into per-pixel sums
//             (k_guides_accumulate_motion also where each hit point was in the scene's previous geometry), and
//             k_guides_resolve forms the means for launch_untile.
//   denoiser  k_denoise_pack turns the guide images into 16-byte records, k_denoise_pack_color forms c_0, and k_atrous
//             runs one level of the edge-avoiding a-trous filter per launch.
//
// Everything is IEEE float arithmetic evaluated as written (-ffp-contract=off, correctly rounded divide), with no
// transcendental and no atomic: the CPU restatements (tests/guides_oracle.cpp, tests/motion_oracle.cpp, tests/denoise_oracle.cpp) give the same bits.
#include "denoise_kernels.h"
#include "pt_device_math.h"

namespace hpt {

namespace {

// ---- guides --------------------------------------------------------------------------------------------------------
// A pixel has at most one hit point per pass, so the lane that holds list entry i is the only one that touches the
// sums of that pixel slot: read, add, write.  Passes follow each other on one stream, hence sample order.
__global__ __launch_bounds__(kBlock)
void k_guides_accumulate(SceneDev sc, PpmHitBuf hb, const uint32_t *hp_count, GuideAccum ga){
    const uint32_t count = *hp_count;
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if(i >= count) return;
    const uint32_t slot = hb.list[i];
    const float4 pm = hb.pos_mat[slot], n = hb.nrm[slot];
    const DevMaterial &dm = sc.mats[__float_as_uint(pm.w)];
    float4 a = ga.alb_cnt[slot], sn = ga.nrm[slot], sp = ga.pos[slot];
    a.x = a.x + dm.base[0]; a.y = a.y + dm.base[1]; a.z = a.z + dm.base[2];
    a.w = __uint_as_float(__float_as_uint(a.w) + 1u);
    sn.x = sn.x + n.x; sn.y = sn.y + n.y; sn.z = sn.z + n.z;
    sp.x = sp.x + pm.x; sp.y = sp.y + pm.y; sp.z = sp.z + pm.z;
    ga.alb_cnt[slot] = a; ga.nrm[slot] = sn; ga.pos[slot] = sp;
}

// dot as the history defines it (include/hpt.h): left to right
HPT_DEV float dot_lr(f3 a, f3 b){ return a.x * b.x + a.y * b.y + a.z * b.z; }

// Where the hit point X on primitive code `prim` (PathBuf::hit.y) was in the previous geometry (include/hpt.h, "motion").
// A primitive whose current and previous bytes are equal returns X itself; nothing else is special-cased, so a zero
// denominator or dead previous vertices give a non-finite point.
HPT_DEV f3 previous_point(const SceneDev &sc, const GuideMotion &gm, uint32_t prim, f3 X){
    if(prim & kHitRoundFlag){
        const uint32_t j = prim & 0x7FFFFFFFu;                   // a hit point is never on a light ball: j < num_spheres
        const DevRound rr = sc.rounds[j];
        const float4 q = gm.prev_rounds[j];
        if(__float_as_uint(rr.c[0]) == __float_as_uint(q.x) && __float_as_uint(rr.c[1]) == __float_as_uint(q.y) && __float_as_uint(rr.c[2]) == __float_as_uint(q.z) && __float_as_uint(rr.r) == __float_as_uint(q.w)) return X;
        const float k = q.w / rr.r;
        return mk3(q.x + (X.x - rr.c[0]) * k, q.y + (X.y - rr.c[1]) * k, q.z + (X.z - rr.c[2]) * k);
    }
    const uint32_t i = __float_as_uint(sc.tris[(size_t) prim * 3].w) - (uint32_t) sc.num_rounds;       // scan ordinal -> input index
    const float *a = gm.verts + (size_t) i * 9, *b = gm.prev_verts + (size_t) i * 9;
    float av[9], bv[9];
    bool same = true;
#pragma unroll
    for(int k = 0; k < 9; ++k){ av[k] = a[k]; bv[k] = b[k]; same = same && __float_as_uint(av[k]) == __float_as_uint(bv[k]); }
    if(same) return X;
    const f3 a0 = mk3(av[0], av[1], av[2]), b0 = mk3(bv[0], bv[1], bv[2]);
    const f3 e1 = mk3(av[3] - a0.x, av[4] - a0.y, av[5] - a0.z), e2 = mk3(av[6] - a0.x, av[7] - a0.y, av[8] - a0.z);
    const f3 d = mk3(X.x - a0.x, X.y - a0.y, X.z - a0.z);
    const float d00 = dot_lr(e1, e1), d01 = dot_lr(e1, e2), d11 = dot_lr(e2, e2), d20 = dot_lr(d, e1), d21 = dot_lr(d, e2);
    const float den = d00 * d11 - d01 * d01;
    const float beta = (d11 * d20 - d01 * d21) / den, gamma = (d00 * d21 - d01 * d20) / den;
    const f3 f1 = mk3(bv[3] - b0.x, bv[4] - b0.y, bv[5] - b0.z), f2 = mk3(bv[6] - b0.x, bv[7] - b0.y, bv[8] - b0.z);
    return mk3((b0.x + f1.x * beta) + f2.x * gamma, (b0.y + f1.y * beta) + f2.y * gamma, (b0.z + f1.z * beta) + f2.z * gamma);
}

// k_guides_accumulate plus the fifth sum.  The same single-owner argument: entry i's lane alone touches its pixel slot.
__global__ __launch_bounds__(kBlock)
void k_guides_accumulate_motion(SceneDev sc, PpmHitBuf hb, const uint2 *hit, const uint32_t *hp_count, GuideAccum ga, GuideMotion gm){
    const uint32_t count = *hp_count;
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if(i >= count) return;
    const uint32_t slot = hb.list[i];
    const float4 pm = hb.pos_mat[slot], n = hb.nrm[slot];
    const DevMaterial &dm = sc.mats[__float_as_uint(pm.w)];
    float4 a = ga.alb_cnt[slot], sn = ga.nrm[slot], sp = ga.pos[slot], sq = ga.prev[slot];
    a.x = a.x + dm.base[0]; a.y = a.y + dm.base[1]; a.z = a.z + dm.base[2];
    a.w = __uint_as_float(__float_as_uint(a.w) + 1u);
    sn.x = sn.x + n.x; sn.y = sn.y + n.y; sn.z = sn.z + n.z;
    sp.x = sp.x + pm.x; sp.y = sp.y + pm.y; sp.z = sp.z + pm.z;
    const f3 Y = previous_point(sc, gm, hit[slot].y, mk3(pm.x, pm.y, pm.z));
    sq.x = sq.x + Y.x; sq.y = sq.y + Y.y; sq.z = sq.z + Y.z;
    ga.alb_cnt[slot] = a; ga.nrm[slot] = sn; ga.pos[slot] = sp; ga.prev[slot] = sq;
}

__global__ __launch_bounds__(kBlock)
void k_guides_resolve(uint32_t n_local, GuideAccum ga, int which, float *d_local){
    const uint32_t p = blockIdx.x * kBlock + threadIdx.x;
    if(p >= n_local) return;
    const float4 a = ga.alb_cnt[p];
    const float c = (float) __float_as_uint(a.w);
    float x = 0.0f, y = 0.0f, z = 0.0f;
    if(which == 3) x = c;
    else if(c > 0.0f){
        const float4 *src = which == 0 ? ga.alb_cnt : which == 1 ? ga.nrm : which == 4 ? ga.prev : ga.pos;
        const float4 v = src[p];
        x = v.x / c; y = v.y / c; z = v.z / c;
    }
    d_local[(size_t) p * 3 + 0] = x;
    d_local[(size_t) p * 3 + 1] = y;
    d_local[(size_t) p * 3 + 2] = z;
}

// ---- denoiser ------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock)
void k_denoise_pack(const float *albedo, const float *normal, const float *position, const float *coverage, DenoiseGuides g, size_t n){
    const size_t p = (size_t) blockIdx.x * kBlock + threadIdx.x;
    if(p >= n) return;
    g.nrm_cov[p] = make_float4(normal[p * 3], normal[p * 3 + 1], normal[p * 3 + 2], coverage[p]);
    g.pos[p] = make_float4(position[p * 3], position[p * 3 + 1], position[p * 3 + 2], 0.0f);
    g.alb[p] = make_float4(fmaxf(albedo[p * 3], 1e-3f), fmaxf(albedo[p * 3 + 1], 1e-3f), fmaxf(albedo[p * 3 + 2], 1e-3f), 0.0f);
}

// An invalid pixel keeps its colour undivided: no tap reads it, every level passes it on, and the last level writes it
// out as it stands, so it leaves the filter with the bits it came in with.
__global__ __launch_bounds__(kBlock)
void k_denoise_pack_color(const float *rgb, DenoiseGuides g, float4 *c0, size_t n, int demod){
    const size_t p = (size_t) blockIdx.x * kBlock + threadIdx.x;
    if(p >= n) return;
    float x = rgb[p * 3], y = rgb[p * 3 + 1], z = rgb[p * 3 + 2];
    if(demod && g.nrm_cov[p].w > 0.0f){
        const float4 a = g.alb[p];
        x = x / a.x; y = y / a.y; z = z / a.z;
    }
    c0[p] = make_float4(x, y, z, 0.0f);
}

// e(x) = max(0, 1 - x / 8)^8: exp(-x) to within 0.03 on [0, 8], exactly zero from 8 on, three squarings
HPT_DEV float falloff(float x){
    float q = fmaxf(0.0f, 1.0f - x * 0.125f);
    q *= q; q *= q; q *= q;
    return q;
}

// taps of the B3 spline, exact floats
HPT_DEV float tap(int k){ return (k == 0 || k == 4) ? 0.0625f : (k == 2 ? 0.375f : 0.25f); }

constexpr int kTileX = 64, kTileY = 4;       // pixels of a 256-thread workgroup: a wave is one row segment of 64 pixels

// One level at stride L.stride, one lane per pixel.  A wave's 64 lanes hold 64 consecutive pixels of one row, so every
// tap is three loads of 64 consecutive 16-byte records.  The 25 taps are added in the order j (rows) outer, i inner.
template <bool LAST>
__global__ __launch_bounds__(kBlock)
void k_atrous(DenoiseLevel L, DenoiseGuides g, const float4 *c_in, float4 *c_out, float *out){
    const int x = (int) (blockIdx.x * kTileX + (threadIdx.x & 63u));
    const int y = (int) (blockIdx.y * kTileY + (threadIdx.x >> 6));
    if(x >= L.W || y >= L.H) return;
    const size_t p = (size_t) y * (size_t) L.W + (size_t) x;
    const float4 cp = c_in[p], np = g.nrm_cov[p];
    float rx = cp.x, ry = cp.y, rz = cp.z;
    const bool valid = np.w > 0.0f;
    if(valid){
        const float4 pp = g.pos[p];
        float sx = 0.0f, sy = 0.0f, sz = 0.0f, wsum = 0.0f;
        bool others = false;                 // a tap besides the centre's took part
#pragma unroll
        for(int j = -2; j <= 2; ++j){
            const int qy = y + j * L.stride;
#pragma unroll
            for(int i = -2; i <= 2; ++i){
                const int qx = x + i * L.stride;
                if(qx < 0 || qx >= L.W || qy < 0 || qy >= L.H) continue;
                const size_t q = (size_t) qy * (size_t) L.W + (size_t) qx;
                const float4 nq = g.nrm_cov[q];
                if(!(nq.w > 0.0f)) continue;
                const float4 cq = c_in[q], pq = g.pos[q];
                if(i != 0 || j != 0) others = true;
                float ec = 1.0f, en = 1.0f, ep = 1.0f;
                if(L.use_c){
                    const float dx = cp.x - cq.x, dy = cp.y - cq.y, dz = cp.z - cq.z;
                    ec = falloff((dx * dx + dy * dy + dz * dz) * L.inv_c);
                }
                if(L.use_n){
                    const float dx = np.x - nq.x, dy = np.y - nq.y, dz = np.z - nq.z;
                    en = falloff((dx * dx + dy * dy + dz * dz) * L.inv_n);
                }
                if(L.use_p){
                    const float t = np.x * (pq.x - pp.x) + np.y * (pq.y - pp.y) + np.z * (pq.z - pp.z);
                    ep = falloff(t * t * L.inv_p);
                }
                const float w = tap(j + 2) * tap(i + 2) * ec * en * ep;
                sx = sx + cq.x * w; sy = sy + cq.y * w; sz = sz + cq.z * w;
                wsum = wsum + w;
            }
        }
        // alone, the centre tap would give fl(fl(c * 9/64) / (9/64)), which is not c for every float: such a pixel keeps c
        if(others){ rx = sx / wsum; ry = sy / wsum; rz = sz / wsum; }
    }
    if(LAST){
        if(L.demod && valid){
            const float4 a = g.alb[p];
            rx = rx * a.x; ry = ry * a.y; rz = rz * a.z;
        }
        out[p * 3 + 0] = rx; out[p * 3 + 1] = ry; out[p * 3 + 2] = rz;
    } else {
        c_out[p] = make_float4(rx, ry, rz, 0.0f);
    }
}

inline uint32_t blocks_for(size_t n){ return (uint32_t) ((n + kBlock - 1) / kBlock); }

} // namespace

void launch_guides_accumulate(hipStream_t s, const SceneDev &sc, PpmHitBuf hb, const uint32_t *hp_count, uint32_t max_items, GuideAccum ga){
    if(max_items == 0u) return;
    hipLaunchKernelGGL(k_guides_accumulate, dim3(blocks_for(max_items)), dim3(kBlock), 0, s, sc, hb, hp_count, ga);
}

void launch_guides_accumulate_motion(hipStream_t s, const SceneDev &sc, PpmHitBuf hb, const uint2 *hit, const uint32_t *hp_count,
                                     uint32_t max_items, GuideAccum ga, GuideMotion gm){
    if(max_items == 0u) return;
    hipLaunchKernelGGL(k_guides_accumulate_motion, dim3(blocks_for(max_items)), dim3(kBlock), 0, s, sc, hb, hit, hp_count, ga, gm);
}

void launch_guides_resolve(hipStream_t s, uint32_t n_local, GuideAccum ga, int which, float *d_local){
    if(n_local == 0u) return;
    hipLaunchKernelGGL(k_guides_resolve, dim3(blocks_for(n_local)), dim3(kBlock), 0, s, n_local, ga, which, d_local);
}

void launch_denoise_pack(hipStream_t s, const float *albedo, const float *normal, const float *position, const float *coverage,
                         DenoiseGuides g, size_t num_pixels){
    hipLaunchKernelGGL(k_denoise_pack, dim3(blocks_for(num_pixels)), dim3(kBlock), 0, s, albedo, normal, position, coverage, g, num_pixels);
}

void launch_denoise_pack_color(hipStream_t s, const float *linear_rgb, DenoiseGuides g, float4 *c0, size_t num_pixels, int demod){
    hipLaunchKernelGGL(k_denoise_pack_color, dim3(blocks_for(num_pixels)), dim3(kBlock), 0, s, linear_rgb, g, c0, num_pixels, demod);
}

void launch_atrous(hipStream_t s, const DenoiseLevel &L, DenoiseGuides g, const float4 *c_in, float4 *c_out, float *out, int last){
    const dim3 grid((uint32_t) ((L.W + kTileX - 1) / kTileX), (uint32_t) ((L.H + kTileY - 1) / kTileY));
    if(last) hipLaunchKernelGGL(k_atrous<true>, grid, dim3(kBlock), 0, s, L, g, c_in, c_out, out);
    else hipLaunchKernelGGL(k_atrous<false>, grid, dim3(kBlock), 0, s, L, g, c_in, c_out, out);
}

} // namespace hpt
