// The one-ray-per-lane traversal of the path-tracing pipeline (pt_kernels.h) for gfx950: the plain binary-tree walk and the reference-order
// triangle scan, behind k_extend / k_connect (which HPT_FLAG_BRUTE_FORCE renders launch instead of k_trace) and the ray probes of the tests.
#include "pt_device_common.h"

namespace hpt {

namespace {

// ---- traversal --------------------------------------------------------------------------
struct Tally { uint32_t boxes, tris, steps, wave_steps; };   // steps: traversal loop trips of this lane;
                                                              // wave_steps: per ray, the wave's longest lane

// Walks the triangle BVH.  ANY: returns true at the first opaque blocker in (1e-3, tmax).
// Closest: refines (best_t, best_slot, best_ord); exact ties go to the lower scan ordinal,
// which is what the reference's in-order scan with a strict '<' keeps.
template <bool ANY, bool COUNT>
HPT_DEV bool walk_bvh(const SceneDev &sc, f3 ro, f3 rd, float tmax, uint32_t *stk,
                      float &best_t, uint32_t &best_slot, uint32_t &best_ord, Tally &tally){
    float dx = fabsf(rd.x) > 1e-20f ? rd.x : copysignf(1e-20f, rd.x);
    float dy = fabsf(rd.y) > 1e-20f ? rd.y : copysignf(1e-20f, rd.y);
    float dz = fabsf(rd.z) > 1e-20f ? rd.z : copysignf(1e-20f, rd.z);
    float ix = 1.0f / dx, iy = 1.0f / dy, iz = 1.0f / dz;
    float ox = ro.x * ix, oy = ro.y * iy, oz = ro.z * iz;
    float limit = ANY ? tmax : best_t;
    uint32_t cur = 0u;
    int sp = 0;
    for(;;){
        bool descend = false;
        if(COUNT) tally.steps += 1;
        if(!(cur & kLeafFlag)){
            const float4 *n = sc.nodes + (size_t) cur * 4;
            float4 n0 = n[0], n1 = n[1], n2 = n[2], n3 = n[3];
            if(COUNT) tally.boxes += 2;
            bool hl, hr; float ln, rn; uint32_t lc, rc;
            bvh2_node_step(n0, n1, n2, n3, ix, iy, iz, ox, oy, oz, limit, hl, hr, ln, rn, lc, rc);
            if(hl && hr){
                bool left_first = ln <= rn;
                stk[sp * kBlock] = left_first ? rc : lc;
                ++sp;
                cur = left_first ? lc : rc;
                descend = true;
            } else if(hl){ cur = lc; descend = true; }
            else if(hr){ cur = rc; descend = true; }
        } else {
            uint32_t first = (cur & 0x7FFFFFFFu) >> 3;
            uint32_t cnt = (cur & 7u) + 1u;
            for(uint32_t k = 0; k < cnt; ++k){
                const float4 *tp = sc.tris + (size_t) (first + k) * 3;
                float4 t0 = tp[0], t1 = tp[1], t2 = tp[2];
                if(COUNT) tally.tris += 1;
                float t;
                if(hit_triangle(ro, rd, xyz(t0), xyz(t1), xyz(t2), ANY ? tmax : 1e20f, t)){
                    if(ANY){
                        if(t > 1e-3f && (f2u(t2.w) & 1u)) return true;
                    } else {
                        uint32_t ord = f2u(t0.w);
                        if(t < best_t || (t == best_t && ord < best_ord)){
                            best_t = t; best_slot = first + k; best_ord = ord; limit = t;
                        }
                    }
                }
            }
        }
        if(!descend){
            if(sp == 0) break;
            --sp;
            cur = stk[sp * kBlock];
        }
    }
    return false;
}

// Reference-order scan over every triangle (tests: BVH == scan).
template <bool ANY, bool COUNT>
HPT_DEV bool scan_tris(const SceneDev &sc, f3 ro, f3 rd, float tmax,
                       float &best_t, uint32_t &best_slot, uint32_t &best_ord, Tally &tally){
    for(int s = 0; s < sc.num_tris; ++s){
        const float4 *tp = sc.tris + (size_t) s * 3;
        float4 t0 = tp[0], t1 = tp[1], t2 = tp[2];
        if(COUNT) tally.tris += 1;
        float t;
        if(hit_triangle(ro, rd, xyz(t0), xyz(t1), xyz(t2), ANY ? tmax : 1e20f, t)){
            if(ANY){
                if(t > 1e-3f && (f2u(t2.w) & 1u)) return true;
            } else {
                uint32_t ord = f2u(t0.w);
                if(t < best_t || (t == best_t && ord < best_ord)){ best_t = t; best_slot = (uint32_t) s; best_ord = ord; }
            }
        }
    }
    return false;
}

// closest hit over spheres, light balls (scan order) and triangles; returns t and primitive code
template <bool BRUTE, bool COUNT>
HPT_DEV void closest_hit(const SceneDev &sc, f3 ro, f3 rd, uint32_t *stk, float &t_out, uint32_t &prim_out, Tally &tally){
    float best_t = 1e20f;
    uint32_t best_prim = kHitMiss, best_ord = 0xFFFFFFFFu;
    for(int i = 0; i < sc.num_rounds; ++i){
        DevRound r = sc.rounds[i];
        float t;
        if(hit_sphere(ro, rd, mk3(r.c[0], r.c[1], r.c[2]), r.r, 1e20f, t) && t < best_t){
            best_t = t; best_prim = kHitRoundFlag | (uint32_t) i; best_ord = (uint32_t) i;
        }
    }
    uint32_t slot = 0xFFFFFFFFu;
    float bt = best_t;
    if(BRUTE) scan_tris<false, COUNT>(sc, ro, rd, 1e20f, bt, slot, best_ord, tally);
    else walk_bvh<false, COUNT>(sc, ro, rd, 1e20f, stk, bt, slot, best_ord, tally);
    if(slot != 0xFFFFFFFFu){ best_t = bt; best_prim = slot; }
    t_out = best_t; prim_out = best_prim;
}

// shadow segment origin p1, unit direction, range (1e-3, max_d): true when unoccluded
template <bool BRUTE, bool COUNT>
HPT_DEV bool segment_visible(const SceneDev &sc, f3 p1, f3 dir, float max_d, uint32_t *stk, Tally &tally){
    for(int i = 0; i < sc.num_spheres; ++i){
        DevRound r = sc.rounds[i];
        float t;
        if(hit_sphere(p1, dir, mk3(r.c[0], r.c[1], r.c[2]), r.r, max_d, t) && t > 1e-3f && (r.flags & 1u)) return false;
    }
    float bt = max_d; uint32_t slot = 0, ord = 0;
    bool blocked = BRUTE ? scan_tris<true, COUNT>(sc, p1, dir, max_d, bt, slot, ord, tally)
                         : walk_bvh<true, COUNT>(sc, p1, dir, max_d, stk, bt, slot, ord, tally);
    return !blocked;
}

HPT_DEV void flush_tally(const Tally &tally, uint32_t rays, WorkCounters *wc, bool shadow){
    // wave reduction, then one atomic per wave and counter
    unsigned long long b = tally.boxes, t = tally.tris, r = rays, st = tally.steps;
    for(int off = 32; off > 0; off >>= 1){
        b += __shfl_down(b, off, 64); t += __shfl_down(t, off, 64); r += __shfl_down(r, off, 64);
        st += __shfl_down(st, off, 64);
    }
    if((threadIdx.x & 63u) == 0u){
        if(st) atomicAdd(shadow ? &wc->lane_steps_shadow : &wc->lane_steps_closest, st);
        if(tally.wave_steps) atomicAdd(shadow ? &wc->wave_steps_shadow : &wc->wave_steps_closest, 64ull * tally.wave_steps);
        if(b) atomicAdd(shadow ? &wc->boxes_shadow : &wc->boxes_closest, b);
        if(t) atomicAdd(shadow ? &wc->tris_shadow : &wc->tris_closest, t);
        if(r) atomicAdd(shadow ? &wc->shadow_rays : &wc->closest_rays, r);
    }
}

template <bool BRUTE, bool COUNT>
__global__ __launch_bounds__(kBlock)
void k_extend(SceneDev sc, PathBuf pb, const uint32_t *queue, const uint32_t *qcount, WorkCounters *wc){
    __shared__ uint32_t s_stack[kStackDepth * kBlock];
    uint32_t count = *qcount;
    uint32_t *stk = s_stack + threadIdx.x;
    Tally tally; tally.boxes = 0; tally.tris = 0; tally.steps = 0; tally.wave_steps = 0;
    uint32_t rays = 0;
    for(uint32_t i = blockIdx.x * kBlock + threadIdx.x; i < count; i += gridDim.x * kBlock){
        uint32_t path = queue ? queue[i] : i;              // null queue: identity (first iteration)
        float4 o = pb.org_eta[path], d = pb.dir_flags[path];
        if(f2u(d.w) & 2u) continue;                        // slot outside the image
        float t; uint32_t prim;
        uint32_t s0 = tally.steps;
        closest_hit<BRUTE, COUNT>(sc, xyz(o), xyz(d), stk, t, prim, tally);
        pb.hit[path] = make_uint2(f2u(t), prim);
        ++rays;
        if(COUNT) tally.wave_steps += wave_max_u32(tally.steps - s0);     // lanes that skipped the trip are not here
    }
    if(COUNT) flush_tally(tally, rays, wc, false);
}

template <bool BRUTE, bool COUNT>
__global__ __launch_bounds__(kBlock)
void k_connect(SceneDev sc, PathBuf pb, ShadowBuf sb, const uint32_t *squeue, const uint32_t *scount, WorkCounters *wc){
    __shared__ uint32_t s_stack[kStackDepth * kBlock];
    uint32_t count = *scount;
    uint32_t *stk = s_stack + threadIdx.x;
    Tally tally; tally.boxes = 0; tally.tris = 0; tally.steps = 0; tally.wave_steps = 0;
    uint32_t rays = 0;
    for(uint32_t i = blockIdx.x * kBlock + threadIdx.x; i < count; i += gridDim.x * kBlock){
        uint32_t r = squeue[i];                                // shadow record index (k_shade)
        float4 a = sb.org_max[r], b = sb.dir[r];
        uint32_t s0 = tally.steps;
        bool vis = segment_visible<BRUTE, COUNT>(sc, xyz(a), xyz(b), a.w, stk, tally);
        ++rays;
        if(COUNT) tally.wave_steps += wave_max_u32(tally.steps - s0);
        if(vis){
            float4 c = sb.contrib[r];
            uint32_t path = f2u(c.w);
            float4 col = pb.col[path];
            col.x = col.x + c.x; col.y = col.y + c.y; col.z = col.z + c.z;
            pb.col[path] = col;
        }
    }
    if(COUNT) flush_tally(tally, rays, wc, true);
}

template <bool BRUTE>
__global__ __launch_bounds__(kBlock)
void k_probe_closest(SceneDev sc, const float *org, const float *dir, int n, float *t_out, int32_t *prim_out){
    __shared__ uint32_t s_stack[kStackDepth * kBlock];
    int i = blockIdx.x * kBlock + threadIdx.x;
    if(i >= n) return;
    Tally tally; tally.boxes = 0; tally.tris = 0; tally.steps = 0; tally.wave_steps = 0;
    float t; uint32_t prim;
    closest_hit<BRUTE, false>(sc, mk3(org[3 * i], org[3 * i + 1], org[3 * i + 2]), mk3(dir[3 * i], dir[3 * i + 1], dir[3 * i + 2]),
                              s_stack + threadIdx.x, t, prim, tally);
    int32_t ord = -1;
    if(prim != kHitMiss){
        if(prim & kHitRoundFlag) ord = (int32_t) (prim & 0x7FFFFFFFu);
        else ord = (int32_t) f2u(sc.tris[(size_t) prim * 3].w);
    }
    t_out[i] = t; prim_out[i] = ord;
}

template <bool BRUTE>
__global__ __launch_bounds__(kBlock)
void k_probe_visibility(SceneDev sc, const float *p1, const float *p2, int n, int32_t *vis_out){
    __shared__ uint32_t s_stack[kStackDepth * kBlock];
    int i = blockIdx.x * kBlock + threadIdx.x;
    if(i >= n) return;
    Tally tally; tally.boxes = 0; tally.tris = 0; tally.steps = 0; tally.wave_steps = 0;
    f3 a = mk3(p1[3 * i], p1[3 * i + 1], p1[3 * i + 2]), b = mk3(p2[3 * i], p2[3 * i + 1], p2[3 * i + 2]);
    f3 diff = b - a;
    float dist = length3(diff);
    f3 d = diff / dist;
    vis_out[i] = segment_visible<BRUTE, false>(sc, a, d, dist - 1e-3f, s_stack + threadIdx.x, tally) ? 1 : 0;
}

} // namespace

// ---- launchers --------------------------------------------------------------------------

void launch_extend(hipStream_t s, const SceneDev &sc, PathBuf pb, const uint32_t *queue, const uint32_t *qcount,
                   uint32_t max_items, int flags, WorkCounters *wc){
    dim3 g(grid_for(max_items)), b(kBlock);
    bool brute = flags & 1, count = flags & 2;
    if(brute && count) hipLaunchKernelGGL((k_extend<true, true>), g, b, 0, s, sc, pb, queue, qcount, wc);
    else if(brute) hipLaunchKernelGGL((k_extend<true, false>), g, b, 0, s, sc, pb, queue, qcount, wc);
    else if(count) hipLaunchKernelGGL((k_extend<false, true>), g, b, 0, s, sc, pb, queue, qcount, wc);
    else hipLaunchKernelGGL((k_extend<false, false>), g, b, 0, s, sc, pb, queue, qcount, wc);
}

void launch_connect(hipStream_t s, const SceneDev &sc, PathBuf pb, ShadowBuf sb, const uint32_t *squeue,
                    const uint32_t *scount, uint32_t max_items, int flags, WorkCounters *wc){
    dim3 g(grid_for(max_items)), b(kBlock);
    bool brute = flags & 1, count = flags & 2;
    if(brute && count) hipLaunchKernelGGL((k_connect<true, true>), g, b, 0, s, sc, pb, sb, squeue, scount, wc);
    else if(brute) hipLaunchKernelGGL((k_connect<true, false>), g, b, 0, s, sc, pb, sb, squeue, scount, wc);
    else if(count) hipLaunchKernelGGL((k_connect<false, true>), g, b, 0, s, sc, pb, sb, squeue, scount, wc);
    else hipLaunchKernelGGL((k_connect<false, false>), g, b, 0, s, sc, pb, sb, squeue, scount, wc);
}

void launch_probe_closest(hipStream_t s, const SceneDev &sc, const float *org, const float *dir, int n, int flags,
                          float *t_out, int32_t *prim_out){
    dim3 g((n + kBlock - 1) / kBlock), b(kBlock);
    if(flags & 1) hipLaunchKernelGGL((k_probe_closest<true>), g, b, 0, s, sc, org, dir, n, t_out, prim_out);
    else hipLaunchKernelGGL((k_probe_closest<false>), g, b, 0, s, sc, org, dir, n, t_out, prim_out);
}

void launch_probe_visibility(hipStream_t s, const SceneDev &sc, const float *p1, const float *p2, int n, int flags,
                             int32_t *vis_out){
    dim3 g((n + kBlock - 1) / kBlock), b(kBlock);
    if(flags & 1) hipLaunchKernelGGL((k_probe_visibility<true>), g, b, 0, s, sc, p1, p2, n, vis_out);
    else hipLaunchKernelGGL((k_probe_visibility<false>), g, b, 0, s, sc, p1, p2, n, vis_out);
}

} // namespace hpt
