// The trace stage of the path-tracing pipeline (pt_kernels.h) for gfx950: k_trace, the merged closest-hit / any-hit kernel, and its
// two launchers -- the first launch over the quantised binary tree, the resume launch for the rays set aside over the four-wide tree.
#include "pt_device_common.h"

namespace hpt {

namespace {

// (m & a) | (~m & b) in one instruction, and the two 16-bit halves of a word as floats (SDWA conversions): the compiler
// expands the first into three and masks before converting the low half
HPT_DEV uint32_t bit_select(uint32_t m, uint32_t a, uint32_t b){ uint32_t r; asm("v_bfi_b32 %0, %1, %2, %3" : "=v"(r) : "v"(m), "v"(a), "v"(b)); return r; }
HPT_DEV float lo16f(uint32_t w){ float r; asm("v_cvt_f32_u32_sdwa %0, %1 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:WORD_0" : "=v"(r) : "v"(w)); return r; }
HPT_DEV float hi16f(uint32_t w){ float r; asm("v_cvt_f32_u32_sdwa %0, %1 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:WORD_1" : "=v"(r) : "v"(w)); return r; }

// ---- merged trace kernel: closest-hit and any-hit rays with dynamic lane refill -----------
// One launch serves the extension rays of iteration i+1 and the shadow rays of iteration i
// (they are independent).  A workgroup owns a contiguous chunk of one queue; its lanes pull
// rays from the chunk through an LDS counter, and a lane whose ray is finished pulls the next
// one as soon as enough lanes of its wave are idle.  Inside, the classic while-while shape:
// lanes walk inner nodes until each holds a leaf, then the (much longer) triangle code runs
// once for all of them.
//
// Measured alternatives on config 3 (1024^2, 32 spp, ms per render; this version 42.3):
//   one ray per lane, separate extend/connect launches, 32 KiB static stack ........ 69.5
//   single loop doing a node OR a leaf step per trip (both code paths every trip) ... 45.5
//   per-trip vote between refill / node step / leaf step ............................. 44.4
//   persistent waves pulling 256-ray batches from one global cursor .................. 55.9
//   persistent waves, 64-ray batches, 32 cursors on ONE 128-B line ................... 207.9
//   same with one cursor per 128-B line (82 VGPRs) ................................... 47.5
// Chunk size: 256 -> 47.3, 512 -> 45.5, 1024 -> 49.6, 2048 -> 59.3 (long chunks leave the tail of
// a launch to a few workgroups); refill threshold 8 -> 51.0, 16 -> 49.6, 32 -> 48.6, 48 -> 48.0.
// k_trace's registers are fitted to eight waves per SIMD -- vector AND scalar: left alone the compiler takes 106 SGPRs, and
// more than 96 cap a CU at six 256-thread workgroups whatever the vector registers allow (78 with this attribute, the
// rest spilled to lanes of a VGPR).  Per instantiation <COUNT, RESUME, TOP, PRIMARY> (scripts/isa_report.py): VGPRs / of them
// spilled to scratch / SGPRs spilled to lanes = <0,0,1,0> 59 / 0 / 54, <0,0,1,1> 64 / 6 / 61, <0,1,0,0> 57 / 0 / 22,
// <0,1,0,1> 63 / 0 / 44, <0,0,0,0> 57 / 0 / 60, <0,0,0,1> 64 / 6 / 77, <1,0,0,0> 64 / 11 / 61 (with two exits and a `continue`
// in trace_chunk's loop: 64 / 2 / 54, 64 / 11 / 87, 58 / 0 / 36, 64 / 0 / 66, 64 / 2 / 59, 64 / 11 / 89, 64 / 56 / 65;
// tests/test_trace_isa_cpu.py and tests/test_trace_register_fit_cpu.py hold the VGPR side).  Measured against the unconstrained build: first launch 11.37 -> 11.00 ms, resume
// 8.14 -> 7.70 per 64-spp pass of config 3, 14.00 -> 13.46 on the 1 M-triangle shape.  `make variant EXTRA=-DHPT_TRACE_WAVES=0`
// builds without it, =7 with seven.
#ifndef HPT_TRACE_WAVES
#define HPT_TRACE_WAVES 8
#endif
#if HPT_TRACE_WAVES > 0
#define HPT_TRACE_ATTR __attribute__((amdgpu_waves_per_eu(HPT_TRACE_WAVES, 8)))
#else
#define HPT_TRACE_ATTR
#endif
constexpr int kTraceChunk = 2048;     // rays per workgroup of the first launch.  Round 1, unsplit step: 512 -> 37.6 ms, 768 -> 36.5, 1024 -> 36.5, 1280 -> 36.1,
                                      // 1536 -> 36.7, 2048 -> 38.4.  Round 3, split step with the four-wide resume, two passes in flight (whose
                                      // kernels fill each other's tails): 1024 -> 126.7 ms per 256-spp render of config 3, 1536 -> 125.8, 2048 -> 125.3,
                                      // 3072 -> 126.1, 4096 -> 125.9; with refill at 56 idle lanes 2048 -> 124.5 (1 M triangles, 4096^2 x 8 spp: 74.2 -> 73.1)
constexpr uint32_t kDoneCode = 0xFFFFFFFEu;   // leaf-flagged code a finished walk parks in cur
constexpr int kRefillMin = 56;        // idle lanes that trigger a refill (24 -> 34.4 ms per 64-spp pass, 32 -> 34.1, 40 -> 33.8, 48 -> 33.8, 56 -> 33.7)
constexpr int kNodeMin = 4;           // fewer lanes than this still walking nodes (while others hold leaves): do the leaves first
                                      // (A/B: off 42.1 ms, 2: 39.9, 4: 39.4, 8: 40.2, 16: 41.3, 32: 43.2)
constexpr uint32_t kTraceShortQueue = 1u << 20;   // below this many rays a workgroup takes 256 instead of kTraceChunk

// The first launch (!RESUME) walks the binary tree with the whole stack in LDS.  The resume launch (RESUME) walks the
// four-wide tree; only the first kResumeLdsLevels stack levels of a lane live in LDS, deeper ones in its column of `deep`
// (global memory, one column per lane of the grid, `deep_stride` words apart): the whole stack in LDS would take 22 KB per
// workgroup at depth 21, 27 KB at 26 (five or six workgroups per CU), while on the benchmark-shaped scenes no ray holds more
// than a dozen pending subtrees (9 to 12 measured; nested boxes that all contain the ray's origin reach 44: DESIGN.md, "The walker")
template <bool ANY, bool COUNT, bool RESUME, bool TOP, bool PRIMARY>
HPT_DEV void trace_chunk(const SceneDev &sc, PathBuf pb, ShadowBuf sb, const uint32_t *queue,
                         uint32_t end, uint32_t *stk, uint32_t *s_next, int refill_min, int node_min, WorkCounters *wc,
                         uint32_t budget, DeferredRay *rec, uint32_t *s_long, uint32_t *s_nlong, const uint4 *top,
                         const PrimaryGen &pg, uint32_t *deep, uint32_t deep_stride){
    bool active = false, exhausted = false;
    uint32_t path = 0u, cur = 0u, steps = 0u;
    int sp = 0;
    f3 ro = mk3(0, 0, 0), rd = mk3(0, 0, 1);
    float ix = 0, iy = 0, iz = 0, ox = 0, oy = 0, oz = 0;
    uint32_t mx = 0u, my = 0u, mz = 0u;          // all ones where the ray runs against the axis (its near plane is a box's upper one)
    float tmax = 0.0f, limit = 0.0f, best_t = 1e20f;
    uint32_t best_prim = kHitMiss, best_ord = 0xFFFFFFFFu;
    unsigned long long n_lane_steps = 0, n_wave_steps = 0, n_boxes = 0, n_tris = 0, n_rays = 0, n_leaf_lane = 0, n_leaf_wave = 0;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t step_limit = budget != 0u ? budget : 0xFFFFFFFFu;
    for(;;){
        if(!RESUME && budget != 0u){
            // a ray that has used its node-step budget is set aside for the second launch (it restarts
            // there with what it found so far as its limit), so this lane goes back to the short rays
            bool defer = active && steps >= budget;
            unsigned long long dm = __ballot(defer);
            if(dm != 0ull){
                uint32_t dn = (uint32_t) __popcll(dm);
                uint32_t dprefix = __builtin_amdgcn_mbcnt_hi((uint32_t) (dm >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t) dm, 0u));
                int dleader = __ffsll((long long) dm) - 1;
                uint32_t dbase = 0u;
                if((int) lane == dleader) dbase = atomicAdd(s_nlong, dn);
                dbase = (uint32_t) __shfl((int) dbase, dleader, 64);
                if(defer){
                    if(!ANY && !PRIMARY && !COUNT){
                        // a closest-hit ray leaves as a dense record: s_nlong started at the chunk's first queue position, a chunk
                        // sets aside at most as many rays as it holds and the chunks' ranges are disjoint, so the places of two
                        // chunks never meet (k_shade's argument for the shadow records).  Everything the resume launch needs to
                        // start the ray is in the lane; pb.hit[path] is written by that launch alone
                        DeferredRay *r = rec + (dbase + dprefix);
                        r->org_t = make_float4(ro.x, ro.y, ro.z, best_t);
                        r->dir_slot = make_float4(rd.x, rd.y, rd.z, u2f(path));
                        r->hit = make_uint4(best_prim, best_ord, 0u, 0u);
                    } else {
                        s_long[dbase + dprefix] = path;
                        if(!ANY) pb.hit[path] = make_uint2(f2u(best_t), best_prim);
                    }
                    active = false;
                }
            }
        }
        unsigned long long idle = __ballot(!active);
        if(idle != 0ull && !exhausted && (idle == ~0ull || __popcll(idle) >= refill_min)){
            // ---- refill: idle lanes pull the next rays of this workgroup's chunk ----
            uint32_t n = (uint32_t) __popcll(idle);
            uint32_t prefix = __builtin_amdgcn_mbcnt_hi((uint32_t) (idle >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t) idle, 0u));
            int leader = __ffsll((long long) idle) - 1;
            uint32_t base = 0u;
            if((int) lane == leader) base = atomicAdd(s_next, n);
            base = (uint32_t) __shfl((int) base, leader, 64);
            exhausted = base + n >= end;
            if(!active){
                uint32_t i = base + prefix;
                if(i < end){
                    path = queue ? queue[i] : i;
                    bool start = true;
                    if(ANY){
                        // a shadow-queue entry is a record index, not a path slot (k_shade); `path` keeps it, also through
                        // s_long into the resume launch, and the slot is read with the contribution at the end
                        float4 a = sb.org_max[path], b = sb.dir[path];
                        ro = xyz(a); rd = xyz(b); tmax = a.w;
                        if(COUNT && !RESUME) n_rays += 1;
                        // spheres first (the reference scans them after the triangles; the result is a boolean);
                        // a resumed ray has passed them already
                        for(int r = 0; r < (RESUME ? 0 : sc.num_spheres); ++r){
                            DevRound rr = sc.rounds[r];
                            float t;
                            if(hit_sphere(ro, rd, mk3(rr.c[0], rr.c[1], rr.c[2]), rr.r, tmax, t) && t > 1e-3f && (rr.flags & 1u)) start = false;
                        }
                        limit = tmax;
                    } else {
                        bool outside;
                        if(RESUME && !PRIMARY){
                            // the queue entry is a record index: the ray, the closest hit of the first launch (the limit the walk
                            // restarts with), its ordinal and the path slot, all from the record -- no gather through the slot
                            const DeferredRay *r = rec + path;
                            float4 o = r->org_t, d = r->dir_slot;
                            uint4 h = r->hit;
                            ro = xyz(o); rd = xyz(d);
                            best_t = o.w; best_prim = h.x; best_ord = h.y;
                            path = f2u(d.w);
                            limit = best_t;
                            outside = false;                                    // a ray that was set aside is inside the image
                        } else if(PRIMARY){
                            // iteration 0 without a generate launch: the camera ray of this slot, recomputed (the first
                            // launch reads the identity queue, the resume launch the slots it was handed)
                            uint64_t rs_unused;
                            outside = !primary_ray(pg, path, ro, rd, rs_unused);
                            if(outside && !RESUME) pb.hit[path] = make_uint2(f2u(1e20f), kHitMiss);
                        } else {
                            float4 o = pb.org_eta[path], d = pb.dir_flags[path];
                            ro = xyz(o); rd = xyz(d);
                            outside = (f2u(d.w) & 2u) != 0u;
                        }
                        if(outside) start = false;                          // slot outside the image
                        else if(RESUME){
                            if(PRIMARY){
                                // iteration 0 handed slots over: restart with the closest hit of the first launch as the limit
                                uint2 h = pb.hit[path];
                                best_t = u2f(h.x); best_prim = h.y; best_ord = 0xFFFFFFFFu;
                                if(best_prim != kHitMiss)
                                    best_ord = (best_prim & kHitRoundFlag) ? (best_prim & ~kHitRoundFlag) : f2u(sc.tris[(size_t) best_prim * 3].w);
                                limit = best_t;
                            }
                        } else {
                            if(COUNT) n_rays += 1;
                            best_t = 1e20f; best_prim = kHitMiss; best_ord = 0xFFFFFFFFu;
                            for(int r = 0; r < sc.num_rounds; ++r){
                                DevRound rr = sc.rounds[r];
                                float t;
                                if(hit_sphere(ro, rd, mk3(rr.c[0], rr.c[1], rr.c[2]), rr.r, 1e20f, t) && t < best_t){
                                    best_t = t; best_prim = kHitRoundFlag | (uint32_t) r; best_ord = (uint32_t) r;
                                }
                            }
                            limit = best_t;
                        }
                    }
                    if(start){
                        float dx = fabsf(rd.x) > 1e-20f ? rd.x : copysignf(1e-20f, rd.x);
                        float dy = fabsf(rd.y) > 1e-20f ? rd.y : copysignf(1e-20f, rd.y);
                        float dz = fabsf(rd.z) > 1e-20f ? rd.z : copysignf(1e-20f, rd.z);
                        // box tests only have to be conservative: the 1-ulp hardware reciprocal is inside the
                        // 2e-6 slack of the slab test (the triangle tests below use exact arithmetic)
                        // (the counting render divides exactly: its node and triangle tallies are then a function of the ray
                        // and the tree alone, which the oracle's host walk of the exported tree reproduces to the last count)
                        if(COUNT){ ix = 1.0f / dx; iy = 1.0f / dy; iz = 1.0f / dz; }
                        else { ix = __builtin_amdgcn_rcpf(dx); iy = __builtin_amdgcn_rcpf(dy); iz = __builtin_amdgcn_rcpf(dz); }
                        // quantised boxes: plane = qorigin + q * qscale, so t = q * (qscale * inv) + (qorigin - o) * inv
                        ox = (sc.qorigin[0] - ro.x) * ix; oy = (sc.qorigin[1] - ro.y) * iy; oz = (sc.qorigin[2] - ro.z) * iz;
                        ix *= sc.qscale[0]; iy *= sc.qscale[1]; iz *= sc.qscale[2];
                        mx = ix < 0.0f ? 0xFFFFFFFFu : 0u; my = iy < 0.0f ? 0xFFFFFFFFu : 0u; mz = iz < 0.0f ? 0xFFFFFFFFu : 0u;
                        cur = 0u; sp = 0; steps = 0u;
                        active = true;
                    }
                }
            }
        }
        // ONE exit, after the refill, and no `continue`.  With an exit in each arm and a `continue` for "the refill started
        // nobody" the register coalescer gives up on the loop-carried ray state and copies all of it (20-24 VGPRs) into a
        // second register set at the top of every trip and back before the node walk: 44-48 v_mov per trip, 49 of the refill
        // block's 66 VALU instructions (scripts/isa_report.py, profiles/r05_experiments.md).  This shape does the same thing:
        //  - no refill and every lane idle happens only with the chunk exhausted (else the refill is taken): exit, as before;
        //  - a refill that started nobody with rays left in the chunk falls through phases 1 and 2, which `active` guards
        //    and which therefore do nothing (and count nothing), and comes round to the next refill -- the old `continue`.
        const unsigned long long idle_at_entry = __ballot(!active);
        if(idle_at_entry == ~0ull && exhausted) break;  // chunk exhausted and every ray finished
        // phase 1: walk inner nodes until this lane holds a leaf (or its ray is finished); when only a
        // few lanes are still descending while others wait with a leaf, go and do the leaves first
        while(active && !(cur & kLeafFlag) && (RESUME || steps < step_limit)){
            if(node_min > 0){
                unsigned long long walking = __ballot(true);
                if(__popcll(walking) < node_min && __popcll(walking) < 64 - (int) __popcll(idle_at_entry)) break;
            }
            if(COUNT){
                n_lane_steps += 1; n_boxes += 2;
                if((int) lane == __ffsll((long long) __ballot(true)) - 1) n_wave_steps += 64;   // one wave trip
            }
            if(!RESUME) steps += 1u;
            if(RESUME){
                // four-wide step: four child boxes from one 64-B node; the nearest hit child is entered, the
                // other hit children are stacked in slot order (ordering them too buys 0.3 % fewer steps on the benchmark
                // meshes: scripts/micro/bvh4_steps.cpp).  t = q * i + o is monotone in q, so the near plane of an axis is the
                // lower one when i >= 0 and the upper one otherwise: one bit-select per word picks it for two children.
                const uint4 *n = sc.wnodes + (size_t) cur * 4;
                const uint4 qx = n[0], qy = n[1], qz = n[2], qc = n[3];
                const uint32_t nx01 = bit_select(mx, qx.z, qx.x), nx23 = bit_select(mx, qx.w, qx.y), fx01 = bit_select(mx, qx.x, qx.z), fx23 = bit_select(mx, qx.y, qx.w);
                const uint32_t ny01 = bit_select(my, qy.z, qy.x), ny23 = bit_select(my, qy.w, qy.y), fy01 = bit_select(my, qy.x, qy.z), fy23 = bit_select(my, qy.y, qy.w);
                const uint32_t nz01 = bit_select(mz, qz.z, qz.x), nz23 = bit_select(mz, qz.w, qz.y), fz01 = bit_select(mz, qz.x, qz.z), fz23 = bit_select(mz, qz.y, qz.w);
                const float tn0 = fmaxf(fmaxf(fmaf(lo16f(nx01), ix, ox), fmaf(lo16f(ny01), iy, oy)), fmaxf(fmaf(lo16f(nz01), iz, oz), 0.0f));
                const float tf0 = fminf(fminf(fmaf(lo16f(fx01), ix, ox), fmaf(lo16f(fy01), iy, oy)), fminf(fmaf(lo16f(fz01), iz, oz), limit));
                const float tn1 = fmaxf(fmaxf(fmaf(hi16f(nx01), ix, ox), fmaf(hi16f(ny01), iy, oy)), fmaxf(fmaf(hi16f(nz01), iz, oz), 0.0f));
                const float tf1 = fminf(fminf(fmaf(hi16f(fx01), ix, ox), fmaf(hi16f(fy01), iy, oy)), fminf(fmaf(hi16f(fz01), iz, oz), limit));
                const float tn2 = fmaxf(fmaxf(fmaf(lo16f(nx23), ix, ox), fmaf(lo16f(ny23), iy, oy)), fmaxf(fmaf(lo16f(nz23), iz, oz), 0.0f));
                const float tf2 = fminf(fminf(fmaf(lo16f(fx23), ix, ox), fmaf(lo16f(fy23), iy, oy)), fminf(fmaf(lo16f(fz23), iz, oz), limit));
                const float tn3 = fmaxf(fmaxf(fmaf(hi16f(nx23), ix, ox), fmaf(hi16f(ny23), iy, oy)), fmaxf(fmaf(hi16f(nz23), iz, oz), 0.0f));
                const float tf3 = fminf(fminf(fmaf(hi16f(fx23), ix, ox), fmaf(hi16f(fy23), iy, oy)), fminf(fmaf(hi16f(fz23), iz, oz), limit));
                // key = entry distance with the slot number in its two lowest bits (distances are >= 0: their bit patterns order
                // like the values), all ones for a child that is missed or absent
                const uint32_t k0 = (tn0 <= tf0 * 1.000002f && qc.x != kEmptyChild) ? (f2u(tn0) & ~3u) : 0xFFFFFFFFu;
                const uint32_t k1 = (tn1 <= tf1 * 1.000002f && qc.y != kEmptyChild) ? ((f2u(tn1) & ~3u) | 1u) : 0xFFFFFFFFu;
                const uint32_t k2 = (tn2 <= tf2 * 1.000002f && qc.z != kEmptyChild) ? ((f2u(tn2) & ~3u) | 2u) : 0xFFFFFFFFu;
                const uint32_t k3 = (tn3 <= tf3 * 1.000002f && qc.w != kEmptyChild) ? ((f2u(tn3) & ~3u) | 3u) : 0xFFFFFFFFu;
                const uint32_t kmin = min(min(k0, k1), min(k2, k3));
                const bool any = kmin != 0xFFFFFFFFu;
                const uint32_t slot = kmin & 3u;
                uint32_t near = qc.x;
                near = slot == 1u ? qc.y : near; near = slot == 2u ? qc.z : near; near = slot == 3u ? qc.w : near;
                // stacked: hit and not the nearest, i.e. kmin < key < all ones -- one add and one unsigned compare per child
                const uint32_t c1 = ~kmin, c2 = c1 - 1u;
                const int e0 = (k0 + c1 < c2) ? 1 : 0, e1 = (k1 + c1 < c2) ? 1 : 0, e2 = (k2 + c1 < c2) ? 1 : 0, e3 = (k3 + c1 < c2) ? 1 : 0;
                uint32_t top;
                int p = sp;
                if(sp + 3 < kResumeLdsLevels){
                    // every level this step can touch is in LDS; a child that is not stacked is written to the spare level
                    top = stk[(sp > 0 ? sp - 1 : 0) * kBlock];
                    stk[(e0 ? p : kResumeLdsLevels) * kBlock] = qc.x; p += e0;
                    stk[(e1 ? p : kResumeLdsLevels) * kBlock] = qc.y; p += e1;
                    stk[(e2 ? p : kResumeLdsLevels) * kBlock] = qc.z; p += e2;
                    stk[(e3 ? p : kResumeLdsLevels) * kBlock] = qc.w; p += e3;
                } else {
                    auto level = [&](int l) -> uint32_t * { return l < kResumeLdsLevels ? stk + l * kBlock : deep + (size_t) (l - kResumeLdsLevels) * deep_stride; };
                    top = *level(sp > 0 ? sp - 1 : 0);
                    if(e0){ *level(p) = qc.x; ++p; }
                    if(e1){ *level(p) = qc.y; ++p; }
                    if(e2){ *level(p) = qc.z; ++p; }
                    if(e3){ *level(p) = qc.w; ++p; }
                }
                cur = any ? near : (sp > 0 ? top : kDoneCode);
                sp = any ? p : (sp > 0 ? sp - 1 : 0);
                continue;
            }
            // TOP: a ray with a budget of kTopLevels node steps only ever reaches nodes of depth < kTopLevels, which the
            // breadth-first node order puts among the first kTopNodes: those sit in LDS (staged once per workgroup)
            const uint4 *n = TOP ? top + cur * 2u : sc.qnodes + (size_t) cur * 2;
            uint4 w0 = n[0], w1 = n[1];
            // per axis one word of lower planes (left | right << 16) and one of upper planes, then the two child codes.  t = q * i + o
            // is monotone in q: the near plane of an axis is the lower one when i >= 0 and the upper one otherwise, so one
            // bit-select per word picks the near (far) planes of both children -- the same values min / max of the pair give
            const uint32_t nx = bit_select(mx, w0.y, w0.x), fx = bit_select(mx, w0.x, w0.y);
            const uint32_t ny = bit_select(my, w0.w, w0.z), fy = bit_select(my, w0.z, w0.w);
            const uint32_t nz = bit_select(mz, w1.y, w1.x), fz = bit_select(mz, w1.x, w1.y);
            float ln = fmaxf(fmaxf(fmaf(lo16f(nx), ix, ox), fmaf(lo16f(ny), iy, oy)), fmaxf(fmaf(lo16f(nz), iz, oz), 0.0f));
            float lf = fminf(fminf(fmaf(lo16f(fx), ix, ox), fmaf(lo16f(fy), iy, oy)), fminf(fmaf(lo16f(fz), iz, oz), limit));
            float rn = fmaxf(fmaxf(fmaf(hi16f(nx), ix, ox), fmaf(hi16f(ny), iy, oy)), fmaxf(fmaf(hi16f(nz), iz, oz), 0.0f));
            float rf = fminf(fminf(fmaf(hi16f(fx), ix, ox), fmaf(hi16f(fy), iy, oy)), fminf(fmaf(hi16f(fz), iz, oz), limit));
            uint32_t lc = w1.z, rc = w1.w;
            bool hl = (ln <= lf * 1.000002f) && (lc != kEmptyChild);
            bool hr = (rn <= rf * 1.000002f) && (rc != kEmptyChild);
            // branch-free step (the exec-mask bookkeeping of nested ifs costs more scalar issue than
            // the selects): always store the far child at the stack top, always fetch the entry below
            // it, then pick by selects.  The stack has one spare level for the unconditional store.
            bool any = hl || hr, both = hl && hr;
            bool left_first = hl && (!hr || ln <= rn);
            uint32_t top = stk[(sp > 0 ? sp - 1 : 0) * kBlock];
            stk[sp * kBlock] = left_first ? rc : lc;
            uint32_t near = left_first ? lc : rc;
            cur = any ? near : (sp > 0 ? top : kDoneCode);
            sp = any ? sp + (both ? 1 : 0) : (sp > 0 ? sp - 1 : 0);
        }
        // phase 2: the leaf (lanes that left phase 1 early still hold an inner node and skip it);
        // kDoneCode = the walk found its stack empty
        if(active && (cur & kLeafFlag)){
            bool blocked = false, finished = cur == kDoneCode;
            if(!finished){
                if(COUNT){
                    n_leaf_lane += 1;
                    if((int) lane == __ffsll((long long) __ballot(true)) - 1) n_leaf_wave += 64;
                }
                uint32_t first = (cur & 0x7FFFFFFFu) >> 3;
                uint32_t cnt = (cur & 7u) + 1u;
                for(uint32_t k = 0; k < cnt; ++k){
                    const float4 *tp = sc.tris + (size_t) (first + k) * 3;
                    float4 t0 = tp[0], t1 = tp[1], t2 = tp[2];
                    if(COUNT) n_tris += 1;
                    float t;
                    if(hit_triangle(ro, rd, xyz(t0), xyz(t1), xyz(t2), ANY ? tmax : 1e20f, t)){
                        if(ANY){
                            if(t > 1e-3f && (f2u(t2.w) & 1u)) blocked = true;
                        } else {
                            uint32_t ord = f2u(t0.w);
                            if(t < best_t || (t == best_t && ord < best_ord)){
                                best_t = t; best_prim = first + k; best_ord = ord; limit = t;
                            }
                        }
                    }
                }
                if(ANY && blocked) finished = true;                   // occluded: no contribution
                else if(sp > 0){
                    --sp;
                    cur = (RESUME && sp >= kResumeLdsLevels) ? deep[(size_t) (sp - kResumeLdsLevels) * deep_stride] : stk[sp * kBlock];
                }
                else finished = true;
            }
            if(finished){
                active = false;
                if(!ANY) pb.hit[path] = make_uint2(f2u(best_t), best_prim);
                else if(!blocked){
                    float4 c = sb.contrib[path];                      // record index; the path slot is in .w
                    const uint32_t slot = f2u(c.w);
                    float4 col = pb.col[slot];
                    col.x = col.x + c.x; col.y = col.y + c.y; col.z = col.z + c.z;
                    pb.col[slot] = col;
                }
            }
        }
    }
    if(COUNT){
        for(int off = 32; off > 0; off >>= 1){
            n_boxes += __shfl_down(n_boxes, off, 64); n_tris += __shfl_down(n_tris, off, 64);
            n_rays += __shfl_down(n_rays, off, 64); n_lane_steps += __shfl_down(n_lane_steps, off, 64);
            n_wave_steps += __shfl_down(n_wave_steps, off, 64); n_leaf_lane += __shfl_down(n_leaf_lane, off, 64);
            n_leaf_wave += __shfl_down(n_leaf_wave, off, 64);
        }
        if(lane == 0u){
            if(n_boxes) atomicAdd(ANY ? &wc->boxes_shadow : &wc->boxes_closest, n_boxes);
            if(n_tris) atomicAdd(ANY ? &wc->tris_shadow : &wc->tris_closest, n_tris);
            if(n_rays) atomicAdd(ANY ? &wc->shadow_rays : &wc->closest_rays, n_rays);
            if(n_lane_steps) atomicAdd(ANY ? &wc->lane_steps_shadow : &wc->lane_steps_closest, n_lane_steps);
            if(n_wave_steps) atomicAdd(ANY ? &wc->wave_steps_shadow : &wc->wave_steps_closest, n_wave_steps);
            if(n_leaf_lane) atomicAdd(ANY ? &wc->leaf_lane_shadow : &wc->leaf_lane_closest, n_leaf_lane);
            if(n_leaf_wave) atomicAdd(ANY ? &wc->leaf_wave_shadow : &wc->leaf_wave_closest, n_leaf_wave);
        }
    }
}

// Two-launch split of one trace step (budget != 0): the first launch gives every ray `budget` node
// steps; rays that need more (the few that run deep into a dense mesh) are set aside -- appended to the
// long queue with one global atomic per workgroup: shadow rays and the closest-hit rays of iteration 0 as
// the queue entries they came with, collected in LDS, closest-hit rays of later iterations as records
// (DeferredRay) written from the chunk's first queue position on -- and a second launch (RESUME) restarts
// them with the partial result as the limit.  Lanes of the first launch are
// therefore never parked on a long ray while the short rays around them wait for a refill; the result
// is the same (closest hit with the ordinal tie-break, or the occlusion boolean, of the same ray).
struct LongQueues { uint32_t *equeue, *ecount, *squeue, *scount; uint32_t budget; DeferredRay *rec; };

template <bool COUNT, bool RESUME, bool TOP, bool PRIMARY>
__global__ __launch_bounds__(kBlock) HPT_TRACE_ATTR
void k_trace(SceneDev sc, PathBuf pb, ShadowBuf sb, const uint32_t *equeue, const uint32_t *ecount_ptr,
             const uint32_t *squeue, const uint32_t *scount_ptr, uint32_t chunk_rays, int refill_min, int node_min,
             int stack_words, LongQueues lq, WorkCounters *wc, PrimaryGen pg, uint32_t *deep){
    extern __shared__ uint32_t s_dyn_stack[];        // [stack level][lane], sized by the BVH depth; then the long-ray list
    __shared__ uint32_t s_next, s_nlong, s_gbase;
    __shared__ uint4 s_top[TOP ? kTopNodes * 2 : 1];  // the top of the quantised tree (first launch of a split step)
    uint32_t *s_long = s_dyn_stack + stack_words;
    if(TOP){
        const uint32_t words = (uint32_t) (sc.num_nodes < kTopNodes ? sc.num_nodes : kTopNodes) * 2u;
        for(uint32_t i = threadIdx.x; i < words; i += kBlock) s_top[i] = sc.qnodes[i];
        // (the first __syncthreads of the chunk loop below orders these stores before any traversal)
    }
    uint32_t ecount = ecount_ptr ? *ecount_ptr : 0u, scount = scount_ptr ? *scount_ptr : 0u;
    // short queues (the delta-bounce tail) get one ray per lane so they spread over every CU
    uint32_t ce = ecount >= kTraceShortQueue ? chunk_rays : (uint32_t) kBlock;
    uint32_t cs = scount >= kTraceShortQueue ? chunk_rays : (uint32_t) kBlock;
    uint32_t ne = (ecount + ce - 1) / ce, ns = (scount + cs - 1) / cs;
    for(uint32_t bid = blockIdx.x; bid < ne + ns; bid += gridDim.x){
        bool shadow = bid >= ne;
        uint32_t chunk = shadow ? bid - ne : bid;
        uint32_t csize = shadow ? cs : ce;
        uint32_t begin = chunk * csize;
        uint32_t total = shadow ? scount : ecount;
        uint32_t end = begin + csize < total ? begin + csize : total;
        // closest-hit rays past iteration 0 are set aside as records at `begin` + rank (trace_chunk): their count starts there
        const bool records = !shadow && !PRIMARY && !COUNT;      // (a counting launch is never split)
        const uint32_t lbase = records ? begin : 0u;
        if(threadIdx.x == 0){ s_next = begin; s_nlong = lbase; }
        __syncthreads();
        uint32_t *deep_lane = RESUME ? deep + (size_t) blockIdx.x * kBlock + threadIdx.x : nullptr;
        const uint32_t deep_stride = gridDim.x * kBlock;
        if(shadow) trace_chunk<true, COUNT, RESUME, TOP, false>(sc, pb, sb, squeue, end, s_dyn_stack + threadIdx.x, &s_next, refill_min, node_min, wc,
                                                                lq.budget, lq.rec, s_long, &s_nlong, s_top, pg, deep_lane, deep_stride);
        else trace_chunk<false, COUNT, RESUME, TOP, PRIMARY>(sc, pb, sb, equeue, end, s_dyn_stack + threadIdx.x, &s_next, refill_min, node_min, wc,
                                                             lq.budget, lq.rec, s_long, &s_nlong, s_top, pg, deep_lane, deep_stride);
        __syncthreads();
        if(!RESUME && lq.budget != 0u){
            uint32_t n = s_nlong - lbase;
            if(n != 0u){
                if(threadIdx.x == 0) s_gbase = atomicAdd(shadow ? lq.scount : lq.ecount, n);
                __syncthreads();
                uint32_t *dst = (shadow ? lq.squeue : lq.equeue) + s_gbase;
                for(uint32_t i = threadIdx.x; i < n; i += kBlock) dst[i] = records ? begin + i : s_long[i];
            }
        }
        __syncthreads();
    }
}

} // namespace

// ---- launchers --------------------------------------------------------------------------

void launch_trace(hipStream_t s, const SceneDev &sc, PathBuf pb, ShadowBuf sb, const uint32_t *equeue,
                  const uint32_t *ecount, uint32_t max_extend, const uint32_t *squeue, const uint32_t *scount,
                  uint32_t max_shadow, int stack_levels, bool count, WorkCounters *wc, const TraceSplit *split,
                  const PrimaryGen *primary, uint32_t max_groups){
    const uint32_t chunk = (uint32_t) kTraceChunk;
    // worst-case grid for either chunking regime of k_trace (long queues: `chunk` rays per workgroup,
    // queues shorter than kTraceShortQueue: kBlock rays per workgroup)
    auto groups = [&](uint32_t items){
        uint32_t a = (items + chunk - 1) / chunk;
        uint32_t shortest = items < kTraceShortQueue ? items : kTraceShortQueue;
        uint32_t b = (shortest + kBlock - 1) / kBlock;
        return a > b ? a : b;
    };
    uint32_t g = (ecount ? groups(max_extend) : 0u) + (scount ? groups(max_shadow) : 0u);
    if(g == 0u) return;
    if(max_groups != 0u && g > max_groups) g = max_groups;          // k_trace walks the chunks with a stride
    if(stack_levels < 1) stack_levels = 1;
    if(stack_levels > kStackDepth) stack_levels = kStackDepth;
    int stack_words = (stack_levels + 1) * kBlock;                            // + the spare level of the branch-free step
    LongQueues lq{};
    if(split && split->budget > 0 && !count){
        lq.equeue = split->equeue; lq.ecount = split->ecount; lq.squeue = split->squeue; lq.scount = split->scount;
        lq.budget = (uint32_t) split->budget; lq.rec = split->rec;
        // a ray of this launch is set aside after `budget` node steps, so its stack never grows past that many entries
        if(stack_levels > split->budget) stack_words = (split->budget + 1) * kBlock;
    }
    size_t lds = (size_t) stack_words * sizeof(uint32_t) + (lq.budget ? (size_t) chunk * sizeof(uint32_t) : 0);
    const bool top = lq.budget != 0u && lq.budget <= (uint32_t) kTopLevels;
    PrimaryGen none{};
    const PrimaryGen &pg = primary ? *primary : none;
#define HPT_LAUNCH_TRACE(C, T, P) hipLaunchKernelGGL((k_trace<C, false, T, P>), dim3(g), dim3(kBlock), lds, s, sc, pb, sb, equeue, ecount, squeue, \
                                                     scount, chunk, kRefillMin, kNodeMin, stack_words, lq, wc, pg, (uint32_t *) nullptr)
    if(count) HPT_LAUNCH_TRACE(true, false, false);
    else if(top && primary) HPT_LAUNCH_TRACE(false, true, true);
    else if(top) HPT_LAUNCH_TRACE(false, true, false);
    else if(primary) HPT_LAUNCH_TRACE(false, false, true);
    else HPT_LAUNCH_TRACE(false, false, false);
#undef HPT_LAUNCH_TRACE
}

// second launch of a split trace step: the rays launch_trace set aside.  Their number is only known on
// the device, so a fixed grid walks the chunks.  The long rays walk the four-wide twin of the tree (up to
// three children stacked per step), kResumeLdsLevels stack levels per lane in LDS and the deeper ones in
// deep_stack (resume_deep_stack_words()); render_local only splits scenes whose tree fits (resume_walk_fits).
void launch_trace_resume(hipStream_t s, const SceneDev &sc, PathBuf pb, ShadowBuf sb, bool extend, bool shadow,
                         uint32_t max_items, WorkCounters *wc, const TraceSplit &split, const PrimaryGen *primary,
                         uint32_t max_groups, uint32_t *deep_stack){
    if(!extend && !shadow) return;
    const int stack_words = (kResumeLdsLevels + 1) * kBlock;
    const size_t lds = (size_t) stack_words * sizeof(uint32_t);
    uint32_t per = (max_items + kBlock - 1) / kBlock;
    uint64_t g = (uint64_t) per * ((extend ? 1u : 0u) + (shadow ? 1u : 0u));
    uint32_t g2 = g < kResumeMaxGroups ? (uint32_t) (g < 1u ? 1u : g) : kResumeMaxGroups;
    if(max_groups != 0u && g2 > max_groups) g2 = max_groups;          // blind tail iterations (HPT_FLAG_NO_HOST_WAIT)
    LongQueues none{};
    none.rec = split.rec;                                             // read here: the rays launch_trace wrote there
    PrimaryGen no_primary{};
    const uint32_t *eq = extend ? split.equeue : nullptr, *ec = extend ? split.ecount : nullptr;
    const uint32_t *sq = shadow ? split.squeue : nullptr, *scn = shadow ? split.scount : nullptr;
    // every ray of this launch is a long one: a workgroup takes more rays (a lane gets ~8 rays, which evens
    // out their lengths), lanes refill sooner and the leaf phase waits for fewer stragglers
#define HPT_LAUNCH_RESUME(P, PG) hipLaunchKernelGGL((k_trace<false, true, false, P>), dim3(g2), dim3(kBlock), lds, s, sc, pb, sb, eq, ec, sq, scn, \
                                                    kLongChunk, kWideRefillMin, kWideNodeMin, stack_words, none, wc, PG, deep_stack)
    if(primary && extend) HPT_LAUNCH_RESUME(true, *primary);
    else HPT_LAUNCH_RESUME(false, no_primary);
#undef HPT_LAUNCH_RESUME
}

size_t resume_deep_stack_words(){ return (size_t) kDeepLevels * kResumeMaxGroups * kBlock; }

} // namespace hpt
