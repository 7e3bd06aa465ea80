// The shade stage of the path-tracing pipeline (pt_kernels.h) for gfx950: k_shade -- light-hit emission, next-event estimation staged
// in LDS and evaluated 64 records at a time, BSDF sampling, compaction of survivors and shadow requests -- and its launcher.
#include "pt_device_common.h"

namespace hpt {

namespace {

#ifndef HPT_LDS_MATS
#define HPT_LDS_MATS 128
#endif
#ifndef HPT_LDS_LIGHTS
#define HPT_LDS_LIGHTS 32
#endif
#ifndef HPT_SHADE_CHUNK
#define HPT_SHADE_CHUNK 1024
#endif
#ifdef HPT_SHADE_WAVES
#define HPT_SHADE_ATTR __attribute__((amdgpu_waves_per_eu(HPT_SHADE_WAVES, 8)))
#else
#define HPT_SHADE_ATTR
#endif
constexpr int kLdsMats = HPT_LDS_MATS;    // material records staged in LDS (6 KiB)
constexpr int kLdsLights = HPT_LDS_LIGHTS;   // light records staged in LDS (3.5 KiB)
constexpr int kShadeChunk = HPT_SHADE_CHUNK;        // paths per workgroup at most (LDS staging capacity)
constexpr int kShadeTargetGroups = 1024; // workgroups a short queue is spread over
// Next-event candidates of a wave are staged in LDS and evaluated 64 at a time (see k_shade): words per record
constexpr int kNeeWords = 20;
// 0-2 wo (local) | 3-5 wi (local) | 6 Lambda(wo) | 7 material index | 8-10 throughput | 11 pdf_light_dir |
// 12-14 shadow segment start | 15-17 shadow segment end | 18 path slot | 19 light index | parallel << 31

// development (-DHPT_SHADE_PROFILE=1|2|5, counting renders only; 3 and 4: probes inside the BSDF functions, pt_device_math.h): how many wave trips enter a section of k_shade and with how many
// lanes, through the eight bd_* counters (four sections per build): scripts/shade_sections.py
#ifdef HPT_SHADE_PROFILE
#define HPT_SECTION(set, idx) do { if(wc && HPT_SHADE_PROFILE == (set)){ unsigned long long m_ = __ballot(true); \
    if((int) (threadIdx.x & 63u) == __ffsll((long long) m_) - 1){ atomicAdd(&wc->bd_pairs + 2 * (idx), 1ull); atomicAdd(&wc->bd_pairs + 2 * (idx) + 1, (unsigned long long) __popcll(m_)); } } } while(0)
#else
#define HPT_SECTION(set, idx) do {} while(0)
#endif

template <bool PRIMARY, bool STRIDED>
__global__ __launch_bounds__(kBlock) HPT_SHADE_ATTR
void k_shade(SceneDev sc, PathBuf pb, const uint32_t *queue, const uint32_t *qcount,
             uint32_t *next_queue, uint32_t *next_count, ShadowBuf sb, uint32_t *squeue, uint32_t *scount,
             int max_depth, int max_delta, int roulette, WorkCounters *wc, PrimaryGen pg){
    __shared__ DevMaterial s_mats[kLdsMats];
    __shared__ DevLight s_lights[kLdsLights];
    // survivors and shadow requests of this workgroup's chunk are compacted in LDS (wave64
    // ballot + mbcnt prefix, one LDS atomic per wave) and flushed with ONE global atomic per
    // queue: same-address global atomics saturate near 88 per microsecond on this chip.
    __shared__ uint32_t s_next[kShadeChunk];
    // A shadow record is stored at a queue position of this workgroup's own chunk, the chunk's first position + the
    // record's rank among the chunk's records: [begin, end) ranges of workgroups are disjoint and a path has at most
    // one pending shadow ray, so the records of a chunk are dense (full cache lines written here, coalesced reads in
    // the trace launch) and the shadow-queue entries of a chunk are just begin + 0, 1, 2, ...
    __shared__ uint32_t s_cnt[4];          // [0] survivors, [1] shadow requests, [2],[3] global bases
    // Next-event estimation is evaluated DENSELY.  Only about a third of the lanes of a trip get past the cosine and
    // cone tests, and the BSDF value + pdf + MIS + shadow-record code behind them is ~30 % of this kernel's time
    // (knock-out: 16.3 -> 11.2 ms per pass).  So a lane that passes leaves a 20-word record in its wave's LDS staging
    // area instead of evaluating; once 64 records are waiting (about three trips) the wave evaluates them with every
    // lane busy.  Same expressions on the same operands, so the contributions are bit-identical; only the order of the
    // shadow queue changes, which nothing depends on.  Wave-private: no barrier, the count lives in a register.
    __shared__ uint32_t s_stage[kBlock / 64][kNeeWords][64];
    uint32_t (*stage)[64] = s_stage[threadIdx.x >> 6];
    uint32_t staged = 0u;                  // records waiting in this wave's staging area (wave-uniform)
    const uint32_t lane = threadIdx.x & 63u;
    // evaluates the first n staged records, one per lane (pt_cu.cu:136-146 parallel lights, :179-196 ball lights);
    // rec_base = first queue position of the chunk the records belong to (staged records never outlive their chunk)
    auto flush_nee = [&](uint32_t n, uint32_t rec_base){
        bool want = false;
        // written where `want` is set and read under it only: no initialisers, a default would be filled in at every join
        uint32_t spath; f3 c, org, dir; float dist;
        if(lane < n){
            HPT_SECTION(2, 3);                                         // section h: staged next-event evaluation
            f3 wo_l = mk3(u2f(stage[0][lane]), u2f(stage[1][lane]), u2f(stage[2][lane]));
            f3 wi_l = mk3(u2f(stage[3][lane]), u2f(stage[4][lane]), u2f(stage[5][lane]));
            ShadePre pre; pre.lam_o = u2f(stage[6][lane]);
            const uint32_t mat_i = stage[7][lane], light_i = stage[19][lane];
            f3 thr = mk3(u2f(stage[8][lane]), u2f(stage[9][lane]), u2f(stage[10][lane]));
            const float pdf_light_dir = u2f(stage[11][lane]);
            f3 p1 = mk3(u2f(stage[12][lane]), u2f(stage[13][lane]), u2f(stage[14][lane]));
            f3 p2 = mk3(u2f(stage[15][lane]), u2f(stage[16][lane]), u2f(stage[17][lane]));
            spath = stage[18][lane];
            const DevMaterial dm = (sc.num_mats <= kLdsMats ? s_mats : sc.mats)[mat_i];
            const DevLight &L = (sc.num_lights <= kLdsLights ? s_lights : sc.lights)[light_i & 0x7FFFFFFFu];
            Mat m; m.base = mk3(dm.base[0], dm.base[1], dm.base[2]); m.roughness = dm.roughness; m.metallic = dm.metallic; m.eta = dm.eta;
            pre.diffuse = mk3(dm.diffuse[0], dm.diffuse[1], dm.diffuse[2]);
            MatPre mp; mp.alpha = dm.alpha; mp.metal = (dm.cls & kMatMetallic) != 0u;
            mp.smooth_dielectric = (dm.cls & kMatSmoothDielectric) != 0u; mp.mirror = (dm.cls & kMatMirror) != 0u;
            f3 illum = mk3(L.illum[0], L.illum[1], L.illum[2]);
            f3 brdf; float pdf_bsdf;
            bsdf_eval_pdf_local(m, wo_l, wi_l, brdf, pdf_bsdf, &pre, &mp);
            const float cos_surface = fmaxf(0.0f, wi_l.z);           // = max(0, dot(normal, wi)): the frame's third axis is the normal
            f3 contrib;
            if(light_i >> 31) contrib = thr * brdf * illum * mk3(1.0f, 1.0f, 1.0f) * cos_surface * (float) sc.num_lights;
            else {
                float p_l = pdf_light_dir * pdf_light_dir;
                float p_b = pdf_bsdf * pdf_bsdf;
                float mis_w = p_l / fmaxf(p_l + p_b, 1e-8f);
                contrib = thr * brdf * illum * mk3(1.0f, 1.0f, 1.0f) * cos_surface / pdf_light_dir * mis_w;
            }
            if(is_valid_color(contrib)){
                HPT_SECTION(5, 3);                                     // next-event contribution kept: shadow record written
                want = true;
                c = clamp_radiance(contrib, 15.0f);
                org = p1;
                f3 diff = p2 - p1;                              // geometric.cuh:298-303
                dist = length3(diff);
                dir = diff / dist;
            }
        }
        uint32_t r = rec_base + lds_push(want, &s_cnt[1]);       // rank within the chunk -> record index
        if(want){
            sb.org_max[r] = make_float4(org.x, org.y, org.z, dist - 1e-3f);
            sb.dir[r] = make_float4(dir.x, dir.y, dir.z, 0.0f);
            sb.contrib[r] = make_float4(c.x, c.y, c.z, u2f(spath));   // the path slot rides along as bits
        }
    };
#ifdef HPT_SHADE_PROFILE
    g_hpt_probe = wc ? &wc->bd_pairs : nullptr;            // every thread stores the same value before it reads it
#endif
    if(threadIdx.x < 4) s_cnt[threadIdx.x] = 0u;
    const bool mats_in_lds = sc.num_mats <= kLdsMats;
    const bool lights_in_lds = sc.num_lights <= kLdsLights;
    if(mats_in_lds){
        const uint32_t *src = (const uint32_t *) sc.mats; uint32_t *dst = (uint32_t *) s_mats;
        for(int w = threadIdx.x; w < sc.num_mats * (int) (sizeof(DevMaterial) / 4); w += kBlock) dst[w] = src[w];
    }
    if(lights_in_lds){
        const uint32_t *src = (const uint32_t *) sc.lights; uint32_t *dst = (uint32_t *) s_lights;
        for(int w = threadIdx.x; w < sc.num_lights * (int) (sizeof(DevLight) / 4); w += kBlock) dst[w] = src[w];
    }
    __syncthreads();
    const DevMaterial *mats = mats_in_lds ? s_mats : sc.mats;
    const DevLight *lights = lights_in_lds ? s_lights : sc.lights;

    uint32_t count = *qcount;
    // contiguous chunk per workgroup: small enough to spread a short queue over the chip,
    // never larger than the LDS staging buffers
    uint32_t chunk = (count + kShadeTargetGroups - 1) / kShadeTargetGroups;
    chunk = (chunk + kBlock - 1) / kBlock * kBlock;
    chunk = chunk < (uint32_t) kBlock ? (uint32_t) kBlock : (chunk > (uint32_t) kShadeChunk ? (uint32_t) kShadeChunk : chunk);
    uint32_t iters = 0;
    // one chunk per workgroup when the grid covers the queue (the usual launch); STRIDED: a smaller grid (the unseen
    // tail iterations of HPT_FLAG_NO_HOST_WAIT) walks the chunks with a stride
    for(uint32_t cb = blockIdx.x; (unsigned long long) cb * chunk < count; cb += gridDim.x){
    if(STRIDED && cb != blockIdx.x){
        __syncthreads();                                   // the previous chunk's lists have been copied out
        if(threadIdx.x < 4) s_cnt[threadIdx.x] = 0u;
        __syncthreads();
    }
    uint32_t begin = cb * chunk;
    uint32_t end = begin + chunk < count ? begin + chunk : count;
    for(uint32_t base = begin; base < end; base += kBlock){
        uint32_t i = base + threadIdx.x;
        bool alive = false, nee = false;
        // `path` is read under `alive` or `nee`, which only a lane with a queue entry sets.  The next-event candidate of this
        // lane's path, if it gets one (record layout: kNeeWords), is read under `nee`: the hit-level words are written at
        // every surface hit, the others in both branches that set `nee` (parallel light, ball light).  None has an initialiser -- the compiler would fill all
        // twenty-one registers with it at the head of every trip and again at the joins of the divergent branches below.
        uint32_t path;
        f3 n_wo, n_wi, n_thr, s_p1, s_p2;
        float n_lam, n_pdf_light; uint32_t n_mat, n_light;
        if(i < count){
            path = queue ? queue[i] : i;
            ++iters;
            HPT_SECTION(1, 0);                                         // section a: a queue entry
            uint2 h = pb.hit[path];
            uint32_t prim = h.y;
            // PRIMARY (iteration 0 without a generate launch): the path state is not in memory yet -- the ray is recomputed
            // from the slot number, throughput 1, depth 0, "last bounce was delta" so a light seen directly counts
            // (pt_cu.cu:41-46); every slot's radiance record is initialised here (emission or zero)
            f3 p_eye = mk3(0, 0, 0), p_dir = mk3(0, 0, 1), first_col = mk3(0, 0, 0); uint64_t p_rs = 0ull;
            if(PRIMARY && !primary_ray(pg, path, p_eye, p_dir, p_rs)) prim = kHitMiss;
            if(prim != kHitMiss){                                     // miss ends the path (pt_cu.cu:54)
                float t = u2f(h.x);
                float4 o4, d4, th4;
                if(PRIMARY){
                    o4 = make_float4(p_eye.x, p_eye.y, p_eye.z, 1.0f); d4 = make_float4(p_dir.x, p_dir.y, p_dir.z, u2f(1u));
                    th4 = make_float4(1.0f, 1.0f, 1.0f, 0.0f);
                } else { o4 = pb.org_eta[path]; d4 = pb.dir_flags[path]; th4 = pb.thr[path]; }
                f3 ro = xyz(o4), rd = xyz(d4), throughput = xyz(th4);
                float ray_eta = o4.w;
                uint32_t flags = f2u(d4.w);
                bool last_is_delta = (flags & 1u) != 0u;
                int depth = (int) ((flags >> 8) & 0xFFu);
                int delta_count = (int) ((flags >> 16) & 0xFFu);
                f3 pos = ro + rd * t;
                f3 wo = rd * -1.0f;
                f3 normal; uint32_t mat_idx; bool is_light = false;
                bool have_frame = false; f3 frame_T, frame_B;                 // the frame: read under have_frame
                if(prim & kHitRoundFlag){
                    DevRound r = sc.rounds[prim & 0x7FFFFFFFu];
                    normal = normalize3(pos - mk3(r.c[0], r.c[1], r.c[2]));
                    is_light = (r.flags & 2u) != 0u;
                    mat_idx = r.material;                             // light balls: the light's index
                    if(dot3(normal, rd) > 0.0f) normal = normal * -1.0f;
                } else {
                    // the triangle's unit normal and the local frames of both orientations were computed once
                    // per scene by k_tri_frames with these same expressions
                    const float4 *fp = sc.tri_frames + (size_t) prim * 4;
                    float4 q0 = fp[0], q1 = fp[1], q2 = fp[2], q3 = fp[3];
                    normal = mk3(q0.x, q0.y, q0.z);
                    mat_idx = f2u(q3.w);
                    have_frame = true;
                    if(dot3(normal, rd) > 0.0f){
                        normal = normal * -1.0f;
                        frame_T = mk3(q2.y, q2.z, q2.w); frame_B = mk3(q3.x, q3.y, q3.z);
                    } else {
                        frame_T = mk3(q0.w, q1.x, q1.y); frame_B = mk3(q1.z, q1.w, q2.x);
                    }
                }

                if(is_light){                                          // pt_cu.cu:59-122
                    HPT_SECTION(1, 1);                                 // section b: light hit
                    const DevLight &hl = lights[mat_idx];
                    f3 emission = mk3(hl.illum[0], hl.illum[1], hl.illum[2]);
                    float area = 1.0f, cone_ratio = 1.0f;
                    bool valid_light = false;
                    for(int li = 0; li < sc.num_lights; ++li){
                        const DevLight &L = lights[li];
                        f3 c2h = pos - mk3(L.pos[0], L.pos[1], L.pos[2]);
                        if(fabsf(length3(c2h) - L.r) < 1e-2f){
                            valid_light = true;
                            area = L.area;
                            if(L.cutoff > 0.0f && !L.is_parallel){
                                cone_ratio = L.cone_ratio;
                                if(depth == 0) cone_ratio = 1.f;
                                else if(dot3(mk3(L.main_dir[0], L.main_dir[1], L.main_dir[2]), normalize3(c2h)) < L.cos_cutoff) cone_ratio = 0.0f;
                            }
                            break;
                        }
                    }
                    if(valid_light && cone_ratio > 0.0f) emission = emission / (area * cone_ratio);
                    else emission = mk3(0, 0, 0);
                    if((emission.x > 0.0f || emission.y > 0.0f || emission.z > 0.0f) && last_is_delta){
                        f3 contrib = throughput * emission;
                        if(is_valid_color(contrib)){
                            f3 c = clamp_radiance(contrib, 15.0f);
                            if(PRIMARY) first_col = mk3(0.0f + c.x, 0.0f + c.y, 0.0f + c.z);       // the sum starts at zero (pt_cu.cu:39)
                            else {
                                float4 col = pb.col[path];
                                col.x = col.x + c.x; col.y = col.y + c.y; col.z = col.z + c.z;
                                pb.col[path] = col;
                            }
                        }
                    }
                    // BSDF-sampled light hits after a non-delta bounce add nothing (the reference's
                    // MIS branch is a stub with pdf_light_dir = 0, pt_cu.cu:103-118); path ends here.
                } else {
                    HPT_SECTION(1, 2);                                 // section c: surface hit
                    DevMaterial dm = mats[mat_idx];
                    Mat m; m.base = mk3(dm.base[0], dm.base[1], dm.base[2]);
                    m.roughness = dm.roughness; m.metallic = dm.metallic; m.eta = dm.eta;
                    ShadePre pre; pre.diffuse = mk3(dm.diffuse[0], dm.diffuse[1], dm.diffuse[2]);     // uploaded with the scene
                    // a delta lobe does not count as a bounce; any other material's path ends at max_depth, so on
                    // its last bounce the sampled direction would never be used (pt_cu.cu:37, 228-241)
                    // (the comparisons on the material's three floats come with the table: DevMaterial::cls, ::alpha)
                    MatPre mp; mp.alpha = dm.alpha; mp.metal = (dm.cls & kMatMetallic) != 0u;
                    mp.smooth_dielectric = (dm.cls & kMatSmoothDielectric) != 0u; mp.mirror = (dm.cls & kMatMirror) != 0u;
                    const bool delta_mat = (dm.cls & (kMatSmoothDielectric | kMatMirror)) != 0u;
                    const bool last_bounce = !delta_mat && depth + 1 >= max_depth;
                    uint64_t rs;
                    if(PRIMARY) rs = p_rs;
                    else { uint2 r2 = pb.rng[path]; rs = ((uint64_t) r2.y << 32) | (uint64_t) r2.x; }
                    ShadeCtx ctx;
                    if(have_frame){ ctx.N = normal; ctx.T = frame_T; ctx.B = frame_B; ctx.wo = to_local(wo, frame_T, frame_B, normal); }
                    else ctx = make_shade_ctx(normal, wo);
                    pre.lam_o = ggx_lambda(ctx.wo, mp.alpha);     // shared by the NEE and the sampled query
                    // the hit-level words of a next-event record are set here, outside the nested branches behind the rejection
                    // loop.  (With them inside both branches hipcc 7.2's SLP vectorizer dropped the y component of the packed
                    // x/y pairs -- green = 0 in every contribution, caught by tests/test_gpu_parity.py on input.txt; the build
                    // now passes -fno-slp-vectorize, see the Makefile.)
                    n_wo = ctx.wo; n_lam = pre.lam_o; n_thr = throughput; n_mat = mat_idx;
                    s_p1 = pos + normal * kEps;

                    // next-event estimation, pt_cu.cu:125-202
                    if((dm.cls & kMatNextEvent) != 0u && sc.num_lights > 0){
                        int l_idx = min((int) (rng_next(rs) * sc.num_lights), sc.num_lights - 1);
                        const DevLight &L = lights[l_idx];
                        if(L.is_parallel){
                            f3 light_dir = mk3(L.neg_dir[0], L.neg_dir[1], L.neg_dir[2]);
                            float cos_surface = fmaxf(0.0f, dot3(normal, light_dir));
                            if(cos_surface > 0.0f){
                                nee = true;
                                n_wi = to_local(light_dir, ctx.T, ctx.B, ctx.N);
                                n_light = (uint32_t) l_idx | 0x80000000u;
                                n_pdf_light = 0.0f;                // a parallel light has no area pdf: the record's word is staged all the same
                                s_p2 = pos + light_dir * 1e4f;
                            }
                        } else {
                            f3 d_local;
                            uint32_t rs_lo = (uint32_t) rs, rs_hi = (uint32_t) (rs >> 32);     // the stream, in halves through the tries
                            do {
                                HPT_SECTION(1, 3);                     // section d: one try of the unit-ball rejection loop
                                // = mk3(a, b, c) * 2.0f - mk3(1.0f, 1.0f, 1.0f) of three rng_next draws, bit for bit
                                const uint32_t a = rng_next_u24(rs_lo, rs_hi), b = rng_next_u24(rs_lo, rs_hi), c = rng_next_u24(rs_lo, rs_hi);
                                d_local = mk3(ball_coordinate(a), ball_coordinate(b), ball_coordinate(c));
                            } while(dot3(d_local, d_local) >= 1.0f);
                            rs = ((uint64_t) rs_hi << 32) | (uint64_t) rs_lo;
                            HPT_SECTION(2, 0);                         // section e: next-event geometry behind the loop
                            if(length3(d_local) > 0.001f) d_local = normalize3(d_local);
                            else d_local = mk3(0, 1, 0);
                            f3 light_pos = mk3(L.pos[0], L.pos[1], L.pos[2]) + d_local * L.r;
                            f3 wi_light = light_pos - pos;
                            float dist2 = dot3(wi_light, wi_light);
                            float dist = sqrtf(dist2);
                            wi_light = wi_light / dist;
                            float cos_surface = fmaxf(0.0f, dot3(normal, wi_light));
                            float cos_light = fmaxf(0.0f, dot3(d_local, wi_light * -1.0f));
                            if(cos_surface > 0.0f && cos_light > 0.0f){
                                bool inside_cone = true;
                                if(L.cutoff > 0.0f){
                                    if(dot3(mk3(L.main_dir[0], L.main_dir[1], L.main_dir[2]), wi_light * -1.0f) < L.cos_cutoff) inside_cone = false;
                                }
                                if(inside_cone){
                                    nee = true;
                                    n_pdf_light = L.pdf_area * dist2 / fmaxf(cos_light, 1e-6f);
                                    n_wi = to_local(wi_light, ctx.T, ctx.B, ctx.N);
                                    n_light = (uint32_t) l_idx;
                                    s_p2 = light_pos + d_local * kEps;
                                }
                            }
                        }
                    }

                    // BSDF sampling and path continuation, pt_cu.cu:204-241
                    // what bsdf_sample hands back is read where pdf_omega > 0 only, and it writes all of it on those paths
                    f3 wi, bsdf_val; float pdf_omega = 0.0f, new_eta; bool is_delta;
                    if(!last_bounce){
                        HPT_SECTION(2, 1);                             // section f: direction sampling
                        float u_rr = rng_next(rs), u1 = rng_next(rs), u2 = rng_next(rs);
                        bsdf_sample<false>(m, ctx, u_rr, u1, u2, ray_eta, wi, bsdf_val, pdf_omega, is_delta, new_eta, &pre, &mp);
                    }
                    if(!(pdf_omega <= 0.0f)){          // pt_cu.cu:214 (and the TIR return, defined: terminate)
                        HPT_SECTION(2, 2);                             // section g: throughput update and continuation
                        f3 new_o;
                        if(is_delta){
                            HPT_SECTION(5, 0);                         // delta continuation
                            throughput = throughput * bsdf_val;
                            ray_eta = new_eta;
                            if(dot3(wi, normal) < 0.0f) new_o = pos - normal * kEps;
                            else new_o = pos + normal * kEps;
                            last_is_delta = true;
                            ++delta_count;
                            alive = is_valid_color(throughput) && delta_count <= max_delta;
                        } else {
                            HPT_SECTION(5, 1);                         // non-delta continuation
                            float cos_wi = fabsf(dot3(normal, wi));
                            throughput = throughput * bsdf_val * cos_wi / pdf_omega;
                            new_o = pos + normal * kEps;
                            last_is_delta = false;
                            ++depth;
                            alive = is_valid_color(throughput);
                            if(alive && roulette){
                                float q = fminf(1.0f, fmaxf(0.05f, fmaxf(throughput.x, fmaxf(throughput.y, throughput.z))));
                                float u = rng_next(rs);
                                alive = u < q;
                                throughput = throughput / q;
                            }
                            alive = alive && depth < max_depth;
                        }
                        if(alive){
                            HPT_SECTION(5, 2);                         // the path goes on: state written back
                            uint32_t nf = (last_is_delta ? 1u : 0u) | ((uint32_t) depth << 8) | ((uint32_t) delta_count << 16);
                            pb.org_eta[path] = make_float4(new_o.x, new_o.y, new_o.z, ray_eta);
                            pb.dir_flags[path] = make_float4(wi.x, wi.y, wi.z, u2f(nf));
                            pb.thr[path] = make_float4(throughput.x, throughput.y, throughput.z, 0.0f);
                            pb.rng[path] = make_uint2((uint32_t) rs, (uint32_t) (rs >> 32));
                        }
                    }
                }
            }
            if(PRIMARY) pb.col[path] = make_float4(first_col.x, first_col.y, first_col.z, 0.0f);
        }
        // stage this trip's next-event candidates; evaluate when the wave's staging area would overflow
        {
            const unsigned long long cm = __ballot(nee);
            if(cm != 0ull){
                const uint32_t k = (uint32_t) __popcll(cm);
                if(staged + k > 64u){ flush_nee(staged, begin); staged = 0u; }
                if(nee){
                    const uint32_t slot = staged + __builtin_amdgcn_mbcnt_hi((uint32_t) (cm >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t) cm, 0u));
                    stage[0][slot] = f2u(n_wo.x); stage[1][slot] = f2u(n_wo.y); stage[2][slot] = f2u(n_wo.z);
                    stage[3][slot] = f2u(n_wi.x); stage[4][slot] = f2u(n_wi.y); stage[5][slot] = f2u(n_wi.z);
                    stage[6][slot] = f2u(n_lam); stage[7][slot] = n_mat;
                    stage[8][slot] = f2u(n_thr.x); stage[9][slot] = f2u(n_thr.y); stage[10][slot] = f2u(n_thr.z);
                    stage[11][slot] = f2u(n_pdf_light);
                    stage[12][slot] = f2u(s_p1.x); stage[13][slot] = f2u(s_p1.y); stage[14][slot] = f2u(s_p1.z);
                    stage[15][slot] = f2u(s_p2.x); stage[16][slot] = f2u(s_p2.y); stage[17][slot] = f2u(s_p2.z);
                    stage[18][slot] = path; stage[19][slot] = n_light;
                }
                staged += k;
            }
        }
        uint32_t qpos = lds_push(alive, &s_cnt[0]);
        if(alive) s_next[qpos] = path;
    }
    if(staged != 0u){ flush_nee(staged, begin); staged = 0u; }
    __syncthreads();
    if(threadIdx.x == 0){
        s_cnt[2] = s_cnt[0] ? atomicAdd(next_count, s_cnt[0]) : 0u;
        s_cnt[3] = s_cnt[1] ? atomicAdd(scount, s_cnt[1]) : 0u;
    }
    __syncthreads();
    for(uint32_t k = threadIdx.x; k < s_cnt[0]; k += kBlock) next_queue[s_cnt[2] + k] = s_next[k];
    for(uint32_t k = threadIdx.x; k < s_cnt[1]; k += kBlock) squeue[s_cnt[3] + k] = begin + k;
    if(!STRIDED) break;
    }
    if(wc){
        unsigned long long v = iters;
        for(int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
        if((threadIdx.x & 63u) == 0u && v) atomicAdd(&wc->path_iters, v);
    }
}

} // namespace

// ---- launchers --------------------------------------------------------------------------

void launch_shade(hipStream_t s, const SceneDev &sc, PathBuf pb, const uint32_t *queue, const uint32_t *qcount,
                  uint32_t max_items, uint32_t *next_queue, uint32_t *next_count, ShadowBuf sb, uint32_t *squeue,
                  uint32_t *scount, int max_depth, int max_delta, int roulette, WorkCounters *wc, const PrimaryGen *primary,
                  uint32_t max_groups){
    // enough workgroups for either chunking regime (see k_shade)
    uint32_t g = (max_items + kShadeChunk - 1) / kShadeChunk;
    if(g < (uint32_t) kShadeTargetGroups) g = (uint32_t) kShadeTargetGroups;
    uint32_t small = (max_items + kBlock - 1) / kBlock;
    if(small < g) g = small < 1u ? 1u : small;
    const bool strided = max_groups != 0u && g > max_groups;        // the kernel then walks the chunks with a stride
    if(strided) g = max_groups;
    PrimaryGen none{};
    if(primary) hipLaunchKernelGGL((k_shade<true, false>), dim3(g), dim3(kBlock), 0, s, sc, pb, queue, qcount, next_queue,
                                   next_count, sb, squeue, scount, max_depth, max_delta, roulette, wc, *primary);
    else if(strided) hipLaunchKernelGGL((k_shade<false, true>), dim3(g), dim3(kBlock), 0, s, sc, pb, queue, qcount, next_queue,
                                        next_count, sb, squeue, scount, max_depth, max_delta, roulette, wc, none);
    else hipLaunchKernelGGL((k_shade<false, false>), dim3(g), dim3(kBlock), 0, s, sc, pb, queue, qcount, next_queue,
                            next_count, sb, squeue, scount, max_depth, max_delta, roulette, wc, none);
}

} // namespace hpt
