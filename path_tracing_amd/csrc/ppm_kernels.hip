// HIP kernels of the photon-mapping path (reference src/ppm_cu.cu), written for gfx950 (MI355X).  One pass:
//
//   eye     launch_generate (seed ^ kPpmEyeKey) -> [ launch_trace -> k_ppm_eye_shade ]*   (ppm_cu.cu:64-150)
//   photon  k_ppm_emit -> [ launch_trace -> k_ppm_photon_shade ]*                          (ppm_cu.cu:156-295)
//   grid    stable radix sort of the deposits' bucket keys, bucket ranges, packed records
//   gather  k_ppm_gather: one lane per hit point, 27 cells, resolve into the pass's radiance (ppm_cu.cu:300-322)
//
// Every closest-hit ray goes through the PT path's trace launches (pt_trace.hip) unchanged: the shade kernels here
// fill the PathBuf slots those launches read (origin, direction, flags) and read back the hit they write.
//
// The reference scatters every photon into a hash grid of hit points with float atomics, so its sums depend on
// arrival order.  Here every photon hit that can take a deposit writes it once, to the fixed slot
// photon * light_depth + depth (at most one per non-delta bounce), and each hit point sums its pairs itself, in a
// defined order: the 27 cells around its own cell (z, y, x from -1 to +1, x fastest), inside a cell ascending slot.
// The set of (photon, hit point) pairs is the reference's: |p - h| < r = cell size puts the two cells within one
// step on every axis, whichever side looks.  No float atomics anywhere, so the image is a function of the seed.
// Built with -ffp-contract=off like the PT kernels (pt_device_math.h).
#include "ppm_kernels.h"
#include "pt_device_common.h"

#include <rocprim/device/device_radix_sort.hpp>

namespace hpt {

namespace {

HPT_DEV void wave_count(bool v, unsigned long long *counter){
    unsigned long long mask = __ballot(v);
    if(mask != 0ull && (int) (threadIdx.x & 63u) == __ffsll((long long) mask) - 1) atomicAdd(counter, (unsigned long long) __popcll(mask));
}

// grid cell of a point: floorf((p - scene_min) / cell) per axis (ppm_cu.cu:34-38, 256-260), clamped to [-2^30, 2^30]
// in float before the conversion (NaN to -2^30), so that it is defined for every input and c +- 1 cannot overflow
HPT_DEV int cell_axis(float p, float smin, float cell){
    return (int) fminf(fmaxf(floorf((p - smin) / cell), -1073741824.0f), 1073741824.0f);
}
HPT_DEV void cell_of(const PpmFrame &fr, f3 p, int &gx, int &gy, int &gz){
    gx = cell_axis(p.x, fr.smin[0], fr.cell);
    gy = cell_axis(p.y, fr.smin[1], fr.cell);
    gz = cell_axis(p.z, fr.smin[2], fr.cell);
}
// bucket of a cell: the reference's spatial hash (ppm_cu.cu:28-30) through a 32-bit finaliser, masked to the table
HPT_DEV uint32_t bucket_of(int gx, int gy, int gz, uint32_t buckets){
    uint32_t h = ((uint32_t) gx * 73856093u) ^ ((uint32_t) gy * 19349663u) ^ ((uint32_t) gz * 83492791u);
    h ^= h >> 16; h *= 0x85EBCA6Bu; h ^= h >> 13; h *= 0xC2B2AE35u; h ^= h >> 16;
    return h & (buckets - 1u);
}

// hit record of a traced PathBuf slot (the decode of k_shade, pt_shade.hip)
struct PpmHit { f3 pos, normal; uint32_t mat; bool is_light; };
HPT_DEV PpmHit decode_hit(const SceneDev &sc, f3 ro, f3 rd, uint2 h){
    PpmHit r;
    float t = u2f(h.x);
    r.pos = ro + rd * t;
    r.is_light = false;
    if(h.y & kHitRoundFlag){
        DevRound rr = sc.rounds[h.y & 0x7FFFFFFFu];
        r.normal = normalize3(r.pos - mk3(rr.c[0], rr.c[1], rr.c[2]));
        r.is_light = (rr.flags & 2u) != 0u;
        r.mat = rr.material;                             // light balls: the light's index
    } else {
        const float4 q0 = sc.tri_frames[(size_t) h.y * 4], q3 = sc.tri_frames[(size_t) h.y * 4 + 3];
        r.normal = mk3(q0.x, q0.y, q0.z);                // normalize(cross(e1, e2)), k_tri_frames
        r.mat = f2u(q3.w);
    }
    if(dot3(r.normal, rd) > 0.0f) r.normal = r.normal * -1.0f;
    return r;
}

HPT_DEV Mat load_mat(const DevMaterial &dm){
    Mat m; m.base = mk3(dm.base[0], dm.base[1], dm.base[2]); m.roughness = dm.roughness; m.metallic = dm.metallic; m.eta = dm.eta;
    return m;
}
// bsdf_sample's delta lobes (smooth dielectric, mirror): a property of the material alone
HPT_DEV bool is_delta_mat(const Mat &m){
    return (m.eta > 0.0f && m.roughness < 0.001f && m.metallic < 0.01f) || (m.metallic > 0.99f && m.roughness < 0.001f);
}

// ---- eye pass, ppm_cu.cu:64-150 --------------------------------------------------------------------------------
// A light ball reached after delta bounces only writes clamp(throughput * illum); the first non-delta hit becomes
// the pixel's hit point and ends the path; delta bounces continue it (capped at max_delta), TIR ends it.
__global__ __launch_bounds__(kBlock)
void k_ppm_eye_shade(SceneDev sc, PathBuf pb, PpmHitBuf hb, const uint32_t *queue, const uint32_t *qcount,
                     uint32_t *next_queue, uint32_t *next_count, uint32_t *hp_count, int max_delta, PpmCounters *pc){
    const uint32_t count = *qcount;
    if(blockIdx.x * kBlock >= count) return;
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    bool alive = false, hit_point = false, direct = false;
    uint32_t path = 0u;
    if(i < count){
        path = queue ? queue[i] : i;
        const uint2 h = pb.hit[path];
        if(h.y != kHitMiss){
            float4 o4 = pb.org_eta[path], d4 = pb.dir_flags[path], th4 = pb.thr[path];
            f3 ro = xyz(o4), rd = xyz(d4), throughput = xyz(th4);
            uint32_t flags = f2u(d4.w);
            int delta_count = (int) ((flags >> 16) & 0xFFu);
            PpmHit hit = decode_hit(sc, ro, rd, h);
            f3 wo = rd * -1.0f;
            if(hit.is_light){
                const DevLight &L = sc.lights[hit.mat];
                f3 contrib = throughput * mk3(L.illum[0], L.illum[1], L.illum[2]);
                if(is_valid_color(contrib)){
                    f3 c = clamp_radiance(contrib, 15.0f);
                    pb.col[path] = make_float4(c.x, c.y, c.z, 0.0f);
                    direct = true;
                }
            } else {
                const Mat m = load_mat(sc.mats[hit.mat]);
                if(!is_delta_mat(m)){
                    // rough surface: the hit point (its bsdf_sample would draw three uniforms the path never uses)
                    hb.pos_mat[path] = make_float4(hit.pos.x, hit.pos.y, hit.pos.z, u2f(hit.mat));
                    hb.nrm[path] = make_float4(hit.normal.x, hit.normal.y, hit.normal.z, 0.0f);
                    hb.wo[path] = make_float4(wo.x, wo.y, wo.z, 0.0f);
                    hb.thr[path] = make_float4(throughput.x, throughput.y, throughput.z, 0.0f);
                    hit_point = true;
                } else {
                    uint2 r2 = pb.rng[path];
                    uint64_t rs = ((uint64_t) r2.y << 32) | (uint64_t) r2.x;
                    ShadeCtx ctx = make_shade_ctx(hit.normal, wo);
                    float u_rr = rng_next(rs), u1 = rng_next(rs), u2 = rng_next(rs);
                    f3 wi, f; float pdf, new_eta; bool is_delta;
                    bsdf_sample(m, ctx, u_rr, u1, u2, o4.w, wi, f, pdf, is_delta, new_eta, nullptr);
                    if(!(pdf <= 0.0f)){
                        throughput = throughput * f;
                        f3 new_o = hit.pos + hit.normal * (dot3(wi, hit.normal) < 0.0f ? -kEps : kEps);
                        ++delta_count;
                        alive = is_valid_color(throughput) && delta_count <= max_delta;
                        if(alive){
                            uint32_t nf = 1u | ((uint32_t) delta_count << 16);
                            pb.org_eta[path] = make_float4(new_o.x, new_o.y, new_o.z, new_eta);
                            pb.dir_flags[path] = make_float4(wi.x, wi.y, wi.z, u2f(nf));
                            pb.thr[path] = make_float4(throughput.x, throughput.y, throughput.z, 0.0f);
                            pb.rng[path] = make_uint2((uint32_t) rs, (uint32_t) (rs >> 32));
                        }
                    }
                }
            }
        }
    }
    uint32_t q = lds_push(alive, next_count);
    if(alive) next_queue[q] = path;
    uint32_t k = lds_push(hit_point, hp_count);
    if(hit_point) hb.list[k] = path;
    wave_count(direct, &pc->direct);
    wave_count(hit_point, &pc->hit_points);
}

// ---- photon emission, ppm_cu.cu:171-209 ------------------------------------------------------------------------
// Photon i leaves light i % nl with flux illum * nl / max(spl, 1) (the reference's normalisation, `* nl` included).
// A parallel light emits from a disc-sized square in front of the scene bounds; a spot light in its cone from the
// surface of its ball, with cos(theta) drawn directly and phi through the polynomial sincos (the BDPT path's form).
__global__ __launch_bounds__(kBlock)
void k_ppm_emit(SceneDev sc, PathBuf pb, uint32_t *qcount, uint32_t n_photons, int spl, uint64_t seed, uint32_t pass, PpmFrame fr){
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if(i == 0u) *qcount = n_photons;
    if(i >= n_photons) return;
    uint64_t rs = rng_seed(seed ^ kPpmPhotonKey, i, pass);
    const DevLight &L = sc.lights[i % (uint32_t) sc.num_lights];
    f3 w = normalize3(mk3(L.raw_dir[0], L.raw_dir[1], L.raw_dir[2]));
    f3 u_vec = (fabsf(w.x) > 0.9f) ? mk3(0, 1, 0) : mk3(1, 0, 0);
    f3 v_vec = normalize3(cross3(w, u_vec));
    u_vec = normalize3(cross3(v_vec, w));
    f3 ro, rd;
    if(L.is_parallel){
        rd = w;
        f3 mn = mk3(fr.smin[0], fr.smin[1], fr.smin[2]), mx = mk3(fr.smax[0], fr.smax[1], fr.smax[2]);
        f3 center = (mn + mx) * 0.5f;
        float radius = length3(mx - mn) * 0.5f;
        float r1 = rng_next(rs), r2 = rng_next(rs);
        float plane = radius * 2.0f;
        float offset_u = (r1 - 0.5f) * plane;
        float offset_v = (r2 - 0.5f) * plane;
        ro = center - rd * (radius * 2.0f) + u_vec * offset_u + v_vec * offset_v;
    } else {
        float u1 = rng_next(rs), u2 = rng_next(rs);
        float cos_t = 1.0f - u1 * (1.0f - L.cos_cutoff);
        float sin_t = sqrtf(fmaxf(0.0f, 1.0f - cos_t * cos_t));
        float sp, cp; sincos_2pi(u2, sp, cp);
        f3 local_dir = mk3(sin_t * cp, sin_t * sp, cos_t);
        rd = normalize3(u_vec * local_dir.x + v_vec * local_dir.y + w * local_dir.z);
        ro = mk3(L.pos[0], L.pos[1], L.pos[2]) + rd * L.r;
    }
    f3 flux = mk3(L.illum[0], L.illum[1], L.illum[2]) * (float) sc.num_lights / fmaxf((float) spl, 1.0f);
    pb.org_eta[i] = make_float4(ro.x, ro.y, ro.z, 1.0f);
    pb.dir_flags[i] = make_float4(rd.x, rd.y, rd.z, u2f(0u));
    pb.thr[i] = make_float4(flux.x, flux.y, flux.z, 0.0f);
    pb.rng[i] = make_uint2((uint32_t) rs, (uint32_t) (rs >> 32));
}

// ---- photon bounce, ppm_cu.cu:211-294 --------------------------------------------------------------------------
// At a hit that is not a light: a surface where no delta bounce can happen takes a deposit in the photon's slot for
// this depth (position, normal, direction to the light, flux; its grid bucket in g.key); then bsdf_sample.  A delta
// bounce multiplies the flux by the BSDF value alone and does not count towards depth.
__global__ __launch_bounds__(kBlock)
void k_ppm_photon_shade(SceneDev sc, PathBuf pb, PpmGrid g, const uint32_t *queue, const uint32_t *qcount,
                        uint32_t *next_queue, uint32_t *next_count, int light_depth, int max_delta, PpmFrame fr, PpmCounters *pc){
    const uint32_t count = *qcount;
    if(blockIdx.x * kBlock >= count) return;
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    bool alive = false, deposit = false;
    uint32_t path = 0u;
    if(i < count){
        path = queue ? queue[i] : i;
        const uint2 h = pb.hit[path];
        if(h.y != kHitMiss){
            float4 o4 = pb.org_eta[path], d4 = pb.dir_flags[path], th4 = pb.thr[path];
            f3 ro = xyz(o4), rd = xyz(d4), flux = xyz(th4);
            uint32_t flags = f2u(d4.w);
            int depth = (int) ((flags >> 8) & 0xFFu);
            int delta_count = (int) ((flags >> 16) & 0xFFu);
            PpmHit hit = decode_hit(sc, ro, rd, h);
            if(!hit.is_light){
                const DevMaterial dm = sc.mats[hit.mat];
                const Mat m = load_mat(dm);
                f3 wi_light = rd * -1.0f;
                if(m.eta <= 0.0f && (m.metallic < 0.99f || m.roughness > 0.01f)){
                    int gx, gy, gz;
                    cell_of(fr, hit.pos, gx, gy, gz);
                    const size_t slot = (size_t) path * (size_t) light_depth + (size_t) depth;
                    g.dep[slot * 4 + 0] = make_float4(hit.pos.x, hit.pos.y, hit.pos.z, u2f((uint32_t) gx));
                    g.dep[slot * 4 + 1] = make_float4(hit.normal.x, hit.normal.y, hit.normal.z, u2f((uint32_t) gy));
                    g.dep[slot * 4 + 2] = make_float4(wi_light.x, wi_light.y, wi_light.z, u2f((uint32_t) gz));
                    g.dep[slot * 4 + 3] = make_float4(flux.x, flux.y, flux.z, 0.0f);
                    g.key[slot] = bucket_of(gx, gy, gz, g.buckets);
                    deposit = true;
                }
                // a non-delta bounce from the last depth would end the loop anyway: its sample is never used
                const bool last = !is_delta_mat(m) && depth + 1 >= light_depth;
                if(!last){
                    uint2 r2 = pb.rng[path];
                    uint64_t rs = ((uint64_t) r2.y << 32) | (uint64_t) r2.x;
                    ShadeCtx ctx = make_shade_ctx(hit.normal, wi_light);
                    ShadePre pre; pre.diffuse = mk3(dm.diffuse[0], dm.diffuse[1], dm.diffuse[2]);
                    pre.lam_o = ggx_lambda(ctx.wo, roughness_to_alpha(m.roughness));
                    float u_rr = rng_next(rs), u1 = rng_next(rs), u2 = rng_next(rs);
                    f3 wi, f; float pdf, new_eta; bool is_delta;
                    bsdf_sample(m, ctx, u_rr, u1, u2, o4.w, wi, f, pdf, is_delta, new_eta, &pre);
                    if(!(pdf <= 0.0f)){
                        float cos_wi = fabsf(dot3(hit.normal, wi));
                        if(is_delta){ flux = flux * f; ++delta_count; }
                        else { flux = flux * f * cos_wi / pdf; ++depth; }
                        alive = is_valid_color(flux) && depth < light_depth && delta_count <= max_delta;
                        if(alive){
                            f3 new_o = hit.pos + hit.normal * (dot3(wi, hit.normal) < 0.0f ? -kEps : kEps);
                            uint32_t nf = (is_delta ? 1u : 0u) | ((uint32_t) depth << 8) | ((uint32_t) delta_count << 16);
                            pb.org_eta[path] = make_float4(new_o.x, new_o.y, new_o.z, new_eta);
                            pb.dir_flags[path] = make_float4(wi.x, wi.y, wi.z, u2f(nf));
                            pb.thr[path] = make_float4(flux.x, flux.y, flux.z, 0.0f);
                            pb.rng[path] = make_uint2((uint32_t) rs, (uint32_t) (rs >> 32));
                        }
                    }
                }
            }
        }
    }
    uint32_t q = lds_push(alive, next_count);
    if(alive) next_queue[q] = path;
    wave_count(i < count, &pc->photon_rays);
    wave_count(deposit, &pc->deposits);
}

// ---- grid ------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock)
void k_ppm_iota(uint32_t *p, uint32_t n){
    uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if(i < n) p[i] = i;
}

// After the sort: every bucket's range in the sorted order, and the deposits copied into that order
// (sentinel keys -- slots without a deposit -- sort last and are skipped)
__global__ __launch_bounds__(kBlock)
void k_ppm_ranges(PpmGrid g, uint32_t n){
    uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if(i >= n) return;
    uint32_t k = g.key_sorted[i];
    if(k >= g.buckets) return;
    if(i == 0u || g.key_sorted[i - 1] != k) g.range[k].x = i;
    if(i + 1u == n || g.key_sorted[i + 1] != k) g.range[k].y = i + 1u;
    size_t s = g.slot_sorted[i];
    g.packed[(size_t) i * 4 + 0] = g.dep[s * 4 + 0];
    g.packed[(size_t) i * 4 + 1] = g.dep[s * 4 + 1];
    g.packed[(size_t) i * 4 + 2] = g.dep[s * 4 + 2];
    g.packed[(size_t) i * 4 + 3] = g.dep[s * 4 + 3];
}

// ---- gather + resolve, ppm_cu.cu:258-322 -----------------------------------------------------------------------
// Everything about the hit point is hoisted out of the pair loop (shading frame, wo in it, Lambda(wo), the diffuse
// lobe); a pair costs the frame transform of the photon's direction and the rest of bsdf_evaluate -- the same
// expressions as the reference's call, so the same bits.
template <bool COUNT>
__global__ __launch_bounds__(kBlock)
void k_ppm_gather(SceneDev sc, PathBuf pb, PpmHitBuf hb, PpmGrid g, const uint32_t *hp_count, PpmFrame fr,
                  uint32_t *cand_out, uint32_t *acc_out, PpmCounters *pc){
    const uint32_t count = *hp_count;
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    unsigned long long n_cand = 0, n_acc = 0;
    if(i < count){
        const uint32_t slot = hb.list[i];
        const float4 pm = hb.pos_mat[slot];
        const f3 hp = xyz(pm), hn = xyz(hb.nrm[slot]), hwo = xyz(hb.wo[slot]), hthr = xyz(hb.thr[slot]);
        const DevMaterial dm = sc.mats[f2u(pm.w)];
        const Mat m = load_mat(dm);
        const ShadeCtx ctx = make_shade_ctx(hn, hwo);
        ShadePre pre; pre.diffuse = mk3(dm.diffuse[0], dm.diffuse[1], dm.diffuse[2]);
        pre.lam_o = ggx_lambda(ctx.wo, roughness_to_alpha(m.roughness));
        int cx, cy, cz;
        cell_of(fr, hp, cx, cy, cz);
        f3 acc = mk3(0, 0, 0);
        for(int z = -1; z <= 1; ++z) for(int y = -1; y <= 1; ++y) for(int x = -1; x <= 1; ++x){
            const int gx = cx + x, gy = cy + y, gz = cz + z;
            const uint2 r = g.range[bucket_of(gx, gy, gz, g.buckets)];
            for(uint32_t e = r.x; e < r.y; ++e){
                const float4 a = g.packed[(size_t) e * 4 + 0], b = g.packed[(size_t) e * 4 + 1], c = g.packed[(size_t) e * 4 + 2];
                if((int) f2u(a.w) != gx || (int) f2u(b.w) != gy || (int) f2u(c.w) != gz) continue;   // another cell in this bucket
                if(COUNT) ++n_cand;
                if(!(dot3(hn, xyz(b)) > 0.01f)) continue;
                const f3 d = hp - xyz(a);
                if(!(dot3(d, d) < fr.r2)) continue;
                if(COUNT) ++n_acc;
                f3 f; float pdf_unused;
                bsdf_eval_pdf_local<true, false>(m, ctx.wo, to_local(xyz(c), ctx.T, ctx.B, ctx.N), f, pdf_unused, &pre);
                if(is_valid_color(f)){
                    const float4 fl = g.packed[(size_t) e * 4 + 3];
                    f3 energy = xyz(fl) * f * hthr;
                    acc = acc + energy;
                }
            }
        }
        f3 radiance = acc / fmaxf(kPi * fr.r2, 1e-6f);
        if(is_valid_color(radiance)){
            float4 col = pb.col[slot];
            f3 cl = clamp_radiance(radiance, 15.0f);
            pb.col[slot] = make_float4(col.x + cl.x, col.y + cl.y, col.z + cl.z, 0.0f);
        }
        if(COUNT){ cand_out[slot] = (uint32_t) n_cand; acc_out[slot] = (uint32_t) n_acc; }
    }
    if(COUNT){
        n_cand = wave_sum(n_cand); n_acc = wave_sum(n_acc);
        if((threadIdx.x & 63u) == 0u){
            if(n_cand) atomicAdd(&pc->candidates, n_cand);
            if(n_acc) atomicAdd(&pc->accepted, n_acc);
        }
    }
}

// ---- progressive photon mapping (DESIGN.md "Progressive photon mapping") ---------------------------------------
// Cell offsets along one axis that a sphere of radius rho (in cells) around u = (h - smin) / cell can reach: -1 only
// if fr < rho + mg, +1 only if fr > 1 - rho - mg (fr = u - floor(u), exact); all three when |u| >= 2^20 or u is not
// a number.  The margin mg = 2^-6 + |u| 2^-20 covers the rounding of u, of a deposit's own u and of rho.
HPT_DEV void sppm_axis(float h, float smin, float cell, float rho, int &lo, int &hi){
    const float u = (h - smin) / cell;
    const float au = fabsf(u);
    lo = -1; hi = 1;
    if(!(au < 1048576.0f)) return;
    const float fr = u - floorf(u);
    const float mg = 0.015625f + au * 9.5367431640625e-07f;
    if(!(fr < rho + mg)) lo = 0;
    if(!(fr > 1.0f - rho - mg)) hi = 0;
}

// k_ppm_gather with the pixel's own R2 and the cull above, and the pixel's update fused in: the lane owns its pixel.
// Skipped cells hold no accepted pair, so the sum, M and the image are those of the full 27 cells, bit for bit.
template <bool COUNT>
__global__ __launch_bounds__(kBlock)
void k_sppm_gather(SceneDev sc, PpmHitBuf hb, PpmGrid g, const uint32_t *hp_count, PpmFrame fr, SppmState st, float alpha,
                   uint32_t *cand_out, uint32_t *acc_out, PpmCounters *pc){
    const uint32_t count = *hp_count;
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    unsigned long long n_cand = 0, n_acc = 0;
    if(i < count){
        const uint32_t slot = hb.list[i];
        const float4 pm = hb.pos_mat[slot];
        const f3 hp = xyz(pm), hn = xyz(hb.nrm[slot]), hwo = xyz(hb.wo[slot]), hthr = xyz(hb.thr[slot]);
        const float r2 = st.tau_r2[slot].w;
        const DevMaterial dm = sc.mats[f2u(pm.w)];
        const Mat m = load_mat(dm);
        const ShadeCtx ctx = make_shade_ctx(hn, hwo);
        ShadePre pre; pre.diffuse = mk3(dm.diffuse[0], dm.diffuse[1], dm.diffuse[2]);
        pre.lam_o = ggx_lambda(ctx.wo, roughness_to_alpha(m.roughness));
        int cx, cy, cz;
        cell_of(fr, hp, cx, cy, cz);
        const float rho = sqrtf(r2) / fr.cell;
        int x0, x1, y0, y1, z0, z1;
        sppm_axis(hp.x, fr.smin[0], fr.cell, rho, x0, x1);
        sppm_axis(hp.y, fr.smin[1], fr.cell, rho, y0, y1);
        sppm_axis(hp.z, fr.smin[2], fr.cell, rho, z0, z1);
        f3 acc = mk3(0, 0, 0);
        uint32_t n_m = 0;
        for(int z = z0; z <= z1; ++z) for(int y = y0; y <= y1; ++y) for(int x = x0; x <= x1; ++x){
            const int gx = cx + x, gy = cy + y, gz = cz + z;
            const uint2 r = g.range[bucket_of(gx, gy, gz, g.buckets)];
            for(uint32_t e = r.x; e < r.y; ++e){
                const float4 a = g.packed[(size_t) e * 4 + 0], b = g.packed[(size_t) e * 4 + 1], c = g.packed[(size_t) e * 4 + 2];
                if((int) f2u(a.w) != gx || (int) f2u(b.w) != gy || (int) f2u(c.w) != gz) continue;   // another cell in this bucket
                if(COUNT) ++n_cand;
                if(!(dot3(hn, xyz(b)) > 0.01f)) continue;
                const f3 d = hp - xyz(a);
                if(!(dot3(d, d) < r2)) continue;
                if(COUNT) ++n_acc;
                f3 f; float pdf_unused;
                bsdf_eval_pdf_local<true, false>(m, ctx.wo, to_local(xyz(c), ctx.T, ctx.B, ctx.N), f, pdf_unused, &pre);
                if(is_valid_color(f)){
                    const float4 fl = g.packed[(size_t) e * 4 + 3];
                    f3 energy = xyz(fl) * f * hthr;
                    acc = acc + energy;
                    ++n_m;
                }
            }
        }
        if(n_m > 0u){
            const float mf = (float) n_m;
            const float n_old = st.photons[slot];
            const float n_new = n_old + alpha * mf;
            const float ratio = n_new / (n_old + mf);
            const f3 tau = (xyz(st.tau_r2[slot]) + acc) * ratio;
            st.tau_r2[slot] = make_float4(tau.x, tau.y, tau.z, r2 * ratio);
            st.photons[slot] = n_new;
        }
        if(COUNT){ cand_out[slot] = (uint32_t) n_cand; acc_out[slot] = (uint32_t) n_acc; }
    }
    if(COUNT){
        n_cand = wave_sum(n_cand); n_acc = wave_sum(n_acc);
        if((threadIdx.x & 63u) == 0u){
            if(n_cand) atomicAdd(&pc->candidates, n_cand);
            if(n_acc) atomicAdd(&pc->accepted, n_acc);
        }
    }
}

__global__ __launch_bounds__(kBlock)
void k_sppm_init(SppmState st, uint32_t n, float r2){
    const uint32_t p = blockIdx.x * kBlock + threadIdx.x;
    if(p >= n) return;
    st.tau_r2[p] = make_float4(0.0f, 0.0f, 0.0f, r2);
    st.photons[p] = 0.0f;
    st.direct[p] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
}

// d = D, p = tau / max(pi R2, 1e-6), both divided by K unless K is 1; the radiance term after PPM's guard and clamp
__global__ __launch_bounds__(kBlock)
void k_sppm_estimate(Tiling tl, SppmState st, float passes, float *d_local){
    const uint32_t p = blockIdx.x * kBlock + threadIdx.x;
    if(p >= (uint32_t) tl.n_local) return;
    const float4 tr = st.tau_r2[p];
    f3 d = xyz(st.direct[p]);
    f3 rad = xyz(tr) / fmaxf(kPi * tr.w, 1e-6f);
    if(passes != 1.0f){ d = d / passes; rad = rad / passes; }
    const f3 v = is_valid_color(rad) ? d + clamp_radiance(rad, 15.0f) : d;
    d_local[(size_t) p * 3 + 0] = v.x;
    d_local[(size_t) p * 3 + 1] = v.y;
    d_local[(size_t) p * 3 + 2] = v.z;
}

__global__ __launch_bounds__(kBlock)
void k_sppm_state(Tiling tl, SppmState st, float *d_local){
    const uint32_t p = blockIdx.x * kBlock + threadIdx.x;
    if(p >= (uint32_t) tl.n_local) return;
    d_local[(size_t) p * 3 + 0] = st.tau_r2[p].w;
    d_local[(size_t) p * 3 + 1] = st.photons[p];
    d_local[(size_t) p * 3 + 2] = 0.0f;
}

uint32_t groups_for(uint32_t n){ return n == 0u ? 1u : (n + kBlock - 1) / kBlock; }

} // namespace

void launch_ppm_eye_shade(hipStream_t s, const SceneDev &sc, PathBuf pb, PpmHitBuf hb, const uint32_t *queue,
                          const uint32_t *qcount, uint32_t max_items, uint32_t *next_queue, uint32_t *next_count,
                          uint32_t *hp_count, int max_delta, PpmCounters *pc){
    hipLaunchKernelGGL(k_ppm_eye_shade, dim3(groups_for(max_items)), dim3(kBlock), 0, s, sc, pb, hb, queue, qcount,
                       next_queue, next_count, hp_count, max_delta, pc);
}

void launch_ppm_emit(hipStream_t s, const SceneDev &sc, PathBuf pb, uint32_t *qcount, uint32_t n_photons, int spl,
                     uint64_t seed, uint32_t pass, PpmFrame fr){
    hipLaunchKernelGGL(k_ppm_emit, dim3(groups_for(n_photons)), dim3(kBlock), 0, s, sc, pb, qcount, n_photons, spl, seed, pass, fr);
}

void launch_ppm_photon_shade(hipStream_t s, const SceneDev &sc, PathBuf pb, PpmGrid g, const uint32_t *queue,
                             const uint32_t *qcount, uint32_t max_items, uint32_t *next_queue, uint32_t *next_count,
                             int light_depth, int max_delta, PpmFrame fr, PpmCounters *pc){
    hipLaunchKernelGGL(k_ppm_photon_shade, dim3(groups_for(max_items)), dim3(kBlock), 0, s, sc, pb, g, queue, qcount,
                       next_queue, next_count, light_depth, max_delta, fr, pc);
}

static int sort_end_bit(uint32_t buckets){
    int b = 0;
    while((1u << b) < buckets) ++b;
    return b + 1;                                  // the sentinel key (= buckets) needs one bit more
}

size_t ppm_sort_tmp_bytes(uint32_t n_slots, uint32_t buckets){
    size_t bytes = 0;
    rocprim::radix_sort_pairs(nullptr, bytes, (uint32_t *) nullptr, (uint32_t *) nullptr, (uint32_t *) nullptr, (uint32_t *) nullptr,
                              (size_t) n_slots, 0, sort_end_bit(buckets));
    return bytes;
}

int launch_ppm_grid(hipStream_t s, PpmGrid g, uint32_t n_slots){
    // LSD radix sort is stable and its input is in slot order: inside a bucket the slots stay ascending
    size_t bytes = g.sort_tmp_bytes;
    hipError_t e = rocprim::radix_sort_pairs(g.sort_tmp, bytes, g.key, g.key_sorted, g.slot_in, g.slot_sorted, (size_t) n_slots,
                                             0, sort_end_bit(g.buckets), s);
    if(e != hipSuccess) return 1;
    hipLaunchKernelGGL(k_ppm_ranges, dim3(groups_for(n_slots)), dim3(kBlock), 0, s, g, n_slots);
    return 0;
}

void launch_ppm_gather(hipStream_t s, const SceneDev &sc, PathBuf pb, PpmHitBuf hb, PpmGrid g, const uint32_t *hp_count,
                       uint32_t max_items, PpmFrame fr, uint32_t *cand, uint32_t *acc, PpmCounters *pc){
    if(cand) hipLaunchKernelGGL(k_ppm_gather<true>, dim3(groups_for(max_items)), dim3(kBlock), 0, s, sc, pb, hb, g, hp_count, fr, cand, acc, pc);
    else hipLaunchKernelGGL(k_ppm_gather<false>, dim3(groups_for(max_items)), dim3(kBlock), 0, s, sc, pb, hb, g, hp_count, fr, cand, acc, pc);
}

void launch_ppm_iota(hipStream_t s, uint32_t *p, uint32_t n){
    hipLaunchKernelGGL(k_ppm_iota, dim3(groups_for(n)), dim3(kBlock), 0, s, p, n);
}

void launch_sppm_init(hipStream_t s, SppmState st, uint32_t n_local, float r2){
    hipLaunchKernelGGL(k_sppm_init, dim3(groups_for(n_local)), dim3(kBlock), 0, s, st, n_local, r2);
}

void launch_sppm_gather(hipStream_t s, const SceneDev &sc, PpmHitBuf hb, PpmGrid g, const uint32_t *hp_count, uint32_t max_items,
                        PpmFrame fr, SppmState st, float alpha, uint32_t *cand, uint32_t *acc, PpmCounters *pc){
    if(cand) hipLaunchKernelGGL(k_sppm_gather<true>, dim3(groups_for(max_items)), dim3(kBlock), 0, s, sc, hb, g, hp_count, fr, st, alpha, cand, acc, pc);
    else hipLaunchKernelGGL(k_sppm_gather<false>, dim3(groups_for(max_items)), dim3(kBlock), 0, s, sc, hb, g, hp_count, fr, st, alpha, cand, acc, pc);
}

void launch_sppm_estimate(hipStream_t s, const Tiling &tl, SppmState st, float passes, float *d_local){
    hipLaunchKernelGGL(k_sppm_estimate, dim3(groups_for((uint32_t) tl.n_local)), dim3(kBlock), 0, s, tl, st, passes, d_local);
}

void launch_sppm_state(hipStream_t s, const Tiling &tl, SppmState st, float *d_local){
    hipLaunchKernelGGL(k_sppm_state, dim3(groups_for((uint32_t) tl.n_local)), dim3(kBlock), 0, s, tl, st, d_local);
}

} // namespace hpt
