// TEST INFRASTRUCTURE ONLY -- CPU restatement of the progressive photon-mapping estimator (include/hpt.h,
// hpt_sppm_*; DESIGN.md "Progressive photon mapping").  Built by tests/sppm_oracle.py with the flags of the PPM
// oracle, whose closest hit, hit-point and deposit records and cell_of it reuses; the eye and photon passes below
// restate ppm_oracle_render's op for op, so a pass's hit points and deposits are those of PPM's pass of that index.
//
// The state (R2, N, tau, D per pixel, row-major) belongs to the caller and is advanced in place; `cull` = 0 visits
// all 27 cells of every hit point instead of the cells its sphere can reach.
#include "ppm_oracle.cpp"

#include <cmath>

namespace {

// the cell offsets along one axis that a sphere of radius rho (in cells) around u can reach (sppm_axis, ppm_kernels.hip)
void sppm_axis(float h, float smin, float cell, float rho, int &lo, int &hi){
    const float u = (h - smin) / cell;
    const float au = fabsf(u);
    lo = -1; hi = 1;
    if(!(au < 1048576.0f)) return;
    const float fr = u - floorf(u);
    const float mg = 0.015625f + au * 9.5367431640625e-07f;
    if(!(fr < rho + mg)) lo = 0;
    if(!(fr > 1.0f - rho - mg)) hi = 0;
}

} // namespace

// state: r2[npx], n[npx], tau[npx * 3], d[npx * 3], *k (passes done), all updated.  image: the estimate after the
// call.  stats_out: photons, photon_rays, deposits, hit_points, direct_pixels, candidates, accepted (this call).
extern "C" int sppm_oracle_render(const void *lights, int nl, const void *spheres, int ns, const void *tris, int nt,
                                  const void *camera, int W, int H, int eye_depth, int light_depth, int spl, float radius, float alpha,
                                  const float *smin, const float *smax, uint64_t seed, int sample_offset, int max_delta,
                                  int passes, int cull, float *r2s, float *ns_, float *taus, float *ds, int64_t *k,
                                  float *image, uint64_t *stats_out){
    Sc sc{ (const RLight *) lights, nl, (const RSphere *) spheres, ns, (const RTriangle *) tris, nt };
    const RCamera &cam = *(const RCamera *) camera;
    if(max_delta <= 0) max_delta = 64;
    if(max_delta > 250) max_delta = 250;
    if(!(radius > 0.0f)) radius = 0.05f;
    const float cell = radius;
    const V3 mn = v3(smin[0], smin[1], smin[2]), mx = v3(smax[0], smax[1], smax[2]);
    const int n_ph = nl > 0 ? nl * spl : 0;
    const size_t npx = (size_t) W * H;
    std::vector<V3> img(npx);
    std::vector<HitPoint> hps(npx);
    std::vector<Deposit> deps((size_t) n_ph * light_depth);
    uint64_t st[7] = { 0, 0, 0, 0, 0, 0, 0 };
    for(int pass = 0; pass < passes; ++pass){
        const uint32_t pidx = (uint32_t) ((int64_t) sample_offset + *k);
        uint64_t direct = 0, nhp = 0, ndep = 0, rays = 0, ncand = 0, nacc = 0;
        // eye pass (ppm_oracle_render)
#pragma omp parallel for schedule(dynamic, 16) reduction(+:direct, nhp)
        for(int py = 0; py < H; ++py) for(int px = 0; px < W; ++px){
            const size_t idx = (size_t) py * W + px;
            HitPoint &hp = hps[idx]; hp.valid = false;
            img[idx] = v3(0, 0, 0);
            Pcg rng; rng.seed(seed ^ kEyeKey, (uint32_t) idx, pidx);
            float pixel_x = (float) px + rng.next();
            float pixel_y = (float) py + rng.next();
            V3 o = cam.eye;
            V3 pixel_pos = cam.UL + cam.dx * pixel_x + cam.dy * pixel_y;
            V3 d = normalize(pixel_pos - o);
            float eta = 1.0f;
            V3 thr = v3(1, 1, 1);
            int deltas = 0;
            for(int depth = 0; depth < eye_depth; depth++){
                Hit h = closest(sc, o, d);
                if(!h.hit) break;
                V3 wo = d * -1.0f;
                if(h.is_light){
                    V3 c = thr * h.mtl.base_color;
                    if(is_valid_color(c)){ img[idx] = clamp_radiance(c, 15.0f); ++direct; }
                    break;
                }
                float u_rr = rng.next(), u1 = rng.next(), u2 = rng.next();
                V3 wi, f; float pdf, new_eta; bool is_delta;
                bsdf_sample(0, h.mtl, wo, h.normal, u_rr, u1, u2, eta, wi, f, pdf, is_delta, new_eta);
                if(is_delta){
                    if(pdf <= 0.0f) break;
                    thr = thr * f;
                    d = wi; eta = new_eta;
                    o = h.pos + h.normal * (dot(wi, h.normal) < 0.0f ? -kEps : kEps);
                    if(!is_valid_color(thr)) break;
                    if(++deltas > max_delta) break;
                    depth--;
                    continue;
                }
                hp.valid = true; hp.pos = h.pos; hp.normal = h.normal; hp.wo = wo; hp.mtl = h.mtl; hp.thr = thr;
                ++nhp;
                break;
            }
        }
        // photon pass (ppm_oracle_render)
        for(Deposit &dp : deps) dp.valid = false;
#pragma omp parallel for schedule(dynamic, 64) reduction(+:ndep, rays)
        for(int i = 0; i < n_ph; ++i){
            Pcg rng; rng.seed(seed ^ kPhotonKey, (uint32_t) i, pidx);
            const RLight &L = sc.lights[i % nl];
            V3 w = normalize(L.dir);
            V3 u_vec = (fabsf(w.x) > 0.9f) ? v3(0, 1, 0) : v3(1, 0, 0);
            V3 v_vec = normalize(cross(w, u_vec));
            u_vec = normalize(cross(v_vec, w));
            V3 o, d;
            if(L.is_parallel){
                d = w;
                V3 center = (mn + mx) * 0.5f;
                float scene_radius = length(mx - mn) * 0.5f;
                float r1 = rng.next(), rr2 = rng.next();
                float plane = scene_radius * 2.0f;
                float offset_u = (r1 - 0.5f) * plane, offset_v = (rr2 - 0.5f) * plane;
                o = center - d * (scene_radius * 2.0f) + u_vec * offset_u + v_vec * offset_v;
            } else {
                float u1 = rng.next(), u2 = rng.next();
                float cos_t = 1.0f - u1 * (1.0f - cosf(L.cutoff));
                float sin_t = sqrtf(fmaxf(0.0f, 1.0f - cos_t * cos_t));
                float sp, cp; sincos_2pi_poly(u2, sp, cp);
                V3 ld = v3(sin_t * cp, sin_t * sp, cos_t);
                d = normalize(u_vec * ld.x + v_vec * ld.y + w * ld.z);
                o = L.pos + d * L.light_ball.r;
            }
            V3 flux = L.illum * (float) nl / fmaxf((float) spl, 1.0f);
            float eta = 1.0f;
            int deltas = 0;
            for(int depth = 0; depth < light_depth; depth++){
                Hit h = closest(sc, o, d);
                ++rays;
                if(!h.hit || h.is_light) break;
                V3 wi_light = d * -1.0f;
                if(h.mtl.eta <= 0.0f && (h.mtl.metallic < 0.99f || h.mtl.roughness > 0.01f)){
                    Deposit &dp = deps[(size_t) i * light_depth + depth];
                    dp.valid = true; dp.pos = h.pos; dp.normal = h.normal; dp.wi = wi_light; dp.flux = flux;
                    cell_of(h.pos, mn, cell, dp.cx, dp.cy, dp.cz);
                    ++ndep;
                }
                float u_rr = rng.next(), u1 = rng.next(), u2 = rng.next();
                V3 wi, f; float pdf, new_eta; bool is_delta;
                bsdf_sample(0, h.mtl, wi_light, h.normal, u_rr, u1, u2, eta, wi, f, pdf, is_delta, new_eta);
                if(pdf <= 0.0f) break;
                float cos_wi = fabsf(dot(h.normal, wi));
                if(is_delta){ flux = flux * f; depth--; }
                else flux = flux * f * cos_wi / pdf;
                if(!is_valid_color(flux)) break;
                if(is_delta && ++deltas > max_delta) break;
                d = wi; eta = new_eta;
                o = h.pos + h.normal * (dot(wi, h.normal) < 0.0f ? -kEps : kEps);
            }
        }
        // gather with the pixel's own radius, the cull, and the update
        Grid grid;
        grid.build(deps);
#pragma omp parallel for schedule(dynamic, 16) reduction(+:ncand, nacc)
        for(int64_t idx = 0; idx < (int64_t) npx; ++idx){
            // D += the guarded direct term (k_resolve)
            V3 c = img[idx];
            if(!is_valid_color(c)) c = v3(0, 0, 0);
            ds[idx * 3 + 0] = ds[idx * 3 + 0] + c.x; ds[idx * 3 + 1] = ds[idx * 3 + 1] + c.y; ds[idx * 3 + 2] = ds[idx * 3 + 2] + c.z;
            const HitPoint &hp = hps[idx];
            if(!hp.valid) continue;
            const float r2 = r2s[idx];
            int cx, cy, cz;
            cell_of(hp.pos, mn, cell, cx, cy, cz);
            int x0 = -1, x1 = 1, y0 = -1, y1 = 1, z0 = -1, z1 = 1;
            if(cull){
                const float rho = sqrtf(r2) / cell;
                sppm_axis(hp.pos.x, mn.x, cell, rho, x0, x1);
                sppm_axis(hp.pos.y, mn.y, cell, rho, y0, y1);
                sppm_axis(hp.pos.z, mn.z, cell, rho, z0, z1);
            }
            V3 acc = v3(0, 0, 0);
            uint32_t m = 0;
            for(int z = z0; z <= z1; z++) for(int y = y0; y <= y1; y++) for(int x = x0; x <= x1; x++){
                auto run = grid.cell(cx + x, cy + y, cz + z);
                for(const Grid::E *q = run.first; q != run.second; ++q){
                    const Deposit &dp = deps[q->slot];
                    ++ncand;
                    if(!(dot(hp.normal, dp.normal) > 0.01f)) continue;
                    V3 dd = hp.pos - dp.pos;
                    if(!(dot(dd, dd) < r2)) continue;
                    ++nacc;
                    V3 brdf = bsdf_evaluate(hp.mtl, hp.wo, dp.wi, hp.normal);
                    if(is_valid_color(brdf)){ acc = acc + dp.flux * brdf * hp.thr; ++m; }
                }
            }
            if(m > 0){
                const float mf = (float) m;
                const float n_old = ns_[idx];
                const float n_new = n_old + alpha * mf;
                const float ratio = n_new / (n_old + mf);
                V3 tau = (v3(taus[idx * 3], taus[idx * 3 + 1], taus[idx * 3 + 2]) + acc) * ratio;
                taus[idx * 3 + 0] = tau.x; taus[idx * 3 + 1] = tau.y; taus[idx * 3 + 2] = tau.z;
                r2s[idx] = r2 * ratio;
                ns_[idx] = n_new;
            }
        }
        *k += 1;
        st[0] += (uint64_t) n_ph; st[1] += rays; st[2] += ndep; st[3] += nhp; st[4] += direct; st[5] += ncand; st[6] += nacc;
    }
    // the estimate
    const float kf = (float) *k;
    for(size_t q = 0; q < npx; ++q){
        V3 d = v3(ds[q * 3], ds[q * 3 + 1], ds[q * 3 + 2]);
        V3 p = v3(taus[q * 3], taus[q * 3 + 1], taus[q * 3 + 2]) / fmaxf(kPi * r2s[q], 1e-6f);
        if(*k != 1){ d = d / kf; p = p / kf; }
        V3 v = is_valid_color(p) ? d + clamp_radiance(p, 15.0f) : d;
        image[q * 3] = v.x; image[q * 3 + 1] = v.y; image[q * 3 + 2] = v.z;
    }
    if(stats_out) for(int q = 0; q < 7; ++q) stats_out[q] = st[q];
    return 0;
}
