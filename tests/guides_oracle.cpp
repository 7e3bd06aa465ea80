// TEST INFRASTRUCTURE ONLY -- CPU restatement of hpt_render_guides (include/hpt.h, "guides and denoiser"): photon
// mapping's eye pass per sample, restated from ppm_oracle_render's loop with its closest hit, stream key and material
// rules, and the per-pixel sums over the samples.  Built by tests/guides_oracle.py with ppm_oracle.CXXFLAGS.
#include "ppm_oracle.cpp"

// hit_points_out (optional, spp): hit points of every sample.  Any image may be null.
extern "C" int guides_oracle_render(const void *lights, int nl, const void *spheres, int ns, const void *tris, int nt,
                                    const void *camera, int W, int H, int spp, uint64_t seed, int sample_offset, int max_delta,
                                    float *albedo, float *normal, float *position, float *coverage, uint64_t *hit_points_out){
    Sc sc{ (const RLight *) lights, nl, (const RSphere *) spheres, ns, (const RTriangle *) tris, nt };
    const RCamera &cam = *(const RCamera *) camera;
    if(spp < 1) return 1;
    if(max_delta <= 0) max_delta = 64;
    if(max_delta > 250) max_delta = 250;
    const size_t npx = (size_t) W * H;
    std::vector<V3> A(npx, v3(0, 0, 0)), N(npx, v3(0, 0, 0)), P(npx, v3(0, 0, 0));
    std::vector<uint32_t> Cn(npx, 0u);
    for(int s = 0; s < spp; ++s){
        const uint32_t pidx = (uint32_t) ((int64_t) sample_offset + s);
        uint64_t nhp = 0;
#pragma omp parallel for schedule(dynamic, 16) reduction(+:nhp)
        for(int py = 0; py < H; ++py) for(int px = 0; px < W; ++px){
            const size_t idx = (size_t) py * W + px;
            Pcg rng; rng.seed(seed ^ kEyeKey, (uint32_t) idx, pidx);
            float pixel_x = (float) px + rng.next();
            float pixel_y = (float) py + rng.next();
            V3 o = cam.eye;
            V3 d = normalize(cam.UL + cam.dx * pixel_x + cam.dy * pixel_y - o);
            float eta = 1.0f;
            V3 thr = v3(1, 1, 1);
            int deltas = 0;
            for(;;){
                Hit h = closest(sc, o, d);
                if(!h.hit || h.is_light) break;
                V3 wo = d * -1.0f;
                float u_rr = rng.next(), u1 = rng.next(), u2 = rng.next();
                V3 wi, f; float pdf, new_eta; bool is_delta;
                bsdf_sample(0, h.mtl, wo, h.normal, u_rr, u1, u2, eta, wi, f, pdf, is_delta, new_eta);
                if(!is_delta){
                    A[idx] = A[idx] + h.mtl.base_color; N[idx] = N[idx] + h.normal; P[idx] = P[idx] + h.pos;
                    ++Cn[idx]; ++nhp;
                    break;
                }
                if(pdf <= 0.0f) break;
                thr = thr * f;
                d = wi; eta = new_eta;
                o = h.pos + h.normal * (dot(wi, h.normal) < 0.0f ? -kEps : kEps);
                if(!is_valid_color(thr)) break;
                if(++deltas > max_delta) break;
            }
        }
        if(hit_points_out) hit_points_out[s] = nhp;
    }
    for(size_t k = 0; k < npx; ++k){
        const float c = (float) Cn[k];
        V3 a = v3(0, 0, 0), n = a, p = a;
        if(Cn[k]){ a = A[k] / c; n = N[k] / c; p = P[k] / c; }
        if(albedo){ albedo[k * 3] = a.x; albedo[k * 3 + 1] = a.y; albedo[k * 3 + 2] = a.z; }
        if(normal){ normal[k * 3] = n.x; normal[k * 3 + 1] = n.y; normal[k * 3 + 2] = n.z; }
        if(position){ position[k * 3] = p.x; position[k * 3 + 1] = p.y; position[k * 3 + 2] = p.z; }
        if(coverage) coverage[k] = c;
    }
    return 0;
}
