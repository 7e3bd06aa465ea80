// TEST INFRASTRUCTURE ONLY -- CPU restatement of hpt_render_guides_motion (include/hpt.h, "motion"): guides_oracle_render's
// loop plus the previous geometry and the fifth sum.  Every hit point X on primitive `Hit::prim` (the global ordinal:
// below ns a sphere, from ns + nl up a triangle) adds Y, where X was one frame ago, to Pprev beside P.  Built by
// tests/motion_oracle.py with ppm_oracle.CXXFLAGS.
#include "ppm_oracle.cpp"

#include <cstring>

namespace {

// dot as the history defines it: a.x*b.x + a.y*b.y + a.z*b.z, left to right
inline float dot_lr(V3 a, V3 b){ return a.x * b.x + a.y * b.y + a.z * b.z; }

V3 previous_point(const Sc &sc, const RTriangle *ptris, const RSphere *pspheres, const Hit &h){
    const V3 X = h.pos;
    if(h.prim < sc.ns){
        const RSphere &s = sc.spheres[h.prim], &q = pspheres[h.prim];
        if(memcmp(&s, &q, 16) == 0) return X;
        const float k = q.r / s.r;
        return v3(q.center.x + (X.x - s.center.x) * k, q.center.y + (X.y - s.center.y) * k, q.center.z + (X.z - s.center.z) * k);
    }
    const int i = h.prim - sc.ns - sc.nl;
    const RTriangle &a = sc.tris[i], &b = ptris[i];
    if(memcmp(&a, &b, 36) == 0) return X;
    const V3 e1 = a.v1 - a.v0, e2 = a.v2 - a.v0, d = X - a.v0;
    const float d00 = dot_lr(e1, e1), d01 = dot_lr(e1, e2), d11 = dot_lr(e2, e2), d20 = dot_lr(d, e1), d21 = dot_lr(d, e2);
    const float den = d00 * d11 - d01 * d01;
    const float beta = (d11 * d20 - d01 * d21) / den, gamma = (d00 * d21 - d01 * d20) / den;
    const V3 f1 = b.v1 - b.v0, f2 = b.v2 - b.v0;
    return v3((b.v0.x + f1.x * beta) + f2.x * gamma, (b.v0.y + f1.y * beta) + f2.y * gamma, (b.v0.z + f1.z * beta) + f2.z * gamma);
}

} // namespace

// prev_tris / prev_spheres: nt / ns records with the layouts of tris / spheres (only vertices, centre and radius are
// read).  hit_points_out (optional, spp): hit points of every sample.  Any image may be null.
extern "C" int motion_oracle_render(const void *lights, int nl, const void *spheres, int ns, const void *tris, int nt,
                                    const void *prev_spheres, const void *prev_tris,
                                    const void *camera, int W, int H, int spp, uint64_t seed, int sample_offset, int max_delta,
                                    float *albedo, float *normal, float *position, float *coverage, float *prev_position,
                                    uint64_t *hit_points_out){
    Sc sc{ (const RLight *) lights, nl, (const RSphere *) spheres, ns, (const RTriangle *) tris, nt };
    const RTriangle *ptris = (const RTriangle *) prev_tris;
    const RSphere *pspheres = (const RSphere *) prev_spheres;
    const RCamera &cam = *(const RCamera *) camera;
    if(spp < 1) return 1;
    if(max_delta <= 0) max_delta = 64;
    if(max_delta > 250) max_delta = 250;
    const size_t npx = (size_t) W * H;
    std::vector<V3> A(npx, v3(0, 0, 0)), N(npx, v3(0, 0, 0)), P(npx, v3(0, 0, 0)), Q(npx, v3(0, 0, 0));
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
                    Q[idx] = Q[idx] + previous_point(sc, ptris, pspheres, h);
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
        V3 a = v3(0, 0, 0), n = a, p = a, q = a;
        if(Cn[k]){ a = A[k] / c; n = N[k] / c; p = P[k] / c; q = Q[k] / c; }
        if(albedo){ albedo[k * 3] = a.x; albedo[k * 3 + 1] = a.y; albedo[k * 3 + 2] = a.z; }
        if(normal){ normal[k * 3] = n.x; normal[k * 3 + 1] = n.y; normal[k * 3 + 2] = n.z; }
        if(position){ position[k * 3] = p.x; position[k * 3 + 1] = p.y; position[k * 3 + 2] = p.z; }
        if(coverage) coverage[k] = c;
        if(prev_position){ prev_position[k * 3] = q.x; prev_position[k * 3 + 1] = q.y; prev_position[k * 3 + 2] = q.z; }
    }
    return 0;
}
