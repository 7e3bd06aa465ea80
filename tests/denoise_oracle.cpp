// TEST INFRASTRUCTURE ONLY -- CPU restatement of the edge-avoiding a-trous filter as include/hpt.h ("guides and
// denoiser") defines it: every operation an IEEE float operation in the order written there.  Built by
// tests/denoise_oracle.py with ppm_oracle.CXXFLAGS (-ffp-contract=off), so the HIP kernels must match it bit for bit.
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

namespace {

struct C3 { float x, y, z; };

float falloff(float x){
    float q = fmaxf(0.0f, 1.0f - x * 0.125f);
    q *= q; q *= q; q *= q;
    return q;
}

// the clamp keeps 0 * inv at the centre tap from being 0 * inf
float inv_sq(float s){ return fminf(1.0f / (s * s), FLT_MAX); }

} // namespace

// flags: 1 demodulate.  sigma < 0: term off; 0: the default (1.0, 0.5, 0.05); iterations 0 -> 5.
// levels_out (optional, (iterations + 1) * W*H*3 floats): c_0 .. c_n, before re-modulation.
extern "C" int denoise_oracle_run(const float *colour, const float *albedo, const float *normal, const float *position,
                                  const float *coverage, float *out, int W, int H, int iterations, float sigma_color,
                                  float sigma_normal, float sigma_position, int flags, float *levels_out){
    if(W <= 0 || H <= 0 || iterations < 0 || iterations > 8) return 1;
    if(iterations == 0) iterations = 5;
    if(sigma_color == 0.0f) sigma_color = 1.0f;
    if(sigma_normal == 0.0f) sigma_normal = 0.5f;
    if(sigma_position == 0.0f) sigma_position = 0.05f;
    const bool demod = (flags & 1) != 0, use_c = sigma_color > 0.0f, use_n = sigma_normal > 0.0f, use_p = sigma_position > 0.0f;
    const size_t npx = (size_t) W * H;
    const float h[5] = { 0.0625f, 0.25f, 0.375f, 0.25f, 0.0625f };
    std::vector<C3> a(npx), cur(npx), nxt(npx);
    auto valid = [&](size_t p){ return coverage[p] > 0.0f; };
    for(size_t p = 0; p < npx; ++p){
        a[p] = C3{ fmaxf(albedo[p * 3], 1e-3f), fmaxf(albedo[p * 3 + 1], 1e-3f), fmaxf(albedo[p * 3 + 2], 1e-3f) };
        C3 c{ colour[p * 3], colour[p * 3 + 1], colour[p * 3 + 2] };
        if(demod && valid(p)) c = C3{ c.x / a[p].x, c.y / a[p].y, c.z / a[p].z };
        cur[p] = c;
    }
    auto keep = [&](int level){ if(levels_out) memcpy(levels_out + (size_t) level * npx * 3, cur.data(), npx * 3 * sizeof(float)); };
    keep(0);
    const float inv_n = use_n ? inv_sq(sigma_normal) : 0.0f;
    const float inv_p = use_p ? inv_sq(sigma_position) : 0.0f;
    for(int k = 0; k < iterations; ++k){
        const int s = 1 << k;
        const float sc = sigma_color * ldexpf(1.0f, -k);
        const float inv_c = use_c ? inv_sq(sc) : 0.0f;
#pragma omp parallel for schedule(static)
        for(int y = 0; y < H; ++y) for(int x = 0; x < W; ++x){
            const size_t p = (size_t) y * W + x;
            if(!valid(p)){ nxt[p] = cur[p]; continue; }
            const C3 cp = cur[p];
            const float *np = normal + p * 3, *pp = position + p * 3;
            float sx = 0.0f, sy = 0.0f, sz = 0.0f, wsum = 0.0f;
            bool others = false;
            for(int j = -2; j <= 2; ++j) for(int i = -2; i <= 2; ++i){
                const int qx = x + i * s, qy = y + j * s;
                if(qx < 0 || qx >= W || qy < 0 || qy >= H) continue;
                const size_t q = (size_t) qy * W + qx;
                if(!valid(q)) continue;
                const C3 cq = cur[q];
                if(i != 0 || j != 0) others = true;
                const float *nq = normal + q * 3, *pq = position + q * 3;
                float ec = 1.0f, en = 1.0f, ep = 1.0f;
                if(use_c){
                    const float dx = cp.x - cq.x, dy = cp.y - cq.y, dz = cp.z - cq.z;
                    ec = falloff((dx * dx + dy * dy + dz * dz) * inv_c);
                }
                if(use_n){
                    const float dx = np[0] - nq[0], dy = np[1] - nq[1], dz = np[2] - nq[2];
                    en = falloff((dx * dx + dy * dy + dz * dz) * inv_n);
                }
                if(use_p){
                    const float t = np[0] * (pq[0] - pp[0]) + np[1] * (pq[1] - pp[1]) + np[2] * (pq[2] - pp[2]);
                    ep = falloff(t * t * inv_p);
                }
                const float w = h[j + 2] * h[i + 2] * ec * en * ep;
                sx = sx + cq.x * w; sy = sy + cq.y * w; sz = sz + cq.z * w;
                wsum = wsum + w;
            }
            // every tap but the centre's skipped: the pixel keeps its value (fl(fl(c * 9/64) / (9/64)) is not always c)
            nxt[p] = others ? C3{ sx / wsum, sy / wsum, sz / wsum } : cp;
        }
        cur.swap(nxt);
        keep(k + 1);
    }
    for(size_t p = 0; p < npx; ++p){
        C3 c = cur[p];
        if(!valid(p)) c = C3{ colour[p * 3], colour[p * 3 + 1], colour[p * 3 + 2] };
        else if(demod) c = C3{ c.x * a[p].x, c.y * a[p].y, c.z * a[p].z };
        out[p * 3] = c.x; out[p * 3 + 1] = c.y; out[p * 3 + 2] = c.z;
    }
    return 0;
}
