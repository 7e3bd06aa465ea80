// HIP kernels of the variance-guided filter (include/hpt.h, "variance-guided filtering"), written for gfx950 (MI355X).
//
//   k_guided_pack        c_0 of the plain filter with the scalar variance v_0 in the record's fourth word.
//   k_atrous_guided      one level per launch, one lane per pixel, the 64 x 4 workgroup of k_atrous: a wave holds 64
//                        consecutive pixels of one row, so each of the 25 taps is three loads of 64 consecutive 16-byte
//                        records, and the variance comes with the colour record.  Before the taps, nine loads of c_in at
//                        stride 1 (the 3 x 3 prefilter of the variance) set the pixel's colour tolerance.
//   k_variance_spatial   the 7 x 7 weighted variance of one frame: 49 taps of one 12-byte colour and two guide records.
//   k_take_fourth_word   the history's length image out of its {mean, n} records.
//
// Everything is IEEE float arithmetic evaluated as written (-ffp-contract=off, correctly rounded divide), with no
// transcendental, no square root, no LDS and no atomic: tests/guided_oracle.py gives the same bits.
#include "guided_kernels.h"
#include "pt_device_math.h"

#include <cfloat>

namespace hpt {

namespace {

// e(x) and the B3 taps of the plain filter (denoise_kernels.hip)
HPT_DEV float falloff(float x){
    float q = fmaxf(0.0f, 1.0f - x * 0.125f);
    q *= q; q *= q; q *= q;
    return q;
}
HPT_DEV float tap(int k){ return (k == 0 || k == 4) ? 0.0625f : (k == 2 ? 0.375f : 0.25f); }
// taps of the variance prefilter
HPT_DEV float gtap(int k){ return k == 1 ? 0.5f : 0.25f; }

constexpr int kTileX = 64, kTileY = 4;       // pixels of a 256-thread workgroup, as k_atrous

__global__ __launch_bounds__(kBlock)
void k_guided_pack(const float *rgb, const float *var, DenoiseGuides g, float4 *c0, size_t n, int demod){
    const size_t p = (size_t) blockIdx.x * kBlock + threadIdx.x;
    if(p >= n) return;
    float x = rgb[p * 3], y = rgb[p * 3 + 1], z = rgb[p * 3 + 2];
    const float vr = var[p * 3], vg = var[p * 3 + 1], vb = var[p * 3 + 2];
    float v;
    if(demod && g.nrm_cov[p].w > 0.0f){
        const float4 a = g.alb[p];
        x = x / a.x; y = y / a.y; z = z / a.z;
        v = fmaxf(vr / (a.x * a.x) + vg / (a.y * a.y) + vb / (a.z * a.z), 0.0f);
    } else {
        v = fmaxf(vr + vg + vb, 0.0f);
    }
    c0[p] = make_float4(x, y, z, v);
}

template <bool LAST>
__global__ __launch_bounds__(kBlock)
void k_atrous_guided(GuidedLevel L, DenoiseGuides g, const float4 *c_in, float4 *c_out, float *out, float *var_out){
    const int x = (int) (blockIdx.x * kTileX + (threadIdx.x & 63u));
    const int y = (int) (blockIdx.y * kTileY + (threadIdx.x >> 6));
    if(x >= L.W || y >= L.H) return;
    const size_t p = (size_t) y * (size_t) L.W + (size_t) x;
    const float4 cp = c_in[p], np = g.nrm_cov[p];
    float rx = cp.x, ry = cp.y, rz = cp.z, rv = cp.w;
    const bool valid = np.w > 0.0f;
    if(valid){
        const float4 pp = g.pos[p];
        float inv_c = 0.0f;
        if(L.use_c){
            float num = 0.0f, den = 0.0f;
#pragma unroll
            for(int j = -1; j <= 1; ++j){
                const int qy = y + j;
#pragma unroll
                for(int i = -1; i <= 1; ++i){
                    const int qx = x + i;
                    if(qx < 0 || qx >= L.W || qy < 0 || qy >= L.H) continue;
                    const size_t q = (size_t) qy * (size_t) L.W + (size_t) qx;
                    if(!(g.nrm_cov[q].w > 0.0f)) continue;
                    const float gw = gtap(j + 1) * gtap(i + 1);
                    num = num + c_in[q].w * gw;
                    den = den + gw;
                }
            }
            const float vbar = num / den;
            inv_c = fminf(1.0f / (L.s2 * vbar + 1e-12f), FLT_MAX);
        }
        float sx = 0.0f, sy = 0.0f, sz = 0.0f, vsum = 0.0f, wsum = 0.0f;
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
                    ec = falloff((dx * dx + dy * dy + dz * dz) * inv_c);
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
                vsum = vsum + cq.w * (w * w);
                wsum = wsum + w;
            }
        }
        // a pixel that stands alone keeps colour and variance (the plain filter's rule, include/hpt.h)
        if(others){ rx = sx / wsum; ry = sy / wsum; rz = sz / wsum; rv = vsum / (wsum * wsum); }
    }
    if(LAST){
        if(L.demod && valid){
            const float4 a = g.alb[p];
            rx = rx * a.x; ry = ry * a.y; rz = rz * a.z;
        }
        out[p * 3 + 0] = rx; out[p * 3 + 1] = ry; out[p * 3 + 2] = rz;
        if(var_out) var_out[p] = rv;
    } else {
        c_out[p] = make_float4(rx, ry, rz, rv);
    }
}

__global__ __launch_bounds__(kBlock)
void k_variance_spatial(VarianceArgs A, DenoiseGuides g){
    const int x = (int) (blockIdx.x * kTileX + (threadIdx.x & 63u));
    const int y = (int) (blockIdx.y * kTileY + (threadIdx.x >> 6));
    if(x >= A.W || y >= A.H) return;
    const size_t p = (size_t) y * (size_t) A.W + (size_t) x;
    const float4 np = g.nrm_cov[p];
    float vx = 0.0f, vy = 0.0f, vz = 0.0f;
    if(np.w > 0.0f){
        const float4 pp = g.pos[p];
        float sx = 0.0f, sy = 0.0f, sz = 0.0f, tx = 0.0f, ty = 0.0f, tz = 0.0f, ws = 0.0f;
#pragma unroll
        for(int j = -3; j <= 3; ++j){
            const int qy = y + j;
#pragma unroll
            for(int i = -3; i <= 3; ++i){
                const int qx = x + i;
                if(qx < 0 || qx >= A.W || qy < 0 || qy >= A.H) continue;
                const size_t q = (size_t) qy * (size_t) A.W + (size_t) qx;
                const float4 nq = g.nrm_cov[q];
                if(!(nq.w > 0.0f)) continue;
                float en = 1.0f, ep = 1.0f;
                if(A.use_n){
                    const float dx = np.x - nq.x, dy = np.y - nq.y, dz = np.z - nq.z;
                    en = falloff((dx * dx + dy * dy + dz * dz) * A.inv_n);
                }
                if(A.use_p){
                    const float4 pq = g.pos[q];
                    const float t = np.x * (pq.x - pp.x) + np.y * (pq.y - pp.y) + np.z * (pq.z - pp.z);
                    ep = falloff(t * t * A.inv_p);
                }
                const float w = en * ep;
                const float cx = A.frame[q * 3], cy = A.frame[q * 3 + 1], cz = A.frame[q * 3 + 2];
                sx = sx + cx * w; sy = sy + cy * w; sz = sz + cz * w;
                tx = tx + (cx * cx) * w; ty = ty + (cy * cy) * w; tz = tz + (cz * cz) * w;
                ws = ws + w;
            }
        }
        const float mx = sx / ws, my = sy / ws, mz = sz / ws;
        vx = fmaxf(tx / ws - mx * mx, 0.0f);
        vy = fmaxf(ty / ws - my * my, 0.0f);
        vz = fmaxf(tz / ws - mz * mz, 0.0f);
        if(A.length){
            const float n = fmaxf(A.length[p], 1.0f);
            vx = vx / n; vy = vy / n; vz = vz / n;
        }
    }
    A.out[p * 3 + 0] = vx; A.out[p * 3 + 1] = vy; A.out[p * 3 + 2] = vz;
}

__global__ __launch_bounds__(kBlock)
void k_take_fourth_word(const float4 *records, float *out, size_t n){
    const size_t p = (size_t) blockIdx.x * kBlock + threadIdx.x;
    if(p < n) out[p] = records[p].w;
}

inline uint32_t blocks_for(size_t n){ return (uint32_t) ((n + kBlock - 1) / kBlock); }
inline dim3 tiles_for(int W, int H){ return dim3((uint32_t) ((W + kTileX - 1) / kTileX), (uint32_t) ((H + kTileY - 1) / kTileY)); }

} // namespace

void launch_guided_pack(hipStream_t s, const float *linear_rgb, const float *variance, DenoiseGuides g, float4 *c0, size_t num_pixels, int demod){
    hipLaunchKernelGGL(k_guided_pack, dim3(blocks_for(num_pixels)), dim3(kBlock), 0, s, linear_rgb, variance, g, c0, num_pixels, demod);
}

void launch_atrous_guided(hipStream_t s, const GuidedLevel &L, DenoiseGuides g, const float4 *c_in, float4 *c_out, float *out, float *var_out, int last){
    const dim3 grid = tiles_for(L.W, L.H);
    if(last) hipLaunchKernelGGL(k_atrous_guided<true>, grid, dim3(kBlock), 0, s, L, g, c_in, c_out, out, var_out);
    else hipLaunchKernelGGL(k_atrous_guided<false>, grid, dim3(kBlock), 0, s, L, g, c_in, c_out, out, var_out);
}

void launch_variance_spatial(hipStream_t s, const VarianceArgs &a, DenoiseGuides g){
    hipLaunchKernelGGL(k_variance_spatial, tiles_for(a.W, a.H), dim3(kBlock), 0, s, a, g);
}

void launch_take_fourth_word(hipStream_t s, const float4 *records, float *out, size_t n){
    hipLaunchKernelGGL(k_take_fourth_word, dim3(blocks_for(n)), dim3(kBlock), 0, s, records, out, n);
}

} // namespace hpt
