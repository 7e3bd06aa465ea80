// The frame-side kernels of the path-tracing pipeline (pt_kernels.h) for gfx950: what runs per pass, per image or per scene around the trace /
// shade loop -- generate, resolve, finalize, untile, the 8-bit tone map, the per-triangle shading frames -- and the tests' function-level probe.
#include "pt_device_common.h"

namespace hpt {

namespace {

__global__ __launch_bounds__(kBlock)
void k_generate(Tiling tl, CameraDev cam, PathBuf pb, uint32_t *qcount,
                uint32_t total, uint32_t first_sample, uint64_t seed, WorkCounters *wc){
    // Slot i is path i: the first iteration's queue is the identity, so no compaction (and no
    // atomics) here.  Slots outside the image are marked dead (flag bit 1) and never traced.
    if(blockIdx.x == 0 && threadIdx.x == 0) *qcount = total;
    uint32_t stride = gridDim.x * kBlock;
    for(uint32_t i = blockIdx.x * kBlock + threadIdx.x; i < total; i += stride){
        PrimaryGen g; g.tl = tl; g.cam = cam; g.first_sample = first_sample; g.pad = 0u; g.seed = seed;
        f3 eye = mk3(0, 0, 0), dir = mk3(0, 0, 1); uint64_t rs = 0ull;
        bool active = primary_ray(g, i, eye, dir, rs);
        if(active){
            pb.org_eta[i] = make_float4(eye.x, eye.y, eye.z, 1.0f);
            pb.dir_flags[i] = make_float4(dir.x, dir.y, dir.z, u2f(1u));      // last_is_delta = true, depth 0
            pb.thr[i] = make_float4(1.0f, 1.0f, 1.0f, 0.0f);
            pb.rng[i] = make_uint2((uint32_t) rs, (uint32_t) (rs >> 32));
        } else {
            pb.dir_flags[i] = make_float4(0.0f, 0.0f, 1.0f, u2f(2u));         // dead slot
            pb.hit[i] = make_uint2(f2u(1e20f), kHitMiss);
        }
        pb.col[i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if(wc){
            unsigned long long m = __ballot(active);
            if((threadIdx.x & 63u) == 0u && m) atomicAdd(&wc->samples, (unsigned long long) __popcll(m));
        }
    }
}

// accum[p] += sum over this pass's samples, in sample order, after the per-sample guard
__global__ __launch_bounds__(kBlock)
void k_resolve(Tiling tl, PathBuf pb, float4 *accum, int samples){
    uint32_t p = blockIdx.x * kBlock + threadIdx.x;
    if(p >= (uint32_t) tl.n_local) return;
    float4 a = accum[p];
    f3 sum = mk3(a.x, a.y, a.z);
    for(int j = 0; j < samples; ++j){
        float4 c4 = pb.col[(size_t) j * tl.n_local + p];
        f3 c = xyz(c4);
        if(!is_valid_color(c)) c = mk3(0, 0, 0);            // pt_cu.cu:243
        sum = sum + c;                                      // pt_cu.cu:245
    }
    accum[p] = make_float4(sum.x, sum.y, sum.z, 0.0f);
}

// Per triangle, once per scene: the unit normal of pt_cu.cu's hit record (normalize(cross(e1, e2)),
// geometric.cuh:286) and the local shading frame of geometric.cuh:421-424 for both orientations of
// that normal (the shading normal is flipped against the ray).  Computed here, on the device, with the
// functions k_shade would otherwise run per hit, so the values are the same bit for bit.
//   q0 = N.xyz T.x | q1 = T.yz B.xy | q2 = B.z T'.xyz | q3 = B'.xyz material   (T', B': frame of -N)
__global__ __launch_bounds__(kBlock)
void k_tri_frames(const float4 *tris, int num_tris, float4 *frames){
    int i = blockIdx.x * kBlock + threadIdx.x;
    if(i >= num_tris) return;
    float4 t1 = tris[(size_t) i * 3 + 1], t2 = tris[(size_t) i * 3 + 2];
    f3 n = normalize3(cross3(xyz(t1), xyz(t2)));
    f3 T, B, T2, B2;
    build_local_frame(n, T, B);
    build_local_frame(n * -1.0f, T2, B2);
    frames[(size_t) i * 4 + 0] = make_float4(n.x, n.y, n.z, T.x);
    frames[(size_t) i * 4 + 1] = make_float4(T.y, T.z, B.x, B.y);
    frames[(size_t) i * 4 + 2] = make_float4(B.z, T2.x, T2.y, T2.z);
    frames[(size_t) i * 4 + 3] = make_float4(B2.x, B2.y, B2.z, t1.w);
}

// d_local[p] = accum[p] / spp (scale_is_div) -- pt_cu.cu:248
__global__ __launch_bounds__(kBlock)
void k_finalize(Tiling tl, const float4 *accum, float *d_local, float divisor){
    uint32_t p = blockIdx.x * kBlock + threadIdx.x;
    if(p >= (uint32_t) tl.n_local) return;
    float4 a = accum[p];
    f3 v = mk3(a.x, a.y, a.z);
    if(divisor != 1.0f) v = v / divisor;
    d_local[(size_t) p * 3 + 0] = v.x;
    d_local[(size_t) p * 3 + 1] = v.y;
    d_local[(size_t) p * 3 + 2] = v.z;
}

// row-major image <- [rank][local slot] packed buffers
__global__ __launch_bounds__(kBlock)
void k_untile(Tiling tl, const float *gathered, float *image){
    uint32_t idx = blockIdx.x * kBlock + threadIdx.x;
    if(idx >= (uint32_t) (tl.W * tl.H)) return;
    uint32_t x = idx % (uint32_t) tl.W, y = idx / (uint32_t) tl.W;
    uint32_t ts = (uint32_t) tl.tile;
    uint32_t tx = x / ts, ty = y / ts;
    uint32_t gt = ty * (uint32_t) tl.tiles_x + (tx + (uint32_t) tl.tiles_x - ty % (uint32_t) tl.tiles_x) % (uint32_t) tl.tiles_x;   // inverse of tile_to_pixel's row rotation
    uint32_t r = gt % (uint32_t) tl.world, lt = gt / (uint32_t) tl.world;
    uint32_t bx = (x % ts) >> 3, by = (y % ts) >> 3;
    uint32_t l = ((y & 7u) << 3) | (x & 7u);
    uint32_t q = (by * (ts >> 3) + bx) * 64u + l;
    size_t src = ((size_t) r * tl.n_local + (size_t) lt * ts * ts + q) * 3;
    size_t dst = (size_t) idx * 3;
    image[dst + 0] = gathered[src + 0];
    image[dst + 1] = gathered[src + 1];
    image[dst + 2] = gathered[src + 2];
}

// 8-bit output stage of the reference CLI (src/main_cli.cpp:227-242): per channel clamp to [0, 1], pow(x, 1/2.2),
// x 255, truncate.  byte(x) is a non-decreasing step function of x, so the device does not evaluate powf at all:
// thr[k] (k = 1..255) is the smallest float whose byte is >= k, found on the HOST with the host's own powf
// (hpt_api.cpp, tonemap_thresholds), and the byte is the number of thresholds <= x -- eight steps of a binary
// search in LDS.  The bytes are therefore exactly what the reference's host loop produces with the same libm;
// NaN compares false everywhere and lands on 0, which is where std::max(0.0f, std::min(NaN, 1.0f)) sends it.
// One thread packs four consecutive output bytes; bgr = 1 writes the reference's cv::Vec3b channel order.
__global__ __launch_bounds__(kBlock)
void k_tonemap(const float *linear, uint32_t *out_words, unsigned long long num_values, int bgr, const float *thr_table){
    __shared__ float s_thr[256];
    s_thr[threadIdx.x] = thr_table[threadIdx.x];
    __syncthreads();
    unsigned long long w = (unsigned long long) blockIdx.x * kBlock + threadIdx.x;
    unsigned long long first = w * 4ull;
    if(first >= num_values) return;
    uint32_t packed = 0u;
    for(int k = 0; k < 4; ++k){
        unsigned long long j = first + (unsigned long long) k;
        if(j >= num_values) break;
        unsigned long long src = j;
        if(bgr){ unsigned long long px = j / 3ull; src = px * 3ull + (2ull - (j - px * 3ull)); }
        float x = linear[src];
        uint32_t lo = 0u;
        for(uint32_t step = 128u; step > 0u; step >>= 1) if(x >= s_thr[lo + step]) lo += step;   // s_thr[0] unused (byte >= 0 always)
        packed |= lo << (8 * k);
    }
    if(first + 4ull <= num_values) out_words[w] = packed;
    else {
        unsigned char *tail = (unsigned char *) out_words + first;
        for(unsigned long long k = 0; first + k < num_values; ++k) tail[k] = (unsigned char) (packed >> (8 * k));
    }
}

// Function-level probe (tests): the device versions of the reference's BSDF / Fresnel / GGX / frame
// functions (reference include/geometric.cuh:119-235, 419-562) on caller-given inputs, called the way k_shade calls
// them -- one shared ShadeCtx per hit, the merged value+pdf query, the precomputed diffuse lobe and Lambda(wo).
// in:  24 floats per record   0-5 material (base rgb, roughness, metallic, eta) | 6-8 N | 9-11 wo | 12-14 wi |
//                             15-17 u_rr u1 u2 | 18 current eta | 19 cosI | 20 etaI | 21 etaT
// out: 40 floats per record   0-2 f(wo, wi) 3 pdf | 4-6 sampled wi 7-9 f 10 pdf 11 is_delta 12 new_eta |
//                             13 FrDielectric(cosI, etaI, etaT) 14-16 FrSchlick(cosI, base) | 17 D(wi_l) 18 Lambda(wi_l)
//                             19 G(wo_l, wi_l) | 20 sin 21 cos of 2 pi u2 | 22-24 visible normal | 25 is_valid_color(f)
//                             26-28 clamp_radiance(20 f, 15) | 29-31 T 32-34 B of the local frame | 35-37 wo in that frame
__global__ __launch_bounds__(kBlock)
void k_probe_functions(const float *in, int n, float *out){
    int i = blockIdx.x * kBlock + threadIdx.x;
    if(i >= n) return;
    const float *r = in + (size_t) i * 24;
    float *o = out + (size_t) i * 40;
    Mat m; m.base = mk3(r[0], r[1], r[2]); m.roughness = r[3]; m.metallic = r[4]; m.eta = r[5];
    f3 N = mk3(r[6], r[7], r[8]), wo_w = mk3(r[9], r[10], r[11]), wi_w = mk3(r[12], r[13], r[14]);
    ShadeCtx ctx = make_shade_ctx(N, wo_w);
    ShadePre pre;
    pre.diffuse = m.base / kPi * (1.0f - m.metallic);
    const float alpha = roughness_to_alpha(m.roughness);
    pre.lam_o = ggx_lambda(ctx.wo, alpha);
    f3 f; float pdf;
    bsdf_eval_pdf(m, ctx, wi_w, f, pdf, &pre);
    o[0] = f.x; o[1] = f.y; o[2] = f.z; o[3] = pdf;
    f3 swi, sf; float spdf, new_eta; bool is_delta;
    bsdf_sample(m, ctx, r[15], r[16], r[17], r[18], swi, sf, spdf, is_delta, new_eta, &pre);
    o[4] = swi.x; o[5] = swi.y; o[6] = swi.z; o[7] = sf.x; o[8] = sf.y; o[9] = sf.z; o[10] = spdf;
    o[11] = is_delta ? 1.0f : 0.0f; o[12] = new_eta;
    o[13] = fr_dielectric(r[19], r[20], r[21]);
    f3 sch = fr_schlick(r[19], m.base);
    o[14] = sch.x; o[15] = sch.y; o[16] = sch.z;
    f3 wi_l = to_local(wi_w, ctx.T, ctx.B, ctx.N);
    o[17] = ggx_D(wi_l, alpha); o[18] = ggx_lambda(wi_l, alpha); o[19] = ggx_G(ctx.wo, wi_l, alpha);
    float sn, cs; sincos_2pi(r[17], sn, cs);
    o[20] = sn; o[21] = cs;
    f3 vn = sample_visible_normal(ctx.wo.z > 0 ? ctx.wo : ctx.wo * -1.0f, alpha, sqrtf(r[16]), sn, cs);
    o[22] = vn.x; o[23] = vn.y; o[24] = vn.z;
    o[25] = is_valid_color(f) ? 1.0f : 0.0f;
    f3 cl = clamp_radiance(f * 20.0f, 15.0f);
    o[26] = cl.x; o[27] = cl.y; o[28] = cl.z;
    o[29] = ctx.T.x; o[30] = ctx.T.y; o[31] = ctx.T.z; o[32] = ctx.B.x; o[33] = ctx.B.y; o[34] = ctx.B.z;
    o[35] = ctx.wo.x; o[36] = ctx.wo.y; o[37] = ctx.wo.z;
    o[38] = 0.0f; o[39] = 0.0f;
}

} // namespace

// ---- launchers --------------------------------------------------------------------------

void launch_generate(hipStream_t s, const Tiling &tl, const CameraDev &cam, PathBuf pb,
                     uint32_t *qcount, int samples_this_pass, uint32_t first_sample, uint64_t seed,
                     WorkCounters *wc){
    uint32_t total = (uint32_t) tl.n_local * (uint32_t) samples_this_pass;
    hipLaunchKernelGGL(k_generate, dim3(grid_for(total)), dim3(kBlock), 0, s, tl, cam, pb, qcount, total,
                       first_sample, seed, wc);
}

void launch_tri_frames(hipStream_t s, const float4 *tris, int num_tris, float4 *frames){
    if(num_tris <= 0) return;
    hipLaunchKernelGGL(k_tri_frames, dim3((num_tris + kBlock - 1) / kBlock), dim3(kBlock), 0, s, tris, num_tris, frames);
}

void launch_resolve(hipStream_t s, const Tiling &tl, PathBuf pb, float4 *accum, int samples_this_pass){
    uint32_t g = ((uint32_t) tl.n_local + kBlock - 1) / kBlock;
    hipLaunchKernelGGL(k_resolve, dim3(g), dim3(kBlock), 0, s, tl, pb, accum, samples_this_pass);
}

void launch_finalize(hipStream_t s, const Tiling &tl, const float4 *accum, float *d_local, float divisor){
    uint32_t g = ((uint32_t) tl.n_local + kBlock - 1) / kBlock;
    hipLaunchKernelGGL(k_finalize, dim3(g), dim3(kBlock), 0, s, tl, accum, d_local, divisor);
}

void launch_untile(hipStream_t s, const Tiling &tl, const float *d_gathered, float *d_image){
    uint32_t g = ((uint32_t) (tl.W * tl.H) + kBlock - 1) / kBlock;
    hipLaunchKernelGGL(k_untile, dim3(g), dim3(kBlock), 0, s, tl, d_gathered, d_image);
}

void launch_tonemap(hipStream_t s, const float *d_linear, void *d_bytes, unsigned long long num_values, int bgr, const float *d_thresholds){
    if(num_values == 0) return;
    unsigned long long words = (num_values + 3ull) / 4ull;
    hipLaunchKernelGGL(k_tonemap, dim3((unsigned) ((words + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, d_linear, (uint32_t *) d_bytes,
                       num_values, bgr, d_thresholds);
}

void launch_probe_functions(hipStream_t s, const float *d_in, int n, float *d_out){
    if(n <= 0) return;
    hipLaunchKernelGGL(k_probe_functions, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, s, d_in, n, d_out);
}

} // namespace hpt
