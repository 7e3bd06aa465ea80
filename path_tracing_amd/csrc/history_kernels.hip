// HIP kernel of the temporal history (include/hpt.h, "history across camera moves"), written for gfx950 (MI355X).
//
//   k_history_advance  one lane per pixel, one launch per frame.  MODE is the same for every lane: the first frame after a
//                      create or reset and a frame from an unmoved camera touch the pixel's own records only and work in
//                      place; a frame from a moved camera projects the pixel's guide point into the previous camera, reads
//                      up to four neighbours' records from the previous set (three 16-byte loads per tap) and writes the
//                      other set; with the motion guide (kHistoryMotion) the point projected is where the guide point was one
//                      frame ago, and a pixel whose point has not moved under a still camera keeps its own record.  MOMENTS (a history created with HPT_HISTORY_MOMENTS) carries the running mean of the
//                      squared frame values through the same steps with the same taps and weights: a fourth 16-byte record
//                      per pixel and a fourth load per tap.
//   k_history_variance one lane per pixel, a pure map: the variance of the mean from mean, second moment and length where
//                      the history is long enough, the caller's fallback elsewhere.
//
// IEEE float evaluated as written (-ffp-contract=off, correctly rounded divide), no float atomic; the two counters are
// integer sums, reduced in the workgroup and added with one 64-bit atomic each, so their order does not show
// (tests/history_oracle.py restates all of it).
#include "history_kernels.h"
#include "pt_kernels.h"

namespace hpt {

namespace {

struct V3 { float x, y, z; };

__device__ __forceinline__ float dot3(V3 a, V3 b){ return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ __forceinline__ V3 ld3(const float *p){ return V3{ p[0], p[1], p[2] }; }

struct Projected { float s, u, v, dist2; };

__device__ __forceinline__ Projected project(const HistoryCamera &c, V3 X){
    const V3 d{ X.x - c.eye[0], X.y - c.eye[1], X.z - c.eye[2] };
    const float den = dot3(d, V3{ c.nrm[0], c.nrm[1], c.nrm[2] });
    const float s = c.an / den;
    const V3 r{ d.x * s - c.a[0], d.y * s - c.a[1], d.z * s - c.a[2] };
    Projected p;
    p.s = s;
    p.u = dot3(r, V3{ c.gu[0], c.gu[1], c.gu[2] });
    p.v = dot3(r, V3{ c.gv[0], c.gv[1], c.gv[2] });
    p.dist2 = dot3(d, d);
    return p;
}

// Lanes past the image take part in the ballots and the barrier with both flags false.  A lane reads its frame colour
// before it writes the mean, so mean_out may be the frame.
template <int MODE, bool GUIDES, bool MOMENTS>
__global__ __launch_bounds__(kBlock)
void k_history_advance(HistoryArgs a){
    __shared__ uint32_t s_part[2][kBlock / 64];
    const uint32_t npx = (uint32_t) a.W * (uint32_t) a.H;
    const uint32_t p = blockIdx.x * kBlock + threadIdx.x;
    bool kept = false, restarted = false;
    if(p < npx){
        const V3 c = ld3(a.frame + 3u * p);
        V3 m{ 0.0f, 0.0f, 0.0f }, m2{ 0.0f, 0.0f, 0.0f };       // m2: the reprojected second moment q_r
        float n_r = 0.0f;
        V3 X{ 0.0f, 0.0f, 0.0f }, N{ 0.0f, 0.0f, 0.0f };
        float cov = 0.0f;
        if(GUIDES){ X = ld3(a.position + 3u * p); N = ld3(a.normal + 3u * p); cov = a.coverage[p]; }
        if(MODE == kHistoryIdentity){
            const float4 mp = a.prev.mean_n[p];
            m = V3{ mp.x, mp.y, mp.z }; n_r = mp.w;
            if(MOMENTS){ const float4 sp = a.sq_prev[p]; m2 = V3{ sp.x, sp.y, sp.z }; }
        }
        // the point that is looked up in the previous frame: the guide point itself, or with the motion guide where it was then
        bool taps = MODE == kHistoryMoved && GUIDES && cov > 0.0f;
        V3 Xr = X;
        if(MODE == kHistoryMotion){
            const V3 Xp = ld3(a.prev_position + 3u * p);
            const bool same = __float_as_uint(Xp.x) == __float_as_uint(X.x) && __float_as_uint(Xp.y) == __float_as_uint(X.y) &&
                              __float_as_uint(Xp.z) == __float_as_uint(X.z);
            if(!(cov > 0.0f)){                       // 2': sky stays sky under a still camera, anything else was something
                if(a.still && !(a.prev.pos_cov[p].w > 0.0f)){
                    const float4 mp = a.prev.mean_n[p];
                    m = V3{ mp.x, mp.y, mp.z }; n_r = mp.w;
                    if(MOMENTS){ const float4 sp = a.sq_prev[p]; m2 = V3{ sp.x, sp.y, sp.z }; }
                }
            } else if(a.still && same){              // 3': the pixel's own record, weight 1, no division
                const float4 pc = a.prev.pos_cov[p];
                bool take = pc.w > 0.0f;
                if(take && a.plane_on){
                    const Projected now = project(a.cam, X);
                    const float t = dot3(N, V3{ pc.x - X.x, pc.y - X.y, pc.z - X.z });
                    take = t * t <= a.tol2 * now.dist2;
                }
                if(take && a.normal_on){
                    const float4 nq = a.prev.nrm[p];
                    take = dot3(N, V3{ nq.x, nq.y, nq.z }) >= a.normal_min;
                }
                if(take){
                    const float4 mp = a.prev.mean_n[p];
                    m = V3{ mp.x, mp.y, mp.z }; n_r = mp.w;
                    if(MOMENTS){ const float4 sp = a.sq_prev[p]; m2 = V3{ sp.x, sp.y, sp.z }; }
                }
            } else { taps = true; Xr = Xp; }         // 4'
        }
        if(taps){
            const uint32_t y = p / (uint32_t) a.W, x = p - y * (uint32_t) a.W;
            const Projected now = project(a.cam, X);
            const bool direct = now.s > 0.0f && fabsf(now.u - ((float) x + 0.5f)) <= 1.0f && fabsf(now.v - ((float) y + 0.5f)) <= 1.0f;
            const Projected was = project(a.cam_prev, Xr);
            const float up = was.u - 0.5f, vp = was.v - 0.5f;
            // compared in float before any conversion: NaN and infinity end here
            if(direct && was.s > 0.0f && up >= -1.0f && up < (float) a.W && vp >= -1.0f && vp < (float) a.H){
                const float fx0 = floorf(up), fy0 = floorf(vp);
                const float fx = up - fx0, fy = vp - fy0;
                const int x0 = (int) fx0, y0 = (int) fy0;
                const float lim = a.tol2 * now.dist2;
                V3 sum{ 0.0f, 0.0f, 0.0f }, qsum{ 0.0f, 0.0f, 0.0f };
                float nsum = 0.0f, wsum = 0.0f;
#pragma unroll
                for(int j = 0; j < 2; ++j){
#pragma unroll
                    for(int i = 0; i < 2; ++i){
                        const int qx = x0 + i, qy = y0 + j;
                        if(qx < 0 || qx >= a.W || qy < 0 || qy >= a.H) continue;
                        const uint32_t q = (uint32_t) qy * (uint32_t) a.W + (uint32_t) qx;
                        const float4 pc = a.prev.pos_cov[q];
                        if(!(pc.w > 0.0f)) continue;
                        if(a.plane_on){
                            const float t = dot3(N, V3{ pc.x - Xr.x, pc.y - Xr.y, pc.z - Xr.z });
                            if(!(t * t <= lim)) continue;
                        }
                        if(a.normal_on){
                            const float4 nq = a.prev.nrm[q];
                            if(!(dot3(N, V3{ nq.x, nq.y, nq.z }) >= a.normal_min)) continue;
                        }
                        const float4 mq = a.prev.mean_n[q];
                        const float w = (i ? fx : 1.0f - fx) * (j ? fy : 1.0f - fy);
                        sum.x = sum.x + mq.x * w; sum.y = sum.y + mq.y * w; sum.z = sum.z + mq.z * w;
                        if(MOMENTS){
                            const float4 sq = a.sq_prev[q];
                            qsum.x = qsum.x + sq.x * w; qsum.y = qsum.y + sq.y * w; qsum.z = qsum.z + sq.z * w;
                        }
                        nsum = nsum + mq.w * w;
                        wsum = wsum + w;
                    }
                }
                if(wsum > 0.01f){
                    m = V3{ sum.x / wsum, sum.y / wsum, sum.z / wsum };
                    if(MOMENTS) m2 = V3{ qsum.x / wsum, qsum.y / wsum, qsum.z / wsum };
                    n_r = nsum / wsum;
                }
            }
        }
        V3 mean = c, msq{ 0.0f, 0.0f, 0.0f };
        if(MOMENTS) msq = V3{ c.x * c.x, c.y * c.y, c.z * c.z };
        float n = 1.0f;
        if(n_r > 0.0f){
            const float n_c = fminf(n_r, a.max_history_m1);
            const float n1 = n_c + 1.0f;
            mean = V3{ (m.x * n_c + c.x) / n1, (m.y * n_c + c.y) / n1, (m.z * n_c + c.z) / n1 };
            if(MOMENTS) msq = V3{ (m2.x * n_c + c.x * c.x) / n1, (m2.y * n_c + c.y * c.y) / n1, (m2.z * n_c + c.z * c.z) / n1 };
            n = n1;
            kept = true;
        } else restarted = MODE != kHistoryFirst;
        a.next.mean_n[p] = make_float4(mean.x, mean.y, mean.z, n);
        if(MOMENTS) a.sq_next[p] = make_float4(msq.x, msq.y, msq.z, 0.0f);
        if(GUIDES){
            a.next.pos_cov[p] = make_float4(X.x, X.y, X.z, cov);
            a.next.nrm[p] = make_float4(N.x, N.y, N.z, 0.0f);
        } else if(MODE != kHistoryIdentity){        // no guides on a first or moved frame: nothing can be carried from here
            a.next.pos_cov[p] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            a.next.nrm[p] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        }
        if(a.mean_out){ float *o = a.mean_out + 3u * p; o[0] = mean.x; o[1] = mean.y; o[2] = mean.z; }
    }
    const uint32_t k_wave = (uint32_t) __popcll(__ballot(kept)), r_wave = (uint32_t) __popcll(__ballot(restarted));
    const uint32_t wave = threadIdx.x >> 6;
    if((threadIdx.x & 63u) == 0u){ s_part[0][wave] = k_wave; s_part[1][wave] = r_wave; }
    __syncthreads();
    if(threadIdx.x == 0){
        uint32_t k = 0u, r = 0u;
        for(int v = 0; v < kBlock / 64; ++v){ k += s_part[0][v]; r += s_part[1][v]; }
        if(k) atomicAdd(&a.metrics[0], (unsigned long long) k);
        if(r) atomicAdd(&a.metrics[1], (unsigned long long) r);
    }
}

// A lane reads its fallback values before it writes, so `out` may be `fallback`.
__global__ __launch_bounds__(kBlock)
void k_history_variance(const float4 *mean_n, const float4 *sq, const float *fallback, float *out, uint32_t npx, float min_length){
    const uint32_t p = blockIdx.x * kBlock + threadIdx.x;
    if(p >= npx) return;
    const float4 mn = mean_n[p];
    V3 v{ 0.0f, 0.0f, 0.0f };
    if(mn.w >= min_length){
        const float4 q = sq[p];
        const float nm1 = mn.w - 1.0f;
        v = V3{ fmaxf(q.x - mn.x * mn.x, 0.0f) / nm1, fmaxf(q.y - mn.y * mn.y, 0.0f) / nm1, fmaxf(q.z - mn.z * mn.z, 0.0f) / nm1 };
    } else if(fallback) v = ld3(fallback + 3u * p);
    float *o = out + 3u * p;
    o[0] = v.x; o[1] = v.y; o[2] = v.z;
}

__global__ __launch_bounds__(kBlock)
void k_take_first_channel(const float *in3, float *out, uint32_t n){
    const uint32_t k = blockIdx.x * kBlock + threadIdx.x;
    if(k < n) out[k] = in3[3u * k];
}

template <bool MOMENTS>
void launch_advance(hipStream_t s, const dim3 &grid, const dim3 &block, const HistoryArgs &a){
    const bool g = a.position != nullptr;
    if(a.mode == kHistoryFirst){
        if(g) hipLaunchKernelGGL((k_history_advance<kHistoryFirst, true, MOMENTS>), grid, block, 0, s, a);
        else hipLaunchKernelGGL((k_history_advance<kHistoryFirst, false, MOMENTS>), grid, block, 0, s, a);
    } else if(a.mode == kHistoryIdentity){
        if(g) hipLaunchKernelGGL((k_history_advance<kHistoryIdentity, true, MOMENTS>), grid, block, 0, s, a);
        else hipLaunchKernelGGL((k_history_advance<kHistoryIdentity, false, MOMENTS>), grid, block, 0, s, a);
    } else if(a.mode == kHistoryMotion){
        hipLaunchKernelGGL((k_history_advance<kHistoryMotion, true, MOMENTS>), grid, block, 0, s, a);      // the host gives all four guides
    } else {
        if(g) hipLaunchKernelGGL((k_history_advance<kHistoryMoved, true, MOMENTS>), grid, block, 0, s, a);
        else hipLaunchKernelGGL((k_history_advance<kHistoryMoved, false, MOMENTS>), grid, block, 0, s, a);
    }
}

} // namespace

void launch_history_advance(hipStream_t s, const HistoryArgs &a){
    const uint32_t npx = (uint32_t) a.W * (uint32_t) a.H;
    const dim3 grid((npx + kBlock - 1) / kBlock), block(kBlock);
    if(a.sq_next) launch_advance<true>(s, grid, block, a);
    else launch_advance<false>(s, grid, block, a);
}

void launch_history_variance(hipStream_t s, const float4 *mean_n, const float4 *sq, const float *fallback, float *out, uint32_t npx,
                             float min_length){
    hipLaunchKernelGGL(k_history_variance, dim3((npx + kBlock - 1) / kBlock), dim3(kBlock), 0, s, mean_n, sq, fallback, out, npx, min_length);
}

void launch_take_first_channel(hipStream_t s, const float *in3, float *out, uint32_t n){
    hipLaunchKernelGGL(k_take_first_channel, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, s, in3, out, n);
}

} // namespace hpt
