// HIP kernels of the progressive display (include/hpt.h, "progressive display"), written for gfx950 (MI355X).
//
//   accumulate  k_accum_add adds one frame into the running sum (and sum of squares) and can write the mean in the same
//               pass; k_accum_resolve forms the mean or the variance of the mean from the sums.
//   present     k_present turns the linear image into bytes with the tone map's threshold table, writes them into a panel
//               of the caller's framebuffer, keeps them as `last`, and sums the squared byte differences against the
//               previous present and against another display.
//
// The float side is IEEE arithmetic evaluated as written (-ffp-contract=off, correctly rounded divide) with no atomic; the
// metrics are integer sums, so the order of the atomics does not show (tests/display_oracle.py restates both).
#include "display_kernels.h"
#include "pt_kernels.h"

namespace hpt {

namespace {

// ---- accumulate ----------------------------------------------------------------------------------------------------
// Lanes 0 .. n4-1 own one 16-byte group each, the lanes after them one value each of the tail that starts at 4 * n4
// (every value when the caller's pointers are not 16-byte aligned: n4 = 0).  A lane reads its frame values before it
// writes the mean, so mean_out may be the frame.
template <bool MOMENTS, bool MEAN>
__global__ __launch_bounds__(kBlock)
void k_accum_add(float *sum, float *sq, const float *frame, float *mean_out, uint32_t n4, uint32_t n, float k){
    const uint32_t t = blockIdx.x * kBlock + threadIdx.x;
    if(t < n4){
        const float4 v = ((const float4 *) frame)[t];
        float4 s = ((float4 *) sum)[t];
        s.x = s.x + v.x; s.y = s.y + v.y; s.z = s.z + v.z; s.w = s.w + v.w;
        ((float4 *) sum)[t] = s;
        if(MOMENTS){
            float4 q = ((float4 *) sq)[t];
            q.x = q.x + v.x * v.x; q.y = q.y + v.y * v.y; q.z = q.z + v.z * v.z; q.w = q.w + v.w * v.w;
            ((float4 *) sq)[t] = q;
        }
        if(MEAN) ((float4 *) mean_out)[t] = make_float4(s.x / k, s.y / k, s.z / k, s.w / k);
        return;
    }
    const uint32_t i = n4 * 4u + (t - n4);
    if(i >= n) return;
    const float v = frame[i];
    const float s = sum[i] + v;
    sum[i] = s;
    if(MOMENTS) sq[i] = sq[i] + v * v;
    if(MEAN) mean_out[i] = s / k;
}

__device__ __forceinline__ float resolve_value(float s, float q, float k, float km1, int variance){
    const float m = s / k;
    if(!variance) return m;
    const float qq = q / k;
    const float d = qq - m * m;
    return fmaxf(d, 0.0f) / km1;
}

__global__ __launch_bounds__(kBlock)
void k_accum_resolve(const float *sum, const float *sq, float *out, uint32_t n4, uint32_t n, float k, float km1, int variance){
    const uint32_t t = blockIdx.x * kBlock + threadIdx.x;
    if(t < n4){
        const float4 s = ((const float4 *) sum)[t];
        float4 q = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if(variance) q = ((const float4 *) sq)[t];
        ((float4 *) out)[t] = make_float4(resolve_value(s.x, q.x, k, km1, variance), resolve_value(s.y, q.y, k, km1, variance),
                                          resolve_value(s.z, q.z, k, km1, variance), resolve_value(s.w, q.w, k, km1, variance));
        return;
    }
    const uint32_t i = n4 * 4u + (t - n4);
    if(i >= n) return;
    out[i] = resolve_value(sum[i], variance ? sq[i] : 0.0f, k, km1, variance);
}

bool aligned16(const void *p){ return ((uintptr_t) p & 15u) == 0u; }

unsigned blocks_for(uint32_t n4, uint32_t n){
    const uint32_t lanes = n4 + (n - n4 * 4u);
    return (lanes + kBlock - 1) / kBlock;
}

// ---- present -------------------------------------------------------------------------------------------------------
// sum over the four bytes of (a - b)^2: at most 4 * 255^2
__device__ __forceinline__ uint32_t ssd4(uint32_t a, uint32_t b){
    uint32_t s = 0u;
    for(int k = 0; k < 4; ++k){
        const int d = (int) ((a >> (8 * k)) & 255u) - (int) ((b >> (8 * k)) & 255u);
        s += (uint32_t) (d * d);
    }
    return s;
}

// One lane owns four consecutive canonical values = one word of `last` (k_tonemap's shape, pt_frame.hip); the byte is
// the number of thresholds <= x, eight steps in LDS.  A lane's squared differences fit a uint32 (<= 260100), a wave's
// (x 64) and a workgroup's (x 256 = 66.6e6) too; they are added up by shuffles, then through LDS, and the workgroup
// issues one 64-bit atomic per metric.  Every lane reaches the barriers and the shuffles: lanes past the image hold 0.
// Panel bytes are written with byte stores only, so nothing outside the panel's H runs of 3 W bytes is touched
// whatever the alignment of pointer, pitch and offset.
template <bool OTHER, bool OUT>
__global__ __launch_bounds__(kBlock)
void k_present(PresentArgs a){
    __shared__ float s_thr[256];
    __shared__ uint32_t s_part[2][kBlock / 64];
    s_thr[threadIdx.x] = a.thresholds[threadIdx.x];
    __syncthreads();
    const uint32_t row3 = 3u * (uint32_t) a.W;
    const uint32_t n = row3 * (uint32_t) a.H;
    const uint32_t w = blockIdx.x * kBlock + threadIdx.x;
    const uint32_t first = w * 4u;
    uint32_t d_prev = 0u, d_other = 0u;
    if(first < n){
        uint32_t packed = 0u;
        for(uint32_t k = 0; k < 4u && first + k < n; ++k){
            const float x = a.linear[first + k];
            uint32_t lo = 0u;
            for(uint32_t step = 128u; step > 0u; step >>= 1) if(x >= s_thr[lo + step]) lo += step;   // s_thr[0] unused (byte >= 0 always)
            packed |= lo << (8u * k);
        }
        if(a.has_prev) d_prev = ssd4(packed, a.last[w]);
        if(OTHER) d_other = ssd4(packed, a.other_last[w]);
        a.last[w] = packed;
        if(OUT){
            uint32_t r = first / row3, rem = first - r * row3;
            for(uint32_t k = 0; k < 4u && first + k < n; ++k){
                const uint32_t px = rem / 3u, c = rem - px * 3u;
                const uint32_t col = a.bgr ? px * 3u + (2u - c) : rem;
                const uint32_t orow = a.flip ? (uint32_t) a.H - 1u - r : r;
                a.out[(long long) orow * a.pitch + (long long) col] = (unsigned char) (packed >> (8u * k));
                if(++rem == row3){ rem = 0u; ++r; }
            }
        }
    }
    for(int off = 32; off > 0; off >>= 1){
        d_prev += __shfl_down(d_prev, off, 64);
        if(OTHER) d_other += __shfl_down(d_other, off, 64);
    }
    const uint32_t wave = threadIdx.x >> 6;
    if((threadIdx.x & 63u) == 0u){ s_part[0][wave] = d_prev; s_part[1][wave] = d_other; }
    __syncthreads();
    if(threadIdx.x == 0){
        uint32_t p = 0u, o = 0u;
        for(int v = 0; v < kBlock / 64; ++v){ p += s_part[0][v]; o += s_part[1][v]; }
        if(p) atomicAdd(&a.metrics[0], (unsigned long long) p);
        if(OTHER && o) atomicAdd(&a.metrics[1], (unsigned long long) o);
    }
}

} // namespace

void launch_accum_add(hipStream_t s, float *sum, float *sq, const float *frame, float *mean_out, uint32_t n, float k){
    const bool vec = aligned16(sum) && (!sq || aligned16(sq)) && aligned16(frame) && (!mean_out || aligned16(mean_out));
    const uint32_t n4 = vec ? n / 4u : 0u;
    const dim3 grid(blocks_for(n4, n)), block(kBlock);
    if(sq && mean_out) hipLaunchKernelGGL((k_accum_add<true, true>), grid, block, 0, s, sum, sq, frame, mean_out, n4, n, k);
    else if(sq) hipLaunchKernelGGL((k_accum_add<true, false>), grid, block, 0, s, sum, sq, frame, mean_out, n4, n, k);
    else if(mean_out) hipLaunchKernelGGL((k_accum_add<false, true>), grid, block, 0, s, sum, sq, frame, mean_out, n4, n, k);
    else hipLaunchKernelGGL((k_accum_add<false, false>), grid, block, 0, s, sum, sq, frame, mean_out, n4, n, k);
}

void launch_accum_resolve(hipStream_t s, const float *sum, const float *sq, float *out, uint32_t n, float k, float km1, int variance){
    const bool vec = aligned16(sum) && (!variance || aligned16(sq)) && aligned16(out);
    const uint32_t n4 = vec ? n / 4u : 0u;
    hipLaunchKernelGGL(k_accum_resolve, dim3(blocks_for(n4, n)), dim3(kBlock), 0, s, sum, sq, out, n4, n, k, km1, variance);
}

void launch_present(hipStream_t s, const PresentArgs &a){
    const uint32_t words = (3u * (uint32_t) a.W * (uint32_t) a.H + 3u) / 4u;
    const dim3 grid((words + kBlock - 1) / kBlock), block(kBlock);
    if(a.other_last && a.out) hipLaunchKernelGGL((k_present<true, true>), grid, block, 0, s, a);
    else if(a.other_last) hipLaunchKernelGGL((k_present<true, false>), grid, block, 0, s, a);
    else if(a.out) hipLaunchKernelGGL((k_present<false, true>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((k_present<false, false>), grid, block, 0, s, a);
}

} // namespace hpt
