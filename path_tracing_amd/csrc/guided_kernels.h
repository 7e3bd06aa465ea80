// Launch interface of the variance-guided filter's kernels (guided_kernels.hip): the a-trous filter whose colour tolerance
// follows a per-pixel variance, the spatial variance estimate, and the history's length image (include/hpt.h,
// "variance-guided filtering").  They read the denoiser's packed guides and use its two ping-pong buffers; the scalar
// variance travels in the fourth word of the colour records, so there is no per-pixel state of their own.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include "denoise_kernels.h"

namespace hpt {

struct GuidedLevel {     // what one guided level needs besides its buffers
    int W, H, stride;
    float s2;                        // sigma_color * sigma_color
    float inv_n, inv_p;              // 1 / sigma^2 of the normal and position terms
    int use_c, use_n, use_p;         // 0: the term is switched off (factor 1.0f)
    int demod;                       // the last level multiplies by alb
};

// c_0 as launch_denoise_pack_color, with v_0 in .w: the sum of the three channel variances (each divided by alb^2 where
// demod is set and the pixel is valid), negative and NaN sums as 0
void launch_guided_pack(hipStream_t s, const float *linear_rgb, const float *variance, DenoiseGuides g, float4 *c0, size_t num_pixels, int demod);
// one level: c_in -> c_out ({c, v} records), or with last != 0 -> out (3 floats per pixel, re-modulated when L.demod) and,
// when not null, var_out (1 float per pixel, not re-modulated)
void launch_atrous_guided(hipStream_t s, const GuidedLevel &L, DenoiseGuides g, const float4 *c_in, float4 *c_out, float *out, float *var_out, int last);

struct VarianceArgs {
    int W, H;
    float inv_n, inv_p;
    int use_n, use_p;
    const float *frame;              // 3 W H
    const float *length;             // W H or null
    float *out;                      // 3 W H
};
// per-channel weighted variance of the frame over the 7 x 7 window of every valid pixel, divided by max(length, 1)
void launch_variance_spatial(hipStream_t s, const VarianceArgs &a, DenoiseGuides g);

// out[p] = records[p].w
void launch_take_fourth_word(hipStream_t s, const float4 *records, float *out, size_t n);

} // namespace hpt
