// Launch interface of the guide-buffer and denoiser kernels (denoise_kernels.hip): the first-hit guides accumulated from
// photon mapping's eye pass, and the edge-avoiding a-trous filter (include/hpt.h, "guides and denoiser").
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include "ppm_kernels.h"

namespace hpt {

// Per local pixel slot, summed over the samples of one hpt_render_guides call.
struct GuideAccum {
    float4 *alb_cnt;     // sum of base colours xyz | number of samples that ended in a hit point (uint32 bits)
    float4 *nrm;         // sum of ray-facing normals xyz | unused
    float4 *pos;         // sum of positions xyz | unused
    float4 *prev;        // sum of previous positions xyz | unused (the motion guide; `pos` again where nothing has moved)
};

// The scene's current and previous geometry as the motion guide reads them (include/hpt.h, "motion"): nine vertex floats
// per triangle in input order, and centre | radius per sphere.  The current spheres are sc.rounds.
struct GuideMotion {
    const float *verts, *prev_verts;
    const float4 *prev_rounds;
};

// one lane per entry of hb.list (their number in *hp_count): the lane owns its pixel slot, plain loads and stores
void launch_guides_accumulate(hipStream_t s, const SceneDev &sc, PpmHitBuf hb, const uint32_t *hp_count, uint32_t max_items, GuideAccum ga);
// the same sums plus ga.prev: where each hit point was in the previous geometry; `hit` is the eye pass's PathBuf::hit,
// whose primitive code a finished path keeps
void launch_guides_accumulate_motion(hipStream_t s, const SceneDev &sc, PpmHitBuf hb, const uint2 *hit, const uint32_t *hp_count,
                                     uint32_t max_items, GuideAccum ga, GuideMotion gm);
// d_local[3 p ..] = the mean of `which` (0 albedo, 1 normal, 2 position, 4 previous position; zero where the count is
// zero) or, which = 3, (count, 0, 0), for launch_untile
void launch_guides_resolve(hipStream_t s, uint32_t n_local, GuideAccum ga, int which, float *d_local);

// The filter's packed records, one per pixel of the row-major image.
struct DenoiseGuides {
    float4 *nrm_cov;     // normal xyz | coverage
    float4 *pos;         // position xyz | 0
    float4 *alb;         // max(albedo, 1e-3) per channel xyz | 0
};
struct DenoiseLevel {    // what one level of the filter needs besides its buffers
    int W, H, stride;
    float inv_c, inv_n, inv_p;       // 1 / sigma^2 of the three edge-stopping terms
    int use_c, use_n, use_p;         // 0: the term is switched off (factor 1.0f)
    int demod;                       // the last level multiplies by alb
};

// the four guide images (layouts of hpt_render_guides) into DenoiseGuides
void launch_denoise_pack(hipStream_t s, const float *albedo, const float *normal, const float *position, const float *coverage,
                         DenoiseGuides g, size_t num_pixels);
// c_0: colour / alb where demod is set and the pixel is valid, else colour
void launch_denoise_pack_color(hipStream_t s, const float *linear_rgb, DenoiseGuides g, float4 *c0, size_t num_pixels, int demod);
// one level: c_in -> c_out (float4 records), or with last != 0 -> out (3 floats per pixel, re-modulated when L.demod)
void launch_atrous(hipStream_t s, const DenoiseLevel &L, DenoiseGuides g, const float4 *c_in, float4 *c_out, float *out, int last);

} // namespace hpt
