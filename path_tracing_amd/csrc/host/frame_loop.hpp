// pt_cli --frames: the progressive loop of the reference's GUI (src/main.cpp:400-531) with its per-frame host work
// done on the device.  This header names neither the reference's records nor HIP's, so both scene_model.cpp (which may
// not see HIP headers, include/hpt_reference_api.hpp) and frame_loop.cpp (which needs them) can include it.
#pragma once
#include "../../../include/hpt.h"

#include <functional>
#include <string>
#include <vector>

namespace hpt_host {

// What a frame loop needs of the scene moved for `mode` ("pt", "bdpt" or "ppm"): the single-device handle (null for a
// fan-out over several devices), its photons / light samples per light, and the run's parameters with the seed taken
// once, so that every frame of the loop draws from the same streams.  False when nothing was moved.  (scene_model.cpp)
struct MovedRun {
    hpt_scene *scene = nullptr; int light_sample = 0; hpt_params params{};
    const void *triangles = nullptr; int num_triangles = 0;      // the moved scene's triangle records (--spin edits copies of them)
};
bool moved_run(const std::string &mode, MovedRun &out);

// `frames` frames of `frame_spp` samples (ppm: passes) each, frame f (from 0) with sample_offset = f * frame_spp, every
// frame accumulated and presented on the device (hpt_accum_add with mean-out, hpt_display_present) on one stream; pt
// and bdpt never bring a frame to the host, ppm uploads its host image.  After frame f (counted from 1)
// "<f> <rms_prev, %.9g>" is appended to `rms_log` (when not empty); the loop ends after `frames`, or earlier after a
// frame >= 2 whose rms_prev <= until_rms (until_rms < 0: off).  `camera` is a CudaCamera; image (W*H*3 floats) receives
// the final mean and rgb8 the last presented bytes (RGB, rows top to bottom).  Returns the number of frames rendered,
// -1 after an error (reported on stderr).  (frame_loop.cpp, part of pt_cli only)
//
// With `motion` (--orbit, --reproject) frame f renders from motion->camera_at(f), when set, instead of `camera`; a frame
// whose camera record differs from the frame's before is a moved frame.  Without reproject the accumulator is reset on
// every moved frame, which is what the reference's GUI does (src/main.cpp:453-466).  With reproject the loop keeps an
// hpt_history instead of the hpt_accum: frame 0 and every moved frame render guide_spp guide samples on the device
// (hpt_render_guides_device, the frame's seed and sample offset) before the frame itself and hand them to
// hpt_history_advance, the other frames advance without guides; the frame's line on stdout then ends in the share of
// pixels that kept their history, "[Frame 7] rms 0.0123 kept 95.1 %".  A null `motion` is the loop as it always was.
//
// With `guided` every frame presents (and `image` receives) the variance-guided filter of the mean instead of the mean
// (hpt_denoiser_run_guided, defaults, demodulated) on a denoiser that lives with the loop.  Guides, now with albedo, are
// rendered on frame 0 and on every moved frame as under reproject.  The variance of the mean: without reproject the
// accumulator keeps moments and from its fourth frame on hpt_accum_variance is used, before that
// hpt_denoiser_estimate_variance of the frame with a length image filled with the frame count; with reproject the
// estimate of the frame with hpt_history_length.  Without `guided` the loop, its launches and its output are unchanged.
//
// With `temporal_variance` (needs reproject and guided; refused otherwise) the history is created with
// HPT_HISTORY_MOMENTS, and after hpt_history_length and hpt_denoiser_estimate_variance the loop calls hpt_history_variance
// in place on the estimate: a pixel whose history is at least four frames long gets its own variance over time, the
// others keep the spatial estimate.  Without it the loop, its launches and its output are unchanged.
//
// With `triangles_at` (--spin) the scene's geometry moves between frames: before frame f > 0 the loop hands it a copy of the
// moved scene's triangle records, which it edits in place (vertices only), and calls hpt_scene_update_triangles.  Without
// reproject the accumulator is reset after every update, which is the advice for a history that is not given the motion
// guide.  With reproject the guides are rendered on every frame with the motion guide (hpt_render_guides_motion_device),
// the history advances through hpt_history_advance_motion and hpt_scene_keep_previous follows (include/hpt.h, "motion").
//
// With `pose_at` (--spin-device; needs `parts_of`, excludes `triangles_at`) the geometry moves the same way without the loop
// copying a record: before frame 0 parts_of fills one part index per triangle from the moved scene's records and returns
// the number of parts, which goes to hpt_scene_set_parts once; before frame f > 0 pose_at fills 12 floats per part and the
// loop calls hpt_scene_pose (include/hpt.h, "poses").  Everything else is as with `triangles_at`.
//
// With `skin_at` (--twist-device; needs `skin_of`, excludes `triangles_at` and `pose_at`) the geometry deforms: before frame 0
// skin_of fills four bones and four weights per corner from the moved scene's records and returns the number of bones, which
// goes to hpt_scene_set_skin once; before frame f > 0 skin_at fills 12 floats per bone and the loop calls hpt_scene_skin
// (include/hpt.h, "skinning").  Everything else is as with `triangles_at`.
//
// With `rebuild_above` = R > 1 (--rebuild-above; needs moving geometry) the loop is the caller's policy of include/hpt.h,
// "rebuild": the tree's sah is measured once after creation (the baseline) and after each frame's update; when it exceeds
// R times the baseline the loop calls hpt_scene_rebuild, prints "[Rebuild] frame <f> sah <before> -> <after> <ms> ms" and takes
// the new sah as the baseline.  The rebuild sits between the update and the motion guides; the previous geometry is untouched,
// so a history keeps following across it.  The image does not depend on it.
//
// With `rebuild_device` (--rebuild-device; needs moving geometry) the rebuilds are hpt_scene_rebuild_device's (include/hpt.h,
// "device builds"): under `rebuild_above` the same policy with the device build in the host rebuild's place, without it a
// device build after every frame's update, one "[Rebuild] frame <f> device nodes <n> depth <d> <ms> ms" line each (the sah is
// not measured then).  A build that fell back to the host builder says "host" for "device".  With `rebuild_depth` >= 0
// (--rebuild-depth; needs `rebuild_device`) those builds are hpt_scene_rebuild_device_bounded's with that max_depth (include/hpt.h,
// "bounded device builds"; 0: the traversal's limit), which the depth of the data's radix tree never sends to the host builder.
//
// With `morph_at` (--morph-device; needs `morphs_of`, excludes `triangles_at`, combines with `pose_at` or `skin_at`) the geometry
// is morphed first: before frame 0 morphs_of fills the sparse targets from the moved scene's records and returns their number,
// which goes to hpt_scene_set_morphs once; before frame f > 0 morph_at fills one weight per target and the loop calls
// hpt_scene_morph, then the deformer's call if there is one (include/hpt.h, "morph targets").
struct FrameMotion {
    std::function<void(int frame, void *camera84)> camera_at;     // fills a CudaCamera (84 bytes); empty: `camera` every frame
    std::function<void(int frame, void *triangles, int count)> triangles_at;      // empty: the geometry stays
    std::function<int(const void *triangles, int count, std::vector<int32_t> &tri_part)> parts_of;
    std::function<void(int frame, float *xforms, int num_parts)> pose_at;         // empty: no poses
    std::function<int(const void *triangles, int count, std::vector<int32_t> &corner_bone, std::vector<float> &corner_weight)> skin_of;
    std::function<void(int frame, float *xforms, int num_bones)> skin_at;         // empty: no skins
    std::function<int(const void *triangles, int count, std::vector<int32_t> &target_begin, std::vector<int32_t> &entry_corner,
                      std::vector<float> &entry_delta)> morphs_of;
    std::function<void(int frame, float *weights, int num_targets)> morph_at;     // empty: no morphs
    bool reproject = false;
    int guide_spp = 4;
    bool guided = false;
    bool temporal_variance = false;
    double rebuild_above = 0.0;           // 0: never
    bool rebuild_device = false;          // rebuilds are device builds; with rebuild_above == 0: after every update
    int rebuild_depth = -1;               // -1: hpt_scene_rebuild_device; 0 .. 30: hpt_scene_rebuild_device_bounded with this max_depth
};
int run_frame_loop(const std::string &mode, const void *camera, float *image, std::vector<unsigned char> &rgb8, int light_depth,
                   int eye_depth, int W, int H, int frames, int frame_spp, int spl, float radius, double until_rms,
                   const std::string &rms_log, const FrameMotion *motion = nullptr);

} // namespace hpt_host
