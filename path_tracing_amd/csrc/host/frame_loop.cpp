// pt_cli --frames (frame_loop.hpp): render, untile, accumulate (or, with --reproject, advance the history), with --guided
// filter the mean under its variance (with --temporal-variance the history's own where it is long enough), and present
// every frame on one stream, read the sums back.
#include "frame_loop.hpp"

#include <hip/hip_runtime_api.h>

#include <cstdio>
#include <cstring>
#include <iostream>

namespace {

struct DeviceMem {      // one allocation, released with the loop
    void *p = nullptr;
    ~DeviceMem(){ if(p) (void) hipFree(p); }
    bool alloc(size_t bytes){ return hipMalloc(&p, bytes) == hipSuccess; }
};

struct Loop {
    hpt_accum *accum = nullptr;
    hpt_display *display = nullptr;
    hpt_history *history = nullptr;
    hpt_denoiser *denoiser = nullptr;
    hipStream_t stream = nullptr;
    FILE *log = nullptr;
    ~Loop(){
        if(log) fclose(log);
        if(stream){ (void) hipStreamSynchronize(stream); (void) hipStreamDestroy(stream); }
        hpt_denoiser_destroy(denoiser);
        hpt_history_destroy(history);
        hpt_display_destroy(display);
        hpt_accum_destroy(accum);
    }
};

int hpt_failed(const char *what){ std::cerr << "[Error] " << what << ": " << hpt_last_error() << std::endl; return -1; }
int hip_failed(const char *what, hipError_t e){ std::cerr << "[Error] " << what << ": " << hipGetErrorString(e) << std::endl; return -1; }

} // namespace

int hpt_host::run_frame_loop(const std::string &mode, const void *camera, float *image, std::vector<unsigned char> &rgb8, int light_depth,
                             int eye_depth, int W, int H, int frames, int frame_spp, int spl, float radius, double until_rms,
                             const std::string &rms_log, const FrameMotion *motion){
    MovedRun run;
    if(!moved_run(mode, run)){ std::cerr << "[Error] --frames: no scene moved to the device" << std::endl; return -1; }
    if(!run.scene){ std::cerr << "[Error] --frames renders on one device" << std::endl; return -1; }
    if(frames < 1 || frame_spp < 1){ std::cerr << "[Error] --frames and --frame-spp must be at least 1" << std::endl; return -1; }
    const bool ppm = mode == "ppm", bdpt = mode == "bdpt";
    hpt_params p = run.params;
    if(ppm) p.flags &= HPT_FLAG_TIME_KERNELS | HPT_FLAG_COUNT_WORK;
    const size_t values = (size_t) W * H * 3;
    const int64_t n_local = hpt_local_pixels(W, H, &p);
    if(n_local < 0) return hpt_failed("tiling");

    const bool reproject = motion && motion->reproject;
    const bool guided = motion && motion->guided;
    const bool temporal = motion && motion->temporal_variance;
    if(temporal && !(reproject && guided)){ std::cerr << "[Error] --temporal-variance needs --reproject and --guided" << std::endl; return -1; }
    if((reproject || guided) && motion->guide_spp < 1){ std::cerr << "[Error] --guide-spp must be at least 1" << std::endl; return -1; }
    DeviceMem d_local, d_frame, d_mean, d_rgb8, d_normal, d_position, d_coverage;      // released after L has waited for its stream
    DeviceMem d_albedo, d_variance, d_length, d_filtered;                              // --guided
    DeviceMem d_prev_position;                                                         // --spin --reproject
    const bool posed = motion && motion->pose_at;                                      // --spin-device
    if(posed && (motion->triangles_at || !motion->parts_of)){ std::cerr << "[Error] a pose needs a part map, and excludes edited records" << std::endl; return -1; }
    const bool skinned = motion && motion->skin_at;                                    // --twist-device
    if(skinned && (motion->triangles_at || posed || !motion->skin_of)){ std::cerr << "[Error] a skin needs an influence table, and excludes poses and edited records" << std::endl; return -1; }
    const bool morphed = motion && motion->morph_at;                                   // --morph-device
    if(morphed && (motion->triangles_at || !motion->morphs_of)){ std::cerr << "[Error] a morph needs its targets, and excludes edited records" << std::endl; return -1; }
    const bool spin = motion && (motion->triangles_at || posed || skinned || morphed);
    if(spin && (!run.triangles || run.num_triangles < 1)){ std::cerr << "[Error] --spin: the scene has no triangles" << std::endl; return -1; }
    const bool rebuilds = motion && motion->rebuild_above != 0.0;                      // --rebuild-above
    if(rebuilds && !(motion->rebuild_above > 1.0)){ std::cerr << "[Error] --rebuild-above needs a ratio above 1" << std::endl; return -1; }
    if(rebuilds && !spin){ std::cerr << "[Error] --rebuild-above needs --spin, --spin-device, --twist-device or --morph-device" << std::endl; return -1; }
    const bool device_builds = motion && motion->rebuild_device;                       // --rebuild-device
    if(device_builds && !spin){ std::cerr << "[Error] --rebuild-device needs --spin, --spin-device, --twist-device or --morph-device" << std::endl; return -1; }
    if(motion && motion->rebuild_depth >= 0 && !device_builds){ std::cerr << "[Error] --rebuild-depth needs --rebuild-device" << std::endl; return -1; }
    if(motion && motion->rebuild_depth > 30){ std::cerr << "[Error] --rebuild-depth needs 0 or a depth of 1 to 30" << std::endl; return -1; }
    // a device build, with the time of its four phases (the host builder's when it fell back)
    auto device_build = [&](double &ms, bool &fell_back) -> int {
        hpt_device_build_info di; hpt_rebuild_info ri;
        if(motion->rebuild_depth >= 0){ if(hpt_scene_rebuild_device_bounded(run.scene, motion->rebuild_depth) != HPT_OK) return hpt_failed("hpt_scene_rebuild_device_bounded"); }
        else if(hpt_scene_rebuild_device(run.scene) != HPT_OK) return hpt_failed("hpt_scene_rebuild_device");
        if(hpt_scene_get_device_build_info(run.scene, &di) != HPT_OK) return hpt_failed("hpt_scene_get_device_build_info");
        if(hpt_scene_get_rebuild_info(run.scene, &ri) != HPT_OK) return hpt_failed("hpt_scene_get_rebuild_info");
        fell_back = di.fell_back != 0;
        ms = fell_back ? ri.ms_download + ri.ms_build + ri.ms_upload : di.ms_sort + di.ms_topology + di.ms_refit + di.ms_collapse;
        return 0;
    };
    double sah_base = 0.0;
    if(rebuilds){
        hpt_tree_cost c;
        if(hpt_scene_tree_cost(run.scene, &c) != HPT_OK) return hpt_failed("hpt_scene_tree_cost");
        sah_base = c.sah;
    }
    std::vector<unsigned char> spun;                                                   // this frame's triangle records
    std::vector<float> xforms;                                                         // this frame's pose, 12 floats per part
    if(posed){       // once: the part map, and the rest pose the scene captures with it
        std::vector<int32_t> tri_part;
        const int num_parts = motion->parts_of(run.triangles, run.num_triangles, tri_part);
        if((int) tri_part.size() != run.num_triangles){ std::cerr << "[Error] --spin-device: one part per triangle" << std::endl; return -1; }
        if(hpt_scene_set_parts(run.scene, tri_part.data(), run.num_triangles, num_parts) != HPT_OK) return hpt_failed("hpt_scene_set_parts");
        xforms.resize((size_t) num_parts * 12);
    }
    if(skinned){     // once: the influence table, and the rest pose the scene captures with it
        std::vector<int32_t> corner_bone; std::vector<float> corner_weight;
        const int num_bones = motion->skin_of(run.triangles, run.num_triangles, corner_bone, corner_weight);
        const size_t entries = (size_t) run.num_triangles * 3 * HPT_SKIN_INFLUENCES;
        if(corner_bone.size() != entries || corner_weight.size() != entries){ std::cerr << "[Error] --twist-device: four influences per corner" << std::endl; return -1; }
        if(hpt_scene_set_skin(run.scene, corner_bone.data(), corner_weight.data(), run.num_triangles, num_bones) != HPT_OK) return hpt_failed("hpt_scene_set_skin");
        xforms.resize((size_t) num_bones * 12);
    }
    std::vector<float> weights;                                                        // this frame's morph, one float per target
    if(morphed){     // once: the targets, beside the deformer if there is one; the scene captures the rest pose again
        std::vector<int32_t> target_begin, entry_corner; std::vector<float> entry_delta;
        const int num_targets = motion->morphs_of(run.triangles, run.num_triangles, target_begin, entry_corner, entry_delta);
        if((int) target_begin.size() != num_targets + 1 || entry_delta.size() != entry_corner.size() * 3){ std::cerr << "[Error] --morph-device: malformed targets" << std::endl; return -1; }
        if(hpt_scene_set_morphs(run.scene, target_begin.data(), entry_corner.data(), entry_delta.data(), (int) entry_corner.size(), run.num_triangles,
                                num_targets) != HPT_OK) return hpt_failed("hpt_scene_set_morphs");
        weights.resize((size_t) num_targets);
    }
    Loop L;
    if(!d_frame.alloc(values * sizeof(float)) || !d_mean.alloc(values * sizeof(float)) || !d_rgb8.alloc(values) ||
       (!ppm && !d_local.alloc((size_t) n_local * 3 * sizeof(float)))){
        std::cerr << "[Error] --frames: out of device memory" << std::endl; return -1;
    }
    if(hipError_t e = hipStreamCreateWithFlags(&L.stream, hipStreamNonBlocking)) return hip_failed("stream", e);
    if(reproject || guided){
        if(!d_normal.alloc(values * sizeof(float)) || !d_position.alloc(values * sizeof(float)) || !d_coverage.alloc(values / 3 * sizeof(float))){
            std::cerr << "[Error] --reproject, --guided: out of device memory" << std::endl; return -1;
        }
    }
    if(spin && reproject && !d_prev_position.alloc(values * sizeof(float))){
        std::cerr << "[Error] --spin --reproject: out of device memory" << std::endl; return -1;
    }
    if(guided){
        if(!d_albedo.alloc(values * sizeof(float)) || !d_variance.alloc(values * sizeof(float)) || !d_length.alloc(values / 3 * sizeof(float)) ||
           !d_filtered.alloc(values * sizeof(float))){
            std::cerr << "[Error] --guided: out of device memory" << std::endl; return -1;
        }
        if(hpt_denoiser_create(W, H, &L.denoiser) != HPT_OK) return hpt_failed("hpt_denoiser_create");
    }
    if(reproject){
        if(hpt_history_create_flags(W, H, temporal ? HPT_HISTORY_MOMENTS : 0, &L.history) != HPT_OK) return hpt_failed("hpt_history_create");
    }
    else if(hpt_accum_create(W, H, guided ? HPT_ACCUM_MOMENTS : 0, &L.accum) != HPT_OK) return hpt_failed("hpt_accum_create");
    if(hpt_display_create(W, H, &L.display) != HPT_OK) return hpt_failed("hpt_display_create");
    if(!rms_log.empty()){
        L.log = fopen(rms_log.c_str(), "w");
        if(!L.log){ std::cerr << "[Error] cannot open " << rms_log << std::endl; return -1; }
    }
    std::vector<float> host_frame(ppm ? values : 0);
    std::vector<float> host_length[3];              // --guided without --reproject: the frame count K = 1, 2, 3 as a length image
    if(guided && !reproject) for(int k = 0; k < 3; ++k) host_length[k].assign(values / 3, (float) (k + 1));
    hpt_guided_params gp{};
    gp.flags = HPT_DENOISE_DEMODULATE;

    unsigned char cam_now[HPT_CAMERA_BYTES], cam_last[HPT_CAMERA_BYTES];
    memcpy(cam_now, camera, sizeof cam_now);
    int done = 0;
    for(int f = 0; f < frames; ++f){
        p.sample_offset = run.params.sample_offset + f * frame_spp;
        int rc;
        if(motion && motion->camera_at){ memcpy(cam_last, cam_now, sizeof cam_now); motion->camera_at(f, cam_now); }
        const bool moved = motion && motion->camera_at && f > 0 && memcmp(cam_now, cam_last, sizeof cam_now) != 0;
        const bool updated = spin && f > 0;
        if(updated){     // blocking, on the null stream: the last frame's work on the loop's stream has ended with its metrics
            if(hipError_t e = hipStreamSynchronize(L.stream)) return hip_failed("stream", e);
            if(morphed){     // one float per target; morph first, then the deformer over the morphed rest pose
                motion->morph_at(f, weights.data(), (int) weights.size());
                if(hpt_scene_morph(run.scene, weights.data(), (int) weights.size()) != HPT_OK) return hpt_failed("hpt_scene_morph");
            }
            if(skinned){     // twelve floats per bone
                motion->skin_at(f, xforms.data(), (int) (xforms.size() / 12));
                if(hpt_scene_skin(run.scene, xforms.data(), (int) (xforms.size() / 12)) != HPT_OK) return hpt_failed("hpt_scene_skin");
            } else if(posed){       // twelve floats per part: no record is copied, no vertex is touched on the host
                motion->pose_at(f, xforms.data(), (int) (xforms.size() / 12));
                if(hpt_scene_pose(run.scene, xforms.data(), (int) (xforms.size() / 12)) != HPT_OK) return hpt_failed("hpt_scene_pose");
            } else if(!morphed){
                spun.assign((const unsigned char *) run.triangles, (const unsigned char *) run.triangles + (size_t) run.num_triangles * HPT_TRIANGLE_BYTES);
                motion->triangles_at(f, spun.data(), run.num_triangles);
                if(hpt_scene_update_triangles(run.scene, spun.data(), run.num_triangles) != HPT_OK) return hpt_failed("hpt_scene_update_triangles");
            }
            if(rebuilds){    // the caller's policy: the refitted tree against the last built one
                hpt_tree_cost before, after;
                if(hpt_scene_tree_cost(run.scene, &before) != HPT_OK) return hpt_failed("hpt_scene_tree_cost");
                if(before.sah > motion->rebuild_above * sah_base){
                    hpt_rebuild_info ri;
                    double ms = 0.0; bool fell_back = false;
                    if(device_builds){ if(int e = device_build(ms, fell_back)) return e; }
                    else {
                        if(hpt_scene_rebuild(run.scene) != HPT_OK) return hpt_failed("hpt_scene_rebuild");
                        if(hpt_scene_get_rebuild_info(run.scene, &ri) != HPT_OK) return hpt_failed("hpt_scene_get_rebuild_info");
                        ms = ri.ms_download + ri.ms_build + ri.ms_upload;
                    }
                    if(hpt_scene_tree_cost(run.scene, &after) != HPT_OK) return hpt_failed("hpt_scene_tree_cost");
                    char line[160];
                    snprintf(line, sizeof line, "[Rebuild] frame %d sah %.4f -> %.4f %.3f ms", f, before.sah, after.sah, ms);
                    std::cout << line << std::endl;
                    sah_base = after.sah;
                }
            } else if(device_builds){    // no ratio: a new tree for every frame's geometry
                double ms = 0.0; bool fell_back = false;
                if(int e = device_build(ms, fell_back)) return e;
                hpt_stats st;
                if(hpt_get_stats(run.scene, &st) != HPT_OK) return hpt_failed("hpt_get_stats");
                char line[160];
                snprintf(line, sizeof line, "[Rebuild] frame %d %s nodes %u depth %u %.3f ms", f, fell_back ? "host" : "device", st.bvh_nodes, st.bvh_depth, ms);
                std::cout << line << std::endl;
            }
        }
        const bool follow = spin && reproject;          // the motion guide every frame
        const bool guides = (reproject || guided) && (f == 0 || moved || spin);
        if(guides){      // blocking, on the scene's own stream: before this frame's render is enqueued, after the last frame's metrics
            hpt_params g{};
            g.seed = p.seed; g.sample_offset = p.sample_offset; g.max_delta = p.max_delta; g.tile = p.tile;
            if(hpt_render_guides_motion_device(run.scene, cam_now, W, H, motion->guide_spp, &g, d_albedo.p, d_normal.p, d_position.p, d_coverage.p,
                                               follow ? d_prev_position.p : nullptr) != HPT_OK)
                return hpt_failed("hpt_render_guides_motion_device");
            if(guided && hpt_denoiser_set_guides(L.denoiser, d_albedo.p, d_normal.p, d_position.p, d_coverage.p, L.stream) != HPT_OK)
                return hpt_failed("hpt_denoiser_set_guides");
        }
        if(ppm){
            rc = hpt_render_ppm(run.scene, cam_now, W, H, eye_depth, light_depth, frame_spp, run.light_sample, radius, nullptr, nullptr,
                                &p, host_frame.data());
            if(rc != HPT_OK) return hpt_failed("hpt_render_ppm");
            if(hipError_t e = hipMemcpyAsync(d_frame.p, host_frame.data(), values * sizeof(float), hipMemcpyHostToDevice, L.stream))
                return hip_failed("frame upload", e);
        } else {
            rc = bdpt ? hpt_render_bdpt_device(run.scene, cam_now, W, H, eye_depth, light_depth, frame_spp, spl, &p, d_local.p, L.stream)
                      : hpt_render_pt_device(run.scene, cam_now, W, H, eye_depth, frame_spp, &p, d_local.p, L.stream);
            if(rc != HPT_OK) return hpt_failed("render");
            if(hpt_untile(d_local.p, d_frame.p, W, H, &p, L.stream) != HPT_OK) return hpt_failed("hpt_untile");
        }
        if(reproject){
            if(hpt_history_advance_motion(L.history, cam_now, d_frame.p, guides ? d_normal.p : nullptr, guides ? d_position.p : nullptr,
                                          guides ? d_coverage.p : nullptr, follow ? d_prev_position.p : nullptr, nullptr, d_mean.p, L.stream) != HPT_OK)
                return hpt_failed("hpt_history_advance_motion");
            // this frame's guides are rendered: its geometry is what the next frame's update is measured against
            if(follow && hpt_scene_keep_previous(run.scene) != HPT_OK) return hpt_failed("hpt_scene_keep_previous");
            if(guided && hpt_history_length(L.history, d_length.p, L.stream) != HPT_OK) return hpt_failed("hpt_history_length");
        } else {
            if((moved || updated) && hpt_accum_reset(L.accum, L.stream) != HPT_OK) return hpt_failed("hpt_accum_reset");
            if(hpt_accum_add(L.accum, d_frame.p, d_mean.p, L.stream) != HPT_OK) return hpt_failed("hpt_accum_add");
        }
        if(guided){
            // the variance of the mean: the accumulator's own from four frames on; before that, and under --reproject, the
            // spatial estimate of this frame divided by the frame count or by each pixel's history length
            const int64_t K = reproject ? 0 : hpt_accum_count(L.accum);
            if(!reproject && K >= 4){
                if(hpt_accum_variance(L.accum, d_variance.p, L.stream) != HPT_OK) return hpt_failed("hpt_accum_variance");
            } else {
                if(!reproject){
                    if(hipError_t e = hipMemcpyAsync(d_length.p, host_length[K - 1].data(), values / 3 * sizeof(float), hipMemcpyHostToDevice, L.stream))
                        return hip_failed("length upload", e);
                }
                if(hpt_denoiser_estimate_variance(L.denoiser, d_frame.p, d_length.p, d_variance.p, &gp, L.stream) != HPT_OK)
                    return hpt_failed("hpt_denoiser_estimate_variance");
                // the history's own variance over time where it is long enough, patched into the estimate
                if(temporal && hpt_history_variance(L.history, d_variance.p, 0.0f, d_variance.p, L.stream) != HPT_OK)
                    return hpt_failed("hpt_history_variance");
            }
            if(hpt_denoiser_run_guided(L.denoiser, d_mean.p, d_variance.p, d_filtered.p, nullptr, &gp, L.stream) != HPT_OK)
                return hpt_failed("hpt_denoiser_run_guided");
        }
        void *shown = guided ? d_filtered.p : d_mean.p;
        if(hpt_display_present(L.display, shown, nullptr, d_rgb8.p, 0, 0, 0, L.stream) != HPT_OK) return hpt_failed("hpt_display_present");
        double rms_prev = 0.0;
        if(hpt_display_metrics(L.display, &rms_prev, nullptr, nullptr, nullptr, nullptr) != HPT_OK) return hpt_failed("hpt_display_metrics");
        done = f + 1;
        if(L.log){ fprintf(L.log, "%d %.9g\n", done, rms_prev); fflush(L.log); }
        if(reproject){
            uint64_t kept = 0;
            if(hpt_history_metrics(L.history, &kept, nullptr, nullptr) != HPT_OK) return hpt_failed("hpt_history_metrics");
            char share[32];
            snprintf(share, sizeof share, "%.1f", 100.0 * (double) kept / ((double) W * H));
            std::cout << "[Frame " << done << "] rms " << rms_prev << " kept " << share << " %" << std::endl;
        }
        else std::cout << "[Frame " << done << "] rms " << rms_prev << std::endl;
        if(until_rms >= 0.0 && done >= 2 && rms_prev <= until_rms) break;
    }
    rgb8.resize(values);
    hipError_t e = hipStreamSynchronize(L.stream);
    if(e == hipSuccess) e = hipMemcpy(image, guided ? d_filtered.p : d_mean.p, values * sizeof(float), hipMemcpyDeviceToHost);
    if(e == hipSuccess) e = hipMemcpy(rgb8.data(), d_rgb8.p, values, hipMemcpyDeviceToHost);
    if(e != hipSuccess) return hip_failed("download", e);
    return done;
}
