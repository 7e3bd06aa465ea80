// pt_cli --frames (frame_loop.hpp): render, untile, accumulate and present every frame on one stream, read two sums back.
#include "frame_loop.hpp"

#include <hip/hip_runtime_api.h>

#include <cstdio>
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
    hipStream_t stream = nullptr;
    FILE *log = nullptr;
    ~Loop(){
        if(log) fclose(log);
        if(stream){ (void) hipStreamSynchronize(stream); (void) hipStreamDestroy(stream); }
        hpt_display_destroy(display);
        hpt_accum_destroy(accum);
    }
};

int hpt_failed(const char *what){ std::cerr << "[Error] " << what << ": " << hpt_last_error() << std::endl; return -1; }
int hip_failed(const char *what, hipError_t e){ std::cerr << "[Error] " << what << ": " << hipGetErrorString(e) << std::endl; return -1; }

} // namespace

int hpt_host::run_frame_loop(const std::string &mode, const void *camera, float *image, std::vector<unsigned char> &rgb8, int light_depth,
                             int eye_depth, int W, int H, int frames, int frame_spp, int spl, float radius, double until_rms,
                             const std::string &rms_log){
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

    DeviceMem d_local, d_frame, d_mean, d_rgb8;      // released after L has waited for its stream
    Loop L;
    if(!d_frame.alloc(values * sizeof(float)) || !d_mean.alloc(values * sizeof(float)) || !d_rgb8.alloc(values) ||
       (!ppm && !d_local.alloc((size_t) n_local * 3 * sizeof(float)))){
        std::cerr << "[Error] --frames: out of device memory" << std::endl; return -1;
    }
    if(hipError_t e = hipStreamCreateWithFlags(&L.stream, hipStreamNonBlocking)) return hip_failed("stream", e);
    if(hpt_accum_create(W, H, 0, &L.accum) != HPT_OK) return hpt_failed("hpt_accum_create");
    if(hpt_display_create(W, H, &L.display) != HPT_OK) return hpt_failed("hpt_display_create");
    if(!rms_log.empty()){
        L.log = fopen(rms_log.c_str(), "w");
        if(!L.log){ std::cerr << "[Error] cannot open " << rms_log << std::endl; return -1; }
    }
    std::vector<float> host_frame(ppm ? values : 0);

    int done = 0;
    for(int f = 0; f < frames; ++f){
        p.sample_offset = run.params.sample_offset + f * frame_spp;
        int rc;
        if(ppm){
            rc = hpt_render_ppm(run.scene, camera, W, H, eye_depth, light_depth, frame_spp, run.light_sample, radius, nullptr, nullptr,
                                &p, host_frame.data());
            if(rc != HPT_OK) return hpt_failed("hpt_render_ppm");
            if(hipError_t e = hipMemcpyAsync(d_frame.p, host_frame.data(), values * sizeof(float), hipMemcpyHostToDevice, L.stream))
                return hip_failed("frame upload", e);
        } else {
            rc = bdpt ? hpt_render_bdpt_device(run.scene, camera, W, H, eye_depth, light_depth, frame_spp, spl, &p, d_local.p, L.stream)
                      : hpt_render_pt_device(run.scene, camera, W, H, eye_depth, frame_spp, &p, d_local.p, L.stream);
            if(rc != HPT_OK) return hpt_failed("render");
            if(hpt_untile(d_local.p, d_frame.p, W, H, &p, L.stream) != HPT_OK) return hpt_failed("hpt_untile");
        }
        if(hpt_accum_add(L.accum, d_frame.p, d_mean.p, L.stream) != HPT_OK) return hpt_failed("hpt_accum_add");
        if(hpt_display_present(L.display, d_mean.p, nullptr, d_rgb8.p, 0, 0, 0, L.stream) != HPT_OK) return hpt_failed("hpt_display_present");
        double rms_prev = 0.0;
        if(hpt_display_metrics(L.display, &rms_prev, nullptr, nullptr, nullptr, nullptr) != HPT_OK) return hpt_failed("hpt_display_metrics");
        done = f + 1;
        if(L.log){ fprintf(L.log, "%d %.9g\n", done, rms_prev); fflush(L.log); }
        std::cout << "[Frame " << done << "] rms " << rms_prev << std::endl;
        if(until_rms >= 0.0 && done >= 2 && rms_prev <= until_rms) break;
    }
    rgb8.resize(values);
    hipError_t e = hipStreamSynchronize(L.stream);
    if(e == hipSuccess) e = hipMemcpy(image, d_mean.p, values * sizeof(float), hipMemcpyDeviceToHost);
    if(e == hipSuccess) e = hipMemcpy(rgb8.data(), d_rgb8.p, values, hipMemcpyDeviceToHost);
    if(e != hipSuccess) return hip_failed("download", e);
    return done;
}
