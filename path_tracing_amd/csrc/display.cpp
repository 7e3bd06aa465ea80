// The progressive display's host side (include/hpt.h, hpt_accum_* and hpt_display_*): the two objects that last across
// frames -- the running sums with their host-side frame count, and the last presented bytes with the pinned words the
// metrics come back in -- and the argument checks, all made before anything touches the device.
#include "hpt_host.h"
#include "display_kernels.h"

#include <cmath>
#include <new>

using namespace hpt;

namespace {

constexpr int32_t kAccumFlags = HPT_ACCUM_MOMENTS;
constexpr int32_t kDisplayFlags = HPT_DISPLAY_BGR | HPT_DISPLAY_FLIP_Y;
constexpr int64_t kMaxAdds = 1ll << 24;              // (float) K is exact up to here
constexpr long long kMaxPixels = 1ll << 28;          // 3 W H stays below 2^30: 32-bit indices in the kernels

int check_size(int W, int H){
    if(W < 1 || H < 1) return fail(HPT_ERR_INVALID, "image size must be positive");
    if((long long) W * H > kMaxPixels) return fail(HPT_ERR_INVALID, "image too large for the progressive display (at most 2^28 pixels)");
    return HPT_OK;
}

int on_device(int device, const char *what){
    int dev = -1;
    if(hipGetDevice(&dev) != hipSuccess || dev != device)
        return fail(HPT_ERR_INVALID, std::string(what) + " lives on another device than the calling thread's current one (hipSetDevice first)");
    return HPT_OK;
}

bool overlap(const void *a, const void *b, size_t bytes){
    const uintptr_t x = (uintptr_t) a, y = (uintptr_t) b;
    return x < y + bytes && y < x + bytes;
}

} // namespace

struct hpt_accum {
    int device = 0, W = 0, H = 0;
    uint32_t n = 0;                  // 3 W H
    bool moments = false;
    int64_t count = 0;               // K: frames enqueued since create / reset
    DevBuf<float> sum, sq;
};

struct hpt_display {
    int device = 0, W = 0, H = 0;
    uint32_t words = 0;              // (3 W H + 3) / 4
    int64_t presented = 0;           // P
    DevBuf<uint32_t> last;           // the bytes of the last present, canonical order, four to a word
    DevBuf<float> thresholds;        // hpt_tonemap_table on the device
    DevBuf<unsigned long long> metrics;      // ssd_prev, ssd_other of the present in flight
    unsigned long long *h_metrics = nullptr; // pinned copy, valid once `done` has passed
    hipEvent_t done = nullptr;
    ~hpt_display(){
        if(done) hipEventDestroy(done);
        if(h_metrics) hipHostFree(h_metrics);
    }
};

extern "C" {

// ---- hpt_accum -------------------------------------------------------------------------------------------------------

int hpt_accum_create(int W, int H, int32_t flags, hpt_accum **out){
    if(!out) return fail(HPT_ERR_INVALID, "null out");
    *out = nullptr;
    if(int rc = check_size(W, H)) return rc;
    if(flags & ~kAccumFlags) return fail(HPT_ERR_INVALID, "hpt_accum_create flags: HPT_ACCUM_MOMENTS only");
    hpt_accum *a = new (std::nothrow) hpt_accum;
    if(!a) return fail(HPT_ERR_NOMEM, "out of host memory");
    a->W = W; a->H = H; a->n = 3u * (uint32_t) W * (uint32_t) H;
    a->moments = (flags & HPT_ACCUM_MOMENTS) != 0;
    hipError_t e = hipGetDevice(&a->device);
    if(e == hipSuccess) e = a->sum.reserve(a->n);
    if(e == hipSuccess && a->moments) e = a->sq.reserve(a->n);
    if(e == hipSuccess) e = hipMemset(a->sum.get(), 0, a->n * sizeof(float));
    if(e == hipSuccess && a->moments) e = hipMemset(a->sq.get(), 0, a->n * sizeof(float));
    if(e == hipSuccess) e = hipDeviceSynchronize();      // zeroed before a first add on any stream
    if(e != hipSuccess){ delete a; return fail_hip("accumulator buffers", e); }
    *out = a;
    return HPT_OK;
}

void hpt_accum_destroy(hpt_accum *a){ delete a; }

int64_t hpt_accum_count(const hpt_accum *a){ return a ? a->count : 0; }

int hpt_accum_add(hpt_accum *a, const void *d_frame_rgb, void *d_mean_out, void *hip_stream){
    if(!a) return fail(HPT_ERR_INVALID, "null accumulator");
    if(!d_frame_rgb) return fail(HPT_ERR_INVALID, "null frame");
    if(d_mean_out && d_mean_out != d_frame_rgb && overlap(d_frame_rgb, d_mean_out, (size_t) a->n * sizeof(float)))
        return fail(HPT_ERR_INVALID, "hpt_accum_add: d_mean_out must be d_frame_rgb itself or not overlap it");
    if(a->count >= kMaxAdds) return fail(HPT_ERR_INVALID, "hpt_accum_add: more than 2^24 frames ((float) K is no longer exact); reset first");
    if(int rc = on_device(a->device, "the accumulator")) return rc;
    a->count += 1;
    launch_accum_add((hipStream_t) hip_stream, a->sum.get(), a->moments ? a->sq.get() : nullptr, (const float *) d_frame_rgb,
                     (float *) d_mean_out, a->n, (float) a->count);
    HIP_TRY(hipGetLastError());
    return HPT_OK;
}

int hpt_accum_mean(hpt_accum *a, void *d_out, void *hip_stream){
    if(!a) return fail(HPT_ERR_INVALID, "null accumulator");
    if(!d_out) return fail(HPT_ERR_INVALID, "null output image");
    if(a->count == 0) return fail(HPT_ERR_INVALID, "hpt_accum_mean before the first hpt_accum_add");
    if(int rc = on_device(a->device, "the accumulator")) return rc;
    launch_accum_resolve((hipStream_t) hip_stream, a->sum.get(), nullptr, (float *) d_out, a->n, (float) a->count, 0.0f, 0);
    HIP_TRY(hipGetLastError());
    return HPT_OK;
}

int hpt_accum_variance(hpt_accum *a, void *d_out, void *hip_stream){
    if(!a) return fail(HPT_ERR_INVALID, "null accumulator");
    if(!d_out) return fail(HPT_ERR_INVALID, "null output image");
    if(!a->moments) return fail(HPT_ERR_INVALID, "hpt_accum_variance needs an accumulator created with HPT_ACCUM_MOMENTS");
    if(int rc = on_device(a->device, "the accumulator")) return rc;
    if(a->count < 2) HIP_TRY(hipMemsetAsync(d_out, 0, (size_t) a->n * sizeof(float), (hipStream_t) hip_stream));
    else {
        launch_accum_resolve((hipStream_t) hip_stream, a->sum.get(), a->sq.get(), (float *) d_out, a->n, (float) a->count,
                             (float) (a->count - 1), 1);
        HIP_TRY(hipGetLastError());
    }
    return HPT_OK;
}

int hpt_accum_reset(hpt_accum *a, void *hip_stream){
    if(!a) return fail(HPT_ERR_INVALID, "null accumulator");
    if(int rc = on_device(a->device, "the accumulator")) return rc;
    HIP_TRY(hipMemsetAsync(a->sum.get(), 0, (size_t) a->n * sizeof(float), (hipStream_t) hip_stream));
    if(a->moments) HIP_TRY(hipMemsetAsync(a->sq.get(), 0, (size_t) a->n * sizeof(float), (hipStream_t) hip_stream));
    a->count = 0;
    return HPT_OK;
}

int hpt_accum_read(hpt_accum *a, float *sum, float *sumsq, int64_t *count){
    if(!a) return fail(HPT_ERR_INVALID, "null accumulator");
    if(sumsq && !a->moments) return fail(HPT_ERR_INVALID, "hpt_accum_read: no sum of squares without HPT_ACCUM_MOMENTS");
    if(int rc = on_device(a->device, "the accumulator")) return rc;
    HIP_TRY(hipDeviceSynchronize());
    if(sum) HIP_TRY(hipMemcpy(sum, a->sum.get(), (size_t) a->n * sizeof(float), hipMemcpyDeviceToHost));
    if(sumsq) HIP_TRY(hipMemcpy(sumsq, a->sq.get(), (size_t) a->n * sizeof(float), hipMemcpyDeviceToHost));
    if(count) *count = a->count;
    return HPT_OK;
}

// ---- hpt_display -----------------------------------------------------------------------------------------------------

int hpt_display_create(int W, int H, hpt_display **out){
    if(!out) return fail(HPT_ERR_INVALID, "null out");
    *out = nullptr;
    if(int rc = check_size(W, H)) return rc;
    hpt_display *d = new (std::nothrow) hpt_display;
    if(!d) return fail(HPT_ERR_NOMEM, "out of host memory");
    d->W = W; d->H = H; d->words = (3u * (uint32_t) W * (uint32_t) H + 3u) / 4u;
    float table[256];
    hpt_tonemap_table(table);
    hipError_t e = hipGetDevice(&d->device);
    if(e == hipSuccess) e = d->last.reserve(d->words);
    if(e == hipSuccess) e = d->thresholds.reserve(256);
    if(e == hipSuccess) e = d->metrics.reserve(2);
    if(e == hipSuccess) e = hipHostMalloc((void **) &d->h_metrics, 2 * sizeof(unsigned long long), hipHostMallocDefault);
    if(e == hipSuccess) e = hipEventCreateWithFlags(&d->done, hipEventDisableTiming);
    if(e == hipSuccess) e = hipMemcpy(d->thresholds.get(), table, sizeof table, hipMemcpyHostToDevice);
    if(e == hipSuccess) e = hipMemset(d->last.get(), 0, (size_t) d->words * sizeof(uint32_t));
    if(e == hipSuccess) e = hipDeviceSynchronize();
    if(e != hipSuccess){ delete d; return fail_hip("display buffers", e); }
    *out = d;
    return HPT_OK;
}

void hpt_display_destroy(hpt_display *d){ delete d; }

int hpt_display_present(hpt_display *d, const void *d_linear_rgb, const hpt_display *other, void *d_rgb8, int64_t pitch_bytes,
                        int64_t x_offset_bytes, int32_t flags, void *hip_stream){
    if(!d) return fail(HPT_ERR_INVALID, "null display");
    if(!d_linear_rgb) return fail(HPT_ERR_INVALID, "null image");
    if(flags & ~kDisplayFlags) return fail(HPT_ERR_INVALID, "hpt_display_present flags: HPT_DISPLAY_BGR and HPT_DISPLAY_FLIP_Y only");
    const int64_t row = 3ll * d->W;
    const int64_t pitch = pitch_bytes == 0 ? row : pitch_bytes;
    if(x_offset_bytes < 0) return fail(HPT_ERR_INVALID, "hpt_display_present: x_offset_bytes must not be negative");
    if(pitch < x_offset_bytes + row) return fail(HPT_ERR_INVALID, "hpt_display_present: pitch_bytes is smaller than x_offset_bytes + 3 W");
    if(other){
        if(other == d) return fail(HPT_ERR_INVALID, "hpt_display_present: `other` must be a different display");
        if(other->W != d->W || other->H != d->H) return fail(HPT_ERR_INVALID, "hpt_display_present: `other` has another size");
        if(other->device != d->device) return fail(HPT_ERR_INVALID, "hpt_display_present: `other` lives on another device");
        if(other->presented < 1) return fail(HPT_ERR_INVALID, "hpt_display_present: `other` has not presented yet");
    }
    if(int rc = on_device(d->device, "the display")) return rc;
    hipStream_t st = (hipStream_t) hip_stream;
    PresentArgs a{};
    a.linear = (const float *) d_linear_rgb; a.thresholds = d->thresholds.get();
    a.last = d->last.get(); a.other_last = other ? other->last.get() : nullptr;
    a.metrics = d->metrics.get();
    a.out = d_rgb8 ? (unsigned char *) d_rgb8 + x_offset_bytes : nullptr;
    a.pitch = pitch; a.W = d->W; a.H = d->H;
    a.has_prev = d->presented > 0 ? 1 : 0;
    a.bgr = (flags & HPT_DISPLAY_BGR) ? 1 : 0; a.flip = (flags & HPT_DISPLAY_FLIP_Y) ? 1 : 0;
    HIP_TRY(hipMemsetAsync(d->metrics.get(), 0, 2 * sizeof(unsigned long long), st));
    launch_present(st, a);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(d->h_metrics, d->metrics.get(), 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipEventRecord(d->done, st));
    d->presented += 1;
    return HPT_OK;
}

int hpt_display_metrics(hpt_display *d, double *rms_prev, double *rms_other, uint64_t *ssd_prev, uint64_t *ssd_other, int64_t *presented){
    if(!d) return fail(HPT_ERR_INVALID, "null display");
    if(d->presented < 1) return fail(HPT_ERR_INVALID, "hpt_display_metrics before the first hpt_display_present");
    if(int rc = on_device(d->device, "the display")) return rc;
    HIP_TRY(hipEventSynchronize(d->done));
    const uint64_t p = d->h_metrics[0], o = d->h_metrics[1];
    if(rms_prev) *rms_prev = std::sqrt((double) p) / 255.0;
    if(rms_other) *rms_other = std::sqrt((double) o) / 255.0;
    if(ssd_prev) *ssd_prev = p;
    if(ssd_other) *ssd_other = o;
    if(presented) *presented = d->presented;
    return HPT_OK;
}

int hpt_display_reset(hpt_display *d, void *hip_stream){
    if(!d) return fail(HPT_ERR_INVALID, "null display");
    if(int rc = on_device(d->device, "the display")) return rc;
    HIP_TRY(hipMemsetAsync(d->last.get(), 0, (size_t) d->words * sizeof(uint32_t), (hipStream_t) hip_stream));
    d->presented = 0;
    return HPT_OK;
}

} // extern "C"
