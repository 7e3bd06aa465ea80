// The temporal history's host side (include/hpt.h, hpt_history_*): the object that lasts across frames -- two sets of
// per-pixel records, the previous camera, the frame count and the pinned words the counters come back in -- the camera
// constants the kernel reads, and the argument checks, all made before anything touches the device.
#include "hpt_host.h"
#include "history_kernels.h"
#include "guided_kernels.h"

#include <cmath>
#include <new>

using namespace hpt;

namespace {

constexpr long long kMaxPixels = 1ll << 28;          // 3 W H stays below 2^30: 32-bit indices in the kernel

int check_size(int W, int H){
    if(W < 1 || H < 1) return fail(HPT_ERR_INVALID, "image size must be positive");
    if((long long) W * H > kMaxPixels) return fail(HPT_ERR_INVALID, "image too large for the history (at most 2^28 pixels)");
    return HPT_OK;
}

int on_device(int device){
    int dev = -1;
    if(hipGetDevice(&dev) != hipSuccess || dev != device)
        return fail(HPT_ERR_INVALID, "the history lives on another device than the calling thread's current one (hipSetDevice first)");
    return HPT_OK;
}

bool overlap(const void *a, size_t na, const void *b, size_t nb){
    const uintptr_t x = (uintptr_t) a, y = (uintptr_t) b;
    return x < y + nb && y < x + na;
}

struct V3 { float x, y, z; };
V3 sub(V3 a, V3 b){ return V3{ a.x - b.x, a.y - b.y, a.z - b.z }; }
float dot(V3 a, V3 b){ return a.x * b.x + a.y * b.y + a.z * b.z; }
V3 cross(V3 a, V3 b){ return V3{ a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x }; }

// the constants of include/hpt.h, in float, evaluated as written; false for a camera no pixel can be projected with
bool camera_constants(const void *camera, HistoryCamera &c){
    float f[21];
    memcpy(f, camera, HPT_CAMERA_BYTES);
    const V3 eye{ f[0], f[1], f[2] }, UL{ f[12], f[13], f[14] }, dx{ f[15], f[16], f[17] }, dy{ f[18], f[19], f[20] };
    const V3 a = sub(UL, eye), nrm = cross(dx, dy);
    const float an = dot(a, nrm);
    const V3 cu = cross(dy, nrm);
    const float du = dot(dx, cu);
    const V3 gu{ cu.x / du, cu.y / du, cu.z / du };
    const V3 cv = cross(nrm, dx);
    const float dv = dot(dy, cv);
    const V3 gv{ cv.x / dv, cv.y / dv, cv.z / dv };
    const float all[16] = { eye.x, eye.y, eye.z, a.x, a.y, a.z, nrm.x, nrm.y, nrm.z, gu.x, gu.y, gu.z, gv.x, gv.y, gv.z, an };
    for(float v : all) if(!std::isfinite(v)) return false;
    if(an == 0.0f) return false;
    memcpy(c.eye, all + 0, 12); memcpy(c.a, all + 3, 12); memcpy(c.nrm, all + 6, 12); memcpy(c.gu, all + 9, 12); memcpy(c.gv, all + 12, 12);
    c.an = an;
    return true;
}

struct Resolved { float max_history_m1, tol2, normal_min; int plane_on, normal_on; };

int resolve_params(const hpt_history_params *p, Resolved &r){
    hpt_history_params q{ 0.0f, 0.0f, 0.0f, 0 };
    if(p) q = *p;
    if(q.flags != 0) return fail(HPT_ERR_INVALID, "hpt_history_params.flags must be 0");
    if(std::isnan(q.max_history) || std::isnan(q.plane_tolerance) || std::isnan(q.normal_min))
        return fail(HPT_ERR_INVALID, "hpt_history_params: NaN");
    const float mh = q.max_history == 0.0f ? 256.0f : q.max_history;
    if(mh < 1.0f) return fail(HPT_ERR_INVALID, "hpt_history_params.max_history must be at least 1 (0 selects 256)");
    const float tol = q.plane_tolerance == 0.0f ? 0.01f : q.plane_tolerance;
    const float nmin = q.normal_min == 0.0f ? 0.9f : q.normal_min;
    r.max_history_m1 = mh - 1.0f;
    r.plane_on = tol < 0.0f ? 0 : 1;
    r.tol2 = tol * tol;
    r.normal_on = nmin < -1.0f ? 0 : 1;
    r.normal_min = nmin;
    return HPT_OK;
}

// every check of an advance that needs no handle; fills the camera constants and the resolved parameters
int check_advance(int W, int H, const void *camera, const void *frame, const void *normal, const void *position, const void *coverage,
                  const void *prev_position, const hpt_history_params *p, const void *mean_out, HistoryCamera &cam, Resolved &res){
    if(int rc = check_size(W, H)) return rc;
    if(!camera) return fail(HPT_ERR_INVALID, "null camera");
    if(!frame) return fail(HPT_ERR_INVALID, "null frame");
    const int given = (normal ? 1 : 0) + (position ? 1 : 0) + (coverage ? 1 : 0);
    if(given != 0 && given != 3) return fail(HPT_ERR_INVALID, "hpt_history_advance: the guide images are given all three or not at all");
    if(prev_position && given != 3) return fail(HPT_ERR_INVALID, "hpt_history_advance_motion: d_prev_position needs the three guide images");
    if(int rc = resolve_params(p, res)) return rc;
    if(!camera_constants(camera, cam)) return fail(HPT_ERR_INVALID, "hpt_history_advance: degenerate camera (its constants are not finite, or UL - eye lies in the image plane)");
    const size_t npx = (size_t) W * H;
    const void *ptr[5] = { frame, normal, position, coverage, mean_out };
    const size_t bytes[5] = { npx * 12, npx * 12, npx * 12, npx * 4, npx * 12 };
    for(int i = 0; i < 5; ++i) for(int j = i + 1; j < 5; ++j){
        if(!ptr[i] || !ptr[j]) continue;
        if(i == 0 && j == 4 && ptr[i] == ptr[j]) continue;                // in place
        if(overlap(ptr[i], bytes[i], ptr[j], bytes[j]))
            return fail(HPT_ERR_INVALID, "hpt_history_advance: the images must not overlap (d_mean_out may be d_frame_rgb itself)");
    }
    if(prev_position && (overlap(prev_position, npx * 12, frame, npx * 12) || (mean_out && overlap(prev_position, npx * 12, mean_out, npx * 12))))
        return fail(HPT_ERR_INVALID, "hpt_history_advance_motion: d_prev_position must not overlap d_frame_rgb or d_mean_out");
    return HPT_OK;
}

// every check of a variance call that needs no handle; fills the resolved minimum length
int check_variance(int W, int H, int32_t create_flags, const void *fallback, float min_length, const void *out, float &L){
    if(int rc = check_size(W, H)) return rc;
    if(create_flags & ~HPT_HISTORY_MOMENTS) return fail(HPT_ERR_INVALID, "hpt_history_create_flags: unknown flag");
    if(!(create_flags & HPT_HISTORY_MOMENTS))
        return fail(HPT_ERR_INVALID, "hpt_history_variance: the history was created without HPT_HISTORY_MOMENTS");
    if(!out) return fail(HPT_ERR_INVALID, "null variance image");
    L = min_length == 0.0f ? 4.0f : min_length;
    if(!(L >= 2.0f)) return fail(HPT_ERR_INVALID, "hpt_history_variance: min_length must be at least 2 (0 selects 4)");
    const size_t bytes = (size_t) W * H * 12;
    if(fallback && fallback != out && overlap(fallback, bytes, out, bytes))
        return fail(HPT_ERR_INVALID, "hpt_history_variance: the images must not overlap (d_fallback may be d_variance_out itself)");
    return HPT_OK;
}

} // namespace

struct hpt_history {
    int device = 0, W = 0, H = 0;
    uint32_t npx = 0;
    int64_t frames = 0;              // K: advances enqueued since create / reset
    int cur = 0;                     // the set that holds the previous state
    unsigned char camera[HPT_CAMERA_BYTES] = {};
    HistoryCamera cam_prev{};
    int32_t flags = 0;               // HPT_HISTORY_MOMENTS
    DevBuf<float4> mean_n[2], pos_cov[2], nrm[2], sq[2];   // sq: allocated with HPT_HISTORY_MOMENTS only
    DevBuf<unsigned long long> metrics;      // kept, restarted of the advance in flight
    unsigned long long *h_metrics = nullptr; // pinned copy, valid once `done` has passed
    hipEvent_t done = nullptr;
    bool moments() const { return (flags & HPT_HISTORY_MOMENTS) != 0; }
    HistorySet set(int k) const { return HistorySet{ mean_n[k].get(), pos_cov[k].get(), nrm[k].get() }; }
    ~hpt_history(){
        if(done) hipEventDestroy(done);
        if(h_metrics) hipHostFree(h_metrics);
    }
};

extern "C" {

int hpt_history_check(int W, int H, const void *camera, const void *d_frame_rgb, const void *d_normal, const void *d_position,
                      const void *d_coverage, const hpt_history_params *p, const void *d_mean_out){
    return hpt_history_motion_check(W, H, camera, d_frame_rgb, d_normal, d_position, d_coverage, nullptr, p, d_mean_out);
}

int hpt_history_motion_check(int W, int H, const void *camera, const void *d_frame_rgb, const void *d_normal, const void *d_position,
                             const void *d_coverage, const void *d_prev_position, const hpt_history_params *p, const void *d_mean_out){
    HistoryCamera cam; Resolved res;
    return check_advance(W, H, camera, d_frame_rgb, d_normal, d_position, d_coverage, d_prev_position, p, d_mean_out, cam, res);
}

int hpt_history_variance_check(int W, int H, int32_t create_flags, const void *d_fallback, float min_length, const void *d_variance_out){
    float L;
    return check_variance(W, H, create_flags, d_fallback, min_length, d_variance_out, L);
}

int hpt_history_create(int W, int H, hpt_history **out){ return hpt_history_create_flags(W, H, 0, out); }

int hpt_history_create_flags(int W, int H, int32_t flags, hpt_history **out){
    if(!out) return fail(HPT_ERR_INVALID, "null out");
    *out = nullptr;
    if(int rc = check_size(W, H)) return rc;
    if(flags & ~HPT_HISTORY_MOMENTS) return fail(HPT_ERR_INVALID, "hpt_history_create_flags: unknown flag");
    hpt_history *h = new (std::nothrow) hpt_history;
    if(!h) return fail(HPT_ERR_NOMEM, "out of host memory");
    h->W = W; h->H = H; h->npx = (uint32_t) W * (uint32_t) H; h->flags = flags;
    hipError_t e = hipGetDevice(&h->device);
    for(int k = 0; k < 2; ++k){
        if(e == hipSuccess) e = h->mean_n[k].reserve(h->npx);
        if(e == hipSuccess) e = h->pos_cov[k].reserve(h->npx);
        if(e == hipSuccess) e = h->nrm[k].reserve(h->npx);
        if(e == hipSuccess) e = hipMemset(h->mean_n[k].get(), 0, (size_t) h->npx * sizeof(float4));
        if(e == hipSuccess) e = hipMemset(h->pos_cov[k].get(), 0, (size_t) h->npx * sizeof(float4));
        if(e == hipSuccess) e = hipMemset(h->nrm[k].get(), 0, (size_t) h->npx * sizeof(float4));
        if(e == hipSuccess && h->moments()) e = h->sq[k].reserve(h->npx);
        if(e == hipSuccess && h->moments()) e = hipMemset(h->sq[k].get(), 0, (size_t) h->npx * sizeof(float4));
    }
    if(e == hipSuccess) e = h->metrics.reserve(2);
    if(e == hipSuccess) e = hipHostMalloc((void **) &h->h_metrics, 2 * sizeof(unsigned long long), hipHostMallocDefault);
    if(e == hipSuccess) e = hipEventCreateWithFlags(&h->done, hipEventDisableTiming);
    if(e == hipSuccess) e = hipDeviceSynchronize();      // zeroed before a first advance on any stream
    if(e != hipSuccess){ delete h; return fail_hip("history buffers", e); }
    *out = h;
    return HPT_OK;
}

void hpt_history_destroy(hpt_history *h){ delete h; }

int hpt_history_advance(hpt_history *h, const void *camera, const void *d_frame_rgb, const void *d_normal, const void *d_position,
                        const void *d_coverage, const hpt_history_params *p, void *d_mean_out, void *hip_stream){
    return hpt_history_advance_motion(h, camera, d_frame_rgb, d_normal, d_position, d_coverage, nullptr, p, d_mean_out, hip_stream);
}

int hpt_history_advance_motion(hpt_history *h, const void *camera, const void *d_frame_rgb, const void *d_normal, const void *d_position,
                               const void *d_coverage, const void *d_prev_position, const hpt_history_params *p, void *d_mean_out,
                               void *hip_stream){
    if(!h) return fail(HPT_ERR_INVALID, "null history");
    HistoryArgs a{};
    Resolved res;
    if(int rc = check_advance(h->W, h->H, camera, d_frame_rgb, d_normal, d_position, d_coverage, d_prev_position, p, d_mean_out, a.cam, res)) return rc;
    if(int rc = on_device(h->device)) return rc;
    hipStream_t st = (hipStream_t) hip_stream;
    const bool still = h->frames != 0 && memcmp(camera, h->camera, HPT_CAMERA_BYTES) == 0;
    a.mode = h->frames == 0 ? kHistoryFirst : d_prev_position ? kHistoryMotion : still ? kHistoryIdentity : kHistoryMoved;
    a.prev_position = (const float *) d_prev_position; a.still = still ? 1 : 0;
    const int next = a.mode >= kHistoryMoved ? h->cur ^ 1 : h->cur;       // only a moved or motion frame reads other pixels' records
    a.prev = h->set(h->cur); a.next = h->set(next);
    if(h->moments()){ a.sq_prev = h->sq[h->cur].get(); a.sq_next = h->sq[next].get(); }
    a.frame = (const float *) d_frame_rgb; a.normal = (const float *) d_normal; a.position = (const float *) d_position;
    a.coverage = (const float *) d_coverage; a.mean_out = (float *) d_mean_out;
    a.metrics = h->metrics.get();
    a.cam_prev = h->cam_prev;
    a.W = h->W; a.H = h->H;
    a.max_history_m1 = res.max_history_m1; a.tol2 = res.tol2; a.normal_min = res.normal_min;
    a.plane_on = res.plane_on; a.normal_on = res.normal_on;
    HIP_TRY(hipMemsetAsync(h->metrics.get(), 0, 2 * sizeof(unsigned long long), st));
    launch_history_advance(st, a);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(h->h_metrics, h->metrics.get(), 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipEventRecord(h->done, st));
    h->cur = next;
    memcpy(h->camera, camera, HPT_CAMERA_BYTES);
    h->cam_prev = a.cam;
    h->frames += 1;
    return HPT_OK;
}

int hpt_history_metrics(hpt_history *h, uint64_t *kept, uint64_t *restarted, int64_t *frames){
    if(!h) return fail(HPT_ERR_INVALID, "null history");
    if(h->frames < 1) return fail(HPT_ERR_INVALID, "hpt_history_metrics before the first hpt_history_advance");
    if(int rc = on_device(h->device)) return rc;
    HIP_TRY(hipEventSynchronize(h->done));
    if(kept) *kept = h->h_metrics[0];
    if(restarted) *restarted = h->h_metrics[1];
    if(frames) *frames = h->frames;
    return HPT_OK;
}

int hpt_history_read(hpt_history *h, float *mean, float *length, int64_t *frames){
    if(!h) return fail(HPT_ERR_INVALID, "null history");
    if(int rc = on_device(h->device)) return rc;
    HIP_TRY(hipDeviceSynchronize());
    if(mean || length){
        std::vector<float4> rec(h->npx);
        HIP_TRY(hipMemcpy(rec.data(), h->mean_n[h->cur].get(), (size_t) h->npx * sizeof(float4), hipMemcpyDeviceToHost));
        for(size_t k = 0; k < rec.size(); ++k){
            if(mean){ mean[3 * k] = rec[k].x; mean[3 * k + 1] = rec[k].y; mean[3 * k + 2] = rec[k].z; }
            if(length) length[k] = rec[k].w;
        }
    }
    if(frames) *frames = h->frames;
    return HPT_OK;
}

int hpt_history_read_moments(hpt_history *h, float *q){
    if(!h) return fail(HPT_ERR_INVALID, "null history");
    if(!h->moments()) return fail(HPT_ERR_INVALID, "hpt_history_read_moments: the history was created without HPT_HISTORY_MOMENTS");
    if(!q) return fail(HPT_ERR_INVALID, "null moments image");
    if(int rc = on_device(h->device)) return rc;
    HIP_TRY(hipDeviceSynchronize());
    std::vector<float4> rec(h->npx);
    HIP_TRY(hipMemcpy(rec.data(), h->sq[h->cur].get(), (size_t) h->npx * sizeof(float4), hipMemcpyDeviceToHost));
    for(size_t k = 0; k < rec.size(); ++k){ q[3 * k] = rec[k].x; q[3 * k + 1] = rec[k].y; q[3 * k + 2] = rec[k].z; }
    return HPT_OK;
}

int hpt_history_variance(hpt_history *h, const void *d_fallback, float min_length, void *d_variance_out, void *hip_stream){
    if(!h) return fail(HPT_ERR_INVALID, "null history");
    float L;
    if(int rc = check_variance(h->W, h->H, h->flags, d_fallback, min_length, d_variance_out, L)) return rc;
    if(h->frames < 1) return fail(HPT_ERR_INVALID, "hpt_history_variance before the first hpt_history_advance");
    if(int rc = on_device(h->device)) return rc;
    launch_history_variance((hipStream_t) hip_stream, h->mean_n[h->cur].get(), h->sq[h->cur].get(), (const float *) d_fallback,
                            (float *) d_variance_out, h->npx, L);
    HIP_TRY(hipGetLastError());
    return HPT_OK;
}

int hpt_history_length(hpt_history *h, void *d_length_out, void *hip_stream){
    if(!h) return fail(HPT_ERR_INVALID, "null history");
    if(!d_length_out) return fail(HPT_ERR_INVALID, "null length image");
    if(h->frames < 1) return fail(HPT_ERR_INVALID, "hpt_history_length before the first hpt_history_advance");
    if(int rc = on_device(h->device)) return rc;
    launch_take_fourth_word((hipStream_t) hip_stream, h->mean_n[h->cur].get(), (float *) d_length_out, h->npx);
    HIP_TRY(hipGetLastError());
    return HPT_OK;
}

int hpt_history_reset(hpt_history *h, void *hip_stream){
    if(!h) return fail(HPT_ERR_INVALID, "null history");
    if(int rc = on_device(h->device)) return rc;
    hipStream_t st = (hipStream_t) hip_stream;
    HIP_TRY(hipMemsetAsync(h->mean_n[h->cur].get(), 0, (size_t) h->npx * sizeof(float4), st));
    HIP_TRY(hipMemsetAsync(h->pos_cov[h->cur].get(), 0, (size_t) h->npx * sizeof(float4), st));
    HIP_TRY(hipMemsetAsync(h->nrm[h->cur].get(), 0, (size_t) h->npx * sizeof(float4), st));
    if(h->moments()) HIP_TRY(hipMemsetAsync(h->sq[h->cur].get(), 0, (size_t) h->npx * sizeof(float4), st));
    h->frames = 0;
    return HPT_OK;
}

} // extern "C"
