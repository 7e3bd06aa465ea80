// The denoiser's host side (include/hpt.h, hpt_denoiser_* and hpt_denoise_host): the object with its packed guides and
// ping-pong colour buffers, the argument checks, the per-level constants and the optional HIP-event timing; and, on the
// same object, the variance-guided filter and the spatial variance estimate (hpt_denoiser_run_guided,
// hpt_denoiser_estimate_variance, hpt_guided_check).
#include "hpt_host.h"
#include "guided_kernels.h"

#include <cfloat>
#include <cmath>
#include <new>

using namespace hpt;

static_assert(sizeof(hpt_denoise_params) == 20, "ABI record: keep path_tracing_amd/__init__.py (DenoiseParams) in step");
static_assert(sizeof(hpt_guided_params) == 20, "ABI record: keep path_tracing_amd/__init__.py (GuidedParams) in step");

namespace {

constexpr int kMaxLevels = 8;
constexpr int32_t kDenoiseFlags = HPT_DENOISE_DEMODULATE | HPT_DENOISE_TIME;

} // namespace

struct hpt_denoiser {
    int device = 0, W = 0, H = 0;
    size_t npx = 0;
    DevBuf<float4> nrm_cov, pos, alb, ping[2];
    DenoiseGuides g{};
    bool guides_set = false;
    // HPT_DENOISE_TIME: events around the colour pack (0, 1) and after every level (2 ..), of the last timed run
    hipEvent_t ev[kMaxLevels + 2] = {};
    int timed_levels = 0;            // 0: the last run was not timed
    ~hpt_denoiser(){ for(hipEvent_t e : ev) if(e) hipEventDestroy(e); }
};

namespace {

int on_denoiser_device(const hpt_denoiser *d){
    int dev = -1;
    if(hipGetDevice(&dev) != hipSuccess || dev != d->device)
        return fail(HPT_ERR_INVALID, "the denoiser lives on another device than the calling thread's current one (hipSetDevice first)");
    return HPT_OK;
}

// *p (zeros for null) with the defaults filled in; a sigma < 0 stays negative (term off)
int take_denoise_params(const hpt_denoise_params *p, hpt_denoise_params &D){
    memset(&D, 0, sizeof D);
    if(p) D = *p;
    if(D.flags & ~kDenoiseFlags) return fail(HPT_ERR_INVALID, "hpt_denoise_params.flags: HPT_DENOISE_DEMODULATE and HPT_DENOISE_TIME only");
    if(D.iterations < 0 || D.iterations > kMaxLevels) return fail(HPT_ERR_INVALID, "hpt_denoise_params.iterations must be in [0, 8]");
    if(D.iterations == 0) D.iterations = 5;
    if(D.sigma_color != D.sigma_color || D.sigma_normal != D.sigma_normal || D.sigma_position != D.sigma_position)
        return fail(HPT_ERR_INVALID, "hpt_denoise_params: a sigma is NaN");
    if(D.sigma_color == 0.0f) D.sigma_color = 1.0f;
    if(D.sigma_normal == 0.0f) D.sigma_normal = 0.5f;
    if(D.sigma_position == 0.0f) D.sigma_position = 0.05f;
    return HPT_OK;
}

// 1 / (s * s), FLT_MAX where s * s is so small that the quotient overflows: an infinite inverse would turn the centre
// tap's zero difference into NaN (include/hpt.h, "the filter")
float inv_sq(float s){ return fminf(1.0f / (s * s), FLT_MAX); }

bool overlap(const void *a, const void *b, size_t bytes){
    const uintptr_t x = (uintptr_t) a, y = (uintptr_t) b;
    return x < y + bytes && y < x + bytes;
}
bool overlap2(const void *a, size_t na, const void *b, size_t nb){
    const uintptr_t x = (uintptr_t) a, y = (uintptr_t) b;
    return x < y + nb && y < x + na;
}

// *p (zeros for null) with the defaults filled in; `filter` false (the estimator) reads the flags and the two guide sigmas only
int take_guided_params(const hpt_guided_params *p, hpt_guided_params &D, bool filter){
    memset(&D, 0, sizeof D);
    if(p) D = *p;
    if(D.flags & ~kDenoiseFlags) return fail(HPT_ERR_INVALID, "hpt_guided_params.flags: HPT_DENOISE_DEMODULATE and HPT_DENOISE_TIME only");
    if(filter){
        if(D.iterations < 0 || D.iterations > kMaxLevels) return fail(HPT_ERR_INVALID, "hpt_guided_params.iterations must be in [0, 8]");
        if(D.iterations == 0) D.iterations = 5;
        if(D.sigma_color != D.sigma_color) return fail(HPT_ERR_INVALID, "hpt_guided_params: a sigma is NaN");
        if(D.sigma_color == 0.0f) D.sigma_color = 2.0f;
    }
    if(D.sigma_normal != D.sigma_normal || D.sigma_position != D.sigma_position) return fail(HPT_ERR_INVALID, "hpt_guided_params: a sigma is NaN");
    if(D.sigma_normal == 0.0f) D.sigma_normal = 0.5f;
    if(D.sigma_position == 0.0f) D.sigma_position = 0.05f;
    return HPT_OK;
}

int check_image_size(int W, int H){
    if(W <= 0 || H <= 0) return fail(HPT_ERR_INVALID, "image size must be positive");
    if((long long) W * H > (1ll << 28)) return fail(HPT_ERR_INVALID, "image too large for the denoiser (at most 2^28 pixels)");
    return HPT_OK;
}

// every check of a guided run that needs no handle; fills the resolved parameters
int check_guided(int W, int H, const void *rgb, const void *variance, const void *out, const void *variance_out,
                 const hpt_guided_params *p, hpt_guided_params &D){
    if(int rc = check_image_size(W, H)) return rc;
    if(!rgb || !out) return fail(HPT_ERR_INVALID, "null image");
    if(!variance) return fail(HPT_ERR_INVALID, "null variance image");
    const size_t npx = (size_t) W * H, b3 = npx * 3 * sizeof(float), b1 = npx * sizeof(float);
    if(overlap2(out, b3, rgb, b3) || overlap2(out, b3, variance, b3))
        return fail(HPT_ERR_INVALID, "hpt_denoiser_run_guided: d_out must not overlap d_linear_rgb or d_variance");
    if(variance_out && (overlap2(variance_out, b1, rgb, b3) || overlap2(variance_out, b1, variance, b3) || overlap2(variance_out, b1, out, b3)))
        return fail(HPT_ERR_INVALID, "hpt_denoiser_run_guided: d_variance_out must not overlap another image");
    return take_guided_params(p, D, true);
}

} // namespace

extern "C" {

int hpt_denoiser_create(int W, int H, hpt_denoiser **out){
    if(!out) return fail(HPT_ERR_INVALID, "null out");
    *out = nullptr;
    if(W <= 0 || H <= 0) return fail(HPT_ERR_INVALID, "image size must be positive");
    if((long long) W * H > (1ll << 28)) return fail(HPT_ERR_INVALID, "image too large for the denoiser (at most 2^28 pixels)");
    hpt_denoiser *d = new (std::nothrow) hpt_denoiser;
    if(!d) return fail(HPT_ERR_NOMEM, "out of host memory");
    d->W = W; d->H = H; d->npx = (size_t) W * H;
    hipError_t e = hipGetDevice(&d->device);
    if(e == hipSuccess) e = reserve_all(d->npx, d->nrm_cov, d->pos, d->alb, d->ping[0], d->ping[1]);
    if(e != hipSuccess){ delete d; return fail_hip("denoiser buffers", e); }
    d->g = DenoiseGuides{ d->nrm_cov.get(), d->pos.get(), d->alb.get() };
    *out = d;
    return HPT_OK;
}

void hpt_denoiser_destroy(hpt_denoiser *d){ delete d; }

int hpt_denoiser_set_guides(hpt_denoiser *d, const void *d_albedo, const void *d_normal, const void *d_position,
                            const void *d_coverage, void *hip_stream){
    if(!d) return fail(HPT_ERR_INVALID, "null denoiser");
    if(!d_albedo || !d_normal || !d_position || !d_coverage) return fail(HPT_ERR_INVALID, "null guide image");
    if(int rc = on_denoiser_device(d)) return rc;
    launch_denoise_pack((hipStream_t) hip_stream, (const float *) d_albedo, (const float *) d_normal, (const float *) d_position,
                        (const float *) d_coverage, d->g, d->npx);
    HIP_TRY(hipGetLastError());
    d->guides_set = true;
    return HPT_OK;
}

int hpt_denoiser_run(hpt_denoiser *d, const void *d_linear_rgb, void *d_out, const hpt_denoise_params *p, void *hip_stream){
    if(!d) return fail(HPT_ERR_INVALID, "null denoiser");
    if(!d_linear_rgb || !d_out) return fail(HPT_ERR_INVALID, "null image");
    if(overlap(d_linear_rgb, d_out, d->npx * 3 * sizeof(float))) return fail(HPT_ERR_INVALID, "hpt_denoiser_run: d_out must not overlap d_linear_rgb");
    if(!d->guides_set) return fail(HPT_ERR_INVALID, "hpt_denoiser_run before hpt_denoiser_set_guides");
    hpt_denoise_params D;
    if(int rc = take_denoise_params(p, D)) return rc;
    if(int rc = on_denoiser_device(d)) return rc;
    hipStream_t st = (hipStream_t) hip_stream;
    const bool timed = (D.flags & HPT_DENOISE_TIME) != 0;
    const int demod = (D.flags & HPT_DENOISE_DEMODULATE) ? 1 : 0;
    d->timed_levels = 0;
    if(timed) for(int k = 0; k < D.iterations + 2; ++k) if(!d->ev[k]) HIP_TRY(hipEventCreate(&d->ev[k]));

    if(timed) HIP_TRY(hipEventRecord(d->ev[0], st));
    launch_denoise_pack_color(st, (const float *) d_linear_rgb, d->g, d->ping[0].get(), d->npx, demod);
    if(timed) HIP_TRY(hipEventRecord(d->ev[1], st));
    DenoiseLevel L{};
    L.W = d->W; L.H = d->H; L.demod = demod;
    L.use_c = D.sigma_color > 0.0f; L.use_n = D.sigma_normal > 0.0f; L.use_p = D.sigma_position > 0.0f;
    L.inv_n = L.use_n ? inv_sq(D.sigma_normal) : 0.0f;
    L.inv_p = L.use_p ? inv_sq(D.sigma_position) : 0.0f;
    for(int k = 0; k < D.iterations; ++k){
        L.stride = 1 << k;
        const float sc = D.sigma_color * ldexpf(1.0f, -k);      // the colour tolerance halves per level
        L.inv_c = L.use_c ? inv_sq(sc) : 0.0f;
        const int last = k + 1 == D.iterations;
        launch_atrous(st, L, d->g, d->ping[k & 1].get(), d->ping[(k + 1) & 1].get(), (float *) d_out, last);
        if(timed) HIP_TRY(hipEventRecord(d->ev[k + 2], st));
    }
    HIP_TRY(hipGetLastError());
    if(timed) d->timed_levels = D.iterations;
    return HPT_OK;
}

int hpt_guided_check(int W, int H, const void *d_linear_rgb, const void *d_variance, const void *d_out, const void *d_variance_out,
                     const hpt_guided_params *p){
    hpt_guided_params D;
    return check_guided(W, H, d_linear_rgb, d_variance, d_out, d_variance_out, p, D);
}

int hpt_denoiser_run_guided(hpt_denoiser *d, const void *d_linear_rgb, const void *d_variance, void *d_out, void *d_variance_out,
                            const hpt_guided_params *p, void *hip_stream){
    if(!d) return fail(HPT_ERR_INVALID, "null denoiser");
    hpt_guided_params D;
    if(int rc = check_guided(d->W, d->H, d_linear_rgb, d_variance, d_out, d_variance_out, p, D)) return rc;
    if(!d->guides_set) return fail(HPT_ERR_INVALID, "hpt_denoiser_run_guided before hpt_denoiser_set_guides");
    if(int rc = on_denoiser_device(d)) return rc;
    hipStream_t st = (hipStream_t) hip_stream;
    const bool timed = (D.flags & HPT_DENOISE_TIME) != 0;
    const int demod = (D.flags & HPT_DENOISE_DEMODULATE) ? 1 : 0;
    d->timed_levels = 0;
    if(timed) for(int k = 0; k < D.iterations + 2; ++k) if(!d->ev[k]) HIP_TRY(hipEventCreate(&d->ev[k]));

    if(timed) HIP_TRY(hipEventRecord(d->ev[0], st));
    launch_guided_pack(st, (const float *) d_linear_rgb, (const float *) d_variance, d->g, d->ping[0].get(), d->npx, demod);
    if(timed) HIP_TRY(hipEventRecord(d->ev[1], st));
    GuidedLevel L{};
    L.W = d->W; L.H = d->H; L.demod = demod;
    L.use_c = D.sigma_color > 0.0f; L.use_n = D.sigma_normal > 0.0f; L.use_p = D.sigma_position > 0.0f;
    L.s2 = L.use_c ? D.sigma_color * D.sigma_color : 0.0f;      // not halved per level: the shrinking variance narrows it
    L.inv_n = L.use_n ? inv_sq(D.sigma_normal) : 0.0f;
    L.inv_p = L.use_p ? inv_sq(D.sigma_position) : 0.0f;
    for(int k = 0; k < D.iterations; ++k){
        L.stride = 1 << k;
        const int last = k + 1 == D.iterations;
        launch_atrous_guided(st, L, d->g, d->ping[k & 1].get(), d->ping[(k + 1) & 1].get(), (float *) d_out, (float *) d_variance_out, last);
        if(timed) HIP_TRY(hipEventRecord(d->ev[k + 2], st));
    }
    HIP_TRY(hipGetLastError());
    if(timed) d->timed_levels = D.iterations;
    return HPT_OK;
}

int hpt_denoiser_estimate_variance(hpt_denoiser *d, const void *d_frame_rgb, const void *d_length, void *d_variance_out,
                                   const hpt_guided_params *p, void *hip_stream){
    if(!d) return fail(HPT_ERR_INVALID, "null denoiser");
    if(!d_frame_rgb) return fail(HPT_ERR_INVALID, "null frame");
    if(!d_variance_out) return fail(HPT_ERR_INVALID, "null variance image");
    const size_t b3 = d->npx * 3 * sizeof(float), b1 = d->npx * sizeof(float);
    if(overlap2(d_variance_out, b3, d_frame_rgb, b3) || (d_length && overlap2(d_variance_out, b3, d_length, b1)))
        return fail(HPT_ERR_INVALID, "hpt_denoiser_estimate_variance: d_variance_out must not overlap d_frame_rgb or d_length");
    hpt_guided_params D;
    if(int rc = take_guided_params(p, D, false)) return rc;
    if(!d->guides_set) return fail(HPT_ERR_INVALID, "hpt_denoiser_estimate_variance before hpt_denoiser_set_guides");
    if(int rc = on_denoiser_device(d)) return rc;
    VarianceArgs A{};
    A.W = d->W; A.H = d->H;
    A.use_n = D.sigma_normal > 0.0f; A.use_p = D.sigma_position > 0.0f;
    A.inv_n = A.use_n ? inv_sq(D.sigma_normal) : 0.0f;
    A.inv_p = A.use_p ? inv_sq(D.sigma_position) : 0.0f;
    A.frame = (const float *) d_frame_rgb; A.length = (const float *) d_length; A.out = (float *) d_variance_out;
    launch_variance_spatial((hipStream_t) hip_stream, A, d->g);
    HIP_TRY(hipGetLastError());
    return HPT_OK;
}

int hpt_denoiser_level_ms(const hpt_denoiser *d, double *ms_levels, int cap){
    if(!d || !ms_levels || cap < 0) return fail(HPT_ERR_INVALID, "null argument");
    if(d->timed_levels == 0) return fail(HPT_ERR_INVALID, "the last hpt_denoiser_run or hpt_denoiser_run_guided was not timed (HPT_DENOISE_TIME)");
    if(int rc = on_denoiser_device(d)) return rc;
    HIP_TRY(hipEventSynchronize(d->ev[d->timed_levels + 1]));
    for(int k = 0; k < cap; ++k){
        float ms = 0.0f;
        if(k < d->timed_levels) HIP_TRY(hipEventElapsedTime(&ms, d->ev[k + 1], d->ev[k + 2]));
        ms_levels[k] = ms;
    }
    return HPT_OK;
}

int hpt_denoiser_last_ms(const hpt_denoiser *d, double *ms_pack, double *ms_filter){
    if(!d) return fail(HPT_ERR_INVALID, "null denoiser");
    if(d->timed_levels == 0) return fail(HPT_ERR_INVALID, "the last hpt_denoiser_run or hpt_denoiser_run_guided was not timed (HPT_DENOISE_TIME)");
    if(int rc = on_denoiser_device(d)) return rc;
    HIP_TRY(hipEventSynchronize(d->ev[d->timed_levels + 1]));
    float a = 0.0f, b = 0.0f;
    HIP_TRY(hipEventElapsedTime(&a, d->ev[0], d->ev[1]));
    HIP_TRY(hipEventElapsedTime(&b, d->ev[1], d->ev[d->timed_levels + 1]));
    if(ms_pack) *ms_pack = a;
    if(ms_filter) *ms_filter = b;
    return HPT_OK;
}

int hpt_denoise_host(const float *linear_rgb, const float *albedo, const float *normal, const float *position,
                     const float *coverage, float *out, int W, int H, const hpt_denoise_params *p){
    if(!linear_rgb || !albedo || !normal || !position || !coverage || !out) return fail(HPT_ERR_INVALID, "null image");
    hpt_denoise_params D;
    if(int rc = take_denoise_params(p, D)) return rc;
    hpt_denoiser *d = nullptr;
    if(int rc = hpt_denoiser_create(W, H, &d)) return rc;
    const size_t npx = d->npx;
    DevBuf<float> in[5], d_out;      // colour, albedo, normal, position, coverage
    const float *src[5] = { linear_rgb, albedo, normal, position, coverage };
    auto body = [&]() -> int {
        for(int k = 0; k < 5; ++k){
            const size_t n = npx * (k == 4 ? 1 : 3);
            HIP_TRY(in[k].reserve(n));
            HIP_TRY(hipMemcpy(in[k].get(), src[k], n * sizeof(float), hipMemcpyHostToDevice));
        }
        HIP_TRY(d_out.reserve(npx * 3));
        if(int rc = hpt_denoiser_set_guides(d, in[1].get(), in[2].get(), in[3].get(), in[4].get(), nullptr)) return rc;
        if(int rc = hpt_denoiser_run(d, in[0].get(), d_out.get(), p, nullptr)) return rc;
        HIP_TRY(hipMemcpy(out, d_out.get(), npx * 3 * sizeof(float), hipMemcpyDeviceToHost));
        return HPT_OK;
    };
    const int rc = body();
    hipDeviceSynchronize();          // nothing of this call is in flight when its buffers go
    hpt_denoiser_destroy(d);
    return rc;
}

} // extern "C"
