// C ABI of libhpt.so (include/hpt.h) outside the render loops: the error text, scene upload and destruction, the steps
// every integrator shares (hpt_host.h), statistics, probes, the 8-bit output stage and the one-shot wrappers with their
// cache.  The integrators are in render_pt.cpp, render_bdpt.cpp and render_ppm.cpp.  Compiled with hipcc (host code only here).
#include "hpt_host.h"

#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <ctime>
#include <mutex>
#include <new>

using namespace hpt;

static_assert(sizeof(hpt_stats) == 312 && sizeof(hpt_params) == 40, "ABI records: keep path_tracing_amd/__init__.py and tests/test_boundary.py in step");

namespace {

thread_local std::string g_err;

} // namespace

namespace hpt {

int fail(int code, const std::string &msg){ g_err = msg; return code; }

int make_tiling(int W, int H, const hpt_params *p, Tiling &tl){
    if(W <= 0 || H <= 0) return fail(HPT_ERR_INVALID, "image size must be positive");
    int world = (p && p->world > 1) ? p->world : 1;
    int rank = (p && p->world > 1) ? p->rank : 0;
    int tile = (p && p->tile > 0) ? p->tile : 32;
    if(tile % 8 != 0 || tile > 1024) return fail(HPT_ERR_INVALID, "tile must be a multiple of 8 (<= 1024)");
    if(rank < 0 || rank >= world) return fail(HPT_ERR_INVALID, "rank outside [0, world)");
    tl.W = W; tl.H = H; tl.tile = tile;
    tl.tiles_x = (W + tile - 1) / tile; tl.tiles_y = (H + tile - 1) / tile;
    tl.ntiles = tl.tiles_x * tl.tiles_y;
    tl.rank = rank; tl.world = world;
    long long per_rank = (tl.ntiles + world - 1) / world;
    long long n_local = per_rank * tile * tile;
    if(n_local > 0x7FFFFFFFll) return fail(HPT_ERR_INVALID, "local framebuffer too large");
    tl.n_local = (int) n_local;
    return HPT_OK;
}

// The scene's buffers live on the device that was current when it was created; launching from a thread whose current
// device is another one would hand those pointers to the wrong GPU (a fault, not an error code).
int on_scene_device(const hpt_scene *s){
    int dev = -1;
    if(hipGetDevice(&dev) != hipSuccess || dev != s->device)
        return fail(HPT_ERR_INVALID, "the scene lives on another device than the calling thread's current one (hipSetDevice first)");
    return HPT_OK;
}

// hpt_params may only hold the documented bits: a stray bit is an error, not a silently different render
int take_params(const hpt_params *params, const ParamRules &rules, hpt_params &P){
    memset(&P, 0, sizeof P);
    if(params) P = *params;
    char msg[160];
    if(rules.one_device && P.world > 1) return fail(HPT_ERR_INVALID, rules.one_device);
    if(P.flags & ~rules.flags){
        snprintf(msg, sizeof msg, "hpt_params.flags: unknown bits 0x%x (HPT_FLAG_* are 0x%x)", (unsigned) (P.flags & ~rules.flags), (unsigned) rules.flags);
        return fail(HPT_ERR_INVALID, rules.flags_msg ? rules.flags_msg : msg);
    }
    if(P.reserved & ~rules.reserved){
        snprintf(msg, sizeof msg, "hpt_params.reserved: bits 0x%x set; only bits 1-6 (the trace budget) may be", (unsigned) (P.reserved & ~rules.reserved));
        return fail(HPT_ERR_INVALID, rules.reserved_msg ? rules.reserved_msg : msg);
    }
    if(P.max_delta <= 0) P.max_delta = 64;
    if(P.max_delta > 250) P.max_delta = 250;
    return HPT_OK;
}

int ensure_own_image(hpt_scene *s, const Tiling &tl){
    HIP_TRY(s->ws.local_own.reserve((size_t) tl.n_local * 3));
    HIP_TRY(s->ws.image_own.reserve((size_t) tl.W * tl.H * 3));
    return HPT_OK;
}

int untile_to_host(hpt_scene *s, const Tiling &tl, hipStream_t st, float *host_image, hipEvent_t after){
    launch_untile(st, tl, s->ws.local_own.get(), s->ws.image_own.get());
    if(after) HIP_TRY(hipEventRecord(after, st));
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(host_image, s->ws.image_own.get(), (size_t) tl.W * tl.H * 3 * sizeof(float), hipMemcpyDeviceToHost));
    return HPT_OK;
}

} // namespace hpt

namespace {

int collect_stats(hpt_scene *s){
    if(!s->tm.stats_pending) return HPT_OK;
    HIP_TRY(hipEventSynchronize(s->tm.ev_stop));
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, s->tm.ev_start, s->tm.ev_stop));
    s->tm.stats.ms_total = ms;
    double sum[5] = { 0, 0, 0, 0, 0 }; uint32_t cnt[5] = { 0, 0, 0, 0, 0 };
    for(const TimedLaunch &t : s->tm.timed){
        float e = 0.f;
        if(hipEventElapsedTime(&e, t.a, t.b) == hipSuccess){ sum[t.cls] += e; cnt[t.cls]++; }
    }
    s->tm.stats.ms_extend = sum[0]; s->tm.stats.ms_shade = sum[1]; s->tm.stats.ms_connect = sum[2]; s->tm.stats.ms_other = sum[3];
    s->tm.stats.n_extend = cnt[0]; s->tm.stats.n_shade = cnt[1]; s->tm.stats.n_connect = cnt[2]; s->tm.stats.n_other = cnt[3];
    s->tm.stats.ms_resume = sum[4]; s->tm.stats.n_resume = cnt[4];
    s->tm.stats.split_budget = (uint32_t) s->ws.last_budget;
    s->tm.stats.traced_rays_last_pass = s->tm.stats.long_rays_last_pass = 0;
    if(s->ws.last_counter_stride > 0 && s->ws.last_counters){
        std::vector<uint32_t> h((size_t) 4 * s->ws.last_counter_stride);
        HIP_TRY(hipMemcpy(h.data(), s->ws.last_counters, h.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
        for(int i = 0; i < s->ws.last_counter_stride; ++i){
            s->tm.stats.traced_rays_last_pass += (uint64_t) h[i] + h[(size_t) s->ws.last_counter_stride + i];
            s->tm.stats.long_rays_last_pass += (uint64_t) h[(size_t) 2 * s->ws.last_counter_stride + i] + h[(size_t) 3 * s->ws.last_counter_stride + i];
        }
    }
    WorkCounters wc;
    HIP_TRY(hipMemcpy(&wc, s->ws.wc.get(), sizeof wc, hipMemcpyDeviceToHost));
    s->tm.stats.samples = wc.samples; s->tm.stats.closest_rays = wc.closest_rays; s->tm.stats.shadow_rays = wc.shadow_rays;
    s->tm.stats.boxes_closest = wc.boxes_closest; s->tm.stats.tris_closest = wc.tris_closest;
    s->tm.stats.boxes_shadow = wc.boxes_shadow; s->tm.stats.tris_shadow = wc.tris_shadow; s->tm.stats.path_iters = wc.path_iters;
    s->tm.stats.lane_steps_closest = wc.lane_steps_closest; s->tm.stats.wave_steps_closest = wc.wave_steps_closest;
    s->tm.stats.lane_steps_shadow = wc.lane_steps_shadow; s->tm.stats.wave_steps_shadow = wc.wave_steps_shadow;
    s->tm.stats.leaf_lane_closest = wc.leaf_lane_closest; s->tm.stats.leaf_wave_closest = wc.leaf_wave_closest;
    s->tm.stats.leaf_lane_shadow = wc.leaf_lane_shadow; s->tm.stats.leaf_wave_shadow = wc.leaf_wave_shadow;
    s->tm.stats.bd_pairs = wc.bd_pairs; s->tm.stats.bd_survivors = wc.bd_survivors; s->tm.stats.bd_shadow_rays = wc.bd_shadow_rays;
    s->tm.stats.bd_unoccluded = wc.bd_unoccluded; s->tm.stats.bd_nodes = wc.bd_nodes; s->tm.stats.bd_tris = wc.bd_tris;
    s->tm.stats.bd_spheres = wc.bd_spheres; s->tm.stats.bd_group_boxes = wc.bd_group_boxes;
    s->tm.stats_pending = false;
    return HPT_OK;
}

// what the one-shot wrappers keep between calls (include/hpt.h, hpt_pt_render_wrapper): the scene of the current
// device, or -- when more than one device is configured (hpt_wrapper_set_devices / HPT_DEVICES) -- the fan-out
struct WrapperCache { std::mutex mu; hpt_scene *scene = nullptr; int device = -1; hpt_multi *multi = nullptr; int devices = 0; } g_wrap;

bool wrapper_cache_enabled(){
    static const bool on = [](){ const char *e = getenv("HPT_WRAPPER_CACHE"); return !(e && e[0] == '0'); }();
    return on;
}

// number of devices the one-shot wrappers render on: hpt_wrapper_set_devices(), else HPT_DEVICES, else 1
int wrapper_devices(){
    if(g_wrap.devices > 0) return g_wrap.devices;
    static const int from_env = [](){ const char *e = getenv("HPT_DEVICES"); int v = e ? atoi(e) : 1; return v > 0 ? v : 1; }();
    return from_env;
}

// g_wrap.mu held.  The kept scene when the arrays are byte-identical to the ones it was built from, else a new one.
int wrapper_scene(const void *lights, int nl, const void *spheres, int ns, const void *tris, int nt, hpt_scene **out){
    int dev = -1;
    if(hipGetDevice(&dev) != hipSuccess) dev = -1;
    hpt_scene *k = g_wrap.scene;
    if(k && wrapper_cache_enabled() && dev == g_wrap.device && nl == k->geo.nl && ns == k->geo.ns && nt == k->geo.nt && nl >= 0 && ns >= 0 && nt >= 0 &&
       same_bytes(k->geo.h_lights, lights, (size_t) nl * HPT_LIGHT_BYTES) && same_bytes(k->geo.h_spheres, spheres, (size_t) ns * HPT_SPHERE_BYTES) &&
       same_bytes(k->geo.h_tris, tris, (size_t) nt * HPT_TRIANGLE_BYTES)){
        *out = k;
        return HPT_OK;
    }
    if(k){ hpt_scene_destroy(k); g_wrap.scene = nullptr; g_wrap.device = -1; }
    int rc = hpt_scene_create(lights, nl, spheres, ns, tris, nt, out);
    if(rc) return rc;
    if(wrapper_cache_enabled()){ g_wrap.scene = *out; g_wrap.device = dev; }
    return HPT_OK;
}

// g_wrap.mu held: a scene that is not kept is destroyed (the error text of the render survives)
void wrapper_release(hpt_scene *s){
    if(s == g_wrap.scene) return;
    std::string keep = g_err;
    hpt_scene_destroy(s);
    g_err = keep;
}

// g_wrap.mu held: the kept fan-out over `devices` devices for these arrays, else a new one
int wrapper_multi(int devices, const void *lights, int nl, const void *spheres, int ns, const void *tris, int nt, hpt_multi **out){
    if(g_wrap.multi && wrapper_cache_enabled() && hpt::multi_matches(g_wrap.multi, devices, lights, nl, spheres, ns, tris, nt)){
        *out = g_wrap.multi;
        return HPT_OK;
    }
    if(g_wrap.multi){ hpt_multi_destroy(g_wrap.multi); g_wrap.multi = nullptr; }
    int rc = hpt_multi_create(lights, nl, spheres, ns, tris, nt, nullptr, devices, 0, out);
    if(rc) return rc;
    if(wrapper_cache_enabled()) g_wrap.multi = *out;
    return HPT_OK;
}

void wrapper_release_multi(hpt_multi *m){
    if(m == g_wrap.multi) return;
    std::string keep = g_err;
    hpt_multi_destroy(m);
    g_err = keep;
}

// the zeroed hpt_params of a one-shot call; a negative seed stands for the reference's clock seed (time(NULL),
// pt_cu.cu:282; time(NULL) + 1234, ppm_cu.cu:358)
hpt_params wrapper_params(int64_t seed){
    hpt_params p; memset(&p, 0, sizeof p);
    p.seed = seed >= 0 ? (uint64_t) seed : (uint64_t) time(nullptr);
    return p;
}

// One blocking render of these arrays: `one` on the kept scene, or -- more than one device configured -- `many` on the
// kept fan-out, which spreads the image tiles over the node's devices internally (RCCL gather): hpt_multi.cpp
template <typename One, typename Many>
int wrapper_render(const void *lights, int nl, const void *spheres, int ns, const void *tris, int nt, One one, Many many){
    std::lock_guard<std::mutex> lock(g_wrap.mu);
    if(wrapper_devices() > 1){
        hpt_multi *m = nullptr;
        int rc = wrapper_multi(wrapper_devices(), lights, nl, spheres, ns, tris, nt, &m);
        if(rc) return rc;
        rc = many(m);
        wrapper_release_multi(m);
        return rc;
    }
    hpt_scene *s = nullptr;
    int rc = wrapper_scene(lights, nl, spheres, ns, tris, nt, &s);
    if(rc) return rc;
    rc = one(s);
    wrapper_release(s);
    return rc;
}

} // namespace

namespace hpt {

// Uploads a flattened scene to the current device (hpt_scene_create = build_host_scene + this; the multi-device
// fan-out builds once and uploads to every device).
int scene_upload(const HostScene &hs, const void *lights, int nl, const void *spheres, int ns, const void *tris, int nt,
                 hpt_scene **out){
    *out = nullptr;
    hpt_scene *s = new (std::nothrow) hpt_scene();
    if(!s) return fail(HPT_ERR_NOMEM, "out of host memory");
    auto t0 = std::chrono::steady_clock::now();
    hipError_t e = hipGetDevice(&s->device);
    if(e == hipSuccess){ hipDeviceProp_t prop; if(hipGetDeviceProperties(&prop, s->device) == hipSuccess && prop.multiProcessorCount > 0) s->num_cus = prop.multiProcessorCount; }
    if(e == hipSuccess) e = s->geo.nodes.upload(hs.nodes);
    if(e == hipSuccess) e = s->geo.qnodes.upload(hs.qnodes);
    if(e == hipSuccess) e = s->geo.wnodes.upload(hs.wnodes);
    if(e == hipSuccess) e = s->geo.tris.upload(hs.tris);
    if(e == hipSuccess) e = s->geo.rounds.upload(hs.rounds);
    if(e == hipSuccess) e = s->geo.mats.upload(hs.materials);
    if(e == hipSuccess) e = s->geo.lights.upload(hs.lights);
    if(e != hipSuccess){ hpt_scene_destroy(s); return fail_hip("scene upload", e); }
    e = s->geo.tri_frames.reserve(std::max<size_t>((size_t) nt, 1) * 4);
    if(e == hipSuccess){
        launch_tri_frames(nullptr, (const float4 *) s->geo.tris.get(), nt, s->geo.tri_frames.get());
        e = hipDeviceSynchronize();
    }
    if(e != hipSuccess){ hpt_scene_destroy(s); return fail_hip("triangle frames", e); }
    auto t1 = std::chrono::steady_clock::now();
    s->geo.sd.nodes = (const float4 *) s->geo.nodes.get(); s->geo.sd.tris = (const float4 *) s->geo.tris.get();
    s->geo.sd.tri_frames = s->geo.tri_frames.get();
    s->geo.sd.qnodes = (const uint4 *) s->geo.qnodes.get();
    s->geo.sd.wnodes = (const uint4 *) s->geo.wnodes.get(); s->geo.sd.wide_depth = hs.wide_depth;
    for(int a = 0; a < 3; ++a){ s->geo.sd.qorigin[a] = hs.qorigin[a]; s->geo.sd.qscale[a] = hs.qscale[a]; }
    s->geo.sd.rounds = s->geo.rounds.get(); s->geo.sd.mats = s->geo.mats.get(); s->geo.sd.lights = s->geo.lights.get();
    s->geo.sd.num_rounds = ns + nl; s->geo.sd.num_spheres = ns; s->geo.sd.num_lights = nl; s->geo.sd.num_tris = nt;
    s->geo.sd.num_mats = (int) hs.materials.size(); s->geo.sd.num_nodes = (int) hs.qnodes.size();
    s->geo.nl = nl; s->geo.ns = ns; s->geo.nt = nt;
    if(nl) s->geo.h_lights.assign((const unsigned char *) lights, (const unsigned char *) lights + (size_t) nl * HPT_LIGHT_BYTES);
    if(ns) s->geo.h_spheres.assign((const unsigned char *) spheres, (const unsigned char *) spheres + (size_t) ns * HPT_SPHERE_BYTES);
    if(nt) s->geo.h_tris.assign((const unsigned char *) tris, (const unsigned char *) tris + (size_t) nt * HPT_TRIANGLE_BYTES);
    memset(&s->tm.stats, 0, sizeof s->tm.stats);
    s->tm.stats.bvh_nodes = (uint32_t) hs.nodes.size(); s->tm.stats.bvh_depth = (uint32_t) hs.bvh_depth;
    s->geo.stack_levels = hs.bvh_depth > 0 ? hs.bvh_depth : 1;     // a leaf at depth d has d inner ancestors: at most d pushes
    s->tm.stats.n_tris = (uint32_t) nt; s->tm.stats.n_materials = (uint32_t) hs.materials.size();
    s->tm.stats.ms_bvh_build = hs.ms_bvh_build;
    s->tm.stats.ms_upload = std::chrono::duration<double, std::milli>(t1 - t0).count();
    // what a refit needs (scene_update.cpp); it goes to the device with the first update
    s->up.level_begin = hs.level_begin; s->up.wide_src = hs.wide_src; s->up.num_wide = (uint32_t) hs.wnodes.size();
    s->up.sphere_material.resize((size_t) ns);
    for(int i = 0; i < ns; ++i) s->up.sphere_material[(size_t) i] = hs.rounds[(size_t) i].material;
    *out = s;
    return HPT_OK;
}

int export_host_tree(const HostScene &hs, hpt_bvh_info *info, void *qnodes_out, size_t qnodes_cap, void *tris_out, size_t tris_cap){
    info->num_nodes = (int32_t) hs.qnodes.size(); info->num_tris = (int32_t) hs.tris.size();
    info->bvh_depth = hs.bvh_depth; info->num_rounds = hs.num_spheres + hs.num_lights;
    for(int a = 0; a < 3; ++a){ info->qorigin[a] = hs.qorigin[a]; info->qscale[a] = hs.qscale[a]; }
    if(qnodes_out){
        if(qnodes_cap < hs.qnodes.size() * sizeof(QBvhNode)) return fail(HPT_ERR_INVALID, "qnodes_out too small");
        memcpy(qnodes_out, hs.qnodes.data(), hs.qnodes.size() * sizeof(QBvhNode));
    }
    if(tris_out){
        if(tris_cap < hs.tris.size() * sizeof(DevTriangle)) return fail(HPT_ERR_INVALID, "tris_out too small");
        memcpy(tris_out, hs.tris.data(), hs.tris.size() * sizeof(DevTriangle));
    }
    return HPT_OK;
}

} // namespace hpt

extern "C" {

const char *hpt_last_error(void){ return g_err.c_str(); }

int hpt_device_count(void){
    int n = 0;
    if(hipGetDeviceCount(&n) != hipSuccess) return -1;
    return n;
}

int hpt_scene_create(const void *lights, int nl, const void *spheres, int ns, const void *tris, int nt,
                     hpt_scene **out){
    if(!out) return fail(HPT_ERR_INVALID, "null out_scene");
    *out = nullptr;
    HostScene hs;
    const char *err = build_host_scene(lights, nl, spheres, ns, tris, nt, hs);
    if(err && *err) return fail(HPT_ERR_INVALID, err);
    return hpt::scene_upload(hs, lights, nl, spheres, ns, tris, nt, out);
}

// device memory is released by its owners' destructors; what is left here is everything else
void hpt_scene_destroy(hpt_scene *s){
    if(!s) return;
    for(PassBuffers &w : s->ws.pass) if(w.h_count) hipHostFree(w.h_count);
    if(s->ws.px_fork) hipEventDestroy(s->ws.px_fork);
    for(int k = 1; k < kMaxPipes; ++k){
        if(s->ws.px_done[k]) hipEventDestroy(s->ws.px_done[k]);
        if(s->ws.px_stream[k]) hipStreamDestroy(s->ws.px_stream[k]);
    }
    for(hipEvent_t e : s->pm.marks) hipEventDestroy(e);
    if(s->up.ev_a) hipEventDestroy(s->up.ev_a);
    if(s->up.ev_b) hipEventDestroy(s->up.ev_b);
    for(hipEvent_t e : s->rb.ev) if(e) hipEventDestroy(e);
    if(s->tm.ev_start) hipEventDestroy(s->tm.ev_start);
    if(s->tm.ev_stop) hipEventDestroy(s->tm.ev_stop);
    for(hipEvent_t e : s->tm.event_pool) hipEventDestroy(e);
    delete s;
}

int64_t hpt_local_pixels(int W, int H, const hpt_params *params){
    Tiling tl;
    if(make_tiling(W, H, params, tl)) return -1;
    return tl.n_local;
}

int hpt_untile(const void *d_gathered, void *d_image, int W, int H, const hpt_params *params, void *hip_stream){
    Tiling tl;
    int rc = make_tiling(W, H, params, tl);
    if(rc) return rc;
    if(!d_gathered || !d_image) return fail(HPT_ERR_INVALID, "null buffer");
    launch_untile((hipStream_t) hip_stream, tl, (const float *) d_gathered, (float *) d_image);
    HIP_TRY(hipGetLastError());
    return HPT_OK;
}


void hpt_wrapper_cache_clear(void){
    std::lock_guard<std::mutex> lock(g_wrap.mu);
    if(g_wrap.scene) hpt_scene_destroy(g_wrap.scene);
    g_wrap.scene = nullptr; g_wrap.device = -1;
    if(g_wrap.multi) hpt_multi_destroy(g_wrap.multi);
    g_wrap.multi = nullptr;
}

int hpt_wrapper_set_devices(int num_devices){
    if(num_devices < 0) return fail(HPT_ERR_INVALID, "negative device count");
    std::lock_guard<std::mutex> lock(g_wrap.mu);
    g_wrap.devices = num_devices;
    return HPT_OK;
}

int hpt_pt_render_wrapper(const void *lights, int nl, const void *spheres, int ns, const void *tris, int nt,
                          const float scene_min[3], const float scene_max[3], const void *camera, float *host_image,
                          int W, int H, int light_depth, int light_sample, int eye_depth, int spp, int64_t seed){
    (void) scene_min; (void) scene_max; (void) light_depth; (void) light_sample;   // ignored by the reference too
    const hpt_params p = wrapper_params(seed);
    return wrapper_render(lights, nl, spheres, ns, tris, nt,
        [&](hpt_scene *s){ return hpt_render_pt(s, camera, W, H, eye_depth, spp, &p, host_image); },
        [&](hpt_multi *m){ return hpt_multi_render_pt(m, camera, W, H, eye_depth, spp, &p, host_image); });
}

// ---- 8-bit output stage ------------------------------------------------------------------------------------------
namespace {

// what the reference's host loop computes per channel (src/main_cli.cpp:233-241)
unsigned char tonemap_byte(float x){
    float c = std::max(0.0f, std::min(x, 1.0f));
    float g = std::pow(c, 1.0f / 2.2f);
    return (unsigned char) (g * 255.0f);
}

// thr[k], k = 1..255: the smallest float in [0, 1] whose byte is >= k (byte(x) is non-decreasing in x, so a binary
// search over the bit patterns of the non-negative floats finds it); thr[0] = -inf
const float *tonemap_thresholds(){
    static float table[256];
    static std::once_flag once;
    std::call_once(once, [](){
        table[0] = -INFINITY;
        for(int k = 1; k < 256; ++k){
            uint32_t lo = 0u, hi = 0x3F800000u;               // bits of 0.0f .. 1.0f; byte(1.0f) = 255 >= k
            while(lo < hi){
                uint32_t mid = lo + (hi - lo) / 2u;
                float x; memcpy(&x, &mid, 4);
                if((int) tonemap_byte(x) >= k) hi = mid; else lo = mid + 1u;
            }
            memcpy(&table[k], &lo, 4);
        }
    });
    return table;
}

// never destroyed: the HIP runtime may be gone by the time static destructors run
struct TonemapDevice { std::mutex mu; DevBuf<float> table[64]; } &g_tonemap = *new TonemapDevice;

// the threshold table on the current device (uploaded once per device)
int tonemap_device_table(const float **out){
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    if(dev < 0 || dev >= 64) return fail(HPT_ERR_INVALID, "device ordinal out of range");
    std::lock_guard<std::mutex> lock(g_tonemap.mu);
    DevBuf<float> &d = g_tonemap.table[dev];
    if(!d.get()){
        HIP_TRY(d.reserve(256));
        hipError_t e = hipMemcpy(d.get(), tonemap_thresholds(), 256 * sizeof(float), hipMemcpyHostToDevice);
        if(e != hipSuccess){ d.release(); return fail(HPT_ERR_DEVICE, std::string("tonemap table upload: ") + hipGetErrorString(e)); }
    }
    *out = d.get();
    return HPT_OK;
}

} // namespace

void hpt_tonemap_table(float thresholds_out[256]){ memcpy(thresholds_out, tonemap_thresholds(), 256 * sizeof(float)); }

void hpt_tonemap_reference(const float *linear_rgb, unsigned char *rgb8, int64_t num_pixels, int bgr){
    for(int64_t p = 0; p < num_pixels; ++p)
        for(int c = 0; c < 3; ++c) rgb8[p * 3 + c] = tonemap_byte(linear_rgb[p * 3 + (bgr ? 2 - c : c)]);
}

int hpt_tonemap(const void *d_linear_rgb, void *d_rgb8, int64_t num_pixels, int bgr, void *hip_stream){
    if(num_pixels < 0 || (num_pixels > 0 && (!d_linear_rgb || !d_rgb8))) return fail(HPT_ERR_INVALID, "bad tonemap argument");
    if(((uintptr_t) d_rgb8 & 3u) != 0u) return fail(HPT_ERR_INVALID, "tonemap output must be 4-byte aligned");
    const float *table = nullptr;
    int rc = tonemap_device_table(&table);
    if(rc) return rc;
    launch_tonemap((hipStream_t) hip_stream, (const float *) d_linear_rgb, d_rgb8, (unsigned long long) num_pixels * 3ull, bgr ? 1 : 0, table);
    HIP_TRY(hipGetLastError());
    return HPT_OK;
}

int hpt_tonemap_host(const float *linear_rgb, unsigned char *rgb8, int64_t num_pixels, int bgr){
    if(num_pixels < 0 || (num_pixels > 0 && (!linear_rgb || !rgb8))) return fail(HPT_ERR_INVALID, "bad tonemap argument");
    if(num_pixels == 0) return HPT_OK;
    DevBuf<float> d_in; DevBuf<unsigned char> d_out;
    size_t n = (size_t) num_pixels * 3;
    HIP_TRY(d_in.reserve(n));
    HIP_TRY(d_out.reserve((n + 3) / 4 * 4));
    HIP_TRY(hipMemcpy(d_in.get(), linear_rgb, n * sizeof(float), hipMemcpyHostToDevice));
    int rc = hpt_tonemap(d_in.get(), d_out.get(), num_pixels, bgr, nullptr);
    if(rc) return rc;
    HIP_TRY(hipMemcpy(rgb8, d_out.get(), n, hipMemcpyDeviceToHost));
    return HPT_OK;
}

int hpt_get_stats(const hpt_scene *scene, hpt_stats *out){
    if(!scene || !out) return fail(HPT_ERR_INVALID, "null argument");
    int rc = collect_stats(const_cast<hpt_scene *>(scene));
    if(rc) return rc;
    *out = scene->tm.stats;
    return HPT_OK;
}

int hpt_trace_closest(hpt_scene *s, const float *origins, const float *dirs, int n, int flags,
                      float *t_out, int32_t *prim_out){
    if(!s || !origins || !dirs || !t_out || !prim_out || n < 0) return fail(HPT_ERR_INVALID, "bad argument");
    if(n == 0) return HPT_OK;
    DevBuf<float> d_o, d_d, d_t; DevBuf<int32_t> d_p;
    size_t b3 = (size_t) n * 3 * sizeof(float);
    HIP_TRY(d_o.reserve((size_t) n * 3)); HIP_TRY(d_d.reserve((size_t) n * 3));
    HIP_TRY(d_t.reserve((size_t) n)); HIP_TRY(d_p.reserve((size_t) n));
    HIP_TRY(hipMemcpy(d_o.get(), origins, b3, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_d.get(), dirs, b3, hipMemcpyHostToDevice));
    launch_probe_closest(nullptr, s->geo.sd, d_o.get(), d_d.get(), n, (flags & HPT_FLAG_BRUTE_FORCE) ? 1 : 0, d_t.get(), d_p.get());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(t_out, d_t.get(), (size_t) n * 4, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(prim_out, d_p.get(), (size_t) n * 4, hipMemcpyDeviceToHost));
    return HPT_OK;
}

int hpt_probe_functions(const float *records_in, int n, float *results_out){
    if(n < 0 || (n > 0 && (!records_in || !results_out))) return fail(HPT_ERR_INVALID, "bad argument");
    if(n == 0) return HPT_OK;
    DevBuf<float> d_in, d_out;
    HIP_TRY(d_in.reserve((size_t) n * 24));
    HIP_TRY(d_out.reserve((size_t) n * 40));
    HIP_TRY(hipMemcpy(d_in.get(), records_in, (size_t) n * 24 * sizeof(float), hipMemcpyHostToDevice));
    launch_probe_functions(nullptr, d_in.get(), n, d_out.get());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(results_out, d_out.get(), (size_t) n * 40 * sizeof(float), hipMemcpyDeviceToHost));
    return HPT_OK;
}

int hpt_scene_set_groups(hpt_scene *s, const int32_t *obj_kind, const int32_t *obj_index, const int32_t *obj_group, int nobj){
    if(!s) return fail(HPT_ERR_INVALID, "null scene");
    if(nobj < 0 || (nobj > 0 && (!obj_kind || !obj_index || !obj_group))) return fail(HPT_ERR_INVALID, "bad group arrays");
    if(nobj != 0 && nobj != s->geo.ns + s->geo.nt) return fail(HPT_ERR_INVALID, "group arrays must list every sphere and triangle once");
    s->geo.g_kind.assign(obj_kind, obj_kind + nobj); s->geo.g_index.assign(obj_index, obj_index + nobj); s->geo.g_group.assign(obj_group, obj_group + nobj);
    s->bd.ready = false;
    return HPT_OK;
}


int hpt_bdpt_render_wrapper(const void *lights, int nl, const void *spheres, int ns, const void *tris, int nt,
                            const float scene_min[3], const float scene_max[3], const void *camera, float *host_image,
                            int W, int H, int light_depth, int light_sample, int eye_depth, int spp, int spl, int64_t seed){
    (void) scene_min; (void) scene_max;
    // The reference's helper hands over illum / light_sample (src/bdpt_cu_helper.cpp:60-62); the
    // estimator built here is cpu_bdpt's, which divides by spl itself, so that pre-division is undone.
    std::vector<unsigned char> L((const unsigned char *) lights, (const unsigned char *) lights + (size_t) std::max(nl, 0) * HPT_LIGHT_BYTES);
    if(light_sample > 1) for(int i = 0; i < nl; ++i){
        float *illum = (float *) (L.data() + (size_t) i * HPT_LIGHT_BYTES + 24);
        for(int c = 0; c < 3; ++c) illum[c] = illum[c] * (float) light_sample;
    }
    const hpt_params p = wrapper_params(seed);
    return wrapper_render(L.data(), nl, spheres, ns, tris, nt,
        [&](hpt_scene *s){ return hpt_render_bdpt(s, camera, W, H, eye_depth, light_depth, spp, spl, &p, host_image); },
        [&](hpt_multi *m){ return hpt_multi_render_bdpt(m, camera, W, H, eye_depth, light_depth, spp, spl, &p, host_image); });
}

int hpt_ppm_render_wrapper(const void *lights, int nl, const void *spheres, int ns, const void *tris, int nt,
                           const float scene_min[3], const float scene_max[3], const void *camera, float *host_image,
                           int W, int H, int light_depth, int light_sample, int eye_depth, int spp, int64_t seed){
    (void) spp;                  // one call is one pass: the reference never reads spp (src/ppm_cu.cu:328-400)
    std::lock_guard<std::mutex> lock(g_wrap.mu);
    hpt_scene *s = nullptr;      // one device whatever hpt_wrapper_set_devices says (include/hpt.h)
    int rc = wrapper_scene(lights, nl, spheres, ns, tris, nt, &s);
    if(rc) return rc;
    const hpt_params p = wrapper_params(seed);
    rc = hpt_render_ppm(s, camera, W, H, eye_depth, light_depth, 1, light_sample, 0.05f, scene_min, scene_max, &p, host_image);
    wrapper_release(s);
    return rc;
}

int hpt_bvh_export_host(const void *lights, int nl, const void *spheres, int ns, const void *tris, int nt, hpt_bvh_info *info,
                        void *qnodes_out, size_t qnodes_cap, void *tris_out, size_t tris_cap){
    if(!info) return fail(HPT_ERR_INVALID, "null info");
    HostScene hs;
    const char *err = build_host_scene(lights, nl, spheres, ns, tris, nt, hs);
    if(err && *err) return fail(HPT_ERR_INVALID, err);
    return export_host_tree(hs, info, qnodes_out, qnodes_cap, tris_out, tris_cap);
}

int hpt_scene_export_bvh(const hpt_scene *s, hpt_bvh_info *info, void *qnodes_out, size_t qnodes_cap, void *tris_out, size_t tris_cap){
    if(!s || !info) return fail(HPT_ERR_INVALID, "null argument");
    if(int rcd = on_scene_device(s)) return rcd;
    info->num_nodes = s->geo.sd.num_nodes; info->num_tris = s->geo.sd.num_tris;
    info->bvh_depth = (int32_t) s->tm.stats.bvh_depth; info->num_rounds = s->geo.sd.num_rounds;
    for(int a = 0; a < 3; ++a){ info->qorigin[a] = s->geo.sd.qorigin[a]; info->qscale[a] = s->geo.sd.qscale[a]; }
    if(qnodes_out){
        const size_t bytes = (size_t) s->geo.sd.num_nodes * sizeof(QBvhNode);
        if(qnodes_cap < bytes) return fail(HPT_ERR_INVALID, "qnodes_out too small");
        HIP_TRY(hipMemcpy(qnodes_out, s->geo.qnodes.get(), bytes, hipMemcpyDeviceToHost));
    }
    if(tris_out){
        const size_t bytes = (size_t) s->geo.sd.num_tris * sizeof(DevTriangle);
        if(tris_cap < bytes) return fail(HPT_ERR_INVALID, "tris_out too small");
        if(bytes) HIP_TRY(hipMemcpy(tris_out, s->geo.tris.get(), bytes, hipMemcpyDeviceToHost));
    }
    return HPT_OK;
}

int hpt_trace_visibility(hpt_scene *s, const float *p1, const float *p2, int n, int flags, int32_t *vis_out){
    if(!s || !p1 || !p2 || !vis_out || n < 0) return fail(HPT_ERR_INVALID, "bad argument");
    if(n == 0) return HPT_OK;
    DevBuf<float> d_a, d_b; DevBuf<int32_t> d_v;
    size_t b3 = (size_t) n * 3 * sizeof(float);
    HIP_TRY(d_a.reserve((size_t) n * 3)); HIP_TRY(d_b.reserve((size_t) n * 3));
    HIP_TRY(d_v.reserve((size_t) n));
    HIP_TRY(hipMemcpy(d_a.get(), p1, b3, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_b.get(), p2, b3, hipMemcpyHostToDevice));
    launch_probe_visibility(nullptr, s->geo.sd, d_a.get(), d_b.get(), n, (flags & HPT_FLAG_BRUTE_FORCE) ? 1 : 0, d_v.get());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(vis_out, d_v.get(), (size_t) n * 4, hipMemcpyDeviceToHost));
    return HPT_OK;
}

} // extern "C"
