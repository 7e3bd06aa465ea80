// The bidirectional (cpu_bdpt-estimator) path's host side (include/hpt.h, hpt_render_bdpt*): the grouped device scene
// built on first use, the eye-path workspace and the render loop.
#include "hpt_host.h"

using namespace hpt;

namespace {

int ensure_bdpt_scene(hpt_scene *s){
    if(s->bd.ready) return HPT_OK;
    HostBdptScene hb;
    const hpt_scene::Geometry &g = s->geo;
    bool grouped = !g.g_kind.empty();
    const unsigned char *h_tris = nullptr;
    if(int rc = host_triangles(s, &h_tris)) return rc;
    const char *err = build_bdpt_host_scene(g.h_lights.data(), g.nl, g.h_spheres.data(), g.ns, h_tris, g.nt,
                                            grouped ? g.g_kind.data() : nullptr, grouped ? g.g_index.data() : nullptr,
                                            grouped ? g.g_group.data() : nullptr, (int) g.g_kind.size(), hb);
    if(err && *err) return fail(HPT_ERR_INVALID, err);
    hpt_scene::Bdpt &b = s->bd;
    hipError_t e = b.nodes.upload(hb.nodes);
    if(e == hipSuccess) e = b.tris.upload(hb.tris);
    if(e == hipSuccess) e = b.spheres.upload(hb.spheres);
    if(e == hipSuccess) e = b.groups.upload(hb.groups);
    if(e == hipSuccess) e = b.mats.upload(hb.materials);
    if(e == hipSuccess) e = b.lights.upload(hb.lights);
    if(e != hipSuccess) return fail(HPT_ERR_DEVICE, std::string("bdpt scene upload: ") + hipGetErrorString(e));
    b.sc.nodes = (const float4 *) b.nodes.get(); b.sc.tris = (const float4 *) b.tris.get(); b.sc.spheres = b.spheres.get();
    b.sc.groups = b.groups.get(); b.sc.mats = b.mats.get(); b.sc.lights = b.lights.get();
    s->bd.sc.num_groups = (int) hb.groups.size(); s->bd.sc.num_lights = s->geo.nl; s->bd.sc.num_mats = (int) hb.materials.size();
    s->bd.sc.stack_levels = std::min(std::max(hb.bvh_depth, 1) + 1, kStackDepth);
    for(int a = 0; a < 3; ++a){ s->bd.sc.scene_min[a] = hb.scene_min[a]; s->bd.sc.scene_max[a] = hb.scene_max[a]; }
    s->bd.ready = true;
    return HPT_OK;
}

// eye-path state for `slots` path slots of `eye_depth` vertices, tables for `n_lv` light vertices
int ensure_bdpt_workspace(hpt_scene::Bdpt &b, size_t slots, int eye_depth, size_t n_lv){
    // a larger pass takes new history and contribution tables whatever the old ones held
    if(slots > b.last_pos_pdf.capacity()){ b.hist_pos_eta.release(); b.hist_pdf.release(); b.contrib.release(); b.valid.release(); }
    hipError_t e = reserve_all(slots, b.last_pos_pdf, b.last_normal, b.vtx_pos, b.vtx_nrm, b.vtx_thr, b.vtx_wo, b.vtx_base);
    if(e == hipSuccess) e = b.ectx.reserve(slots * 7);
    if(e == hipSuccess) e = b.cqueue.reserve(slots);
    if(e == hipSuccess) e = reserve_all(slots * (size_t) eye_depth, b.hist_pos_eta, b.hist_pdf);
    if(e == hipSuccess) e = b.contrib.reserve(slots * n_lv);
    if(e == hipSuccess) e = b.valid.reserve(slots * ((n_lv + 63) / 64));
    if(e == hipSuccess) e = b.lv.reserve(n_lv);
    if(e == hipSuccess) e = b.lctx.reserve(n_lv);
    b.bp = BdptPathBuf{ b.last_pos_pdf.get(), b.last_normal.get(), b.vtx_pos.get(), b.vtx_nrm.get(), b.vtx_thr.get(), b.vtx_wo.get(),
                        b.vtx_base.get(), b.hist_pos_eta.get(), b.hist_pdf.get(), b.contrib.get(), b.valid.get(), b.ectx.get() };
    if(e != hipSuccess) return fail_hip("bdpt workspace", e);
    return HPT_OK;
}

} // namespace

extern "C" {

// the bidirectional render loop (reference src/cpu_bdpt.cpp:173-488), enqueued on `stream`
int hpt_render_bdpt_device(hpt_scene *s, const void *camera, int W, int H, int eye_depth, int light_depth, int spp, int spl,
                           const hpt_params *params, void *d_local, void *hip_stream){
    const hipStream_t stream = (hipStream_t) hip_stream;
    if(!s) return fail(HPT_ERR_INVALID, "null scene");
    if(!camera || !d_local) return fail(HPT_ERR_INVALID, "null camera or output");
    if(spp <= 0 || spl <= 0 || eye_depth <= 0 || eye_depth > 255 || light_depth <= 0 || light_depth > 255)
        return fail(HPT_ERR_INVALID, "spp, spl must be > 0 and depths in [1, 255]");
    if(int rcd = on_scene_device(s)) return rcd;
    hpt_params P;
    if(int rcp = take_params(params, kRenderParams, P)) return rcp;     // max_delta: the CPU renderer has no cap (cpu_bdpt.cpp:458)
    Tiling tl;
    int rc = make_tiling(W, H, &P, tl);
    if(rc) return rc;
    rc = ensure_bdpt_scene(s);
    if(rc) return rc;

    // light vertices: nl * spl subpaths of light_depth vertices each; the contribution table holds one 16-B entry
    // per (path slot, light vertex) pair and at least one image's worth of slots, so it is bounded here
    const long long n_lv64 = (long long) s->geo.nl * spl * light_depth;
    if(n_lv64 > (1ll << 24)) return fail(HPT_ERR_INVALID, "too many light vertices (num_lights * spl * light_depth > 2^24)");
    const int total_light_paths = s->geo.nl * spl;
    const int n_lv = (int) n_lv64;
    // slots per pass: bound the contribution table (16 B per pair) to about 1 GiB
    int spass = P.samples_per_pass;
    if(spass <= 0){
        long long pairs = 64ll << 20;
        long long slots = std::max<long long>(tl.n_local, std::min<long long>(4ll << 20, pairs / std::max(n_lv, 1)));
        spass = (int) std::max<long long>(1, slots / tl.n_local);
    }
    spass = std::min(spass, spp);
    size_t slots = (size_t) tl.n_local * spass;
    if(slots > 0x7FFFFFF0ull) return fail(HPT_ERR_INVALID, "too many path slots per pass");
    if((double) slots * (double) std::max(n_lv, 1) * 16.0 > 64.0 * 1073741824.0)
        return fail(HPT_ERR_INVALID, "contribution table (path slots x light vertices x 16 B) would exceed 64 GiB: lower spl, light_depth, "
                                     "the image size per rank or samples_per_pass");
    const int max_iters = eye_depth + P.max_delta + 1;
    int n_counters = 2 * (max_iters + 2);
    // nothing is refused past this point: the counters of the last PT render stop being read before they can move (a call
    // refused above leaves hpt_get_stats with what the last render reported)
    s->ws.last_counter_stride = 0; s->ws.last_budget = 0;
    rc = ensure_workspace(s, slots, tl.n_local, n_counters);
    if(rc) return rc;
    rc = ensure_bdpt_workspace(s->bd, slots, eye_depth, (size_t) std::max(n_lv, 1));
    if(rc) return rc;

    CameraDev cam;
    set_camera(cam, camera);
    reset_render_stats(s);
    const bool timek = (P.flags & HPT_FLAG_TIME_KERNELS) != 0;

    HIP_TRY(hipMemsetAsync(s->ws.wc.get(), 0, sizeof(WorkCounters), stream));
    HIP_TRY(hipMemsetAsync(s->ws.accum.get(), 0, (size_t) tl.n_local * sizeof(float4), stream));
    HIP_TRY(hipEventRecord(s->tm.ev_start, stream));
    if(s->geo.nl > 0){                                       // no lights: the CPU renderer returns at once (cpu_bdpt.cpp:178)
        { LaunchTimer t(s, stream, timek, 3);
          launch_bdpt_light_trace(stream, s->bd.sc, s->bd.lv.get(), total_light_paths, light_depth, spl, P.seed, P.max_delta);
          launch_bdpt_light_ctx(stream, s->bd.lv.get(), s->bd.lctx.get(), n_lv, light_depth); }
        for(int done = 0; done < spp; done += spass){
            int sthis = std::min(spass, spp - done);
            uint32_t nslots = (uint32_t) tl.n_local * (uint32_t) sthis;
            HIP_TRY(hipMemsetAsync(s->ws.pass[0].counters.get(), 0, (size_t) n_counters * sizeof(uint32_t), stream));
            uint32_t *qcnt = s->ws.pass[0].counters.get(), *ccnt = s->ws.pass[0].counters.get() + (max_iters + 2);
            { LaunchTimer t(s, stream, timek, 3);
              launch_bdpt_generate(stream, tl, cam, s->ws.pass[0].pb, s->bd.bp, &qcnt[0], sthis, (uint32_t) (P.sample_offset + done), P.seed); }
            int cur = 0;
            for(int it = 0; it < max_iters; ++it){
                const int ci = it;                             // counter slot of this iteration
                // past eye_depth only paths on free delta bounces are alive: the host looks every other iteration (an
                // iteration on an empty queue costs four empty launches), or never with HPT_FLAG_NO_HOST_WAIT
                if(it >= eye_depth && !(P.flags & HPT_FLAG_NO_HOST_WAIT) && ((it - eye_depth) & 1) == 0){
                    HIP_TRY(hipMemcpyAsync(s->ws.pass[0].h_count, &qcnt[ci], sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
                    HIP_TRY(hipStreamSynchronize(stream));
                    if(*s->ws.pass[0].h_count == 0u) break;
                }
                const uint32_t *eq = it == 0 ? nullptr : s->ws.pass[0].queue[cur].get();
                // unseen tail iterations: small fixed grids for the three kernels that walk their queue with a stride
                // (k_bdpt_vertex keeps its grid: one chunk per workgroup, an empty one returns at once)
                const uint32_t cap = (it >= eye_depth && (P.flags & HPT_FLAG_NO_HOST_WAIT)) ? (uint32_t) std::max(s->num_cus, 1) * 8u : 0u;
                { LaunchTimer t(s, stream, timek, 0);
                  launch_bdpt_extend(stream, s->bd.sc, s->ws.pass[0].pb, eq, &qcnt[ci], nslots, cap); }
                { LaunchTimer t(s, stream, timek, 1);
                  launch_bdpt_vertex(stream, s->bd.sc, s->ws.pass[0].pb, s->bd.bp, eq, &qcnt[ci], nslots, s->ws.pass[0].queue[cur ^ 1].get(), &qcnt[ci + 1],
                                     s->bd.cqueue.get(), &ccnt[ci], eye_depth, P.max_delta, (uint32_t) slots, cam.eye); }
                { LaunchTimer t(s, stream, timek, 2);
                  launch_bdpt_connect(stream, s->bd.sc, s->ws.pass[0].pb, s->bd.bp, s->bd.lv.get(), s->bd.lctx.get(), n_lv, light_depth, s->bd.cqueue.get(), &ccnt[ci], nslots,
                                      (uint32_t) slots, cap, (P.flags & HPT_FLAG_COUNT_WORK) ? s->ws.wc.get() : nullptr); }
                { LaunchTimer t(s, stream, timek, 3);
                  launch_bdpt_reduce(stream, s->ws.pass[0].pb, s->bd.bp, n_lv, s->bd.cqueue.get(), &ccnt[ci], nslots, cap); }
                cur ^= 1;
            }
            { LaunchTimer t(s, stream, timek, 3);
              launch_resolve(stream, tl, s->ws.pass[0].pb, s->ws.accum.get(), sthis); }
        }
    }
    float divisor = (P.flags & HPT_FLAG_OUTPUT_SUM) ? 1.0f : (float) spp;
    { LaunchTimer t(s, stream, timek, 3);
      launch_finalize(stream, tl, s->ws.accum.get(), (float *) d_local, divisor); }
    HIP_TRY(hipEventRecord(s->tm.ev_stop, stream));
    HIP_TRY(hipGetLastError());
    s->tm.stats_pending = true;
    return HPT_OK;
}

int hpt_render_bdpt(hpt_scene *s, const void *camera, int W, int H, int eye_depth, int light_depth, int spp, int spl,
                    const hpt_params *params, float *host_image){
    if(!s) return fail(HPT_ERR_INVALID, "null scene");
    if(!host_image) return fail(HPT_ERR_INVALID, "null image");
    if(params && params->world > 1) return fail(HPT_ERR_INVALID, "hpt_render_bdpt renders the whole image: world must be 0 or 1");
    Tiling tl;
    int rc = make_tiling(W, H, params, tl);
    if(rc) return rc;
    rc = ensure_own_image(s, tl);
    if(rc) return rc;
    rc = hpt_render_bdpt_device(s, camera, W, H, eye_depth, light_depth, spp, spl, params, s->ws.local_own.get(), nullptr);
    if(rc) return rc;
    return untile_to_host(s, tl, nullptr, host_image);
}

} // extern "C"
