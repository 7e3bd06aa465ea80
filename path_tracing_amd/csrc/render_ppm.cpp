// Photon mapping's host side (include/hpt.h, hpt_render_ppm and hpt_sppm_*): the pass both share (eye, photon and grid
// phases), its workspace and statistics, the one-shot render and the progressive state; and hpt_render_guides, which
// runs the eye phase alone.
#include "hpt_host.h"
#include "history_kernels.h"

#include <new>

using namespace hpt;

namespace {

// the scene's bounds as the reference's helper computes them (src/ppm_cu_helper.cpp:21-52): spheres +- r and triangle
// vertices, light balls left out, starting from +-1e9
int ppm_scene_bounds(hpt_scene *s){
    if(s->pm.bounds_ready) return HPT_OK;
    const unsigned char *h_tris = nullptr;
    if(int rc = host_triangles(s, &h_tris)) return rc;
    float mn[3] = { 1e9f, 1e9f, 1e9f }, mx[3] = { -1e9f, -1e9f, -1e9f };
    for(int i = 0; i < s->geo.ns; ++i){
        float c[4]; memcpy(c, s->geo.h_spheres.data() + (size_t) i * HPT_SPHERE_BYTES, 16);
        for(int a = 0; a < 3; ++a){ mx[a] = std::max(mx[a], c[a] + c[3]); mn[a] = std::min(mn[a], c[a] - c[3]); }
    }
    for(int i = 0; i < s->geo.nt; ++i){
        float v[9]; memcpy(v, h_tris + (size_t) i * HPT_TRIANGLE_BYTES, 36);
        for(int a = 0; a < 3; ++a){
            mx[a] = std::max({ mx[a], v[a], v[3 + a], v[6 + a] });
            mn[a] = std::min({ mn[a], v[a], v[3 + a], v[6 + a] });
        }
    }
    for(int a = 0; a < 3; ++a){ s->pm.min[a] = mn[a]; s->pm.max[a] = mx[a]; }
    s->pm.bounds_ready = true;
    return HPT_OK;
}

constexpr ParamRules kPpmParams{ "hpt_render_ppm renders the whole image on one device: world must be 0 or 1",
                                 HPT_FLAG_OUTPUT_SUM | HPT_FLAG_TIME_KERNELS | HPT_FLAG_COUNT_WORK,
                                 "hpt_render_ppm accepts HPT_FLAG_OUTPUT_SUM, TIME_KERNELS and COUNT_WORK only",
                                 0, "hpt_params.reserved must be zero for hpt_render_ppm" };
constexpr ParamRules kGuideParams{ "hpt_render_guides renders the whole image on one device: world must be 0 or 1",
                                   HPT_FLAG_TIME_KERNELS, "hpt_render_guides accepts HPT_FLAG_TIME_KERNELS only",
                                   0, "hpt_params.reserved must be zero for hpt_render_guides" };
constexpr ParamRules kSppmParams{ "progressive photon mapping renders the whole image on one device: world must be 0 or 1",
                                  0, "hpt_sppm_create: hpt_params.flags must be zero (render flags go to hpt_sppm_render)",
                                  0, "hpt_params.reserved must be zero for progressive photon mapping" };

// What the passes of one photon-mapping render share (hpt_render_ppm, hpt_sppm_render).  The caller fills P (max_delta
// clamped), tl, cam and fr (bounds, cell, r2); ppm_prepare sizes the rest and grows the scene's PPM workspace.
struct PpmRun {
    hpt_params P; Tiling tl; CameraDev cam; PpmFrame fr;
    int light_depth = 0, spl = 0, eye_iters = 0, ph_iters = 0, M = 0, n_counters = 0;
    uint64_t n_ph64 = 0; uint32_t n_ph = 0, n_dep = 0, n_local = 0, buckets = 0;
    bool count = false, timek = false;
    uint32_t *hp_count(const hpt_scene *s) const { return s->ws.pass[0].counters.get() + 4 * M; }
};

// `passes`: how many passes the call renders (TIME_KERNELS: five events each)
int ppm_prepare(hpt_scene *s, PpmRun &r, int light_depth, int spl, int passes){
    const hpt_params &P = r.P;
    r.light_depth = light_depth; r.spl = spl;
    r.n_ph64 = s->geo.nl > 0 ? (uint64_t) s->geo.nl * (uint64_t) spl : 0u;
    const uint64_t n_dep64 = r.n_ph64 * (uint64_t) light_depth;
    if(n_dep64 > (1ull << 30))
        return fail(HPT_ERR_NOMEM, "num_lights * spl * light_depth photon deposits do not fit (at most 2^30 per pass)");
    const uint32_t n_ph = (uint32_t) r.n_ph64, n_dep = (uint32_t) n_dep64;
    uint32_t buckets = 1024u;
    while(buckets < 2u * n_dep) buckets <<= 1;
    r.fr.buckets = buckets;
    r.n_ph = n_ph; r.n_dep = n_dep; r.buckets = buckets;
    const uint32_t n_local = (uint32_t) r.tl.n_local;
    r.n_local = n_local;
    const size_t paths = std::max<size_t>(n_local, n_ph);
    r.eye_iters = 1 + P.max_delta; r.ph_iters = light_depth + P.max_delta;
    r.M = std::max(r.eye_iters, r.ph_iters) + 2;
    r.n_counters = 4 * r.M + 2;
    int rc = ensure_workspace(s, paths, r.tl.n_local, r.n_counters);
    if(rc) return rc;
    r.count = (P.flags & HPT_FLAG_COUNT_WORK) != 0; r.timek = (P.flags & HPT_FLAG_TIME_KERNELS) != 0;
    hpt_scene::Ppm &m = s->pm;
    const size_t dep_cap = std::max<size_t>(n_dep, 1);
    const size_t tmp = std::max<size_t>(ppm_sort_tmp_bytes(n_dep, buckets), 1);
    hipError_t e = reserve_all(n_local, m.pos_mat, m.nrm, m.wo, m.thr, m.list);
    if(e == hipSuccess && r.count) e = reserve_all(n_local, m.cand, m.acc);
    if(e == hipSuccess) e = reserve_all(dep_cap * 4, m.dep, m.packed);
    if(e == hipSuccess) e = reserve_all(dep_cap, m.key, m.slot_in, m.key_sorted, m.slot_sorted);
    if(e == hipSuccess) e = m.range.reserve(buckets);
    if(e == hipSuccess) e = m.sort_tmp.reserve(tmp);
    if(e == hipSuccess) e = m.pc.reserve(1);
    m.hb = PpmHitBuf{ m.pos_mat.get(), m.nrm.get(), m.wo.get(), m.thr.get(), m.list.get() };
    m.grid = PpmGrid{ m.dep.get(), m.key.get(), m.slot_in.get(), m.key_sorted.get(), m.slot_sorted.get(), m.packed.get(), m.range.get(),
                      buckets, m.sort_tmp.get(), tmp };
    if(e != hipSuccess) return fail_hip("photon map workspace", e);
    rc = ensure_own_image(s, r.tl);
    if(rc) return rc;
    const size_t n_marks = r.timek ? (size_t) passes * 5 : 0;
    while(s->pm.marks.size() < n_marks){ hipEvent_t ev; HIP_TRY(hipEventCreate(&ev)); s->pm.marks.push_back(ev); }
    return HPT_OK;
}

void ppm_mark(hpt_scene *s, const PpmRun &r, int pass, int k){ if(r.timek) hipEventRecord(s->pm.marks[(size_t) pass * 5 + k], nullptr); }

// The trace step and the queue look that the eye and the photon phase share, on pass[0]'s buffers.
struct PpmStep {
    hpt_scene *s; const PpmRun &r; hipStream_t st; PassBuffers &w; uint32_t *no_shadow; int budget;
    PpmStep(hpt_scene *s_, const PpmRun &r_) : s(s_), r(r_), st(nullptr), w(s_->ws.pass[0]), no_shadow(w.counters.get() + 4 * r_.M + 1),
                                                budget(resume_walk_fits(s_->geo.sd) ? kTraceBudget : 0) {}
    // closest-hit rays of the queue in cnt[it] (it = 0: the identity queue), the PT path's split trace step
    void trace(int it, const uint32_t *queue, uint32_t *cnt, uint32_t *lcnt, uint32_t max_items) const {
        TraceSplit split{ w.lqueue[0].get(), &lcnt[it], w.lqueue[1].get(), no_shadow, budget, w.rec.get() };
        launch_trace(st, s->geo.sd, w.pb, w.sb, queue, &cnt[it], max_items, nullptr, nullptr, 0, s->geo.stack_levels, false, nullptr, &split, nullptr, 0u);
        if(budget > 0) launch_trace_resume(st, s->geo.sd, w.pb, w.sb, true, false, max_items, nullptr, split, nullptr, 0u, w.deep_stack.get());
    }
    // the host looks at a queue's length before an iteration that only delta bounces can fill
    int queue_empty(const uint32_t *cnt, bool &empty) const {
        HIP_TRY(hipMemcpyAsync(w.h_count, cnt, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        empty = *w.h_count == 0u;
        return HPT_OK;
    }
};

// The eye phase of photon-mapping pass `pidx` (the counters zeroed by the caller): slot = local pixel, stream
// (seed ^ kPpmEyeKey, pixel, pass), jitter first.  Leaves the hit points in s->pm.hb (their number in r.hp_count(s))
// and the direct terms in pass[0].pb.col.  hpt_render_guides runs this phase alone.
int ppm_eye_phase(hpt_scene *s, const PpmRun &r, const PpmStep &step, uint32_t pidx){
    const hpt_params &P = r.P;
    hipStream_t st = step.st;
    PassBuffers &w = step.w;
    uint32_t *eq = w.counters.get(), *elc = w.counters.get() + r.M;
    launch_generate(st, r.tl, r.cam, w.pb, &eq[0], 1, pidx, P.seed ^ kPpmEyeKey, nullptr);
    int cur = 0;
    for(int it = 0; it < r.eye_iters; ++it){
        if(it >= 1){ bool empty; if(int rc = step.queue_empty(&eq[it], empty)) return rc; if(empty) break; }
        const uint32_t *q = it == 0 ? nullptr : w.queue[cur].get();
        step.trace(it, q, eq, elc, r.n_local);
        launch_ppm_eye_shade(st, s->geo.sd, w.pb, s->pm.hb, q, &eq[it], r.n_local, w.queue[cur ^ 1].get(), &eq[it + 1], r.hp_count(s), P.max_delta, s->pm.pc.get());
        cur ^= 1;
    }
    return HPT_OK;
}

// The eye, photon and grid phases of photon-mapping pass `pidx`, marks 0-3 of the call's pass `pass`: the hit points
// in s->pm.hb (their number in r.hp_count(s)), the direct terms in pass[0].pb.col, the deposits' grid in s->pm.grid.
int ppm_phases(hpt_scene *s, const PpmRun &r, int pass, uint32_t pidx){
    const hpt_params &P = r.P;
    const PpmFrame &fr = r.fr;
    const uint32_t n_ph = r.n_ph, n_dep = r.n_dep;
    const int M = r.M, light_depth = r.light_depth;
    const PpmStep step(s, r);
    hipStream_t st = step.st;
    PassBuffers &w = step.w;
    uint32_t *pq = w.counters.get() + 2 * M, *plc = w.counters.get() + 3 * M;
    HIP_TRY(hipMemsetAsync(w.counters.get(), 0, (size_t) r.n_counters * sizeof(uint32_t), st));
    ppm_mark(s, r, pass, 0);
    if(int rc = ppm_eye_phase(s, r, step, pidx)) return rc;
    ppm_mark(s, r, pass, 1);
    if(n_ph){
        HIP_TRY(hipMemsetD32Async((hipDeviceptr_t) s->pm.grid.key, (int) r.buckets, n_dep, st));
        launch_ppm_emit(st, s->geo.sd, w.pb, &pq[0], n_ph, r.spl, P.seed, pidx, fr);
        int cur = 0;
        for(int it = 0; it < r.ph_iters; ++it){
            if(it >= light_depth){ bool empty; if(int rc = step.queue_empty(&pq[it], empty)) return rc; if(empty) break; }
            const uint32_t *q = it == 0 ? nullptr : w.queue[cur].get();
            step.trace(it, q, pq, plc, n_ph);
            launch_ppm_photon_shade(st, s->geo.sd, w.pb, s->pm.grid, q, &pq[it], n_ph, w.queue[cur ^ 1].get(), &pq[it + 1], light_depth,
                                    P.max_delta, fr, s->pm.pc.get());
            cur ^= 1;
        }
    }
    ppm_mark(s, r, pass, 2);
    HIP_TRY(hipMemsetAsync(s->pm.grid.range, 0, (size_t) r.buckets * sizeof(uint2), st));
    if(n_dep && launch_ppm_grid(st, s->pm.grid, n_dep)) return fail(HPT_ERR_DEVICE, "photon grid: radix sort launch failed");
    ppm_mark(s, r, pass, 3);
    return HPT_OK;
}

// statistics of a finished render of `passes` passes (blocking) into s->pm.stats
int ppm_collect_stats(hpt_scene *s, const PpmRun &r, int passes){
    hpt_ppm_stats &ps = s->pm.stats;
    memset(&ps, 0, sizeof ps);
    PpmCounters pc;
    HIP_TRY(hipMemcpy(&pc, s->pm.pc.get(), sizeof pc, hipMemcpyDeviceToHost));
    ps.photons = r.n_ph64 * (uint64_t) passes; ps.photon_rays = pc.photon_rays; ps.deposits = pc.deposits;
    ps.hit_points = pc.hit_points; ps.direct_pixels = pc.direct; ps.candidates = pc.candidates; ps.accepted = pc.accepted;
    ps.grid_buckets = r.buckets;
    float ms = 0.0f;
    HIP_TRY(hipEventElapsedTime(&ms, s->tm.ev_start, s->tm.ev_stop));
    ps.ms_total = ms;
    if(r.timek){
        double *phase[4] = { &ps.ms_eye, &ps.ms_photon, &ps.ms_grid, &ps.ms_gather };
        for(int pass = 0; pass < passes; ++pass) for(int k = 0; k < 4; ++k){
            float e = 0.0f;
            if(hipEventElapsedTime(&e, s->pm.marks[(size_t) pass * 5 + k], s->pm.marks[(size_t) pass * 5 + k + 1]) == hipSuccess) *phase[k] += e;
        }
    }
    if(r.count){
        const uint32_t n_local = r.n_local;
        uint32_t nhp = 0;
        HIP_TRY(hipMemcpy(&nhp, r.hp_count(s), sizeof nhp, hipMemcpyDeviceToHost));
        std::vector<uint32_t> list(nhp), cand(n_local), acc(n_local);
        if(nhp){
            HIP_TRY(hipMemcpy(list.data(), s->pm.hb.list, (size_t) nhp * 4, hipMemcpyDeviceToHost));
            HIP_TRY(hipMemcpy(cand.data(), s->pm.cand.get(), (size_t) n_local * 4, hipMemcpyDeviceToHost));
            HIP_TRY(hipMemcpy(acc.data(), s->pm.acc.get(), (size_t) n_local * 4, hipMemcpyDeviceToHost));
            std::vector<uint32_t> c(nhp), a(nhp);
            for(uint32_t k = 0; k < nhp; ++k){ c[k] = cand[list[k]]; a[k] = acc[list[k]]; }
            std::nth_element(c.begin(), c.begin() + nhp / 2, c.end()); ps.cand_median = c[nhp / 2];
            std::nth_element(a.begin(), a.begin() + nhp / 2, a.end()); ps.acc_median = a[nhp / 2];
            ps.cand_max = *std::max_element(c.begin(), c.end()); ps.acc_max = *std::max_element(a.begin(), a.end());
        }
    }
    // hpt_get_stats after this render reports its total time only: the per-class times are reset here, and the work
    // counters it copies back were cleared on the stream when the render began
    reset_render_stats(s);
    s->tm.stats_pending = true;
    return HPT_OK;
}

} // namespace

extern "C" {

// the photon-mapping render (reference src/ppm_cu.cu:328-400, `spp` passes), blocking, whole image into host_image
int hpt_render_ppm(hpt_scene *s, const void *camera, int W, int H, int eye_depth, int light_depth, int spp, int spl, float radius,
                   const float *scene_min, const float *scene_max, const hpt_params *params, float *host_image){
    if(!s) return fail(HPT_ERR_INVALID, "null scene");
    if(!camera || !host_image) return fail(HPT_ERR_INVALID, "null camera or image");
    if(spp <= 0 || spl < 0 || eye_depth <= 0 || eye_depth > 255 || light_depth <= 0 || light_depth > 255)
        return fail(HPT_ERR_INVALID, "spp must be > 0, spl >= 0 and depths in [1, 255]");
    if(int rcd = on_scene_device(s)) return rcd;
    PpmRun r;
    hpt_params &P = r.P;
    if(int rcp = take_params(params, kPpmParams, P)) return rcp;
    int rc = make_tiling(W, H, &P, r.tl);
    if(rc) return rc;
    if(!(radius > 0.0f)) radius = 0.05f;                                    // PPM_RADIUS, include/ppm_cu.cuh:4
    PpmFrame &fr = r.fr;
    if(int rcb = ppm_scene_bounds(s)) return rcb;
    for(int a = 0; a < 3; ++a){ fr.smin[a] = scene_min ? scene_min[a] : s->pm.min[a]; fr.smax[a] = scene_max ? scene_max[a] : s->pm.max[a]; }
    fr.cell = radius; fr.r2 = radius * radius;
    set_camera(r.cam, camera);
    rc = ppm_prepare(s, r, light_depth, spl, spp);
    if(rc) return rc;

    hipStream_t st = nullptr;
    PassBuffers &w = s->ws.pass[0];
    const Tiling &tl = r.tl;
    HIP_TRY(hipMemsetAsync(s->pm.pc.get(), 0, sizeof(PpmCounters), st));
    HIP_TRY(hipMemsetAsync(s->ws.wc.get(), 0, sizeof(WorkCounters), st));     // nothing here counts into it: hpt_get_stats reads zeros
    HIP_TRY(hipMemsetAsync(s->ws.accum.get(), 0, (size_t) tl.n_local * sizeof(float4), st));
    if(r.n_dep) launch_ppm_iota(st, s->pm.grid.slot_in, r.n_dep);
    HIP_TRY(hipEventRecord(s->tm.ev_start, st));
    for(int pass = 0; pass < spp; ++pass){
        rc = ppm_phases(s, r, pass, (uint32_t) ((int64_t) P.sample_offset + pass));
        if(rc) return rc;
        launch_ppm_gather(st, s->geo.sd, w.pb, s->pm.hb, s->pm.grid, r.hp_count(s), r.n_local, fr, r.count ? s->pm.cand.get() : nullptr,
                          r.count ? s->pm.acc.get() : nullptr, s->pm.pc.get());
        launch_resolve(st, tl, w.pb, s->ws.accum.get(), 1);
        ppm_mark(s, r, pass, 4);
    }
    launch_finalize(st, tl, s->ws.accum.get(), s->ws.local_own.get(), (P.flags & HPT_FLAG_OUTPUT_SUM) ? 1.0f : (float) spp);
    rc = untile_to_host(s, tl, st, host_image, s->tm.ev_stop);
    if(rc) return rc;
    return ppm_collect_stats(s, r, spp);
}

} // extern "C"

namespace {

// First-hit guide buffers (include/hpt.h): PPM's eye pass per sample, its hit points summed per pixel, the means
// un-tiled into whichever images the caller asks for -- host images (hpt_render_guides) or, with `device`, device
// images (hpt_render_guides_device).  Blocking, one device.
int render_guides(hpt_scene *s, const void *camera, int W, int H, int spp, const hpt_params *params,
                  float *albedo, float *normal, float *position, float *coverage, float *prev_position, bool device){
    if(!s) return fail(HPT_ERR_INVALID, "null scene");
    if(!camera) return fail(HPT_ERR_INVALID, "null camera");
    if(spp < 1) return fail(HPT_ERR_INVALID, "spp must be >= 1");
    if(!albedo && !normal && !position && !coverage && !prev_position) return fail(HPT_ERR_INVALID, "hpt_render_guides: every output is null");
    if(int rcd = on_scene_device(s)) return rcd;
    PpmRun r;
    hpt_params &P = r.P;
    if(int rcp = take_params(params, kGuideParams, P)) return rcp;
    int rc = make_tiling(W, H, &P, r.tl);
    if(rc) return rc;
    // the bounds place photons and grid cells, and a guide render has neither: a scene whose host records are behind its
    // device vertices (a pose, device vertices) is not made to download them for a box no kernel here reads
    if(!s->up.h_tris_stale) if(int rcb = ppm_scene_bounds(s)) return rcb;
    for(int a = 0; a < 3; ++a){ r.fr.smin[a] = s->pm.min[a]; r.fr.smax[a] = s->pm.max[a]; }
    r.fr.cell = 0.05f; r.fr.r2 = 0.05f * 0.05f;                             // no photons: the grid is not built
    set_camera(r.cam, camera);
    rc = ppm_prepare(s, r, 1, 0, spp);
    if(rc) return rc;
    const size_t n_local = r.n_local;
    hipError_t e = reserve_all(n_local, s->pm.g_alb, s->pm.g_nrm, s->pm.g_pos);
    if(e != hipSuccess) return fail_hip("guide accumulators", e);
    // the motion guide (include/hpt.h, "motion"): a fifth sum, filled only where the scene holds a previous geometry -- until
    // the first update G' is G, every previous point is the point itself and the image is resolved from the positions
    const bool motion = prev_position && s->up.prev_ready;
    if(motion){
        e = s->pm.g_prev.reserve(s->pm.g_alb.capacity());
        if(e != hipSuccess) return fail_hip("guide accumulators", e);
    }
    const GuideAccum ga{ s->pm.g_alb.get(), s->pm.g_nrm.get(), s->pm.g_pos.get(), motion ? s->pm.g_prev.get() : s->pm.g_pos.get() };
    const GuideMotion gm{ s->up.verts.get(), s->up.prev_verts.get(), s->up.prev_rounds.get() };

    const PpmStep step(s, r);
    hipStream_t st = step.st;
    HIP_TRY(hipMemsetAsync(s->pm.pc.get(), 0, sizeof(PpmCounters), st));
    HIP_TRY(hipMemsetAsync(s->ws.wc.get(), 0, sizeof(WorkCounters), st));     // nothing here counts into it: hpt_get_stats reads zeros
    HIP_TRY(hipMemsetAsync(ga.alb_cnt, 0, n_local * sizeof(float4), st));
    HIP_TRY(hipMemsetAsync(ga.nrm, 0, n_local * sizeof(float4), st));
    HIP_TRY(hipMemsetAsync(ga.pos, 0, n_local * sizeof(float4), st));
    if(motion) HIP_TRY(hipMemsetAsync(ga.prev, 0, n_local * sizeof(float4), st));
    HIP_TRY(hipEventRecord(s->tm.ev_start, st));
    for(int pass = 0; pass < spp; ++pass){
        HIP_TRY(hipMemsetAsync(step.w.counters.get(), 0, (size_t) r.n_counters * sizeof(uint32_t), st));
        ppm_mark(s, r, pass, 0);
        rc = ppm_eye_phase(s, r, step, (uint32_t) ((int64_t) P.sample_offset + pass));
        if(rc) return rc;
        if(motion) launch_guides_accumulate_motion(st, s->geo.sd, s->pm.hb, step.w.pb.hit, r.hp_count(s), r.n_local, ga, gm);
        else launch_guides_accumulate(st, s->geo.sd, s->pm.hb, r.hp_count(s), r.n_local, ga);
        for(int k = 1; k <= 4; ++k) ppm_mark(s, r, pass, k);                // the eye phase is the only one: ms_eye
    }
    float *outs[5] = { albedo, normal, position, coverage, prev_position };
    const size_t npx = (size_t) W * H;
    std::vector<float> tmp;
    for(int which = 0; which < 5; ++which){
        if(!outs[which]) continue;
        launch_guides_resolve(st, r.n_local, ga, which, s->ws.local_own.get());
        if(device){      // the three-channel images straight into the caller's; coverage is the first channel of one
            launch_untile(st, r.tl, s->ws.local_own.get(), which != 3 ? outs[which] : s->ws.image_own.get());
            if(which == 3) launch_take_first_channel(st, s->ws.image_own.get(), coverage, (uint32_t) npx);
            HIP_TRY(hipGetLastError());
            continue;
        }
        launch_untile(st, r.tl, s->ws.local_own.get(), s->ws.image_own.get());
        HIP_TRY(hipGetLastError());
        if(which != 3){
            HIP_TRY(hipMemcpy(outs[which], s->ws.image_own.get(), npx * 3 * sizeof(float), hipMemcpyDeviceToHost));
        } else {
            tmp.resize(npx * 3);
            HIP_TRY(hipMemcpy(tmp.data(), s->ws.image_own.get(), npx * 3 * sizeof(float), hipMemcpyDeviceToHost));
            for(size_t k = 0; k < npx; ++k) coverage[k] = tmp[k * 3];
        }
    }
    HIP_TRY(hipEventRecord(s->tm.ev_stop, st));
    HIP_TRY(hipEventSynchronize(s->tm.ev_stop));
    return ppm_collect_stats(s, r, spp);
}

} // namespace

extern "C" {

int hpt_render_guides(hpt_scene *s, const void *camera, int W, int H, int spp, const hpt_params *params,
                      float *albedo, float *normal, float *position, float *coverage){
    return render_guides(s, camera, W, H, spp, params, albedo, normal, position, coverage, nullptr, false);
}

int hpt_render_guides_device(hpt_scene *s, const void *camera, int W, int H, int spp, const hpt_params *params,
                             void *d_albedo, void *d_normal, void *d_position, void *d_coverage){
    return render_guides(s, camera, W, H, spp, params, (float *) d_albedo, (float *) d_normal, (float *) d_position, (float *) d_coverage, nullptr, true);
}

int hpt_render_guides_motion(hpt_scene *s, const void *camera, int W, int H, int spp, const hpt_params *params,
                             float *albedo, float *normal, float *position, float *coverage, float *prev_position){
    return render_guides(s, camera, W, H, spp, params, albedo, normal, position, coverage, prev_position, false);
}

int hpt_render_guides_motion_device(hpt_scene *s, const void *camera, int W, int H, int spp, const hpt_params *params,
                                    void *d_albedo, void *d_normal, void *d_position, void *d_coverage, void *d_prev_position){
    return render_guides(s, camera, W, H, spp, params, (float *) d_albedo, (float *) d_normal, (float *) d_position, (float *) d_coverage,
                         (float *) d_prev_position, true);
}

int hpt_ppm_get_stats(const hpt_scene *s, hpt_ppm_stats *out){
    if(!s || !out) return fail(HPT_ERR_INVALID, "null argument");
    *out = s->pm.stats;
    return HPT_OK;
}

} // extern "C"

// Progressive photon mapping (include/hpt.h, hpt_sppm_*): the per-pixel state of one (scene, camera, image) lives
// here, not in the scene's workspace, so renders of other kinds on the same scene in between leave it alone.
struct hpt_sppm {
    hpt_scene *scene = nullptr;
    unsigned char camera[HPT_CAMERA_BYTES];
    int W = 0, H = 0, eye_depth = 0, light_depth = 0, spl = 0;
    float radius = 0.05f, alpha = 1.0f;
    float smin[3] = { 0, 0, 0 }, smax[3] = { 0, 0, 0 };
    bool scene_smin = false, scene_smax = false;      // created with scene_min / scene_max NULL: hpt_sppm_reset re-reads the scene's
    hpt_params P{};                  // seed, sample_offset, max_delta (clamped), tile
    Tiling tl{};
    int64_t passes = 0;              // K
    DevBuf<float4> tau_r2, direct; DevBuf<float> photons;
    SppmState st{};                  // view of the three buffers above
    DevBuf<float> local, image;      // hpt_sppm_read_state's untile
};

extern "C" {

int hpt_sppm_reset(hpt_sppm *z){
    if(!z) return fail(HPT_ERR_INVALID, "null state");
    if(int rcd = on_scene_device(z->scene)) return rcd;
    // bounds the caller left to the scene are the scene's of now: an update since the last reset has invalidated them
    if(z->scene_smin || z->scene_smax){
        if(int rcb = ppm_scene_bounds(z->scene)) return rcb;
        for(int a = 0; a < 3; ++a){
            if(z->scene_smin) z->smin[a] = z->scene->pm.min[a];
            if(z->scene_smax) z->smax[a] = z->scene->pm.max[a];
        }
    }
    launch_sppm_init(nullptr, z->st, (uint32_t) z->tl.n_local, z->radius * z->radius);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(nullptr));
    z->passes = 0;
    return HPT_OK;
}

void hpt_sppm_destroy(hpt_sppm *state){ delete state; }

int hpt_sppm_create(hpt_scene *s, const void *camera, int W, int H, int eye_depth, int light_depth, int spl, float radius, float alpha,
                    const float *scene_min, const float *scene_max, const hpt_params *params, hpt_sppm **out){
    if(!out) return fail(HPT_ERR_INVALID, "null out");
    *out = nullptr;
    if(!s) return fail(HPT_ERR_INVALID, "null scene");
    if(!camera) return fail(HPT_ERR_INVALID, "null camera");
    if(spl < 0 || eye_depth <= 0 || eye_depth > 255 || light_depth <= 0 || light_depth > 255)
        return fail(HPT_ERR_INVALID, "spl must be >= 0 and depths in [1, 255]");
    if(!(alpha > 0.0f && alpha <= 1.0f)) return fail(HPT_ERR_INVALID, "alpha must be in (0, 1]");
    if(int rcd = on_scene_device(s)) return rcd;
    hpt_params P;
    if(int rcp = take_params(params, kSppmParams, P)) return rcp;
    Tiling tl;
    int rc = make_tiling(W, H, &P, tl);
    if(rc) return rc;
    if(!(radius > 0.0f)) radius = 0.05f;
    hpt_sppm *z = new (std::nothrow) hpt_sppm;
    if(!z) return fail(HPT_ERR_NOMEM, "out of host memory");
    z->scene = s; memcpy(z->camera, camera, HPT_CAMERA_BYTES);
    z->W = W; z->H = H; z->eye_depth = eye_depth; z->light_depth = light_depth; z->spl = spl;
    z->radius = radius; z->alpha = alpha; z->P = P; z->tl = tl;
    z->scene_smin = !scene_min; z->scene_smax = !scene_max;              // filled by hpt_sppm_reset below
    for(int a = 0; a < 3; ++a){ if(scene_min) z->smin[a] = scene_min[a]; if(scene_max) z->smax[a] = scene_max[a]; }
    const size_t n = (size_t) tl.n_local;
    hipError_t e = z->tau_r2.reserve(n);
    if(e == hipSuccess) e = z->photons.reserve(n);
    if(e == hipSuccess) e = z->direct.reserve(n);
    if(e == hipSuccess) e = z->local.reserve(n * 3);
    if(e == hipSuccess) e = z->image.reserve((size_t) W * H * 3);
    if(e != hipSuccess){
        delete z;
        return fail_hip("progressive photon map state", e);
    }
    z->st = SppmState{ z->tau_r2.get(), z->photons.get(), z->direct.get() };
    rc = hpt_sppm_reset(z);
    if(rc){ delete z; return rc; }
    *out = z;
    return HPT_OK;
}

constexpr int32_t kSppmFlags = HPT_FLAG_TIME_KERNELS | HPT_FLAG_COUNT_WORK;

// `passes` more passes of PPM's estimator into the state, then the estimate into host_image (blocking)
int hpt_sppm_render(hpt_sppm *z, int passes, int32_t flags, float *host_image){
    if(!z) return fail(HPT_ERR_INVALID, "null state");
    if(!host_image) return fail(HPT_ERR_INVALID, "null image");
    if(passes <= 0) return fail(HPT_ERR_INVALID, "passes must be > 0");
    if(flags & ~kSppmFlags) return fail(HPT_ERR_INVALID, "hpt_sppm_render accepts HPT_FLAG_TIME_KERNELS and COUNT_WORK only");
    hpt_scene *s = z->scene;
    if(int rcd = on_scene_device(s)) return rcd;
    PpmRun r;
    r.P = z->P; r.P.flags = flags; r.tl = z->tl;
    set_camera(r.cam, z->camera);
    for(int a = 0; a < 3; ++a){ r.fr.smin[a] = z->smin[a]; r.fr.smax[a] = z->smax[a]; }
    r.fr.cell = z->radius; r.fr.r2 = z->radius * z->radius;             // the cell stays the initial radius
    int rc = ppm_prepare(s, r, z->light_depth, z->spl, passes);
    if(rc) return rc;

    hipStream_t st = nullptr;
    PassBuffers &w = s->ws.pass[0];
    HIP_TRY(hipMemsetAsync(s->pm.pc.get(), 0, sizeof(PpmCounters), st));
    HIP_TRY(hipMemsetAsync(s->ws.wc.get(), 0, sizeof(WorkCounters), st));     // nothing here counts into it: hpt_get_stats reads zeros
    if(r.n_dep) launch_ppm_iota(st, s->pm.grid.slot_in, r.n_dep);
    HIP_TRY(hipEventRecord(s->tm.ev_start, st));
    for(int pass = 0; pass < passes; ++pass){
        rc = ppm_phases(s, r, pass, (uint32_t) ((int64_t) r.P.sample_offset + z->passes + pass));
        if(rc) return rc;
        launch_sppm_gather(st, s->geo.sd, s->pm.hb, s->pm.grid, r.hp_count(s), r.n_local, r.fr, z->st, z->alpha,
                           r.count ? s->pm.cand.get() : nullptr, r.count ? s->pm.acc.get() : nullptr, s->pm.pc.get());
        launch_resolve(st, r.tl, w.pb, z->st.direct, 1);                  // D += the guarded direct term
        ppm_mark(s, r, pass, 4);
    }
    z->passes += passes;
    launch_sppm_estimate(st, r.tl, z->st, (float) z->passes, s->ws.local_own.get());
    rc = untile_to_host(s, r.tl, st, host_image, s->tm.ev_stop);
    if(rc) return rc;
    return ppm_collect_stats(s, r, passes);
}

int hpt_sppm_read_state(const hpt_sppm *z, float *radius2, float *photons, int64_t *passes){
    if(!z) return fail(HPT_ERR_INVALID, "null state");
    if(passes) *passes = z->passes;
    if(!radius2 && !photons) return HPT_OK;
    if(int rcd = on_scene_device(z->scene)) return rcd;
    launch_sppm_state(nullptr, z->tl, z->st, z->local.get());
    launch_untile(nullptr, z->tl, z->local.get(), z->image.get());
    HIP_TRY(hipGetLastError());
    const size_t npx = (size_t) z->W * z->H;
    std::vector<float> img(npx * 3);
    HIP_TRY(hipMemcpy(img.data(), z->image.get(), npx * 3 * sizeof(float), hipMemcpyDeviceToHost));
    for(size_t k = 0; k < npx; ++k){
        if(radius2) radius2[k] = img[k * 3 + 0];
        if(photons) photons[k] = img[k * 3 + 1];
    }
    return HPT_OK;
}

} // extern "C"
