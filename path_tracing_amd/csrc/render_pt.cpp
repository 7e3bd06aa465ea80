// The path tracer's host side (include/hpt.h, hpt_render_pt*): pass workspaces, pipelines and the wavefront render
// loop.  Compiled with hipcc (host code only here).
//
// Render loop per pass (S samples of every local pixel in flight):
//   generate -> repeat { trace, shade } until the queue drains -> trace -> resolve
// with two passes in flight at a time on two streams (hpt_render_pt_device).
// Queue counters live in device memory, one slot per iteration, so the host issues the first
// eye_depth iterations without ever reading the device back; only scenes whose paths are still
// alive after that (chains of free delta bounces, reference src/pt_cu.cu:228) cost one
// counter read-back per extra iteration.
#include "hpt_host.h"

using namespace hpt;

namespace {

// device memory per path slot of one pipeline (ensure_pass): path state 80 B, pending shadow ray 48 B, five queues of 4 B,
// the record of a closest-hit ray set aside for the resume launch 48 B
constexpr double kBytesPerPathSlot = 196.0;

int ensure_pass(PassBuffers &w, size_t paths, int n_counters){
    const hipError_t e = reserve_all(paths, w.org_eta, w.dir_flags, w.thr, w.col, w.rng, w.hit, w.org_max, w.dir, w.contrib,
                                     w.queue[0], w.queue[1], w.squeue, w.lqueue[0], w.lqueue[1], w.rec);
    w.pb = PathBuf{ w.org_eta.get(), w.dir_flags.get(), w.thr.get(), w.col.get(), w.rng.get(), w.hit.get() };
    w.sb = ShadowBuf{ w.org_max.get(), w.dir.get(), w.contrib.get() };
    if(e != hipSuccess) return fail_hip("path workspace", e);
    HIP_TRY(w.deep_stack.reserve(resume_deep_stack_words()));
    HIP_TRY(w.counters.reserve((size_t) n_counters));
    if(!w.h_count) HIP_TRY(hipHostMalloc((void **) &w.h_count, 64));
    return HPT_OK;
}

// stream and events of the second pipeline (the first runs on the caller's stream)
int ensure_pipes(hpt_scene::Workspace &ws, hipStream_t caller, int npipes){
    // The pipelines only overlap if their streams sit on different hardware queues.  The runtime maps streams
    // of one priority onto a small pool of queues (GPU_MAX_HW_QUEUES, 4 by default) by reference count, so once a
    // process holds a few more streams -- RCCL's, after a communicator exists -- a second stream of the caller's
    // priority can land on the caller's queue and the passes serialise (measured: 169 ms per config-3 render
    // instead of 161).  Streams of another priority come from another pool: the second pipeline takes the highest
    // priority unless the caller's stream already has it, then the default one.
    int pr_least = 0, pr_greatest = 0, pr_caller = 0;
    HIP_TRY(hipDeviceGetStreamPriorityRange(&pr_least, &pr_greatest));
    if(hipStreamGetPriority(caller, &pr_caller) != hipSuccess){ (void) hipGetLastError(); pr_caller = 0; }
    std::vector<int> levels;                                   // every level but the caller's, highest first
    for(int l = pr_greatest; l <= pr_least; ++l) if(l != pr_caller) levels.push_back(l);
    if(levels.empty()) levels.push_back(pr_caller);
    for(int k = 1; k < npipes; ++k){
        const int want = levels[(size_t) (k - 1) % levels.size()];
        if(ws.px_stream[k] && ws.px_priority[k] != want){ hipStreamSynchronize(ws.px_stream[k]); hipStreamDestroy(ws.px_stream[k]); ws.px_stream[k] = nullptr; }
        if(!ws.px_stream[k]){
            HIP_TRY(hipStreamCreateWithPriority(&ws.px_stream[k], hipStreamNonBlocking, want));
            ws.px_priority[k] = want;
        }
        if(!ws.px_done[k]) HIP_TRY(hipEventCreateWithFlags(&ws.px_done[k], hipEventDisableTiming));
    }
    if(!ws.px_fork) HIP_TRY(hipEventCreateWithFlags(&ws.px_fork, hipEventDisableTiming));
    return HPT_OK;
}

} // namespace

int hpt::ensure_workspace(hpt_scene *s, size_t paths, size_t n_local, int n_counters){
    int rc = ensure_pass(s->ws.pass[0], paths, n_counters);
    if(rc) return rc;
    HIP_TRY(s->ws.accum.reserve(n_local));
    HIP_TRY(s->ws.wc.reserve(1));
    if(!s->tm.ev_start){ HIP_TRY(hipEventCreate(&s->tm.ev_start)); HIP_TRY(hipEventCreate(&s->tm.ev_stop)); }
    return HPT_OK;
}

extern "C" {

// the wavefront render loop; everything is enqueued on `stream`
int hpt_render_pt_device(hpt_scene *s, const void *camera, int W, int H, int eye_depth, int spp,
                         const hpt_params *params, void *d_local, void *hip_stream){
    const hipStream_t stream = (hipStream_t) hip_stream;
    if(!s) return fail(HPT_ERR_INVALID, "null scene");
    if(!camera || !d_local) return fail(HPT_ERR_INVALID, "null camera or output");
    if(spp <= 0 || eye_depth <= 0 || eye_depth > 255) return fail(HPT_ERR_INVALID, "spp must be > 0 and eye_depth in [1, 255]");
    if(int rcd = on_scene_device(s)) return rcd;
    hpt_params P;
    if(int rcp = take_params(params, kRenderParams, P)) return rcp;
    Tiling tl;
    int rc = make_tiling(W, H, &P, tl);
    if(rc) return rc;
    CameraDev cam;
    set_camera(cam, camera);

    const int flags = P.flags;
    const bool count = (flags & HPT_FLAG_COUNT_WORK) != 0;
    const bool timek = (flags & HPT_FLAG_TIME_KERNELS) != 0;
    const bool brute = (flags & HPT_FLAG_BRUTE_FORCE) != 0;      // separate extend/connect kernels (the scan variants)
    const int kflags = (brute ? 1 : 0) | (count ? 2 : 0);

    // Samples in flight per pass: about 128 Mi path slots (24.5 GiB of path state, queues, shadow and deferred-ray records per pipeline:
    // little on a 288 GB device).  Fewer, larger passes amortise the low-occupancy tail iterations of every pass
    // (config 3, ms per 256-spp render, one pipeline: 4 Mi slots 291, 16 Mi 219, 64 Mi 146, 128 Mi 142, 256 Mi 139).
    // Two passes are in flight at a time, on two streams with a workspace each: while one pipeline's kernel drains or
    // waits on memory the other's waves take the issue slots (64 Mi slots each: 138.1 ms, 128 Mi each: 135.7).  A render
    // that fits one pass is cut into two half passes for the same reason -- the share of one rank of a multi-GPU render
    // is such a render (rank 0 of 4 at config 3, 64 Mi slots: one pass 37.2-37.4 ms, two half passes 35.3-36.5; of 2:
    // 72.1 -> 68.2; of 8: 19.5 -> 18.7; on another box 35.4 against 35.6: never a loss beyond the noise) -- unless it is
    // so small (< 1 Mi slots) that launch latencies are what it costs.
    int npipes = (!(flags & HPT_FLAG_SINGLE_PIPELINE) && !count && !brute) ? kMaxPipes : 1;
    int spass = P.samples_per_pass;
    if(spass <= 0){
        long long target = 128ll << 20;
        // ... on a device that has the memory for it: when the workspace would have to grow, the pass is sized so that
        // both pipelines' state fits in 70 % of what is free now plus what the scene already holds (a smaller device,
        // or several scenes on one device, get smaller passes instead of HPT_ERR_NOMEM; the image does not depend on it)
        size_t have = 0; for(const PassBuffers &w : s->ws.pass) have += w.cap_paths();
        if((size_t) std::min<long long>(target, (long long) tl.n_local * spp) > s->ws.pass[0].cap_paths()){
            size_t free_b = 0, total_b = 0;
            if(hipMemGetInfo(&free_b, &total_b) == hipSuccess){
                const double usable = 0.7 * ((double) free_b + (double) have * kBytesPerPathSlot);
                const long long fit = (long long) (usable / (kBytesPerPathSlot * (double) npipes));
                if(fit < target){
                    target = std::max<long long>(fit, tl.n_local);
                    // a workspace sized this way earlier is kept (no reallocation for a few per cent more)
                    if((long long) s->ws.pass[0].cap_paths() >= target * 3 / 4) target = (long long) s->ws.pass[0].cap_paths();
                }
            } else (void) hipGetLastError();
        }
        spass = (int) std::max<long long>(1, target / tl.n_local);
        spass = std::min(spass, spp);
        // every round of the render keeps all pipelines busy: the passes of the render are cut to a multiple of their number
        if(npipes > 1 && spp >= npipes && (long long) tl.n_local * spp >= (1ll << 20)){
            const int rounds = (spp + spass * npipes - 1) / (spass * npipes);
            spass = (spp + rounds * npipes - 1) / (rounds * npipes);
        }
    }
    spass = std::min(spass, spp);
    const int npass = (spp + spass - 1) / spass;
    if(npass < npipes) npipes = npass;
    size_t paths = (size_t) tl.n_local * spass;
    if(paths > 0x7FFFFFF0ull) return fail(HPT_ERR_INVALID, "too many path slots per pass");
    int max_iters = eye_depth + P.max_delta + 1;
    int n_counters = 4 * (max_iters + 2);
    rc = ensure_workspace(s, paths, tl.n_local, n_counters);
    if(rc) return rc;
    for(int k = 1; k < npipes; ++k){ rc = ensure_pass(s->ws.pass[k], paths, n_counters); if(rc) return rc; }
    if(npipes > 1){ rc = ensure_pipes(s->ws, stream, npipes); if(rc) return rc; }

    WorkCounters *wc = count ? s->ws.wc.get() : nullptr;
    reset_render_stats(s);

    // node-step budget of the first trace launch (reserved bits 1-6: 0 = default, 63 = no split).  Unsplit: counting
    // renders (their work counts are those of the plain single-launch traversal), the scan variants, and scenes whose
    // four-wide tree is too deep for the resume launch's stack
    int budget = (P.reserved >> 1) & 0x3F;
    budget = budget == 0 ? kTraceBudget : (budget == 0x3F ? 0 : budget);
    if(count || brute || !resume_walk_fits(s->geo.sd)) budget = 0;
    s->ws.last_budget = budget;
    const int roulette = (flags & HPT_FLAG_RUSSIAN_ROULETTE) ? 1 : 0;

    HIP_TRY(hipMemsetAsync(s->ws.wc.get(), 0, sizeof(WorkCounters), stream));
    HIP_TRY(hipMemsetAsync(s->ws.accum.get(), 0, (size_t) tl.n_local * sizeof(float4), stream));
    HIP_TRY(hipEventRecord(s->tm.ev_start, stream));

    // one pass in flight on one pipeline
    struct Pass {
        PathBuf pb; ShadowBuf sb; DeferredRay *rec; uint32_t *queue[2], *squeue, *lqueue[2], *deep_stack; uint32_t *counters, *h_count; hipStream_t st;
        int sthis = 0, cur = 0, pending_shadow = -1; uint32_t slots = 0; PrimaryGen primary{};
        uint32_t *qcnt = nullptr, *scnt = nullptr, *lecnt = nullptr, *lscnt = nullptr;
    };
    Pass pipe[kMaxPipes]{};
    for(int k = 0; k < npipes; ++k){
        const PassBuffers &w = s->ws.pass[k];
        Pass &q = pipe[k];
        q.pb = w.pb; q.sb = w.sb; q.rec = w.rec.get(); q.queue[0] = w.queue[0].get(); q.queue[1] = w.queue[1].get(); q.squeue = w.squeue.get();
        q.lqueue[0] = w.lqueue[0].get(); q.lqueue[1] = w.lqueue[1].get();
        q.deep_stack = w.deep_stack.get();
        q.counters = w.counters.get(); q.h_count = w.h_count; q.st = k == 0 ? stream : s->ws.px_stream[k];
    }
    for(Pass &q : pipe){
        if(!q.counters) continue;
        q.qcnt = q.counters;                              // qcnt[i]: paths entering iteration i
        q.scnt = q.counters + (max_iters + 2);            // scnt[i]: shadow rays of iteration i
        q.lecnt = q.counters + 2 * (max_iters + 2);       // lecnt[i] / lscnt[i]: rays the trace launch of
        q.lscnt = q.counters + 3 * (max_iters + 2);       // iteration i set aside for its second launch
    }

    // Iteration 0 needs no generate launch: its trace and shade kernels recompute the camera ray of a slot from the slot
    // number (PRIMARY variants; -3 % per render: the launch and the 72 B per path it writes and iteration 0 reads back).
    // The counting and the scan variants keep the stored form.
    const bool in_flight_primaries = !count && !brute;
    auto begin_pass = [&](Pass &q, int done) -> int {
        q.sthis = std::min(spass, spp - done);
        q.slots = (uint32_t) tl.n_local * (uint32_t) q.sthis;
        q.cur = 0; q.pending_shadow = -1;
        HIP_TRY(hipMemsetAsync(q.counters, 0, (size_t) n_counters * sizeof(uint32_t), q.st));
        q.primary.tl = tl; q.primary.cam = cam; q.primary.first_sample = (uint32_t) (P.sample_offset + done); q.primary.pad = 0u; q.primary.seed = P.seed;
        if(in_flight_primaries){
            HIP_TRY(hipMemsetD32Async((hipDeviceptr_t) &q.qcnt[0], (int) q.slots, 1, q.st));
        } else {
            LaunchTimer t(s, q.st, timek, 3);
            launch_generate(q.st, tl, cam, q.pb, &q.qcnt[0], q.sthis, q.primary.first_sample, P.seed, wc);
        }
        return HPT_OK;
    };
    // HPT_FLAG_NO_HOST_WAIT enqueues the iterations past eye_depth without knowing whether a path is left: those launches
    // get a grid of 8 workgroups per CU instead of one sized for a full queue (an empty launch then costs a few
    // microseconds instead of ~80), and the kernels walk the chunks of whatever the queue holds with a stride
    const uint32_t blind_groups = (flags & HPT_FLAG_NO_HOST_WAIT) ? (uint32_t) std::max(s->num_cus, 1) * 8u : 0u;
    auto iteration = [&](Pass &q, int it){
        const uint32_t *eq = it == 0 ? nullptr : q.queue[q.cur];
        const PrimaryGen *primary = (it == 0 && in_flight_primaries) ? &q.primary : nullptr;
        const uint32_t cap = it >= eye_depth ? blind_groups : 0u;
        if(brute){
            LaunchTimer t(s, q.st, timek, 0);
            launch_extend(q.st, s->geo.sd, q.pb, eq, &q.qcnt[it], q.slots, kflags, wc);
        } else {
            // extension rays of this iteration + shadow rays of the previous one, one launch
            TraceSplit split{ q.lqueue[0], &q.lecnt[it], q.lqueue[1], &q.lscnt[it], budget, q.rec };
            { LaunchTimer t(s, q.st, timek, 0);
              launch_trace(q.st, s->geo.sd, q.pb, q.sb, eq, &q.qcnt[it], q.slots, q.squeue,
                           q.pending_shadow >= 0 ? &q.scnt[q.pending_shadow] : nullptr, q.slots, s->geo.stack_levels, count, wc, &split, primary, cap); }
            if(split.budget > 0){
                LaunchTimer t(s, q.st, timek, 4);
                launch_trace_resume(q.st, s->geo.sd, q.pb, q.sb, true, q.pending_shadow >= 0, q.slots, wc, split, primary, cap, q.deep_stack);
            }
            q.pending_shadow = -1;
        }
        { LaunchTimer t(s, q.st, timek, 1);
          launch_shade(q.st, s->geo.sd, q.pb, eq, &q.qcnt[it], q.slots, q.queue[q.cur ^ 1],
                       &q.qcnt[it + 1], q.sb, q.squeue, &q.scnt[it], eye_depth, P.max_delta, roulette, wc, primary, cap); }
        if(brute){
            LaunchTimer t(s, q.st, timek, 2);
            launch_connect(q.st, s->geo.sd, q.pb, q.sb, q.squeue, &q.scnt[it], q.slots, kflags, wc);
        } else q.pending_shadow = it;
        q.cur ^= 1;
    };
    // Iterations past eye_depth: only paths that took free delta bounces are still alive (reference src/pt_cu.cu:228),
    // and how many more iterations they need is known on the device only.  The host looks before it launches, every
    // other iteration (an empty launch costs less than a read-back): the counter of each pipeline in flight is read
    // back on that pipeline's stream FIRST, then the host waits for one after the other, so the pipelines keep running
    // side by side while it does.  This is the one place where hpt_render_pt_device blocks the calling thread
    // (include/hpt.h); a scene without delta materials never gets here with a non-empty queue and pays one read-back.
    const bool no_host_wait = (flags & HPT_FLAG_NO_HOST_WAIT) != 0;     // enqueue every tail iteration unseen
    auto tails = [&](int npipes) -> int {
        bool live[kMaxPipes]; int nlive = npipes;
        for(int k = 0; k < kMaxPipes; ++k) live[k] = k < npipes;
        for(int it = eye_depth; it < max_iters && nlive > 0; ++it){
            const bool look = !no_host_wait && ((it - eye_depth) & 1) == 0;
            if(look) for(int k = 0; k < npipes; ++k) if(live[k])
                HIP_TRY(hipMemcpyAsync(pipe[k].h_count, &pipe[k].qcnt[it], sizeof(uint32_t), hipMemcpyDeviceToHost, pipe[k].st));
            for(int k = 0; k < npipes; ++k){
                if(!live[k]) continue;
                if(look){
                    HIP_TRY(hipStreamSynchronize(pipe[k].st));
                    if(*pipe[k].h_count == 0u){ live[k] = false; --nlive; continue; }
                }
                iteration(pipe[k], it);
            }
        }
        for(int k = 0; k < npipes; ++k){
            Pass &q = pipe[k];
            if(q.pending_shadow < 0) continue;
            TraceSplit split{ q.lqueue[0], &q.lecnt[max_iters], q.lqueue[1], &q.lscnt[max_iters], budget, q.rec };
            { LaunchTimer t(s, q.st, timek, 2);
              launch_trace(q.st, s->geo.sd, q.pb, q.sb, nullptr, nullptr, 0, q.squeue, &q.scnt[q.pending_shadow], q.slots,
                           s->geo.stack_levels, count, wc, &split, nullptr, blind_groups); }
            if(split.budget > 0){
                LaunchTimer t(s, q.st, timek, 4);
                launch_trace_resume(q.st, s->geo.sd, q.pb, q.sb, false, true, q.slots, wc, split, nullptr, blind_groups, q.deep_stack);
            }
        }
        return HPT_OK;
    };

    for(int done = 0; done < spp; done += spass * npipes){
        int active = 0;                                     // pipelines with a pass in this round
        while(active < npipes && done + active * spass < spp) ++active;
        if(active > 1){
            // the other pipelines start after everything already queued on the caller's stream (the previous
            // resolve of their radiance buffers included)
            HIP_TRY(hipEventRecord(s->ws.px_fork, stream));
            for(int k = 1; k < active; ++k) HIP_TRY(hipStreamWaitEvent(s->ws.px_stream[k], s->ws.px_fork, 0));
        }
        for(int k = 0; k < active; ++k){ rc = begin_pass(pipe[k], done + k * spass); if(rc) return rc; }
        for(int it = 0; it < eye_depth && it < max_iters; ++it)
            for(int k = 0; k < active; ++k) iteration(pipe[k], it);
        rc = tails(active); if(rc) return rc;
        // the per-pixel sums are added in sample order: pipeline 0's pass, then the next one's, ...
        for(int k = 0; k < active; ++k){
            if(k > 0){
                HIP_TRY(hipEventRecord(s->ws.px_done[k], s->ws.px_stream[k]));
                HIP_TRY(hipStreamWaitEvent(stream, s->ws.px_done[k], 0));
            }
            LaunchTimer t(s, stream, timek, 3);
            launch_resolve(stream, tl, pipe[k].pb, s->ws.accum.get(), pipe[k].sthis);
            s->ws.last_counters = pipe[k].counters;
        }
    }
    float divisor = (flags & HPT_FLAG_OUTPUT_SUM) ? 1.0f : (float) spp;
    { LaunchTimer t(s, stream, timek, 3);
      launch_finalize(stream, tl, s->ws.accum.get(), (float *) d_local, divisor); }
    HIP_TRY(hipEventRecord(s->tm.ev_stop, stream));
    HIP_TRY(hipGetLastError());
    s->tm.stats_pending = true;
    s->ws.last_counter_stride = max_iters + 2;
    return HPT_OK;
}

int hpt_render_pt(hpt_scene *s, const void *camera, int W, int H, int eye_depth, int spp,
                  const hpt_params *params, float *host_image){
    if(!s) return fail(HPT_ERR_INVALID, "null scene");
    if(!host_image) return fail(HPT_ERR_INVALID, "null image");
    if(params && params->world > 1) return fail(HPT_ERR_INVALID, "hpt_render_pt renders the whole image: world must be 0 or 1");
    Tiling tl;
    int rc = make_tiling(W, H, params, tl);
    if(rc) return rc;
    rc = ensure_own_image(s, tl);
    if(rc) return rc;
    rc = hpt_render_pt_device(s, camera, W, H, eye_depth, spp, params, s->ws.local_own.get(), nullptr);
    if(rc) return rc;
    return untile_to_host(s, tl, nullptr, host_image);
}

} // extern "C"
