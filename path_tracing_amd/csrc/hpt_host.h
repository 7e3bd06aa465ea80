// Host side of libhpt.so, shared by its translation units (hpt_api.cpp, render_pt.cpp, render_bdpt.cpp, render_ppm.cpp,
// denoise.cpp, hpt_multi.cpp, scene_update.cpp, scene_rebuild.cpp, scene_rebuild_device.cpp): the error channel, the owner of device memory, struct hpt_scene and the steps every integrator takes.
// Internal and host only; compiled as HIP because it includes the launch interfaces.
#pragma once
#include "../../include/hpt.h"
#include "hpt_scene.h"
#include "pt_kernels.h"
#include "bdpt_kernels.h"
#include "ppm_kernels.h"
#include "denoise_kernels.h"
#include "refit_kernels.h"
#include "lbvh_kernels.h"

#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

namespace hpt {

// sets the calling thread's hpt_last_error text; returns `code`
int fail(int code, const std::string &msg);

// a failed HIP call as an error code: "<what>: <the runtime's text>"
inline int fail_hip(const std::string &what, hipError_t e){
    return fail(e == hipErrorOutOfMemory ? HPT_ERR_NOMEM : HPT_ERR_DEVICE, what + ": " + hipGetErrorString(e));
}

#define HIP_TRY(expr) do { hipError_t e_ = (expr); if(e_ != hipSuccess) return hpt::fail_hip(#expr, e_); } while(0)

// One device allocation and the number of elements it holds; the capacity is kept here and nowhere else.  Grow-only, one
// hipMalloc per buffer, old contents are not kept: reserve() releases before it allocates, and a failed allocation
// leaves the buffer empty with capacity 0, so the next reserve() allocates again (or fails again) and get() is null
// until then.  Released by the destructor.
template <typename T>
class DevBuf {
    T *p_ = nullptr; size_t cap_ = 0;
public:
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    ~DevBuf(){ release(); }
    T *get() const { return p_; }
    size_t capacity() const { return cap_; }
    void release(){ if(p_) hipFree(p_); p_ = nullptr; cap_ = 0; }
    void swap(DevBuf &o){ std::swap(p_, o.p_); std::swap(cap_, o.cap_); }
    hipError_t reserve(size_t n){
        if(n <= cap_) return hipSuccess;
        release();
        hipError_t e = hipMalloc((void **) &p_, n * sizeof(T));
        if(e != hipSuccess){ p_ = nullptr; return e; }
        cap_ = n;
        return hipSuccess;
    }
    // a fresh allocation that holds the vector's elements (one element for an empty vector)
    template <typename A>
    hipError_t upload(const std::vector<T, A> &v){
        release();
        hipError_t e = reserve(std::max<size_t>(v.size(), 1));
        if(e == hipSuccess && !v.empty()) e = hipMemcpy(p_, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice);
        return e;
    }
};

// Buffers that share one capacity: when they are too small all of them are released before any is allocated, and a
// failed allocation leaves all of them empty.  The capacity of the set is the capacity of any member.
template <typename First, typename... Rest>
hipError_t reserve_all(size_t n, First &first, Rest &... rest){
    if(n <= first.capacity()) return hipSuccess;
    first.release(); (rest.release(), ...);
    hipError_t e = first.reserve(n);
    ((e = e == hipSuccess ? rest.reserve(n) : e), ...);
    if(e != hipSuccess){ first.release(); (rest.release(), ...); }
    return e;
}

struct TimedLaunch { hipEvent_t a, b; int cls; };
constexpr int kMaxPipes = 2;             // passes of a render in flight at a time, at most

} // namespace hpt

struct hpt_scene {
    int device = 0;
    int num_cus = 256;

    // scene geometry: the flattened scene on the device, and the records and grouping it was built from (the wrapper
    // cache compares them; the bidirectional scene is built from them on first use)
    struct Geometry {
        hpt::SceneDev sd{};
        hpt::DevBuf<hpt::BvhNode> nodes; hpt::DevBuf<hpt::QBvhNode> qnodes; hpt::DevBuf<hpt::WideNode> wnodes;
        hpt::DevBuf<hpt::DevTriangle> tris; hpt::DevBuf<hpt::DevRound> rounds;
        hpt::DevBuf<hpt::DevMaterial> mats; hpt::DevBuf<hpt::DevLight> lights;
        hpt::DevBuf<float4> tri_frames;
        int stack_levels = hpt::kStackDepth;       // traversal stack entries per lane
        std::vector<unsigned char> h_lights, h_spheres, h_tris;
        int nl = 0, ns = 0, nt = 0;
        std::vector<int32_t> g_kind, g_index, g_group;
    } geo;

    // workspace, grown on demand.  Two passes of a PT render are in flight at a time (hpt_render_pt_device), each with its
    // own path state, queues and counters (pass[0] on the caller's stream, pass[1] on px_stream[1]) -- the kernels of one
    // fill the issue slots the other leaves idle; everything else (BDPT, photon mapping) uses pass[0]
    struct PassBuffers {
        hpt::DevBuf<float4> org_eta, dir_flags, thr, col; hpt::DevBuf<uint2> rng, hit;      // pb
        hpt::DevBuf<float4> org_max, dir, contrib;                                          // sb
        hpt::PathBuf pb{}; hpt::ShadowBuf sb{};      // views of the buffers above, filled by ensure_pass
        hpt::DevBuf<uint32_t> queue[2];              // path queues (ping-pong)
        hpt::DevBuf<uint32_t> squeue;                // shadow queue (record indices)
        hpt::DevBuf<uint32_t> lqueue[2];             // rays set aside by the first trace launch: closest-hit, shadow
        hpt::DevBuf<hpt::DeferredRay> rec;           // ... the closest-hit ones past iteration 0 as records (lqueue[0] lists their indices)
        hpt::DevBuf<uint32_t> deep_stack;            // stack levels of the resume launch past its LDS share (launch_trace_resume)
        hpt::DevBuf<uint32_t> counters;
        uint32_t *h_count = nullptr;                 // pinned read-back word
        size_t cap_paths() const { return org_eta.capacity(); }
    };
    struct Workspace {
        PassBuffers pass[hpt::kMaxPipes];
        hipStream_t px_stream[hpt::kMaxPipes] = {}; int px_priority[hpt::kMaxPipes] = {};    // pipelines 1..: own streams
        hipEvent_t px_fork = nullptr, px_done[hpt::kMaxPipes] = {};
        const uint32_t *last_counters = nullptr;     // counters of the last pass rendered (either pipeline)
        int last_counter_stride = 0;          // layout of `counters` after the last PT render (0: not a PT render)
        int last_budget = 0;                  // node-step budget of the last PT render's first trace launch (0: unsplit)
        hpt::DevBuf<float4> accum;
        hpt::DevBuf<hpt::WorkCounters> wc;
        hpt::DevBuf<float> local_own, image_own;     // the blocking renders' packed local framebuffer and row-major image
    } ws;

    // bidirectional (cpu_bdpt-estimator) path: device scene built on first use, eye-path state and light vertices
    struct Bdpt {
        bool ready = false;
        hpt::BdptSceneDev sc{};
        hpt::DevBuf<hpt::BvhNode> nodes; hpt::DevBuf<hpt::DevTriangle> tris; hpt::DevBuf<hpt::DevRound> spheres;
        hpt::DevBuf<hpt::DevGroup> groups; hpt::DevBuf<hpt::DevMaterial> mats; hpt::DevBuf<hpt::DevLight> lights;
        hpt::DevBuf<float4> last_pos_pdf, last_normal, vtx_pos, vtx_nrm, vtx_thr, vtx_wo, vtx_base, ectx, hist_pos_eta, contrib;
        hpt::DevBuf<float2> hist_pdf; hpt::DevBuf<unsigned long long> valid;
        hpt::BdptPathBuf bp{};                       // view of the buffers above, filled by ensure_bdpt_workspace
        hpt::DevBuf<hpt::LightVertexDev> lv; hpt::DevBuf<hpt::LightVertexCtx> lctx; hpt::DevBuf<uint32_t> cqueue;
    } bd;

    // photon-mapping path (hpt_render_ppm, hpt_sppm_render): hit points, deposits and grid, grown on demand
    struct Ppm {
        bool bounds_ready = false; float min[3] = {0, 0, 0}, max[3] = {0, 0, 0};   // the scene's own bounds
        hpt::DevBuf<float4> pos_mat, nrm, wo, thr; hpt::DevBuf<uint32_t> list;                // hb
        hpt::DevBuf<float4> dep, packed; hpt::DevBuf<uint32_t> key, slot_in, key_sorted, slot_sorted;   // grid
        hpt::DevBuf<uint2> range; hpt::DevBuf<unsigned char> sort_tmp;
        hpt::PpmHitBuf hb{}; hpt::PpmGrid grid{};    // views of the buffers above, filled by ppm_prepare
        hpt::DevBuf<uint32_t> cand, acc;
        hpt::DevBuf<hpt::PpmCounters> pc;
        hpt::DevBuf<float4> g_alb, g_nrm, g_pos;     // hpt_render_guides: per-pixel sums over the call's samples (GuideAccum)
        hpt::DevBuf<float4> g_prev;                  // ... and of the previous positions, once a call asks for the motion guide
        std::vector<hipEvent_t> marks;               // TIME_KERNELS: five events per pass (eye, photon, grid, gather, end)
        hpt_ppm_stats stats{};
    } pm;

    // scene updates (scene_update.cpp): what the build left for a refit, kept on the host until the first update, and
    // the refit's scratch on the device, allocated by the first update and kept
    struct Update {
        std::vector<uint32_t> level_begin;           // levels of the breadth-first binary tree (HostScene::level_begin)
        hpt::pod_vector<uint32_t> wide_src;          // four per wide node (HostScene::wide_src)
        std::vector<uint32_t> sphere_material;       // material number of every sphere (the update does not re-intern)
        uint32_t num_wide = 0;
        bool ready = false;                          // d_wide_src holds wide_src
        hpt::DevBuf<uint4> d_wide_src;
        hpt::DevBuf<float> verts, slot_box, exact, partial, result;      // 9 / slot 6 / node 6 / block 6 floats; 6 floats + the dead count
        std::vector<float> h_verts;
        hipEvent_t ev_a = nullptr, ev_b = nullptr;
        hpt_update_info info{};
        // the previous geometry G' (include/hpt.h, "motion"), allocated by the first update from the records the scene
        // keeps: the vertices as `verts` holds them (which from then on is the current geometry's) and centre | radius of
        // every sphere.  Until then G' is G and nothing is held.
        bool prev_ready = false;
        bool motion = false;                         // an update succeeded since creation / the last hpt_scene_keep_previous
        hpt::DevBuf<float> prev_verts;
        hpt::DevBuf<float4> prev_rounds;
        // poses (include/hpt.h, "poses"), allocated by hpt_scene_set_parts: the rest pose as `verts` held it then (and as every
        // later update that is not a pose leaves it), each triangle's part, and the table of the last pose
        int num_parts = 0;                           // 0: no parts
        hpt::DevBuf<float> rest_verts, xforms;       // 9 floats per triangle; 12 per part
        hpt::DevBuf<int32_t> tri_part;
        // skinning (include/hpt.h, "skinning"), allocated by hpt_scene_set_skin: per corner four 16-bit bone indices in one
        // 8-byte word and four weights.  A scene holds parts or a skin, never both; the two share rest_verts and xforms
        int num_bones = 0;                           // 0: no skin
        hpt::DevBuf<uint2> skin_bone;
        hpt::DevBuf<float4> skin_weight;
        // morph targets (include/hpt.h, "morph targets"), allocated by hpt_scene_set_morphs: the targets turned round into one
        // run of 16-byte entries per corner (transpose_morphs, scene_build.cpp) and the weights of the last morph.  Morphs sit
        // beside the deformer, not in its place: with both, a morph writes the morphed rest pose into morph_verts and the
        // deformer reads that instead of rest_verts; with morphs alone the morph writes `verts` and morph_verts stays empty.
        // deformer_identity: no pose or skin since the rest pose was last captured, so the deformer's table is the identity
        int num_targets = 0;                         // 0: no morphs
        hpt::DevBuf<uint32_t> morph_begin;           // 3 * nt + 1
        hpt::DevBuf<uint4> morph_entries;
        hpt::DevBuf<float> morph_weights, morph_verts;      // one per target; 9 floats per triangle
        bool deformer_identity = true;
        // an update that brought no records (device vertices, a pose) leaves the vertex bytes of geo.h_tris behind `verts`:
        // host_triangles() brings them up to date for the few readers there are
        bool h_tris_stale = false;
    } up;

    // tree cost and rebuild (scene_rebuild.cpp): the cost kernel's result, allocated by the first hpt_scene_tree_cost, and
    // the description of the last rebuild
    struct Rebuild {
        hpt::DevBuf<unsigned long long> cost;        // kCostResultWords
        hpt_rebuild_info info{};
        hpt_device_build_info dinfo{};               // the last hpt_scene_rebuild_device (scene_rebuild_device.cpp)
        hpt_bounded_build_info binfo{};              // the last hpt_scene_rebuild_device_bounded
        hipEvent_t ev[5] = {};                       // ... and the events around its four phases
    } rb;

    // timing and statistics of the last render
    struct Timing {
        hipEvent_t ev_start = nullptr, ev_stop = nullptr;
        std::vector<hpt::TimedLaunch> timed; std::vector<hipEvent_t> event_pool; size_t event_next = 0;
        hpt_stats stats{};
        bool stats_pending = false;
    } tm;
};

namespace hpt {

using PassBuffers = hpt_scene::PassBuffers;

// ---- steps every integrator takes (hpt_api.cpp unless said otherwise) ---------------------------------------------

// The scene's buffers live on the device that was current when it was created; launching from a thread whose current
// device is another one would hand those pointers to the wrong GPU (a fault, not an error code).
int on_scene_device(const hpt_scene *s);

// What hpt_params may hold for one entry point.  A null message stands for the generic text that names the stray bits.
struct ParamRules {
    const char *one_device;       // not null: world > 1 is refused with this text
    int32_t flags; const char *flags_msg;
    int32_t reserved; const char *reserved_msg;
};
// the documented bits of hpt_params (include/hpt.h): flags HPT_FLAG_*, reserved bits 1-6 (the trace budget)
constexpr int32_t kKnownFlags = HPT_FLAG_BRUTE_FORCE | HPT_FLAG_COUNT_WORK | HPT_FLAG_OUTPUT_SUM | HPT_FLAG_TIME_KERNELS |
                                HPT_FLAG_RUSSIAN_ROULETTE | HPT_FLAG_SINGLE_PIPELINE | HPT_FLAG_NO_HOST_WAIT;
constexpr int32_t kReservedBudgetBits = 0x3F << 1;
constexpr ParamRules kRenderParams{ nullptr, kKnownFlags, nullptr, kReservedBudgetBits, nullptr };   // hpt_render_pt*, hpt_render_bdpt*
// P = *params (zeros for null), checked against `rules` (world, flags, reserved, in this order), max_delta defaulted
// to 64 and clamped to 250
int take_params(const hpt_params *params, const ParamRules &rules, hpt_params &P);

int make_tiling(int W, int H, const hpt_params *p, Tiling &tl);

// CudaCamera: eye, U, V, W, UL, dx, dy (12 B each)
inline void set_camera(CameraDev &cam, const void *camera){
    const float *cf = (const float *) camera;
    memcpy(cam.eye, cf + 0, 12); memcpy(cam.UL, cf + 12, 12); memcpy(cam.dx, cf + 15, 12); memcpy(cam.dy, cf + 18, 12);
}

// pass[0], the accumulator, the work counters and the render's two events (render_pt.cpp)
int ensure_workspace(hpt_scene *s, size_t paths, size_t n_local, int n_counters);

// the scene's own local framebuffer and image hold this tiling
int ensure_own_image(hpt_scene *s, const Tiling &tl);
// ws.local_own -> row-major image -> host_image (blocking); `after`, when given, is recorded behind the untile
int untile_to_host(hpt_scene *s, const Tiling &tl, hipStream_t st, float *host_image, hipEvent_t after = nullptr);

// A render starts: no timed launches, no per-class times, no PT counters to read (hpt_get_stats reports the total
// time only unless the render says otherwise afterwards)
inline void reset_render_stats(hpt_scene *s){
    s->tm.timed.clear(); s->tm.event_next = 0;
    s->ws.last_counter_stride = 0; s->ws.last_budget = 0;
    s->tm.stats.ms_total = s->tm.stats.ms_extend = s->tm.stats.ms_shade = s->tm.stats.ms_connect = s->tm.stats.ms_other = 0.0;
    s->tm.stats.n_extend = s->tm.stats.n_shade = s->tm.stats.n_connect = s->tm.stats.n_other = 0;
}

inline hipEvent_t pool_event(hpt_scene *s){
    if(s->tm.event_next == s->tm.event_pool.size()){
        hipEvent_t e; hipEventCreate(&e); s->tm.event_pool.push_back(e);
    }
    return s->tm.event_pool[s->tm.event_next++];
}

struct LaunchTimer {        // brackets one launch with events when TIME_KERNELS is set
    hpt_scene *s; hipStream_t st; bool on; TimedLaunch tl;
    LaunchTimer(hpt_scene *s_, hipStream_t st_, bool on_, int cls) : s(s_), st(st_), on(on_) {
        if(on){ tl.a = pool_event(s); tl.b = pool_event(s); tl.cls = cls; hipEventRecord(tl.a, st); }
    }
    ~LaunchTimer(){ if(on){ hipEventRecord(tl.b, st); s->tm.timed.push_back(tl); } }
};

inline bool same_bytes(const std::vector<unsigned char> &kept, const void *given, size_t bytes){
    return kept.size() == bytes && (bytes == 0 || memcmp(kept.data(), given, bytes) == 0);
}

// The records the handle holds now, geo.h_tris: the scene's 84 non-vertex bytes with the current vertices.  After an update
// that brought vertices on the device only (scene_update.cpp) this downloads `verts` and splices the 36 bytes per record --
// once, and only here, so a handle whose records nobody reads never pays for it.  Readers of the vertex bytes go through it.
int host_triangles(hpt_scene *s, const unsigned char **tris);

// scene_update.cpp, shared with the device build (scene_rebuild_device.cpp).  ensure_previous: the device vertices (and the
// previous geometry) of a scene that was never updated, from the records it keeps.  ensure_scratch: the refit's scratch for
// the handle's tree.  refit_tree_boxes: the refit's launches up to the quantised binary tree -- leaf records, slot boxes, the
// live box, node boxes level by level, the grid, qnodes -- on the tree handed over (the handle's own, or one being built),
// from up.verts through the handle's scratch; `exact` holds 6 floats per node.
int ensure_previous(hpt_scene *s);
int ensure_scratch(hpt_scene *s);
struct RefitTree { float4 *nodes; uint4 *qnodes; float4 *tris; float *exact; uint32_t num_nodes; const std::vector<uint32_t> *level_begin; };
int refit_tree_boxes(hpt_scene *s, const RefitTree &t, RefitGrid &grid, uint32_t &ndead);

// the arrays and the description hpt_bvh_export_host hands out, of a scene built (or refitted) on the host (hpt_api.cpp)
int export_host_tree(const HostScene &hs, hpt_bvh_info *info, void *qnodes_out, size_t qnodes_cap, void *tris_out, size_t tris_cap);

// hpt_multi.cpp: the fan-out kept by the one-shot wrappers is reused for byte-identical arrays
bool multi_matches(const hpt_multi *m, int n_devices, const void *lights, int nl, const void *spheres, int ns, const void *tris, int nt);

} // namespace hpt
