// Tree cost and rebuild (include/hpt.h): a live tree measured where it lies (cost_kernels.hip, to the integers of
// tree_cost_sums_host; the doubles by tree_cost_compose, scene_build.cpp), and a new tree built by the host builder of
// hpt_scene_create from the records the handle holds now, swapped in under everything else the handle keeps.
// Compiled with hipcc (host code only).
#include "hpt_host.h"

#include <chrono>
#include <cstdio>

using namespace hpt;

static_assert(sizeof(hpt_tree_cost) == 120 && offsetof(hpt_tree_cost, root_extent) == kCostCounters * 8 && sizeof(hpt_rebuild_info) == 48,
              "ABI records: keep path_tracing_amd/__init__.py in step");

namespace {

constexpr uint32_t kMaxCostNodes = 1u << 24;       // the bound behind "no sum reaches 2^60" (include/hpt.h)

double ms_since(std::chrono::steady_clock::time_point t0){
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

} // namespace

extern "C" {

int hpt_bvh_cost_host(const hpt_bvh_info *info, const void *qnodes, size_t qnodes_bytes, hpt_tree_cost *out){
    if(!info || !qnodes || !out) return fail(HPT_ERR_INVALID, "null argument");
    if(info->num_nodes < 1) return fail(HPT_ERR_INVALID, "a tree has at least one node");
    if((uint32_t) info->num_nodes >= kMaxCostNodes) return fail(HPT_ERR_INVALID, "a tree has fewer than 2^24 nodes");
    if(qnodes_bytes < (size_t) info->num_nodes * sizeof(QBvhNode)) return fail(HPT_ERR_INVALID, "qnodes_bytes is below num_nodes * 32");
    tree_cost_sums_host((const QBvhNode *) qnodes, (uint32_t) info->num_nodes, *out);
    tree_cost_compose(info->qscale, *out);
    return HPT_OK;
}

int hpt_scene_tree_cost(hpt_scene *s, hpt_tree_cost *out){
    if(!s || !out) return fail(HPT_ERR_INVALID, "null argument");
    if(int rc = on_scene_device(s)) return rc;
    const hpt_scene::Geometry &g = s->geo;
    if(g.sd.num_nodes < 1 || (uint32_t) g.sd.num_nodes >= kMaxCostNodes) return fail(HPT_ERR_INVALID, "internal error: node count out of range");
    HIP_TRY(s->rb.cost.reserve(kCostResultWords));
    HIP_TRY(hipMemsetAsync(s->rb.cost.get(), 0, kCostResultWords * sizeof(unsigned long long), nullptr));
    launch_tree_cost(nullptr, (const uint4 *) g.qnodes.get(), (uint32_t) g.sd.num_nodes, s->rb.cost.get());
    HIP_TRY(hipGetLastError());
    unsigned long long res[kCostResultWords];
    HIP_TRY(hipMemcpy(res, s->rb.cost.get(), sizeof res, hipMemcpyDeviceToHost));
    memset(out, 0, sizeof *out);
    memcpy(out, res, kCostCounters * sizeof(uint64_t) + 3 * sizeof(uint32_t));       // the sums, then root_extent
    out->num_nodes = (uint32_t) g.sd.num_nodes;
    tree_cost_compose(g.sd.qscale, *out);
    return HPT_OK;
}

int hpt_scene_rebuild(hpt_scene *s){
    if(!s) return fail(HPT_ERR_INVALID, "null scene");
    if(int rc = on_scene_device(s)) return rc;
    hpt_scene::Geometry &g = s->geo;
    hpt_scene::Update &u = s->up;
    const int nt = g.nt;

    auto t0 = std::chrono::steady_clock::now();
    const unsigned char *tris = nullptr;
    if(int rc = host_triangles(s, &tris)) return rc;
    const double ms_download = ms_since(t0);

    t0 = std::chrono::steady_clock::now();
    HostScene hs;
    const char *err = build_host_scene(g.h_lights.data(), g.nl, g.h_spheres.data(), g.ns, tris, nt, hs);
    const double ms_build = ms_since(t0);
    if(err && *err) return fail(HPT_ERR_DEVICE, std::string("rebuild: the builder refused the scene's own records: ") + err);
    // the non-vertex bytes never change, so the builder interns the table the handle holds
    std::vector<DevMaterial> kept((size_t) std::max(g.sd.num_mats, 0));
    if(!kept.empty()) HIP_TRY(hipMemcpy(kept.data(), g.mats.get(), kept.size() * sizeof(DevMaterial), hipMemcpyDeviceToHost));
    if(hs.materials.size() != kept.size() || (!kept.empty() && memcmp(hs.materials.data(), kept.data(), kept.size() * sizeof(DevMaterial)) != 0))
        return fail(HPT_ERR_DEVICE, "rebuild: the material table of the scene's records is not the one the handle holds");
    if(hs.level_begin.size() < 2 || hs.level_begin.back() != (uint32_t) hs.nodes.size() || hs.qnodes.size() != hs.nodes.size())
        return fail(HPT_ERR_DEVICE, "rebuild: internal error: the builder left no refit tables");

    // fresh buffers; the handle is touched only when all of them are filled
    t0 = std::chrono::steady_clock::now();
    DevBuf<BvhNode> nodes; DevBuf<QBvhNode> qnodes; DevBuf<WideNode> wnodes; DevBuf<DevTriangle> dtris; DevBuf<float4> frames;
    hipError_t e = nodes.upload(hs.nodes);
    if(e == hipSuccess) e = qnodes.upload(hs.qnodes);
    if(e == hipSuccess) e = wnodes.upload(hs.wnodes);
    if(e == hipSuccess) e = dtris.upload(hs.tris);
    if(e == hipSuccess) e = frames.reserve(std::max<size_t>((size_t) nt, 1) * 4);
    if(e != hipSuccess) return fail_hip("rebuild: tree upload", e);
    launch_tri_frames(nullptr, (const float4 *) dtris.get(), nt, frames.get());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
    const double ms_upload = ms_since(t0);

    hpt_rebuild_info &ri = s->rb.info;
    ri.nodes_before = s->tm.stats.bvh_nodes; ri.depth_before = s->tm.stats.bvh_depth;
    g.nodes.swap(nodes); g.qnodes.swap(qnodes); g.wnodes.swap(wnodes); g.tris.swap(dtris); g.tri_frames.swap(frames);
    g.sd.nodes = (const float4 *) g.nodes.get(); g.sd.tris = (const float4 *) g.tris.get(); g.sd.tri_frames = g.tri_frames.get();
    g.sd.qnodes = (const uint4 *) g.qnodes.get(); g.sd.wnodes = (const uint4 *) g.wnodes.get(); g.sd.wide_depth = hs.wide_depth;
    for(int a = 0; a < 3; ++a){ g.sd.qorigin[a] = hs.qorigin[a]; g.sd.qscale[a] = hs.qscale[a]; }
    g.sd.num_nodes = (int) hs.qnodes.size();
    g.stack_levels = hs.bvh_depth > 0 ? hs.bvh_depth : 1;
    s->tm.stats.bvh_nodes = (uint32_t) hs.nodes.size(); s->tm.stats.bvh_depth = (uint32_t) hs.bvh_depth;
    s->tm.stats.ms_bvh_build = hs.ms_bvh_build;
    // the next refit uploads the new wide map and re-reserves its scratch for the new node count
    u.level_begin = hs.level_begin; u.wide_src = hs.wide_src; u.num_wide = (uint32_t) hs.wnodes.size(); u.ready = false;
    ri.rebuilds += 1; ri.nodes_after = s->tm.stats.bvh_nodes; ri.depth_after = s->tm.stats.bvh_depth;
    ri.ms_download = ms_download; ri.ms_build = ms_build; ri.ms_upload = ms_upload;
    return HPT_OK;
}

int hpt_scene_get_rebuild_info(const hpt_scene *s, hpt_rebuild_info *out){
    if(!s || !out) return fail(HPT_ERR_INVALID, "null argument");
    *out = s->rb.info;
    return HPT_OK;
}

} // extern "C"
