// Device builds (include/hpt.h): a live handle's tree rebuilt on the device from the vertices the device holds, to the bytes
// of lbvh_host_scene (scene_build.cpp), which is the definition.  The kernels of lbvh_kernels.hip produce the topology -- keys,
// the sort, the radix tree, the breadth-first numbers, the four-wide collapse -- and the refit launches (scene_update.cpp,
// refit_tree_boxes) everything that is a function of the vertex positions.  The host's share is the level loops (4 bytes read
// back per level, capped by a constant, never by a device condition), the limits, the guard and the swap.
// A bounded build (hpt_scene_rebuild_device_bounded, to the bytes of lbvh_bounded_host_scene) runs the same stages around another
// topology step: no radix tree, but a level loop whose lanes split their node's range (forced or Karras' split), capped by max_depth.
// Compiled with hipcc (host code only).
#include "hpt_host.h"

#include <cstdio>

using namespace hpt;

static_assert(sizeof(hpt_device_build_info) == 64, "ABI record: keep path_tracing_amd/__init__.py in step");
static_assert(sizeof(hpt_bounded_build_info) == 16, "ABI record: keep path_tracing_amd/__init__.py in step");
static_assert(kMaxLeafTris == 2, "lbvh_kernels.hip builds leaves of two triangles (kLeafTris)");

namespace {

bool wide_fits(int wide_depth){ SceneDev sd{}; sd.wide_depth = wide_depth; return resume_walk_fits(sd); }

// nothing is swapped: the host path of hpt_scene_rebuild instead, its code returned
int fall_back(hpt_scene *s){
    hpt_device_build_info &di = s->rb.dinfo;
    const uint32_t nodes_before = s->tm.stats.bvh_nodes, depth_before = s->tm.stats.bvh_depth;
    if(int rc = hpt_scene_rebuild(s)) return rc;
    di.builds += 1; di.fell_back = 1;
    di.nodes_before = nodes_before; di.depth_before = depth_before;
    di.nodes_after = s->tm.stats.bvh_nodes; di.depth_after = s->tm.stats.bvh_depth; di.wide_depth = (uint32_t) s->geo.sd.wide_depth;
    di.ms_sort = di.ms_topology = di.ms_refit = di.ms_collapse = 0.0;
    return HPT_OK;
}

// Both device builds.  max_depth == 0: hpt_scene_rebuild_device, the radix tree, which falls back beyond kMaxBvhDepth levels;
// else a bounded build of at most max_depth levels (checked by the caller).
int build_on_device(hpt_scene *s, int max_depth){
    const bool bounded = max_depth > 0;
    hpt_scene::Geometry &g = s->geo;
    hpt_scene::Update &u = s->up;
    hpt_scene::Rebuild &rb = s->rb;
    const int nt = g.nt;
    const uint32_t n = (uint32_t) nt, num_rounds = (uint32_t) g.sd.num_rounds;
    const uint32_t max_nodes = std::max<uint32_t>(n, 1u);     // an inner node has two non-empty subtrees: fewer than nt of them

    // a scene that was never updated: its device vertices, as the first update makes them; the refit's scratch
    if(int rc = ensure_previous(s)) return rc;
    if(int rc = ensure_scratch(s)) return rc;
    for(hipEvent_t &e : rb.ev) if(!e) HIP_TRY(hipEventCreate(&e));

    // fresh buffers and the builder's scratch; the handle is touched only when all of them are filled
    DevBuf<BvhNode> nodes; DevBuf<QBvhNode> qnodes; DevBuf<WideNode> wnodes; DevBuf<DevTriangle> dtris; DevBuf<float4> frames; DevBuf<uint4> wide_src;
    DevBuf<unsigned long long> keys, keys_sorted; DevBuf<uint32_t> idx, idx_sorted, rank, from, cnt, block_sum, total; DevBuf<uint2> child;
    DevBuf<uint4> kid_code; DevBuf<float> exact; DevBuf<unsigned char> sort_tmp; DevBuf<uint32_t> forced;
    const size_t sort_bytes = std::max<size_t>(lbvh_sort_tmp_bytes(n), 1);
    hipError_t e = reserve_all(max_nodes, nodes, qnodes, wnodes, wide_src, kid_code, cnt, child);
    if(e == hipSuccess) e = reserve_all(max_nodes, dtris, keys, keys_sorted, idx, idx_sorted, rank);
    if(e == hipSuccess) e = frames.reserve((size_t) max_nodes * 4);
    if(e == hipSuccess) e = from.reserve((size_t) max_nodes + 1);
    if(e == hipSuccess) e = exact.reserve((size_t) max_nodes * 6);
    if(e == hipSuccess) e = block_sum.reserve(lbvh_blocks(max_nodes) + 1u);
    if(e == hipSuccess) e = total.reserve(1);
    if(e == hipSuccess && bounded) e = forced.reserve((size_t) kMaxBvhDepth);
    if(e == hipSuccess) e = sort_tmp.reserve(sort_bytes);
    if(e == hipSuccess) e = rb.cost.reserve(kCostResultWords);
    if(e != hipSuccess) return fail_hip("device build: buffers", e);
    float4 *d_nodes = (float4 *) nodes.get(), *d_tris = (float4 *) dtris.get();

    // ---- keys and the sort: a refit pass over the identity order leaves slot_box[i] the box of input triangle i and the live box
    HIP_TRY(hipEventRecord(rb.ev[0], nullptr));
    launch_lbvh_identity(nullptr, d_tris, idx.get(), n, num_rounds);
    HIP_TRY(hipMemsetAsync(u.result.get(), 0, 8 * sizeof(float), nullptr));
    launch_refit_tris(nullptr, u.verts.get(), d_tris, n, num_rounds, u.slot_box.get(), u.partial.get(), (uint32_t *) (u.result.get() + 6));
    launch_refit_reduce(nullptr, u.partial.get(), nt ? refit_blocks(n) : 0u, u.result.get());
    HIP_TRY(hipGetLastError());
    float res[8];
    HIP_TRY(hipMemcpy(res, u.result.get(), sizeof res, hipMemcpyDeviceToHost));
    LbvhCells cells;
    for(int a = 0; a < 3; ++a){
        cells.lo[a] = res[a];
        const float ext = res[3 + a] - res[a];
        cells.scale[a] = ext > 0.0f ? 2097152.0f / ext : 0.0f;
    }
    launch_lbvh_keys(nullptr, u.slot_box.get(), n, cells, keys.get());
    if(launch_lbvh_sort(nullptr, sort_tmp.get(), sort_bytes, keys.get(), keys_sorted.get(), idx.get(), idx_sorted.get(), n) != 0)
        return fail(HPT_ERR_DEVICE, "device build: the sort failed");
    HIP_TRY(hipGetLastError());

    // ---- topology: slots, the radix tree, breadth-first numbers
    HIP_TRY(hipEventRecord(rb.ev[1], nullptr));
    launch_lbvh_rank(nullptr, idx_sorted.get(), n, rank.get());
    launch_lbvh_permute(nullptr, (const float4 *) g.tris.get(), rank.get(), n, num_rounds, d_tris);
    std::vector<uint32_t> level_begin;
    uint32_t num_nodes = 1;
    hpt_bounded_build_info bb{ (uint32_t) max_depth, 0u, 0xFFFFFFFFu, 0u };
    if(nt <= kMaxLeafTris){
        BvhNode root; memset(&root, 0, sizeof root);
        for(int a = 0; a < 3; ++a){ root.lmin[a] = root.rmin[a] = INFINITY; root.lmax[a] = root.rmax[a] = -INFINITY; }
        root.left = nt > 0 ? (kLeafFlag | (uint32_t) (nt - 1)) : kEmptyChild;
        root.right = kEmptyChild;
        HIP_TRY(hipMemcpy(nodes.get(), &root, sizeof root, hipMemcpyHostToDevice));
        level_begin = { 0u, 1u };
    } else if(bounded){
        // a node is its range of sorted positions, at its breadth-first number: `child` holds the ranges, `rank` (free again
        // after the permutation) the splits; the forced nodes are counted per level
        uint2 *range = child.get();
        const uint2 whole = make_uint2(0u, n);
        HIP_TRY(hipMemcpyAsync(range, &whole, sizeof whole, hipMemcpyHostToDevice, nullptr));
        HIP_TRY(hipMemsetAsync(forced.get(), 0, (size_t) kMaxBvhDepth * sizeof(uint32_t), nullptr));
        uint32_t first = 0, count = 1;
        bool done = false;
        for(int level = 0; level < max_depth && !done; ++level){
            level_begin.push_back(first);
            uint32_t next = 0;
            launch_lbvh_bounded_count(nullptr, keys_sorted.get(), n, range, first, count, max_nodes, max_depth - level, rank.get(), cnt.get(),
                                      block_sum.get(), forced.get() + level);
            launch_lbvh_scan(nullptr, block_sum.get(), lbvh_blocks(count), total.get());
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipMemcpy(&next, total.get(), sizeof next, hipMemcpyDeviceToHost));
            if((uint64_t) first + count + next > max_nodes) return fail(HPT_ERR_DEVICE, "device build: internal error: more nodes than triangles");
            launch_lbvh_bounded_scatter(nullptr, range, rank.get(), n, first, count, cnt.get(), block_sum.get(), d_nodes, max_nodes);
            first += count; count = next;
            done = count == 0;
        }
        HIP_TRY(hipGetLastError());
        if(!done){ HIP_TRY(hipDeviceSynchronize()); return fail(HPT_ERR_DEVICE, "device build: internal error: inner nodes below max_depth; the handle is as it was"); }
        level_begin.push_back(first);
        num_nodes = first;
        uint32_t per_level[kMaxBvhDepth];
        HIP_TRY(hipMemcpy(per_level, forced.get(), sizeof per_level, hipMemcpyDeviceToHost));
        for(int level = 0; level < kMaxBvhDepth; ++level){
            if(per_level[level] && bb.first_forced_level == 0xFFFFFFFFu) bb.first_forced_level = (uint32_t) level;
            bb.forced_nodes += per_level[level];
        }
    } else {
        const uint32_t num_inner = n - 1u;
        launch_lbvh_radix(nullptr, keys_sorted.get(), n, child.get());
        HIP_TRY(hipMemsetAsync(from.get(), 0, sizeof(uint32_t), nullptr));       // the root is radix node 0
        uint32_t first = 0, count = 1;
        bool done = false;
        for(int level = 0; level < kMaxBvhDepth && !done; ++level){
            level_begin.push_back(first);
            uint32_t next = 0;
            launch_lbvh_level_count(nullptr, child.get(), num_inner, from.get(), first, count, cnt.get(), block_sum.get());
            launch_lbvh_scan(nullptr, block_sum.get(), lbvh_blocks(count), total.get());
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipMemcpy(&next, total.get(), sizeof next, hipMemcpyDeviceToHost));
            if((uint64_t) first + count + next > max_nodes) return fail(HPT_ERR_DEVICE, "device build: internal error: more nodes than triangles");
            launch_lbvh_level_scatter(nullptr, child.get(), num_inner, from.get(), first, count, cnt.get(), block_sum.get(), d_nodes, max_nodes);
            first += count; count = next;
            done = count == 0;
        }
        HIP_TRY(hipGetLastError());
        if(!done){ HIP_TRY(hipDeviceSynchronize()); return fall_back(s); }        // more than kMaxBvhDepth levels: nodes still inner at the cap
        level_begin.push_back(first);
        num_nodes = first;
    }
    const int bvh_depth = nt > 0 ? (int) level_begin.size() - 1 : 0;

    // ---- everything that is a function of the vertex positions: the refit's own launches on the new topology
    HIP_TRY(hipEventRecord(rb.ev[2], nullptr));
    RefitGrid grid; uint32_t ndead = 0;
    const RefitTree tree{ d_nodes, (uint4 *) qnodes.get(), d_tris, exact.get(), num_nodes, &level_begin };
    if(int rc = refit_tree_boxes(s, tree, grid, ndead)) return rc;

    // ---- the four-wide twin: the collapse over the boxes just written, level by level
    HIP_TRY(hipEventRecord(rb.ev[3], nullptr));
    uint32_t *todo = from.get();
    HIP_TRY(hipMemsetAsync(todo, 0, sizeof(uint32_t), nullptr));                 // wide node 0 is collapsed from binary node 0
    uint32_t num_wide = 0; int wide_depth = 0;
    {   uint32_t first = 0, count = 1;
        for(int level = 0; level <= kMaxBvhDepth && count > 0; ++level){         // a wide level spans a binary level at least
            uint32_t next = 0;
            launch_lbvh_wide_collapse(nullptr, d_nodes, num_nodes, todo, first, count, kid_code.get(), wide_src.get(), cnt.get(), block_sum.get());
            launch_lbvh_scan(nullptr, block_sum.get(), lbvh_blocks(count), total.get());
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipMemcpy(&next, total.get(), sizeof next, hipMemcpyDeviceToHost));
            if((uint64_t) first + count + next > max_nodes) return fail(HPT_ERR_DEVICE, "device build: internal error: more wide nodes than binary ones");
            launch_lbvh_wide_scatter(nullptr, kid_code.get(), todo, first, count, cnt.get(), block_sum.get(), (uint4 *) wnodes.get(), max_nodes);
            first += count; count = next;
            ++wide_depth;
        }
        if(count > 0) return fail(HPT_ERR_DEVICE, "device build: internal error: the four-wide tree is deeper than the binary one");
        num_wide = first;
    }
    launch_refit_wide(nullptr, d_nodes, num_nodes, (uint4 *) wnodes.get(), wide_src.get(), num_wide, grid);
    launch_tri_frames(nullptr, d_tris, nt, frames.get());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(rb.ev[4], nullptr));
    HIP_TRY(hipDeviceSynchronize());
    if(!wide_fits(wide_depth)){
        if(int rc = fall_back(s)) return rc;
        if(bounded) rb.binfo = bb;
        return HPT_OK;
    }

    // ---- the guard: the new tree measured where it lies; a malformed one never reaches a trace kernel
    HIP_TRY(hipMemsetAsync(rb.cost.get(), 0, kCostResultWords * sizeof(unsigned long long), nullptr));
    launch_tree_cost(nullptr, (const uint4 *) qnodes.get(), num_nodes, rb.cost.get());
    HIP_TRY(hipGetLastError());
    unsigned long long cost[kCostResultWords];
    HIP_TRY(hipMemcpy(cost, rb.cost.get(), sizeof cost, hipMemcpyDeviceToHost));
    if(cost[3] != (unsigned long long) nt || cost[0] + 1ull != (unsigned long long) num_nodes){
        char msg[200];
        snprintf(msg, sizeof msg, "device build: the new tree is malformed (%llu leaf slots for %d triangles, %llu inner children for %u nodes); the handle is as it was",
                 cost[3], nt, cost[0], num_nodes);
        return fail(HPT_ERR_DEVICE, msg);
    }
    float ms[4] = { 0, 0, 0, 0 };
    for(int k = 0; k < 4; ++k) HIP_TRY(hipEventElapsedTime(&ms[k], rb.ev[k], rb.ev[k + 1]));

    // ---- the swap
    hpt_device_build_info &di = rb.dinfo;
    di.nodes_before = s->tm.stats.bvh_nodes; di.depth_before = s->tm.stats.bvh_depth;
    g.nodes.swap(nodes); g.qnodes.swap(qnodes); g.wnodes.swap(wnodes); g.tris.swap(dtris); g.tri_frames.swap(frames);
    g.sd.nodes = (const float4 *) g.nodes.get(); g.sd.tris = (const float4 *) g.tris.get(); g.sd.tri_frames = g.tri_frames.get();
    g.sd.qnodes = (const uint4 *) g.qnodes.get(); g.sd.wnodes = (const uint4 *) g.wnodes.get(); g.sd.wide_depth = wide_depth;
    for(int a = 0; a < 3; ++a){ g.sd.qorigin[a] = grid.qorigin[a]; g.sd.qscale[a] = grid.qscale[a]; }
    g.sd.num_nodes = (int) num_nodes;
    g.stack_levels = bvh_depth > 0 ? bvh_depth : 1;
    s->tm.stats.bvh_nodes = num_nodes; s->tm.stats.bvh_depth = (uint32_t) bvh_depth;
    s->tm.stats.ms_bvh_build = (double) ms[0] + (double) ms[1] + (double) ms[2] + (double) ms[3];
    // one set of refit tables: the levels on the host, the wide map where the collapse wrote it -- no stale copy to upload
    u.level_begin = level_begin; u.d_wide_src.swap(wide_src); u.num_wide = num_wide; u.wide_src.clear(); u.ready = true;
    di.builds += 1; di.fell_back = 0;
    di.nodes_after = num_nodes; di.depth_after = (uint32_t) bvh_depth; di.wide_depth = (uint32_t) wide_depth;
    di.ms_sort = ms[0]; di.ms_topology = ms[1]; di.ms_refit = ms[2]; di.ms_collapse = ms[3];
    if(bounded) rb.binfo = bb;
    return HPT_OK;
}

} // namespace

extern "C" {

int hpt_scene_rebuild_device(hpt_scene *s){
    if(!s) return fail(HPT_ERR_INVALID, "null scene");
    if(int rc = on_scene_device(s)) return rc;
    return build_on_device(s, 0);
}

int hpt_scene_rebuild_device_bounded(hpt_scene *s, int max_depth){
    if(!s) return fail(HPT_ERR_INVALID, "null scene");
    char msg[160]; int D = 0;
    if(const char *e = lbvh_check_depth(s->geo.nt, max_depth, D, msg, sizeof msg); *e) return fail(HPT_ERR_INVALID, e);
    if(int rc = on_scene_device(s)) return rc;
    return build_on_device(s, D);
}

int hpt_scene_get_bounded_build_info(const hpt_scene *s, hpt_bounded_build_info *out){
    if(!s || !out) return fail(HPT_ERR_INVALID, "null argument");
    *out = s->rb.binfo;
    return HPT_OK;
}

int hpt_scene_get_device_build_info(const hpt_scene *s, hpt_device_build_info *out){
    if(!s || !out) return fail(HPT_ERR_INVALID, "null argument");
    *out = s->rb.dinfo;
    return HPT_OK;
}

int hpt_bvh_device_build_host(const void *lights, int nl, const void *spheres, int ns, const void *tris, const void *new_tris, int nt,
                              hpt_bvh_info *info, hpt_device_build_info *binfo, void *qnodes_out, size_t qnodes_cap, void *tris_out, size_t tris_cap){
    if(!info) return fail(HPT_ERR_INVALID, "null info");
    HostScene hs;
    const char *err = lbvh_host_scene(lights, nl, spheres, ns, tris, nt, hs);
    if(err && *err) return fail(HPT_ERR_INVALID, err);
    if(new_tris){
        char msg[200];
        err = check_triangle_update(tris, nt, new_tris, nt, msg, sizeof msg);
        if(err && *err) return fail(HPT_ERR_INVALID, err);
        err = refit_host_scene(hs, new_tris, nt);
        if(err && *err) return fail(HPT_ERR_INVALID, err);
    }
    if(binfo){
        memset(binfo, 0, sizeof *binfo);
        binfo->builds = 1;
        binfo->fell_back = (hs.bvh_depth > kMaxBvhDepth || !wide_fits(hs.wide_depth)) ? 1u : 0u;
        binfo->nodes_after = (uint32_t) hs.nodes.size(); binfo->depth_after = (uint32_t) hs.bvh_depth; binfo->wide_depth = (uint32_t) hs.wide_depth;
    }
    return export_host_tree(hs, info, qnodes_out, qnodes_cap, tris_out, tris_cap);
}

int hpt_bvh_device_build_bounded_host(const void *lights, int nl, const void *spheres, int ns, const void *tris, const void *new_tris, int nt,
                                      hpt_bvh_info *info, hpt_device_build_info *binfo, void *qnodes_out, size_t qnodes_cap, void *tris_out, size_t tris_cap,
                                      int max_depth, hpt_bounded_build_info *bbinfo){
    if(!info) return fail(HPT_ERR_INVALID, "null info");
    HostScene hs; BoundedInfo bi;
    const char *err = lbvh_bounded_host_scene(lights, nl, spheres, ns, tris, nt, max_depth, hs, bi);
    if(err && *err) return fail(HPT_ERR_INVALID, err);
    if(new_tris){
        char msg[200];
        err = check_triangle_update(tris, nt, new_tris, nt, msg, sizeof msg);
        if(err && *err) return fail(HPT_ERR_INVALID, err);
        err = refit_host_scene(hs, new_tris, nt);
        if(err && *err) return fail(HPT_ERR_INVALID, err);
    }
    if(binfo){
        memset(binfo, 0, sizeof *binfo);
        binfo->builds = 1;
        binfo->fell_back = wide_fits(hs.wide_depth) ? 0u : 1u;
        binfo->nodes_after = (uint32_t) hs.nodes.size(); binfo->depth_after = (uint32_t) hs.bvh_depth; binfo->wide_depth = (uint32_t) hs.wide_depth;
    }
    if(bbinfo) *bbinfo = hpt_bounded_build_info{ bi.max_depth, bi.forced_nodes, bi.first_forced_level, 0u };
    return export_host_tree(hs, info, qnodes_out, qnodes_cap, tris_out, tris_cap);
}

} // extern "C"
