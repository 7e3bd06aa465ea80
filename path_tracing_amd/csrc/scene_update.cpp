// Scene updates (include/hpt.h): a live scene's triangles, spheres and lights moved in place.  The triangles' tree is
// refitted on the device (refit_kernels.hip) to the bytes of refit_host_scene (scene_build.cpp), which is the definition;
// the host's share here is the refusals, packing and uploading the vertices, and the few builder lines that sit between
// the launches (pad_abs and the dead point from the scene box, the grid from node 0).  Poses (include/hpt.h, "poses") are two
// more feeds into the same refit: vertices that are on the device already, and one 3 x 4 record per part applied to a rest
// pose by k_pose_verts, to the bytes of pose_vertex_host (scene_build.cpp).  A skin (include/hpt.h, "skinning") is a third:
// four weighted bones per corner blended over the same rest pose by k_skin_verts, to the bytes of skin_vertex_host.  Morph
// targets (include/hpt.h, "morph targets") are a fourth, and the only one that composes: k_morph_verts sums weighted deltas
// over the rest pose to the bytes of morph_vertex_host, and where the scene has parts or a skin as well the deformer then
// runs over that morphed rest pose with the table it was last given.
// Compiled with hipcc (host code only).
#include "hpt_host.h"

#include <chrono>
#include <cmath>
#include <cstdio>

using namespace hpt;

namespace {

double ms_since(std::chrono::steady_clock::time_point t0){
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

// the refusals of hpt_scene_update_triangles, in the header's order
int check_triangles(const hpt_scene *s, const void *tris, int nt){
    if(!s) return fail(HPT_ERR_INVALID, "null scene");
    char msg[200];
    const char *err = check_triangle_update(s->geo.h_tris.data(), s->geo.nt, tris, nt, msg, sizeof msg);
    if(err && *err) return fail(HPT_ERR_INVALID, err);
    return on_scene_device(s);
}

} // namespace

// scratch of the refit, and the build's wide-node map on the device: allocated by the first update and kept
int hpt::ensure_scratch(hpt_scene *s){
    hpt_scene::Update &u = s->up;
    const size_t nt = (size_t) s->geo.nt, nn = (size_t) s->geo.sd.num_nodes;
    HIP_TRY(u.verts.reserve(std::max<size_t>(nt * 9, 1)));
    HIP_TRY(u.slot_box.reserve(std::max<size_t>(nt * 6, 1)));
    HIP_TRY(u.exact.reserve(std::max<size_t>(nn * 6, 1)));
    HIP_TRY(u.partial.reserve(std::max<size_t>((size_t) refit_blocks((uint32_t) nt) * 6, 6)));
    HIP_TRY(u.result.reserve(8));
    if(!u.ev_a) HIP_TRY(hipEventCreate(&u.ev_a));
    if(!u.ev_b) HIP_TRY(hipEventCreate(&u.ev_b));
    if(!u.ready){
        if(u.wide_src.size() != (size_t) u.num_wide * 4 || u.level_begin.size() < 2 || u.level_begin.back() != (uint32_t) nn)
            return fail(HPT_ERR_INVALID, "internal error: the scene keeps no refit tables");
        HIP_TRY(u.d_wide_src.reserve(std::max<size_t>(u.num_wide, 1)));
        if(u.num_wide) HIP_TRY(hipMemcpy(u.d_wide_src.get(), u.wide_src.data(), (size_t) u.num_wide * 16, hipMemcpyHostToDevice));
        u.ready = true;
    }
    return HPT_OK;
}

namespace {
// centre | radius of every sphere record
std::vector<float4> pack_spheres(const std::vector<unsigned char> &h_spheres, int ns){
    std::vector<float4> r((size_t) ns);
    for(size_t i = 0; i < (size_t) ns; ++i) memcpy(&r[i], h_spheres.data() + i * HPT_SPHERE_BYTES, 16);
    return r;
}

} // namespace

// The previous geometry, before the first update changes the current one: G' = G from the records the scene keeps.  `verts`
// is filled too, so that from here on it holds the current geometry whichever update comes first.
int hpt::ensure_previous(hpt_scene *s){
    hpt_scene::Update &u = s->up;
    if(u.prev_ready) return HPT_OK;
    const hpt_scene::Geometry &g = s->geo;
    const size_t nt = (size_t) g.nt, ns = (size_t) g.ns;
    std::vector<float> v(nt * 9);
    for(size_t i = 0; i < nt; ++i) memcpy(v.data() + i * 9, g.h_tris.data() + i * HPT_TRIANGLE_BYTES, 36);
    HIP_TRY(u.verts.reserve(std::max<size_t>(nt * 9, 1)));
    HIP_TRY(u.prev_verts.reserve(std::max<size_t>(nt * 9, 1)));
    HIP_TRY(u.prev_rounds.reserve(std::max<size_t>(ns, 1)));
    if(nt){
        HIP_TRY(hipMemcpy(u.verts.get(), v.data(), nt * 36, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(u.prev_verts.get(), v.data(), nt * 36, hipMemcpyHostToDevice));
    }
    if(ns){
        const std::vector<float4> r = pack_spheres(g.h_spheres, g.ns);
        HIP_TRY(hipMemcpy(u.prev_rounds.get(), r.data(), ns * sizeof(float4), hipMemcpyHostToDevice));
    }
    u.prev_ready = true;
    return HPT_OK;
}

int hpt::refit_tree_boxes(hpt_scene *s, const RefitTree &t, RefitGrid &grid, uint32_t &ndead){
    hpt_scene::Update &u = s->up;
    hpt_scene::Geometry &g = s->geo;
    const int nt = g.nt;
    const uint32_t num_nodes = t.num_nodes;
    float4 *nodes = t.nodes;
    const std::vector<uint32_t> &level_begin = *t.level_begin;
    // leaf records, slot boxes, the live triangles' box and the dead count
    HIP_TRY(hipMemsetAsync(u.result.get(), 0, 8 * sizeof(float), nullptr));
    launch_refit_tris(nullptr, u.verts.get(), t.tris, (uint32_t) nt, (uint32_t) g.sd.num_rounds, u.slot_box.get(), u.partial.get(),
                      (uint32_t *) (u.result.get() + 6));
    launch_refit_reduce(nullptr, u.partial.get(), nt ? refit_blocks((uint32_t) nt) : 0u, u.result.get());
    HIP_TRY(hipGetLastError());
    float res[8];
    HIP_TRY(hipMemcpy(res, u.result.get(), sizeof res, hipMemcpyDeviceToHost));
    memcpy(&ndead, &res[6], 4);
    // the dead point and pad_abs, as the builder has them (scene_build.cpp, triangle_boxes and box_padding)
    float mn[3] = { res[0], res[1], res[2] }, mx[3] = { res[3], res[4], res[5] }, at[3] = { 0.0f, 0.0f, 0.0f };
    if(ndead > 0){
        for(int a = 0; a < 3; ++a){
            at[a] = ndead < (uint32_t) nt ? mn[a] : 0.0f;
            mn[a] = std::min(mn[a], at[a]); mx[a] = std::max(mx[a], at[a]);
        }
    }
    const float pad_abs = box_padding_of(mn, mx, nt);
    // node boxes, deepest level first
    for(size_t l = level_begin.size() - 1; l-- > 0; )
        launch_refit_level(nullptr, nodes, num_nodes, level_begin[l], level_begin[l + 1] - level_begin[l], u.slot_box.get(), (uint32_t) nt,
                           t.exact, pad_abs, at[0], at[1], at[2]);
    HIP_TRY(hipGetLastError());
    // the grid is the union of the stored boxes, which is the union of the root's two (padding is monotone)
    BvhNode root;
    HIP_TRY(hipMemcpy(&root, nodes, sizeof root, hipMemcpyDeviceToHost));
    float lo[3] = { INFINITY, INFINITY, INFINITY }, hi[3] = { -INFINITY, -INFINITY, -INFINITY };
    for(int a = 0; a < 3; ++a){
        if(root.left != kEmptyChild){ lo[a] = std::min(lo[a], std::min(root.lmin[a], root.lmax[a])); hi[a] = std::max(hi[a], std::max(root.lmin[a], root.lmax[a])); }
        if(root.right != kEmptyChild){ lo[a] = std::min(lo[a], std::min(root.rmin[a], root.rmax[a])); hi[a] = std::max(hi[a], std::max(root.rmin[a], root.rmax[a])); }
    }
    grid_of_box(lo, hi, grid.qorigin, grid.qscale);
    launch_refit_quantise(nullptr, nodes, t.qnodes, num_nodes, grid);
    return HPT_OK;
}

namespace {

// What an update brings: records from the host (hpt_scene_update_triangles, packed into up.h_verts by the caller), nine floats
// per triangle on the device, one record per part applied to the rest pose, one record per bone blended over it, or one
// weight per morph target.  `kind` says which; a scene of zero triangles brings null arrays.
struct Feed {
    enum Kind { Records, DeviceVerts, Pose, Skin, Morph } kind;
    const void *records = nullptr; const float *d_verts = nullptr; const float *xforms = nullptr; const float *weights = nullptr;
};

// Every call that captures a rest pose ends here: R = the geometry `verts` holds, all morph weights at zero -- so M, which is
// held only where the scene has morphs and a deformer (`both`), has R's bits -- and the deformer's table at identity.
int capture_rest(hpt_scene::Update &u, size_t nt, bool both){
    HIP_TRY(u.rest_verts.reserve(std::max<size_t>(nt * 9, 1)));
    if(both) HIP_TRY(u.morph_verts.reserve(std::max<size_t>(nt * 9, 1)));
    if(nt){
        HIP_TRY(hipMemcpy(u.rest_verts.get(), u.verts.get(), nt * 36, hipMemcpyDeviceToDevice));
        if(both) HIP_TRY(hipMemcpy(u.morph_verts.get(), u.verts.get(), nt * 36, hipMemcpyDeviceToDevice));
    }
    u.deformer_identity = true;
    return HPT_OK;
}

// The part every triangle update shares: the feed into `verts`, the refit's launches, and the bookkeeping.  With host records
// it enqueues what hpt_scene_update_triangles always has.
int refit_from(hpt_scene *s, const Feed &f, double ms_pack){
    hpt_scene::Update &u = s->up;
    hpt_scene::Geometry &g = s->geo;
    const int nt = g.nt;
    const bool pose = f.kind == Feed::Pose || f.kind == Feed::Skin || f.kind == Feed::Morph;      // applied to the rest pose, which it leaves
    const bool deformer = u.num_parts || u.num_bones;
    const int num_records = f.kind == Feed::Skin ? u.num_bones : u.num_parts;

    auto t0 = std::chrono::steady_clock::now();
    if(int rc = ensure_scratch(s)) return rc;
    if(f.kind == Feed::Records){
        if(nt) HIP_TRY(hipMemcpy(u.verts.get(), u.h_verts.data(), (size_t) nt * 36, hipMemcpyHostToDevice));
    } else if(f.kind == Feed::DeviceVerts){
        if(nt) HIP_TRY(hipMemcpy(u.verts.get(), f.d_verts, (size_t) nt * 36, hipMemcpyDeviceToDevice));
        HIP_TRY(hipStreamSynchronize(nullptr));
    } else if(f.kind == Feed::Morph){
        HIP_TRY(hipMemcpy(u.morph_weights.get(), f.weights, (size_t) u.num_targets * sizeof(float), hipMemcpyHostToDevice));
    } else {
        HIP_TRY(u.xforms.reserve((size_t) num_records * 12));
        HIP_TRY(hipMemcpy(u.xforms.get(), f.xforms, (size_t) num_records * 48, hipMemcpyHostToDevice));
    }
    const double ms_upload = ms_since(t0);

    const uint32_t num_nodes = (uint32_t) g.sd.num_nodes;
    float4 *nodes = (float4 *) g.nodes.get();
    HIP_TRY(hipEventRecord(u.ev_a, nullptr));
    // morph first, then the deformer: with morphs the deformer's rest vertex is M, which a morph has written just before (or
    // some time ago, or a capture has set to R); a morph on a scene whose deformer was never given a table hands M on as it is
    const float *rest = u.num_targets && deformer ? u.morph_verts.get() : u.rest_verts.get();
    bool run_parts = f.kind == Feed::Pose, run_skin = f.kind == Feed::Skin;
    if(f.kind == Feed::Morph){
        launch_morph_verts(nullptr, u.rest_verts.get(), u.morph_begin.get(), u.morph_entries.get(), u.morph_weights.get(), (uint32_t) u.num_targets,
                           (uint32_t) nt, deformer ? u.morph_verts.get() : u.verts.get());
        if(deformer && u.deformer_identity){
            if(nt) HIP_TRY(hipMemcpyAsync(u.verts.get(), u.morph_verts.get(), (size_t) nt * 36, hipMemcpyDeviceToDevice, nullptr));
        } else { run_parts = u.num_parts != 0; run_skin = u.num_bones != 0; }
    }
    if(run_parts) launch_pose_verts(nullptr, rest, u.tri_part.get(), u.xforms.get(), (uint32_t) u.num_parts, (uint32_t) nt, u.verts.get());
    if(run_skin) launch_skin_verts(nullptr, rest, u.skin_bone.get(), u.skin_weight.get(), u.xforms.get(), (uint32_t) u.num_bones, (uint32_t) nt, u.verts.get());
    RefitGrid grid; uint32_t ndead = 0;
    const RefitTree tree{ nodes, (uint4 *) g.qnodes.get(), (float4 *) g.tris.get(), u.exact.get(), num_nodes, &u.level_begin };
    if(int rc = refit_tree_boxes(s, tree, grid, ndead)) return rc;
    for(int a = 0; a < 3; ++a){ g.sd.qorigin[a] = grid.qorigin[a]; g.sd.qscale[a] = grid.qscale[a]; }
    launch_refit_wide(nullptr, nodes, num_nodes, (uint4 *) g.wnodes.get(), u.d_wide_src.get(), u.num_wide, grid);
    launch_tri_frames(nullptr, (const float4 *) g.tris.get(), nt, g.tri_frames.get());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(u.ev_b, nullptr));
    HIP_TRY(hipDeviceSynchronize());
    float ms_refit = 0.0f;
    HIP_TRY(hipEventElapsedTime(&ms_refit, u.ev_a, u.ev_b));

    // the rest-pose rule: an update that is not a pose, a skin or a morph leaves the rest pose, every part or bone at identity
    // and every morph weight at zero
    if(!pose && (deformer || u.num_targets)){
        if(int rc = capture_rest(u, (size_t) nt, deformer && u.num_targets)) return rc;
        HIP_TRY(hipDeviceSynchronize());
    }
    if(f.kind == Feed::Pose || f.kind == Feed::Skin) u.deformer_identity = false;
    if(f.kind == Feed::Records){
        if(nt) g.h_tris.assign((const unsigned char *) f.records, (const unsigned char *) f.records + (size_t) nt * HPT_TRIANGLE_BYTES);
        u.h_tris_stale = false;
    } else u.h_tris_stale = nt > 0;
    s->bd.ready = false; s->pm.bounds_ready = false;
    u.info.updates += 1; u.info.dead_tris = ndead; u.info.live_tris = (uint64_t) nt - ndead;
    u.info.ms_pack = ms_pack; u.info.ms_upload = ms_upload; u.info.ms_refit = ms_refit;
    u.motion = true;
    return HPT_OK;
}

// the refusals the new triangle calls share with the count of check_triangle_update
int check_count(const hpt_scene *s, int nt){
    if(!s) return fail(HPT_ERR_INVALID, "null scene");
    if(nt < 0) return fail(HPT_ERR_INVALID, "negative triangle count");
    if(nt != s->geo.nt){
        char msg[200];
        snprintf(msg, sizeof msg, "an update keeps the triangle count: the scene has %d triangles, %d were handed over", s->geo.nt, nt);
        return fail(HPT_ERR_INVALID, msg);
    }
    return HPT_OK;
}

} // namespace

int hpt::host_triangles(hpt_scene *s, const unsigned char **tris){
    hpt_scene::Update &u = s->up;
    hpt_scene::Geometry &g = s->geo;
    if(u.h_tris_stale){
        const size_t nt = (size_t) g.nt;
        u.h_verts.resize(nt * 9);
        if(nt) HIP_TRY(hipMemcpy(u.h_verts.data(), u.verts.get(), nt * 36, hipMemcpyDeviceToHost));
        for(size_t i = 0; i < nt; ++i) memcpy(g.h_tris.data() + i * HPT_TRIANGLE_BYTES, u.h_verts.data() + i * 9, 36);
        u.h_tris_stale = false;
    }
    *tris = g.h_tris.data();
    return HPT_OK;
}

extern "C" {

int hpt_scene_keep_previous(hpt_scene *s){
    if(!s) return fail(HPT_ERR_INVALID, "null scene");
    if(int rc = on_scene_device(s)) return rc;
    hpt_scene::Update &u = s->up;
    if(u.prev_ready){         // a scene that was never updated holds no G': it is G
        const size_t nt = (size_t) s->geo.nt, ns = (size_t) s->geo.ns;
        if(nt) HIP_TRY(hipMemcpy(u.prev_verts.get(), u.verts.get(), nt * 36, hipMemcpyDeviceToDevice));
        if(ns){
            const std::vector<float4> r = pack_spheres(s->geo.h_spheres, s->geo.ns);
            HIP_TRY(hipMemcpy(u.prev_rounds.get(), r.data(), ns * sizeof(float4), hipMemcpyHostToDevice));
        }
        HIP_TRY(hipDeviceSynchronize());
    }
    u.motion = false;
    return HPT_OK;
}

int hpt_scene_has_motion(const hpt_scene *s){
    if(!s){ fail(HPT_ERR_INVALID, "null scene"); return -1; }
    return s->up.motion ? 1 : 0;
}

int hpt_scene_update_check(const hpt_scene *s, const void *tris, int nt){ return check_triangles(s, tris, nt); }

int hpt_scene_update_triangles(hpt_scene *s, const void *tris, int nt){
    if(int rc = check_triangles(s, tris, nt)) return rc;
    hpt_scene::Update &u = s->up;
    if(int rc = ensure_previous(s)) return rc;

    // the nine floats of every triangle, input order
    auto t0 = std::chrono::steady_clock::now();
    u.h_verts.resize((size_t) nt * 9);
    for(size_t i = 0; i < (size_t) nt; ++i) memcpy(u.h_verts.data() + i * 9, (const unsigned char *) tris + i * HPT_TRIANGLE_BYTES, 36);
    const double ms_pack = ms_since(t0);

    Feed f{Feed::Records}; f.records = tris;
    return refit_from(s, f, ms_pack);
}

int hpt_scene_update_vertices_device(hpt_scene *s, const void *d_verts, int nt){
    if(int rc = check_count(s, nt)) return rc;
    if(nt > 0 && !d_verts) return fail(HPT_ERR_INVALID, "null vertex array");
    if(int rc = on_scene_device(s)) return rc;
    if(int rc = ensure_previous(s)) return rc;
    Feed f{Feed::DeviceVerts}; f.d_verts = (const float *) d_verts;
    return refit_from(s, f, 0.0);
}

int hpt_scene_set_parts(hpt_scene *s, const int32_t *tri_part, int nt, int num_parts){
    if(int rc = check_count(s, nt)) return rc;
    char msg[200];
    const char *err = check_parts(tri_part, nt, num_parts, msg, sizeof msg);
    if(err && *err) return fail(HPT_ERR_INVALID, err);
    if(int rc = on_scene_device(s)) return rc;
    if(int rc = ensure_previous(s)) return rc;          // `verts` holds the current geometry from here on
    hpt_scene::Update &u = s->up;
    const size_t n = (size_t) nt;
    u.num_parts = 0;                                     // (a failed allocation leaves the scene without parts)
    u.num_bones = 0; u.skin_bone.release(); u.skin_weight.release();      // one deformer per scene: the skin goes
    if(int rc = capture_rest(u, n, u.num_targets != 0)) return rc;
    HIP_TRY(u.tri_part.reserve(std::max<size_t>(n, 1)));
    if(n){
        if(tri_part) HIP_TRY(hipMemcpy(u.tri_part.get(), tri_part, n * sizeof(int32_t), hipMemcpyHostToDevice));
        else HIP_TRY(hipMemset(u.tri_part.get(), 0, n * sizeof(int32_t)));
    }
    HIP_TRY(hipDeviceSynchronize());
    u.num_parts = num_parts;
    return HPT_OK;
}

int hpt_scene_pose(hpt_scene *s, const float *xforms, int num_parts){
    if(!s) return fail(HPT_ERR_INVALID, "null scene");
    if(s->up.num_parts == 0) return fail(HPT_ERR_INVALID, "hpt_scene_pose before hpt_scene_set_parts: the scene has no parts");
    if(num_parts != s->up.num_parts){
        char msg[200];
        snprintf(msg, sizeof msg, "a pose keeps the number of parts: the scene has %d parts, %d records were handed over", s->up.num_parts, num_parts);
        return fail(HPT_ERR_INVALID, msg);
    }
    if(!xforms) return fail(HPT_ERR_INVALID, "null transform array");
    if(int rc = on_scene_device(s)) return rc;
    Feed f{Feed::Pose}; f.xforms = xforms;
    return refit_from(s, f, 0.0);
}

int hpt_scene_set_skin(hpt_scene *s, const int32_t *corner_bone, const float *corner_weight, int nt, int num_bones){
    if(int rc = check_count(s, nt)) return rc;
    char msg[200];
    const char *err = check_skin(corner_bone, corner_weight, nt, num_bones, msg, sizeof msg);
    if(err && *err) return fail(HPT_ERR_INVALID, err);
    if(int rc = on_scene_device(s)) return rc;
    if(int rc = ensure_previous(s)) return rc;          // `verts` holds the current geometry from here on
    hpt_scene::Update &u = s->up;
    const size_t n = (size_t) nt, corners = n * 3;
    std::vector<uint16_t> bones(corners * kSkinInfluences);                  // 16 bits per index: check_skin has bounded them
    for(size_t i = 0; i < bones.size(); ++i) bones[i] = (uint16_t) corner_bone[i];
    u.num_bones = 0;                                     // (a failed allocation leaves the scene without a skin)
    u.num_parts = 0; u.tri_part.release();               // one deformer per scene: the parts go
    if(int rc = capture_rest(u, n, u.num_targets != 0)) return rc;
    HIP_TRY(u.skin_bone.reserve(std::max<size_t>(corners, 1)));
    HIP_TRY(u.skin_weight.reserve(std::max<size_t>(corners, 1)));
    if(n){
        HIP_TRY(hipMemcpy(u.skin_bone.get(), bones.data(), corners * sizeof(uint2), hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(u.skin_weight.get(), corner_weight, corners * sizeof(float4), hipMemcpyHostToDevice));
    }
    HIP_TRY(hipDeviceSynchronize());
    u.num_bones = num_bones;
    return HPT_OK;
}

int hpt_scene_skin(hpt_scene *s, const float *xforms, int num_bones){
    if(!s) return fail(HPT_ERR_INVALID, "null scene");
    if(s->up.num_bones == 0) return fail(HPT_ERR_INVALID, "hpt_scene_skin before hpt_scene_set_skin: the scene has no skin");
    if(num_bones != s->up.num_bones){
        char msg[200];
        snprintf(msg, sizeof msg, "a skin keeps the number of bones: the scene has %d bones, %d records were handed over", s->up.num_bones, num_bones);
        return fail(HPT_ERR_INVALID, msg);
    }
    if(!xforms) return fail(HPT_ERR_INVALID, "null transform array");
    if(int rc = on_scene_device(s)) return rc;
    Feed f{Feed::Skin}; f.xforms = xforms;
    return refit_from(s, f, 0.0);
}

int hpt_skin_host(const void *tris, int nt, const int32_t *corner_bone, const float *corner_weight, const float *xforms, int num_bones,
                  void *out){
    char msg[200];
    const char *err = skin_host_records(tris, nt, corner_bone, corner_weight, xforms, num_bones, out, msg, sizeof msg);
    if(err && *err) return fail(HPT_ERR_INVALID, err);
    return HPT_OK;
}

int hpt_scene_set_morphs(hpt_scene *s, const int32_t *target_begin, const int32_t *entry_corner, const float *entry_delta, int num_entries,
                         int nt, int num_targets){
    if(int rc = check_count(s, nt)) return rc;
    char msg[200];
    const char *err = check_morphs(target_begin, entry_corner, entry_delta, num_entries, nt, num_targets, msg, sizeof msg);
    if(err && *err) return fail(HPT_ERR_INVALID, err);
    if(int rc = on_scene_device(s)) return rc;
    if(int rc = ensure_previous(s)) return rc;          // `verts` holds the current geometry from here on
    hpt_scene::Update &u = s->up;
    std::vector<uint32_t> corner_begin; std::vector<MorphEntry> entries;
    transpose_morphs(target_begin, entry_corner, entry_delta, nt, num_targets, corner_begin, entries);
    u.num_targets = 0;                                   // (a failed allocation leaves the scene without morphs)
    HIP_TRY(u.morph_begin.reserve(corner_begin.size()));
    HIP_TRY(u.morph_entries.reserve(std::max<size_t>(entries.size(), 1)));
    HIP_TRY(u.morph_weights.reserve((size_t) num_targets));
    if(int rc = capture_rest(u, (size_t) nt, u.num_parts || u.num_bones)) return rc;
    HIP_TRY(hipMemcpy(u.morph_begin.get(), corner_begin.data(), corner_begin.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    if(!entries.empty()) HIP_TRY(hipMemcpy(u.morph_entries.get(), entries.data(), entries.size() * sizeof(MorphEntry), hipMemcpyHostToDevice));
    HIP_TRY(hipMemset(u.morph_weights.get(), 0, (size_t) num_targets * sizeof(float)));
    HIP_TRY(hipDeviceSynchronize());
    u.num_targets = num_targets;
    return HPT_OK;
}

int hpt_scene_morph(hpt_scene *s, const float *weights, int num_targets){
    if(!s) return fail(HPT_ERR_INVALID, "null scene");
    if(s->up.num_targets == 0) return fail(HPT_ERR_INVALID, "hpt_scene_morph before hpt_scene_set_morphs: the scene has no morph targets");
    if(num_targets != s->up.num_targets){
        char msg[200];
        snprintf(msg, sizeof msg, "a morph keeps the number of targets: the scene has %d targets, %d weights were handed over", s->up.num_targets, num_targets);
        return fail(HPT_ERR_INVALID, msg);
    }
    if(!weights) return fail(HPT_ERR_INVALID, "null weight array");
    if(int rc = on_scene_device(s)) return rc;
    Feed f{Feed::Morph}; f.weights = weights;
    return refit_from(s, f, 0.0);
}

int hpt_morph_host(const void *tris, int nt, const int32_t *target_begin, const int32_t *entry_corner, const float *entry_delta, int num_entries,
                   int num_targets, const float *weights, void *out){
    char msg[200];
    const char *err = morph_host_records(tris, nt, target_begin, entry_corner, entry_delta, num_entries, num_targets, weights, out, msg, sizeof msg);
    if(err && *err) return fail(HPT_ERR_INVALID, err);
    return HPT_OK;
}

int hpt_scene_read_triangles(hpt_scene *s, void *out, int nt){
    if(int rc = check_count(s, nt)) return rc;
    if(nt > 0 && !out) return fail(HPT_ERR_INVALID, "null triangle array");
    if(int rc = on_scene_device(s)) return rc;
    const unsigned char *tris = nullptr;
    if(int rc = host_triangles(s, &tris)) return rc;
    if(nt) memcpy(out, tris, (size_t) nt * HPT_TRIANGLE_BYTES);
    return HPT_OK;
}

int hpt_pose_host(const void *tris, int nt, const int32_t *tri_part, const float *xforms, int num_parts, void *out){
    char msg[200];
    const char *err = pose_host_records(tris, nt, tri_part, xforms, num_parts, out, msg, sizeof msg);
    if(err && *err) return fail(HPT_ERR_INVALID, err);
    return HPT_OK;
}

int hpt_scene_update_rounds(hpt_scene *s, const void *lights, int nl, const void *spheres, int ns){
    if(!s) return fail(HPT_ERR_INVALID, "null scene");
    hpt_scene::Geometry &g = s->geo;
    char msg[200];
    const char *err = check_rounds_update(g.h_spheres.data(), g.ns, g.nl, lights, nl, spheres, ns, msg, sizeof msg);
    if(err && *err) return fail(HPT_ERR_INVALID, err);
    if(int rc = on_scene_device(s)) return rc;
    std::vector<DevRound> rounds; std::vector<DevLight> dl;
    err = flatten_rounds_host(lights, nl, spheres, ns, s->up.sphere_material.data(), rounds, dl);
    if(err && *err) return fail(HPT_ERR_INVALID, err);
    if(int rc = ensure_previous(s)) return rc;
    if(!rounds.empty()) HIP_TRY(hipMemcpy(g.rounds.get(), rounds.data(), rounds.size() * sizeof(DevRound), hipMemcpyHostToDevice));
    if(!dl.empty()) HIP_TRY(hipMemcpy(g.lights.get(), dl.data(), dl.size() * sizeof(DevLight), hipMemcpyHostToDevice));
    HIP_TRY(hipDeviceSynchronize());
    if(nl) g.h_lights.assign((const unsigned char *) lights, (const unsigned char *) lights + (size_t) nl * HPT_LIGHT_BYTES);
    if(ns) g.h_spheres.assign((const unsigned char *) spheres, (const unsigned char *) spheres + (size_t) ns * HPT_SPHERE_BYTES);
    s->bd.ready = false; s->pm.bounds_ready = false;
    s->up.motion = true;
    return HPT_OK;
}

int hpt_scene_get_update_info(const hpt_scene *s, hpt_update_info *out){
    if(!s || !out) return fail(HPT_ERR_INVALID, "null argument");
    *out = s->up.info;
    return HPT_OK;
}

int hpt_bvh_refit_host(const void *lights, int nl, const void *spheres, int ns, const void *tris, const void *new_tris, int nt,
                       hpt_bvh_info *info, void *qnodes_out, size_t qnodes_cap, void *tris_out, size_t tris_cap){
    if(!info) return fail(HPT_ERR_INVALID, "null info");
    HostScene hs;
    const char *err = build_host_scene(lights, nl, spheres, ns, tris, nt, hs);
    if(err && *err) return fail(HPT_ERR_INVALID, err);
    char msg[200];
    err = check_triangle_update(tris, nt, new_tris, nt, msg, sizeof msg);
    if(err && *err) return fail(HPT_ERR_INVALID, err);
    err = refit_host_scene(hs, new_tris, nt);
    if(err && *err) return fail(HPT_ERR_INVALID, err);
    return export_host_tree(hs, info, qnodes_out, qnodes_cap, tris_out, tris_cap);
}

} // extern "C"
