// Device-side scene layout of the path-tracing hot path, shared by the host flattening /
// BVH code (scene_build.cpp) and the HIP kernels (pt_*.hip).  Plain structs only.
//
// Everything is 16-byte records so one lane fetches a record with dwordx4 loads:
//   BVH node      64 B  both children's boxes + child codes (one fetch tests two boxes)
//   triangle      48 B  v0 | e1 = v1-v0 | e2 = v2-v0, in BVH leaf order
//   round prim    32 B  spheres followed by light balls (the reference's scan order)
//   material      32 B  de-duplicated CudaMaterial records
//   light        112 B  CudaLight with the per-light invariants hoisted
#pragma once
#include <cstdint>
#include <memory>
#include <utility>
#include <vector>

namespace hpt {

constexpr uint32_t kLeafFlag = 0x80000000u;   // child code: leaf | first_tri << 3 | (count - 1)
constexpr uint32_t kEmptyChild = 0xFFFFFFFFu; // child code of an absent child (box is inverted)
constexpr int kMaxLeafTris = 2;              // triangles per leaf (A/B on four scenes, DESIGN.md section 5: 2 beats 1, 3, 4, 6, 8)
constexpr int kMaxBvhDepth = 30;              // traversal stack holds kStackDepth entries
constexpr int kStackDepth = 32;

struct Float4 { float x, y, z, w; };

// std::vector whose resize() leaves trivially constructible elements uninitialised: the scene arrays are tens to hundreds of
// megabytes, every element is written by the (multi-threaded) build, and a zero fill by the one thread that resizes them --
// page faults included -- was a fifth of the build
template <typename T>
struct default_init_allocator : std::allocator<T> {
    template <typename U> struct rebind { using other = default_init_allocator<U>; };
    default_init_allocator() = default;
    template <typename U> default_init_allocator(const default_init_allocator<U> &){}
    template <typename U> void construct(U *p){ ::new((void *) p) U; }
    template <typename U, typename... A> void construct(U *p, A &&... a){ ::new((void *) p) U(std::forward<A>(a)...); }
};
template <typename T> using pod_vector = std::vector<T, default_init_allocator<T>>;

struct BvhNode {           // 64 B
    float lmin[3]; uint32_t left;
    float lmax[3]; uint32_t right;
    float rmin[3]; uint32_t pad0;
    float rmax[3]; uint32_t pad1;
};

// Quantised twin of BvhNode, 32 B: child boxes as 16-bit grid coordinates of the scene box
// (min rounded down, max rounded up, so the quantised box contains the float box); two dwordx4
// fetches per node visit instead of four.  Traversal only needs conservative boxes.
// plane[axis][0 = lower, 1 = upper][0 = left child, 1 = right child]: word 2 * axis holds the lower planes of both children, word
// 2 * axis + 1 the upper ones -- t = q * i + o is monotone in q, so a ray takes its near planes from one word and its far planes
// from the other by the sign of its direction (one bit-select per word, no min / max per plane pair)
struct QBvhNode {
    uint16_t plane[3][2][2];
    uint32_t left, right;
};

// Four-wide twin of the tree (development: the resume launch's A/B), 64 B: the binary tree
// collapsed greedily (the child with the largest box is opened until a node has four children or only leaves are left),
// child boxes on the same 16-bit grid.  Words 0-3 x, 4-7 y, 8-11 z: lo(c0)|lo(c1)<<16, lo(c2)|lo(c3)<<16, hi(c0)|hi(c1)<<16,
// hi(c2)|hi(c3)<<16 -- a ray picks the near and far planes of two children with one bit-select per word; words 12-15 the
// child codes (leaf codes as in the binary tree, inner = index into the wide node array, kEmptyChild).
struct WideNode { uint32_t w[16]; };

struct DevTriangle {       // 48 B
    float v0[3]; uint32_t ordinal;   // reference scan ordinal (num_spheres + num_lights + input index)
    float e1[3]; uint32_t material;  // index into the material table
    float e2[3]; uint32_t flags;     // bit 0: opaque to shadow rays (mtl.eta <= 0)
};

struct DevRound {          // 32 B: sphere or light ball
    float c[3]; float r;
    uint32_t material;     // spheres: material index; light balls: light index
    uint32_t flags;        // bit 0: opaque to shadow rays; bit 1: is a light ball
    uint32_t pad[2];
};

// What a material is to the shade stage, one bit per question k_shade and bsdf_sample ask of every hit; each bit is the
// comparison those ask, on the same three floats (material_class below, filled with the table)
constexpr uint32_t kMatSmoothDielectric = 1u;   // eta > 0 && roughness < 0.001 && metallic < 0.01: the delta transmission lobe
constexpr uint32_t kMatMirror = 2u;             // metallic > 0.99 && roughness < 0.001: the delta reflection lobe
constexpr uint32_t kMatNextEvent = 4u;          // eta <= 0 && (metallic < 0.99 || roughness > 0.01): gets a next-event candidate
constexpr uint32_t kMatMetallic = 8u;           // metallic > 0: Schlick Fresnel, specular weight 1

struct DevMaterial {       // 48 B
    float base[3]; float roughness;
    float metallic; float eta; uint32_t type; uint32_t cls;     // cls: kMat* bits (read by k_shade only)
    float diffuse[3]; float alpha;           // base / pi * (1 - metallic): the diffuse lobe of every BSDF value (geometric.cuh:433);
                                             // alpha = max(roughness, 1e-3)^2, the GGX width (read by k_shade only)
};

inline uint32_t material_class(float roughness, float metallic, float eta){
    return ((eta > 0.0f && roughness < 0.001f && metallic < 0.01f) ? kMatSmoothDielectric : 0u) |
           ((metallic > 0.99f && roughness < 0.001f) ? kMatMirror : 0u) |
           ((eta <= 0.0f && (metallic < 0.99f || roughness > 0.01f)) ? kMatNextEvent : 0u) |
           (metallic > 0.0f ? kMatMetallic : 0u);
}

struct DevLight {          // 112 B
    float pos[3]; float r;
    float main_dir[3]; float cos_cutoff;     // normalize(dir); cosf(cutoff) from the host libm
    float neg_dir[3]; float cutoff;          // normalize(dir * -1) for parallel lights
    float illum[3]; float area;              // 4 * pi * r * r
    uint32_t is_parallel; float cone_ratio;  // (1 - cos_cutoff) / 2
    float pdf_area; uint32_t pad;            // 1 / (number of lights * area), the area pdf of a next-event sample (read by k_shade only)
    float raw_dir[3]; uint32_t pad2;         // light.dir as handed over (the BDPT path normalises it itself)
    float ball_c[3]; uint32_t pad3;          // light_ball.center (equals pos for parsed scenes)
};

static_assert(sizeof(BvhNode) == 64 && sizeof(DevTriangle) == 48 && sizeof(DevRound) == 32, "layout");
static_assert(sizeof(QBvhNode) == 32 && sizeof(WideNode) == 64, "layout");
static_assert(sizeof(DevMaterial) == 48 && sizeof(DevLight) == 112, "layout");

// Host-side flattened scene, ready to upload.
struct HostScene {
    pod_vector<BvhNode> nodes;         // nodes[0] is the root (always an inner node)
    pod_vector<QBvhNode> qnodes;       // same tree, quantised boxes
    pod_vector<WideNode> wnodes;       // four-wide collapse of it (the resume launch's tree)
    int wide_depth = 0;
    // what a refit needs besides the arrays (scene updates, include/hpt.h): per wide node and child the binary child its box
    // is taken from (node * 2 + side, kEmptyChild for an absent child), and where each level of the breadth-first binary
    // tree begins (level_begin[l] .. level_begin[l + 1]; the last entry is the node count)
    pod_vector<uint32_t> wide_src;
    std::vector<uint32_t> level_begin;
    float qorigin[3] = {0, 0, 0}, qscale[3] = {1, 1, 1};   // grid: coordinate = qorigin + q * qscale
    pod_vector<DevTriangle> tris;      // leaf order
    std::vector<DevRound> rounds;      // spheres, then light balls
    std::vector<DevMaterial> materials;
    std::vector<DevLight> lights;
    int num_spheres = 0, num_lights = 0, num_tris = 0;
    int bvh_depth = 0;
    double ms_bvh_build = 0.0;
};

// ---- scene of the bidirectional (cpu_bdpt-estimator) path -------------------------------------
// The reference's CPU renderer traces a one-level list of groups (reference src/cpu_bdpt.cpp:43-61,
// src/object.cpp:104-146): a group's box is slab-tested, then its objects are tried in insertion
// order with an inclusive range, so among equal distances the LAST object wins.  Each group gets
// its own BVH here; `ordinal` of a triangle / `pad[0]` of a sphere hold that iteration order.
struct DevGroup {          // 48 B
    float mn[3]; uint32_t root;            // child code of the group's BVH (leaf, inner or kEmptyChild)
    float mx[3]; uint32_t sphere_first;
    uint32_t sphere_count; uint32_t pad[3];
};
static_assert(sizeof(DevGroup) == 48, "layout");

struct HostBdptScene {
    std::vector<BvhNode> nodes;
    std::vector<DevTriangle> tris;       // leaf order per group
    std::vector<DevRound> spheres;       // grouped, insertion order inside a group
    std::vector<DevGroup> groups;        // map order
    std::vector<DevMaterial> materials;
    std::vector<DevLight> lights;
    float scene_min[3], scene_max[3];    // union of the group boxes (parallel-light emission)
    int bvh_depth = 0;
};

// obj_kind[i] (0 sphere, 1 triangle), obj_index[i] (into spheres / tris), obj_group[i]: the scene
// file's objects in insertion order; null arrays = one group holding the spheres then the triangles.
const char *build_bdpt_host_scene(const void *lights, int nl, const void *spheres, int ns, const void *tris, int nt,
                                  const int32_t *obj_kind, const int32_t *obj_index, const int32_t *obj_group, int nobj,
                                  HostBdptScene &out);

// Flattens reference records (layouts in include/hpt.h) and builds the BVH.
// Returns an empty string on success, an error message otherwise.
const char *build_host_scene(const void *lights, int nl, const void *spheres, int ns,
                             const void *tris, int nt, HostScene &out);

// ---- scene updates: the tree's topology is kept and everything that is a function of the vertex positions is recomputed ----

// Spheres then light balls, and the light records, of a scene (build_host_scene and hpt_scene_update_rounds run these lines);
// sphere_material[i] is the material number of sphere i.
const char *flatten_rounds_host(const void *lights, int nl, const void *spheres, int ns, const uint32_t *sphere_material,
                                std::vector<DevRound> &rounds, std::vector<DevLight> &lights_out);

// The refusals of an update: "" when `tris` (nt records) may replace `kept` (kept_nt records) -- the same count and, in every
// record, the same 84 bytes behind the vertices -- else the message (a literal or `msg`).  Likewise for the spheres' 84 bytes.
const char *check_triangle_update(const void *kept, int kept_nt, const void *tris, int nt, char *msg, size_t msg_cap);
const char *check_rounds_update(const void *kept_spheres, int kept_ns, int kept_nl, const void *lights, int nl, const void *spheres, int ns,
                                char *msg, size_t msg_cap);

// The definition of a refit: hs (built by build_host_scene from records that differ from `tris` in the vertices only) gets the
// leaf records, node boxes, grid and both quantised trees of the new vertices; child codes, counts and depths stay.  The
// device's refit (refit_kernels.hip) is held to these bytes.  dead_out: the number of triangles no ray can hit.
const char *refit_host_scene(HostScene &hs, const void *tris, int nt, uint64_t *dead_out = nullptr);

// The definition of a device build (include/hpt.h, "device builds"): the Morton-order linear BVH over `tris` -- 63-bit keys of
// the live centroids on the live triangles' box, a stable sort, the binary radix tree with leaves of kMaxLeafTris triangles
// or fewer, build_host_scene's breadth-first numbering and greedy four-wide collapse -- with every box, the grid and both
// quantised trees from refit_host_scene on that topology.  hs.bvh_depth may exceed kMaxBvhDepth: the depth of a radix tree
// is the data's (the device falls back to the host builder then).  The device builder (lbvh_kernels.hip) is held to these bytes.
const char *lbvh_host_scene(const void *lights, int nl, const void *spheres, int ns, const void *tris, int nt, HostScene &out);

// The definition of a bounded device build (include/hpt.h, "bounded device builds"): lbvh_host_scene's keys, order, leaf
// records, numbering, boxes and collapse, over a topology made top-down.  A node at level d whose range needs every one of
// the D - d levels left (lbvh_need) is split into balanced halves of full leaves -- Builder::build_node's rule -- and any
// other node by Karras' split of its range.  hs.bvh_depth <= D; while no node is forced the tree is lbvh_host_scene's.
// max_depth: 0 for kMaxBvhDepth, else within [lbvh_need(nt), kMaxBvhDepth] (lbvh_check_depth: "" or the refusal in msg).
struct BoundedInfo { uint32_t max_depth = 0, forced_nodes = 0, first_forced_level = 0xFFFFFFFFu; };
int lbvh_need(int64_t count);          // the smallest k >= 1 with 2^k >= (count + 1) / 2: the levels a range of count triangles needs
const char *lbvh_check_depth(int nt, int max_depth, int &effective, char *msg, size_t msg_cap);
const char *lbvh_bounded_host_scene(const void *lights, int nl, const void *spheres, int ns, const void *tris, int nt, int max_depth,
                                    HostScene &out, BoundedInfo &info);

// ---- poses (include/hpt.h, "poses"): per-part 3 x 4 transforms applied to a rest pose ----

constexpr int kMaxParts = 1 << 20;
// The refusals the pose calls share: "" when tri_part (nt entries, or null with num_parts == 1) names parts of [0, num_parts)
// and num_parts lies in [1, kMaxParts], else the message (a literal or `msg`, which names the first triangle out of range).
const char *check_parts(const int32_t *tri_part, int nt, int num_parts, char *msg, size_t msg_cap);
// The definition of a pose: one vertex (x, y, z) under the record r (three rows a, b, c, t), one float operation at a time,
// left to right; a record whose 48 bytes are the identity's keeps the vertex's bits, a result that is not finite makes all
// three words 0x7FC00000.  k_pose_verts (refit_kernels.hip) is held to these bytes.
void pose_vertex_host(const float r[12], const float in[3], float out[3]);
// records out[i] = tris[i] with its three vertices posed by xforms[tri_part[i]]; out may be tris itself
const char *pose_host_records(const void *tris, int nt, const int32_t *tri_part, const float *xforms, int num_parts, void *out,
                              char *msg, size_t msg_cap);

// ---- skinning (include/hpt.h, "skinning"): four (bone, weight) influences per corner blended over a rest pose ----

constexpr int kSkinInfluences = 4;
constexpr int kMaxBones = 1 << 16;         // a bone index travels as 16 bits on the device
// The refusals the skin calls share: "" when corner_bone and corner_weight (nt * 3 * 4 entries each) name bones of
// [0, num_bones), active or not, carry weights that are finite with a clear sign bit, and num_bones lies in [1, kMaxBones];
// else the message (a literal or `msg`, which names the first triangle and corner at fault).
const char *check_skin(const int32_t *corner_bone, const float *corner_weight, int nt, int num_bones, char *msg, size_t msg_cap);
// The definition of a skin: one corner's rest vertex under its four influences and the table xforms (12 floats per bone, the
// rows of a pose).  An influence is active when its weight's 32 bits are not zero.  keep: every active influence's record has
// the identity's 48 bytes (or none is active) -- the vertex keeps its bits.  rigid: one active influence of weight 1.0f -- the
// bytes of pose_vertex_host with that record.  blend: p_j = the rows applied to the vertex, acc = w_j * p_j for the first
// active influence and acc = acc + w_j * p_j for each later one, in index order.  A result that is not finite makes all
// three words 0x7FC00000.  `out` may be `in`.  k_skin_verts (refit_kernels.hip) is held to these bytes.
void skin_vertex_host(const int32_t bone[4], const float weight[4], const float *xforms, const float in[3], float out[3]);
// records out[i] = tris[i] with its three corners skinned; out may be tris itself
const char *skin_host_records(const void *tris, int nt, const int32_t *corner_bone, const float *corner_weight, const float *xforms,
                              int num_bones, void *out, char *msg, size_t msg_cap);

// ---- morph targets (include/hpt.h, "morph targets"): weighted per-corner deltas summed over a rest pose ----

constexpr int kMaxMorphTargets = 4096;     // the weights of one morph fit the 16 KB of LDS k_morph_verts stages them in
// One entry of the table as the device walks it: which target, and its delta for the corner the entry belongs to.
struct MorphEntry { uint32_t target; float dx, dy, dz; };
static_assert(sizeof(MorphEntry) == 16, "one 16-byte load per entry");
// The refusals the morph calls share: "" when num_targets lies in [1, kMaxMorphTargets], target_begin (num_targets + 1 values)
// starts at 0, never decreases and ends at num_entries, and within every target the corners lie in [0, 3 * nt) and ascend
// strictly; else the message (a literal or `msg`, which names the target and the entry at fault).
const char *check_morphs(const int32_t *target_begin, const int32_t *entry_corner, const float *entry_delta, int num_entries, int nt,
                         int num_targets, char *msg, size_t msg_cap);
// The caller's targets (checked by check_morphs) turned round for a lane per corner: corner c owns entries
// corner_begin[c] .. corner_begin[c + 1] - 1, in ascending target order, which is the order of the definition's sum.
void transpose_morphs(const int32_t *target_begin, const int32_t *entry_corner, const float *entry_delta, int nt, int num_targets,
                      std::vector<uint32_t> &corner_begin, std::vector<MorphEntry> &entries);
// The definition of a morph for one corner, over the corner's own entries: a target is active when its weight is neither +0
// nor -0.  keep: no entry's target is active -- the vertex keeps its bits.  Otherwise per component acc = the rest value, and
// acc = acc + w * d for every active entry in order, the product rounded before the sum; a result that is not finite makes
// all three words 0x7FC00000.  `out` may be `in`.  k_morph_verts (refit_kernels.hip) is held to these bytes.
void morph_vertex_host(const MorphEntry *entries, size_t count, const float *weights, const float in[3], float out[3]);
// records out[i] = tris[i] with every corner morphed, from the caller's layout (no transposition: target after target, which
// gives each corner the same sum in the same order); out may be tris itself
const char *morph_host_records(const void *tris, int nt, const int32_t *target_begin, const int32_t *entry_corner, const float *entry_delta,
                               int num_entries, int num_targets, const float *weights, void *out, char *msg, size_t msg_cap);

// the builder's lines the device's refit needs on the host between its launches
float box_padding_of(const float scene_min[3], const float scene_max[3], int nt);                      // pad_abs of a scene box
void grid_of_box(const float lo[3], const float hi[3], float qorigin[3], float qscale[3]);         // the 16-bit grid over a box

} // namespace hpt

// ---- tree cost (include/hpt.h, "tree cost") ----
struct hpt_tree_cost;
namespace hpt {
// The definition's integers: the ten sums, root_extent and num_nodes of `out` over the quantised binary tree q; the doubles
// are zeroed.  k_tree_cost (cost_kernels.hip) is held to these integers.
void tree_cost_sums_host(const QBvhNode *q, uint32_t num_nodes, hpt_tree_cost &out);
// The definition's doubles from the integers of `c` and the grid's scale: IEEE double, evaluated as written, left to right.
// The one place they are composed, for the host's sums and the device's alike.
void tree_cost_compose(const float qscale[3], hpt_tree_cost &c);
} // namespace hpt

struct hpt_scene;
namespace hpt {
// uploads a flattened scene to the current HIP device (hpt_api.cpp; struct hpt_scene is in hpt_host.h); the records are kept for the bidirectional path
int scene_upload(const HostScene &hs, const void *lights, int nl, const void *spheres, int ns, const void *tris, int nt,
                 hpt_scene **out);
} // namespace hpt
