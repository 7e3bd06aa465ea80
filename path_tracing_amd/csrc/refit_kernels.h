// Launch interface of the refit kernels (refit_kernels.hip): a live scene's tree refitted to new vertex positions on the
// device (include/hpt.h, "scene updates").  The topology -- child codes, leaf slots, node and level counts -- is the
// build's; everything that is a function of the vertices is recomputed, to the bytes of refit_host_scene
// (scene_build.cpp), which is the definition.  All launches are one lane per element, plain streaming code.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace hpt {

// the 16-bit grid of the quantised trees: coordinate = qorigin + q * qscale
struct RefitGrid { float qorigin[3], qscale[3]; };

constexpr int kRefitBlock = 256;
inline uint32_t refit_blocks(uint32_t n){ return (n + (uint32_t) kRefitBlock - 1u) / (uint32_t) kRefitBlock; }

// One lane per leaf slot: tris[slot] (3 x float4) gets v0, e1, e2 of input triangle `ordinal - num_rounds` out of verts (nine
// floats per triangle, input order); ordinal, material and flags stay.  slot_box[slot] (6 floats: min, max) gets the
// triangle's box, or an inverted box for a dead triangle (an edge component that is not finite).  partial[6 * block] gets
// the block's live box; *dead_count grows by the block's dead triangles (one integer atomic per block; zeroed by the caller).
void launch_refit_tris(hipStream_t s, const float *verts, float4 *tris, uint32_t num_tris, uint32_t num_rounds, float *slot_box,
                       float *partial, uint32_t *dead_count);
// one block: out6 = the union of `blocks` partial boxes (launch_refit_tris)
void launch_refit_reduce(hipStream_t s, const float *partial, uint32_t blocks, float *out6);

// One lane per node of [first, first + count), a level of the breadth-first tree whose deeper levels are done: the exact box
// of a leaf child is the union of its slots' boxes (a dead slot is the point dead_at), of an inner child exact[child]; the
// node stores each padded (pad_abs, then two float neighbours each way) and exact[node] (6 floats) gets their union.
void launch_refit_level(hipStream_t s, float4 *nodes, uint32_t num_nodes, uint32_t first, uint32_t count, const float *slot_box,
                        uint32_t num_tris, float *exact, float pad_abs, float dead_x, float dead_y, float dead_z);

// one lane per binary node: qnodes[node] (2 x uint4) from the stored boxes of nodes[node] on the grid
void launch_refit_quantise(hipStream_t s, const float4 *nodes, uint4 *qnodes, uint32_t num_nodes, RefitGrid grid);
// one lane per four-wide node: words 0-11 from the stored boxes of the binary children wide_src[wide node] names
// (node * 2 + side, 0xFFFFFFFF: absent); the child codes in words 12-15 stay
void launch_refit_wide(hipStream_t s, const float4 *nodes, uint32_t num_nodes, uint4 *wnodes, const uint4 *wide_src, uint32_t num_wide,
                       RefitGrid grid);

// ---- poses (include/hpt.h, "poses") ----
constexpr int kPoseLdsParts = 256;        // tables of up to this many parts (12 KB) are staged in LDS
constexpr int kPoseMaxBlocks = 2048;      // the grid's cap; a grid-stride loop covers the rest
// One lane per vertex: verts[v] = the record xforms[tri_part[v / 3]] (three rows a, b, c, t) applied to rest[v], to the bytes
// of pose_vertex_host (scene_build.cpp), which is the definition: an identity record keeps the vertex's bits, a result that
// is not finite becomes three canonical NaNs.  rest and verts hold nine floats per triangle, input order.
void launch_pose_verts(hipStream_t s, const float *rest, const int32_t *tri_part, const float *xforms, uint32_t num_parts, uint32_t num_tris,
                       float *verts);

// ---- skinning (include/hpt.h, "skinning") ----
// One lane per corner (vertex v of the 3 * num_tris): verts[v] = rest[v] under the four influences corner_bone[v] (four
// 16-bit bone indices in one 8-byte word, influence 0 lowest) and corner_weight[v] over the table xforms (12 floats per bone),
// to the bytes of skin_vertex_host (scene_build.cpp), which is the definition.  Tables of up to kPoseLdsParts bones are
// staged in LDS; the grid is capped at kPoseMaxBlocks.  24 bytes of influences per corner, 148 bytes moved per triangle.
void launch_skin_verts(hipStream_t s, const float *rest, const uint2 *corner_bone, const float4 *corner_weight, const float *xforms,
                       uint32_t num_bones, uint32_t num_tris, float *verts);

// ---- morph targets (include/hpt.h, "morph targets") ----
constexpr int kMorphMaxTargets = 4096;    // HPT_MORPH_MAX_TARGETS: one morph's weights are 16 KB of LDS
// One lane per corner: verts[v] = rest[v] plus the weighted deltas of the corner's entries, entries[corner_begin[v]] ..
// entries[corner_begin[v + 1] - 1] (16 bytes each: the target's index, then dx, dy, dz as float bits; sorted by corner, then
// target), to the bytes of morph_vertex_host (scene_build.cpp), which is the definition: an entry whose target has the
// weight +0 or -0 is skipped, a corner with no active entry keeps its bits, a result that is not finite becomes three
// canonical NaNs.  corner_begin holds 3 * num_tris + 1 values; the grid is capped at kPoseMaxBlocks.  4 bytes per corner
// and 16 per entry, next to the 24 bytes of vertices read and written.
void launch_morph_verts(hipStream_t s, const float *rest, const uint32_t *corner_begin, const uint4 *entries, const float *weights,
                        uint32_t num_targets, uint32_t num_tris, float *verts);

// ---- tree cost (include/hpt.h, "tree cost"; cost_kernels.hip) ----
constexpr int kCostCounters = 10;         // the integer sums of hpt_tree_cost, in its order
constexpr int kCostResultWords = 12;      // 64-bit words of `result`: the sums, then root_extent[3] as 32-bit words and a pad
constexpr int kCostMaxBlocks = 256;       // the grid's cap (one workgroup per CU); a grid-stride loop covers the rest
// One lane per node of the quantised binary tree, both children per lane: result[0 .. 9] grow by the sums (one 64-bit
// integer atomic per workgroup and counter; zeroed by the caller) and the lane that reads node 0 stores the root's extent
// behind them, to the integers of tree_cost_sums_host (scene_build.cpp), which is the definition.
void launch_tree_cost(hipStream_t s, const uint4 *qnodes, uint32_t num_nodes, unsigned long long *result);

} // namespace hpt
