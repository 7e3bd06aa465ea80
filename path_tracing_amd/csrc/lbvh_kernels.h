// Launch interface of the device builder (lbvh_kernels.hip): the topology of a Morton-order linear BVH over the vertices the
// device holds (include/hpt.h, "device builds"), to the bytes of lbvh_host_scene (scene_build.cpp), which is the definition.
// The kernels produce topology only -- sorted leaf slots, child codes, breadth-first numbers, the four-wide collapse;
// every box, the grid and both quantised trees come from the refit launches (refit_kernels.h) on that topology.
// No launch waits on another lane: nodes are numbered level by level (count, scan, scatter), never bottom-up.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace hpt {

constexpr int kLbvhBlock = 256;
constexpr int kLbvhMaxBlocks = 2048;      // the cap of the grid-stride launches
inline uint32_t lbvh_blocks(uint32_t n){ return (n + (uint32_t) kLbvhBlock - 1u) / (uint32_t) kLbvhBlock; }

// the cells of the keys: per axis the low corner of the live triangles' box and 2^21 / extent (0 where the extent is not positive)
struct LbvhCells { float lo[3], scale[3]; };

// one lane per input triangle i: tris[i] (3 x float4) gets the ordinal num_rounds + i in word 3 (the identity order: a pass of
// launch_refit_tris over it leaves slot_box[i] the box of input triangle i); idx[i] = i
void launch_lbvh_identity(hipStream_t s, float4 *tris, uint32_t *idx, uint32_t num_tris, uint32_t num_rounds);
// one lane per input triangle: keys[i] from box[i] (6 floats: min, max; inverted = dead, the key of all ones)
void launch_lbvh_keys(hipStream_t s, const float *box, uint32_t num_tris, LbvhCells cells, unsigned long long *keys);
// stable sort of (key, index) pairs by key; tmp_bytes: lbvh_sort_tmp_bytes(num_tris).  Returns a hipError_t as int.
size_t lbvh_sort_tmp_bytes(uint32_t num_tris);
int launch_lbvh_sort(hipStream_t s, void *tmp, size_t tmp_bytes, const unsigned long long *keys, unsigned long long *keys_sorted,
                     const uint32_t *idx, uint32_t *idx_sorted, uint32_t num_tris);
// one lane per new slot p: rank[idx_sorted[p]] = p; then one lane per old slot: the words ordinal, material, flags of
// old_tris[slot] go to new_tris[rank[ordinal - num_rounds]] (the geometry words are the refit's to write)
void launch_lbvh_rank(hipStream_t s, const uint32_t *idx_sorted, uint32_t num_tris, uint32_t *rank);
void launch_lbvh_permute(hipStream_t s, const float4 *old_tris, const uint32_t *rank, uint32_t num_tris, uint32_t num_rounds, float4 *new_tris);
// one lane per inner node of the binary radix tree over the sorted keys (num_tris - 1 of them, num_tris > kMaxLeafTris):
// child[node] = its two child codes in radix numbering, a range of kMaxLeafTris triangles or fewer as a leaf code
void launch_lbvh_radix(hipStream_t s, const unsigned long long *keys_sorted, uint32_t num_tris, uint2 *child);

// Breadth-first numbering, one level per call: from[first .. first + count) holds the radix numbers of the level's nodes.
// count: per lane its inner children (0 .. 2) into cnt, per block their sum into block_sum.  scan: one block turns block_sum
// (blocks entries) into exclusive offsets and stores the total in *total.  scatter: nodes[node] (4 x float4) gets its two
// child codes -- inner children numbered first + count + offset, in order, left before right -- with zero pads and
// inverted boxes, and from[] gets the next level's radix numbers.  Nothing is written at or beyond max_nodes.
// num_inner: the entries of `child` (a radix number at or beyond it is not followed).
void launch_lbvh_level_count(hipStream_t s, const uint2 *child, uint32_t num_inner, const uint32_t *from, uint32_t first, uint32_t count, uint32_t *cnt,
                             uint32_t *block_sum);
void launch_lbvh_scan(hipStream_t s, uint32_t *block_sum, uint32_t blocks, uint32_t *total);
void launch_lbvh_level_scatter(hipStream_t s, const uint2 *child, uint32_t num_inner, uint32_t *from, uint32_t first, uint32_t count, const uint32_t *cnt,
                               const uint32_t *block_sum, float4 *nodes, uint32_t max_nodes);

// Bounded builds ("bounded device builds"), one level per call, count - launch_lbvh_scan - scatter as above, but a node
// carries its range of sorted positions at its breadth-first number: range[node] = (first, count), count > kMaxLeafTris.
// count: per lane the split of its node into split[node] (the left child's triangles; 0 for a range that is none) -- forced
// when the range needs all of levels_left (balanced halves of full leaves), else Karras' split by a bisection over
// keys_sorted of at most 32 trips -- and its inner children into cnt, per block their sum into block_sum and the block's
// forced nodes added to *forced (one atomicAdd per block).  scatter: nodes[node] exactly as launch_lbvh_level_scatter writes
// it, and range[] of the inner children at their new numbers.  Every range and number read is checked against num_tris and
// max_nodes; a lane that fails a check writes nothing.  Blocks stride over the level under kLbvhMaxBlocks.
void launch_lbvh_bounded_count(hipStream_t s, const unsigned long long *keys_sorted, uint32_t num_tris, const uint2 *range, uint32_t first, uint32_t count,
                               uint32_t max_nodes, int levels_left, uint32_t *split, uint32_t *cnt, uint32_t *block_sum, uint32_t *forced);
void launch_lbvh_bounded_scatter(hipStream_t s, uint2 *range, const uint32_t *split, uint32_t num_tris, uint32_t first, uint32_t count, const uint32_t *cnt,
                                 const uint32_t *block_sum, float4 *nodes, uint32_t max_nodes);

// The four-wide collapse, one level per call, the same three steps: todo[first .. first + count) holds the binary node every
// wide node of the level is collapsed from.  collapse: the greedy opening of build_host_scene over the stored float boxes of
// `nodes` (the inner child of the largest half area first, strict >, first found), the up to four children as binary child
// codes into kid_code and their sources (node * 2 + side) into wide_src; cnt and block_sum as above.  scatter: words 12-15 of
// wnodes[wide node] get the child codes, inner ones numbered first + count + offset in order, and todo[] the next level.
void launch_lbvh_wide_collapse(hipStream_t s, const float4 *nodes, uint32_t num_nodes, const uint32_t *todo, uint32_t first, uint32_t count,
                               uint4 *kid_code, uint4 *wide_src, uint32_t *cnt, uint32_t *block_sum);
void launch_lbvh_wide_scatter(hipStream_t s, const uint4 *kid_code, uint32_t *todo, uint32_t first, uint32_t count, const uint32_t *cnt,
                              const uint32_t *block_sum, uint4 *wnodes, uint32_t max_wide);

} // namespace hpt
