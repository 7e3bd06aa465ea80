// Launch interface between the C ABI (hpt_api.cpp) and the HIP kernels of the unidirectional path-tracing hot path,
// written for gfx950 (MI355X): a wavefront pipeline over queues of path slots
//
//   generate -> [ trace -> shade ]* -> trace -> resolve -> finalize
//
// generate  primary rays for (pixel, sample) slots                 (reference src/pt_cu.cu:36-46)          pt_frame.hip
// trace     one merged launch per iteration: closest hit of every queued path (spheres + light balls       pt_trace.hip
//           by scan, triangles by BVH; what it must return: reference include/geometric.cuh:327-388)
//           and the any-hit shadow rays of the previous iteration, whose unoccluded contributions are
//           added to the sample's radiance (include/geometric.cuh:293-325, src/pt_cu.cu:136-146,
//           174-196).  A trace step is two launches: every ray gets a budget of node steps, the few
//           that need more are set aside and finished by the resume launch.
// shade     light-hit emission, next-event estimation set-up, BSDF sampling, throughput update;            pt_shade.hip
//           survivors and shadow requests are compacted in LDS (wave64 ballot + mbcnt prefix) and
//           flushed with one global atomic per workgroup            (reference src/pt_cu.cu:54-241)
// resolve   per pixel, adds this pass's samples in sample order (src/pt_cu.cu:243-245)                     pt_frame.hip
// finalize  mean over samples into the packed local framebuffer      (src/pt_cu.cu:248)                    pt_frame.hip
// k_extend / k_connect are the one-ray-per-lane forms kept for the brute-force scan variants (tests).      pt_scan.hip
//
// One lane owns one path for the whole launch, every (pixel, sample) owns one slot for the
// whole pass, and sums run in a fixed order, so results do not depend on scheduling, queue
// order, pass size or the number of devices.  Built with -ffp-contract=off (pt_device_math.h); shared device helpers: pt_device_common.h.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include "hpt_scene.h"

namespace hpt {

struct SceneDev {
    const float4 *nodes;        // BvhNode as 4 x float4
    const uint4 *qnodes;        // QBvhNode as 2 x uint4 (k_trace)
    const uint4 *wnodes;        // WideNode as 4 x uint4 (the resume launch's tree)
    int wide_depth;
    float qorigin[3], qscale[3];
    const float4 *tris;         // DevTriangle as 3 x float4, leaf order
    const float4 *tri_frames;   // per triangle 4 x float4: shading normal and both local frames (launch_tri_frames)
    const DevRound *rounds;     // spheres then light balls
    const DevMaterial *mats;
    const DevLight *lights;
    int num_rounds, num_spheres, num_lights, num_tris, num_mats, num_nodes;
};

// Path state, structure of arrays indexed by path slot (one slot per (pixel, sample) in flight).
struct PathBuf {
    float4 *org_eta;     // ray origin xyz | current medium eta
    float4 *dir_flags;   // ray direction xyz | bit 0 last_is_delta, bits 8-15 depth, bits 16-23 delta count
    float4 *thr;         // throughput xyz | unused
    float4 *col;         // radiance accumulated by this sample xyz | unused
    uint2 *rng;          // PCG32 state
    uint2 *hit;          // extend result: as_uint(t) | primitive code
};

// Pending shadow rays of an iteration, structure of arrays indexed by RECORD index: k_shade stores the records of a
// workgroup's chunk densely from the chunk's first queue position on (a path has at most one pending shadow ray, so a
// chunk never has more records than queue positions, and never more than there are path slots).  The shadow queue is a
// compacted list of record indices; the path slot a record belongs to travels in contrib.w.
struct ShadowBuf {
    float4 *org_max;     // p1 xyz | max_d
    float4 *dir;         // unit direction xyz | unused
    float4 *contrib;     // clamped contribution if unoccluded xyz | path slot (as bits)
};

// Image tiling shared by ray generation, resolve and untile (see DESIGN.md "Tiling").
struct Tiling {
    int W, H, tile, tiles_x, tiles_y, ntiles, rank, world;
    int n_local;         // packed local framebuffer slots = ceil(ntiles / world) * tile * tile
};

struct CameraDev { float eye[3], UL[3], dx[3], dy[3]; };

// What it takes to recompute the primary ray of a path slot (reference src/pt_cu.cu:36-46): handed to the PRIMARY
// variants of k_trace / k_shade, which run iteration 0 of a pass without a generate launch.
struct PrimaryGen { Tiling tl; CameraDev cam; uint32_t first_sample; uint32_t pad; uint64_t seed; };

struct WorkCounters {    // device counters, COUNT_WORK only
    unsigned long long boxes_closest, tris_closest, boxes_shadow, tris_shadow, closest_rays, shadow_rays, path_iters, samples,
                       lane_steps_closest, wave_steps_closest, lane_steps_shadow, wave_steps_shadow,
                       leaf_lane_closest, leaf_wave_closest, leaf_lane_shadow, leaf_wave_shadow,
                       // connection stage of the bidirectional path (k_bdpt_connect): candidate (eye vertex, light vertex) pairs, pairs that
                       // pass the culls, shadow rays traced, unoccluded ones; node visits, triangle, sphere and group-box tests of those rays
                       bd_pairs, bd_survivors, bd_shadow_rays, bd_unoccluded, bd_nodes, bd_tris, bd_spheres, bd_group_boxes;
};

// primitive code in PathBuf::hit.y
constexpr uint32_t kHitMiss = 0xFFFFFFFFu;
constexpr uint32_t kHitRoundFlag = 0x80000000u;   // | index into rounds; else triangle slot

constexpr int kBlock = 256;
// rays per workgroup of the resume launch of a split step (every ray in it is a long one)
constexpr uint32_t kLongChunk = 4096;       // with two passes in flight: 2048 -> 4096 = -3.0 % / -2.1 % on 100 k / 20 k random triangles, -0.5 % on the sphere scenes
                                            // (one pass in flight: +2 % on random triangles: a launch's tail is then nobody's to fill)
constexpr int kResumeLdsLevels = 12; // stack levels of a resume-launch lane kept in LDS (deeper: the deep-stack buffer in global memory)
constexpr uint32_t kResumeMaxGroups = 8192;   // grid cap of the resume launch
constexpr int kDeepLevels = 48;      // global-memory stack levels per lane of the resume launch (the four-wide walk stacks up to three children per step)
constexpr int kWideRefillMin = 24;   // idle lanes that trigger a refill in the resume launch, and its early-leaf-break threshold
constexpr int kWideNodeMin = 16;     // (A/B grid 16/24/32 x 12/16/24 on configs 3 and 5)
#ifndef HPT_TRACE_BUDGET             // development A/B: `make variant EXTRA="-DHPT_TRACE_BUDGET=7 -DHPT_TOP_LEVELS=7"`
#define HPT_TRACE_BUDGET 6
#endif
#ifndef HPT_TOP_LEVELS
#define HPT_TOP_LEVELS 6
#endif
constexpr int kTraceBudget = HPT_TRACE_BUDGET;   // node steps a ray gets in the first trace launch before it is set aside
constexpr int kTopLevels = HPT_TOP_LEVELS;       // a budget of at most this many steps keeps a ray among the first kTopNodes nodes
constexpr int kTopNodes = 1 << kTopLevels;       // (breadth-first order, scene_build.cpp): 2^kTopLevels - 1 = 63 nodes of 32 B, staged in LDS

void launch_generate(hipStream_t s, const Tiling &tl, const CameraDev &cam, PathBuf pb,
                     uint32_t *qcount, int samples_this_pass, uint32_t first_sample, uint64_t seed,
                     WorkCounters *wc);
void launch_extend(hipStream_t s, const SceneDev &sc, PathBuf pb, const uint32_t *queue, const uint32_t *qcount,
                   uint32_t max_items, int flags, WorkCounters *wc);
void launch_shade(hipStream_t s, const SceneDev &sc, PathBuf pb, const uint32_t *queue, const uint32_t *qcount,
                  uint32_t max_items, uint32_t *next_queue, uint32_t *next_count, ShadowBuf sb, uint32_t *squeue,
                  uint32_t *scount, int max_depth, int max_delta, int roulette, WorkCounters *wc, const PrimaryGen *primary = nullptr,
                  uint32_t max_groups = 0);        // max_groups != 0 caps the grid (the kernels walk their chunks with a stride)
void launch_connect(hipStream_t s, const SceneDev &sc, PathBuf pb, ShadowBuf sb, const uint32_t *squeue,
                    const uint32_t *scount, uint32_t max_items, int flags, WorkCounters *wc);
// merged closest-hit (equeue) + any-hit (squeue) launch; either queue may be absent (null count)
// split != null && split->budget > 0: rays needing more than `budget` node steps are set aside into the
// long queues (their counters must be zero on entry) and finished by a second launch
// `rec`: the closest-hit rays set aside past iteration 0 travel as records, one per queue position at most; equeue then
// holds record indices, not path slots.  Three 16-B cells in one place: a lane writes (and the resume launch reads) 48
// contiguous bytes, the records of neighbouring lanes follow each other, and the kernels carry one pointer
struct DeferredRay {
    float4 org_t;          // origin, t of the closest hit so far (1e20: none)
    float4 dir_slot;       // direction, path slot as bits
    uint4 hit;             // best primitive (PathBuf::hit.y), its ordinal, two spare words
};
struct TraceSplit { uint32_t *equeue, *ecount, *squeue, *scount; int budget; DeferredRay *rec; };
void launch_trace(hipStream_t s, const SceneDev &sc, PathBuf pb, ShadowBuf sb, const uint32_t *equeue,
                  const uint32_t *ecount, uint32_t max_extend, const uint32_t *squeue, const uint32_t *scount,
                  uint32_t max_shadow, int stack_levels, bool count, WorkCounters *wc,
                  const TraceSplit *split = nullptr, const PrimaryGen *primary = nullptr, uint32_t max_groups = 0);
// the resume launch walks the four-wide tree with kResumeLdsLevels stack levels in LDS and up to kDeepLevels more in
// deep_stack: a scene may only be split if resume_walk_fits() it
void launch_trace_resume(hipStream_t s, const SceneDev &sc, PathBuf pb, ShadowBuf sb, bool extend, bool shadow,
                         uint32_t max_items, WorkCounters *wc, const TraceSplit &split, const PrimaryGen *primary,
                         uint32_t max_groups, uint32_t *deep_stack);
inline bool resume_walk_fits(const SceneDev &sc){ return 3 * sc.wide_depth + 2 <= kResumeLdsLevels + kDeepLevels; }
// words of the buffer launch_trace_resume's deep_stack needs (one column per lane of its largest grid)
size_t resume_deep_stack_words();
// fills frames[4 * num_tris] from tris (once per scene)
void launch_tri_frames(hipStream_t s, const float4 *tris, int num_tris, float4 *frames);
void launch_resolve(hipStream_t s, const Tiling &tl, PathBuf pb, float4 *accum, int samples_this_pass);
void launch_finalize(hipStream_t s, const Tiling &tl, const float4 *accum, float *d_local, float scale);
void launch_untile(hipStream_t s, const Tiling &tl, const float *d_gathered, float *d_image);

// 8-bit output stage: num_values = 3 * pixels floats in, as many bytes out (d_bytes 4-byte aligned); d_thresholds: 256 floats
void launch_tonemap(hipStream_t s, const float *d_linear, void *d_bytes, unsigned long long num_values, int bgr, const float *d_thresholds);

// function-level probe (tests): 24 floats in, 40 floats out per record (layout: k_probe_functions)
void launch_probe_functions(hipStream_t s, const float *d_in, int n, float *d_out);
// ray-level probes (tests)
void launch_probe_closest(hipStream_t s, const SceneDev &sc, const float *org, const float *dir, int n, int flags,
                          float *t_out, int32_t *prim_out);
void launch_probe_visibility(hipStream_t s, const SceneDev &sc, const float *p1, const float *p2, int n, int flags,
                             int32_t *vis_out);

} // namespace hpt
