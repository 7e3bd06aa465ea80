/* hpt.h -- C ABI of the MI355X-native path-tracing hot path (libhpt.so).
 *
 * Drop-in boundary for the reference renderer's unidirectional path-tracing launch
 * API.  Every entry point takes plain pointers and sizes; the scene records are the
 * reference's own host PODs, byte for byte:
 *
 *   light    144 B  reference include/geometric.cuh:73-78   (CudaLight)
 *   sphere   100 B  reference include/geometric.cuh:29-35   (CudaSphere)
 *   triangle 120 B  reference include/geometric.cuh:37-42   (CudaTriangle)
 *   camera    84 B  reference include/geometric.cuh:67-69   (CudaCamera)
 *   image    W*H*3 float32, row-major, row 0 = top, linear RGB mean radiance
 *            (reference src/pt_cu.cu:30,248)
 *
 * The fields of a material (base_color, roughness, metallic, eta) and of a light (pos, dir,
 * illum, cutoff, is_parallel, light_ball.center and light_ball.r) are NOT validated: any bit
 * pattern is accepted, and the image is what the reference's expressions give on those values,
 * bit for bit -- NaN, infinities, negative and denormal values and -0.0 included, a zero or
 * non-finite `dir` (normalize divides by its length all the same), a radius of 0 (the area pdf
 * 1 / (n * 4 pi r^2) is then infinite and the sample is dropped by the colour guard), and a
 * light whose light_ball.center differs from its pos (the closest-hit scan uses the ball; the
 * light-hit shell test and the next-event sample use pos, as the reference does).  The
 * per-scene tables the library derives from these fields (material class, GGX width, light
 * area, pdf, cos(cutoff), normalised directions) are the reference's per-hit expressions on the
 * same operands.  No call fails or faults because of such values: hpt_scene_create,
 * hpt_scene_update_rounds and every render return HPT_OK for them.  Nothing is rejected either:
 * a caller who wants ordinary materials checks them itself.  (tests/shade_cases.py is the table
 * of values this is tested on; DESIGN.md, "Hostile material and light records".)
 *
 * What each entry point replaces in the reference:
 *
 *   hpt_pt_render_wrapper     pt_render_wrapper, include/pt_cu.cuh:6-13 (defined
 *                             src/pt_cu.cu:255-297): alloc + upload + render + download
 *                             in one blocking call.  include/hpt_reference_api.hpp
 *                             declares the C++-linkage adapter of the same name.
 *   hpt_scene_create/destroy  the per-call cudaMalloc/cudaMemcpy/cudaFree of the scene,
 *                             src/pt_cu.cu:270-278,292-296, hoisted so a caller that
 *                             renders repeatedly (reference src/main.cpp:416) uploads and
 *                             builds the BVH once.
 *   hpt_render_pt             cuda_path_trace_kernel launch + D2H, src/pt_cu.cu:282-290.
 *   hpt_render_pt_device      same, leaving the result in device memory on a caller
 *                             stream (no reference equivalent; used for multi-GPU tiling
 *                             and for timing with inputs resident in HBM).
 *
 * All functions return 0 on success, non-zero on error; hpt_last_error() describes the
 * last error of the calling thread.  Calls on one scene handle are not re-entrant.
 */
#ifndef HPT_H
#define HPT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HPT_OK 0
#define HPT_ERR_INVALID 1
#define HPT_ERR_DEVICE 2
#define HPT_ERR_NOMEM 3

#define HPT_LIGHT_BYTES 144
#define HPT_SPHERE_BYTES 100
#define HPT_TRIANGLE_BYTES 120
#define HPT_CAMERA_BYTES 84

typedef struct hpt_scene hpt_scene;

/* Render parameters that the reference fixes at compile time or leaves to the clock. */
typedef struct hpt_params {
    uint64_t seed;            /* RNG stream key (the reference seeds cuRAND from time(NULL), pt_cu.cu:282) */
    int32_t sample_offset;    /* global index of this call's first sample (progressive rendering) */
    int32_t max_delta;        /* cap on free delta bounces per sample (reference: uncapped, pt_cu.cu:228); 0 -> 64 */
    int32_t rank;             /* image-tile partition: this device renders tiles t with t % world == rank */
    int32_t world;            /* number of devices sharing the image; 0 or 1 -> whole image */
    int32_t tile;             /* tile edge in pixels, multiple of 8; 0 -> 32 */
    int32_t samples_per_pass; /* samples of every local pixel in flight at once; 0 -> auto */
    int32_t flags;            /* HPT_FLAG_*; any other bit: HPT_ERR_INVALID */
    int32_t reserved;         /* bits 1-6 (testing and tuning): node steps a PT ray gets in the first trace launch
                               * before it is set aside for the resume launch; 0 = default, 63 = no split.  Every
                               * other bit must be zero (HPT_ERR_INVALID) */
} hpt_params;

#define HPT_FLAG_BRUTE_FORCE 1   /* scan every primitive instead of the BVH (tests) */
#define HPT_FLAG_COUNT_WORK 2    /* count BVH boxes/triangles tested (slower; fills hpt_stats) */
#define HPT_FLAG_OUTPUT_SUM 4    /* leave the per-pixel sum over this call's samples, not the mean */
#define HPT_FLAG_TIME_KERNELS 8  /* bracket every kernel launch with HIP events (fills hpt_stats.ms_*) */
#define HPT_FLAG_RUSSIAN_ROULETTE 16 /* PT: unbiased roulette after every non-delta bounce, survival
                                      * q = clamp(max throughput channel, 0.05, 1).  The reference has no
                                      * roulette: off by default; it costs one extra uniform per
                                      * bounce, so images differ from the roulette-free ones sample by sample */
#define HPT_FLAG_SINGLE_PIPELINE 32 /* PT: one pass in flight at a time (default: two passes of a render run
                                      * concurrently on two streams with a workspace each; same image) */
#define HPT_FLAG_NO_HOST_WAIT 64    /* hpt_render_pt_device / hpt_render_bdpt_device never wait for the device.  Every
                                      * iteration up to eye_depth + max_delta is enqueued whether or not a path is still
                                      * alive; the iterations past eye_depth get small fixed grids (8 workgroups per CU;
                                      * the trace, resume and shade kernels of the PT path and the extend, connect and
                                      * reduce kernels of the BDPT path walk their queues with a stride; k_bdpt_vertex keeps
                                      * its one-chunk-per-workgroup grid, whose workgroups return at once on an empty
                                      * queue), so an iteration that finds its queue empty costs a few microseconds per
                                      * launch: config 3 with the default max_delta of 64, of which it needs 4, renders
                                      * in the same 131 ms either way.  What it costs is a fixed ~200 (PT) / ~260 (BDPT)
                                      * launches per pass, i.e. about a millisecond on a render of a few milliseconds --
                                      * hence opt-in; the default looks at a 4-byte counter every other tail iteration.
                                      * Same image */

/* Statistics of the LAST render on the scene, whichever integrator it was; every render starts them from zero.
 *   always             ms_total, and the scene constants bvh_nodes, bvh_depth, n_tris, n_materials, ms_bvh_build and
 *                      ms_upload, which change only with hpt_scene_rebuild
 *   hpt_render_pt*     split_budget, traced_rays_last_pass, long_rays_last_pass; with COUNT_WORK samples, closest_rays,
 *                      shadow_rays, path_iters, boxes_*, tris_*, lane_steps_*, wave_steps_*, leaf_*; with TIME_KERNELS
 *                      ms_extend .. ms_other, ms_resume and the launch counts n_*
 *   hpt_render_bdpt*   with COUNT_WORK bd_*; with TIME_KERNELS ms_extend .. ms_other and n_extend .. n_other
 *   hpt_render_ppm, hpt_sppm_render, hpt_render_guides
 *                      nothing else: every other field is zero (their counts and phase times are in hpt_ppm_stats)
 * A field no row names for the last render is zero. */
typedef struct hpt_stats {
    uint64_t samples;         /* camera samples traced by the last render (PT with COUNT_WORK) */
    uint64_t closest_rays;    /* closest-hit rays */
    uint64_t shadow_rays;     /* any-hit rays */
    uint64_t boxes_closest;   /* child boxes slab-tested by closest-hit rays (2 per inner node); COUNT_WORK only */
    uint64_t tris_closest;    /* triangle tests by closest-hit rays; COUNT_WORK only */
    uint64_t boxes_shadow;    /* same, any-hit rays */
    uint64_t tris_shadow;
    uint64_t path_iters;      /* (path, bounce) shading steps */
    double ms_total;          /* device time first-to-last kernel of the last render (HIP events) */
    double ms_extend, ms_shade, ms_connect, ms_other;   /* per-kernel-class sums; TIME_KERNELS only */
    uint32_t n_extend, n_shade, n_connect, n_other;     /* launches per class */
    uint32_t bvh_nodes, bvh_depth, n_tris, n_materials;
    double ms_bvh_build, ms_upload;
    /* SIMD efficiency of the traversal loops (COUNT_WORK only): lane_steps = loop trips summed over
     * lanes, wave_steps = 64 x the longest lane's trips summed over the wave's rays */
    uint64_t lane_steps_closest, wave_steps_closest, lane_steps_shadow, wave_steps_shadow;   /* inner-node trips */
    uint64_t leaf_lane_closest, leaf_wave_closest, leaf_lane_shadow, leaf_wave_shadow;       /* leaf trips */
    /* split trace step: the first launch gives every ray split_budget node steps, the second (resume)
     * launch finishes the rays that needed more */
    double ms_resume;                 /* resume launches; TIME_KERNELS only (ms_extend / ms_connect then hold the first launches) */
    uint32_t n_resume, split_budget;  /* split_budget 0: single-launch trace steps */
    uint64_t traced_rays_last_pass, long_rays_last_pass;   /* rays entering the trace steps of the last pass / set aside for resume */
    /* connection stage of a bidirectional render (COUNT_WORK only; reference loop src/cpu_bdpt.cpp:387-440): candidate (eye vertex,
     * light vertex) pairs, pairs that pass the culls (zero throughput, distance, cosines, emission cone), shadow rays traced (both
     * BSDF values non-zero), unoccluded ones; and the work of those shadow rays: BVH nodes visited (64 B each), triangle, sphere
     * and group-box tests */
    uint64_t bd_pairs, bd_survivors, bd_shadow_rays, bd_unoccluded, bd_nodes, bd_tris, bd_spheres, bd_group_boxes;
} hpt_stats;

const char *hpt_last_error(void);

/* Number of visible HIP devices (<0 on error). */
int hpt_device_count(void);

/* Flattens the reference records into the device layout, builds the BVH on the host and
 * uploads everything to the current HIP device.  Records are copied; the caller keeps
 * ownership of its arrays. */
int hpt_scene_create(const void *lights, int num_lights,
                     const void *spheres, int num_spheres,
                     const void *triangles, int num_triangles,
                     hpt_scene **out_scene);
void hpt_scene_destroy(hpt_scene *scene);

/* Number of float3 slots of the packed local framebuffer for this (W, H, params) -- the
 * size hpt_render_pt_device writes and hpt_untile reads per rank. */
int64_t hpt_local_pixels(int W, int H, const hpt_params *params);

/* Blocking render into a caller-owned host image of W*H*3 floats (whole image:
 * params->world must be 0 or 1). */
int hpt_render_pt(hpt_scene *scene, const void *camera, int W, int H,
                  int eye_depth, int spp, const hpt_params *params, float *host_image);

/* Render of this rank's tiles into device memory: d_local holds hpt_local_pixels() float3 records in local
 * tile order.  Everything is enqueued on hip_stream (plus one stream of the scene, joined back before the
 * call returns); the result is complete when the stream reaches the end of what the call enqueued.  The call
 * returns without waiting for the device as long as no path outlives eye_depth iterations; paths kept alive by
 * free delta bounces (mirror, glass: reference src/pt_cu.cu:228) need further iterations whose number only the
 * device knows, and for those the calling thread waits on a 4-byte read-back every other iteration -- i.e. on
 * scenes with delta materials the call MAY BLOCK THE HOST for most of the render's duration.  It never blocks
 * the device: both pipelines of a render keep running while the host waits.  With HPT_FLAG_NO_HOST_WAIT the call
 * only enqueues (blind launches instead of read-backs).
 * Work on one scene is ordered only by the streams the caller passes, and every blocking entry point uses the null
 * stream.  Before a call on the same scene that uses another stream, the caller waits for the earlier one. */
int hpt_render_pt_device(hpt_scene *scene, const void *camera, int W, int H,
                         int eye_depth, int spp, const hpt_params *params,
                         void *d_local, void *hip_stream);

/* Scatters `world` packed local framebuffers, laid out [rank][local pixel] in d_gathered,
 * into the row-major W*H image d_image (both device pointers). */
int hpt_untile(const void *d_gathered, void *d_image, int W, int H,
               const hpt_params *params, void *hip_stream);

/* One-shot equivalent of the reference's pt_render_wrapper (include/pt_cu.cuh:6-13):
 * scene_min/scene_max/light_depth/light_sample are accepted and ignored there too
 * (src/pt_cu.cu:259-262).  seed < 0 -> seed from the clock like the reference.
 *
 * The reference uploads the scene and allocates its buffers on every call (src/pt_cu.cu:270-296), and
 * its interactive front-end calls the wrapper once per frame (src/main.cpp:416).  Here the two one-shot
 * wrappers keep the last scene (device records, BVH, workspace) and reuse it when the next call on the
 * same device passes byte-identical light/sphere/triangle arrays; anything else rebuilds.  The images
 * are the same either way.  hpt_wrapper_cache_clear() releases the kept scene; HPT_WRAPPER_CACHE=0 in
 * the environment switches the reuse off. */
void hpt_wrapper_cache_clear(void);
int hpt_pt_render_wrapper(const void *lights, int num_lights,
                          const void *spheres, int num_spheres,
                          const void *triangles, int num_triangles,
                          const float scene_min[3], const float scene_max[3],
                          const void *camera, float *host_image, int W, int H,
                          int light_depth, int light_sample, int eye_depth, int spp,
                          int64_t seed);

/* ---- bidirectional estimator of the reference's CPU renderer ------------------------------------
 * Replaces bdpt_render_wrapper (reference include/bdpt_cu.cuh:30-37, src/bdpt_cu.cu:538-674) and
 * run_cuda_bdpt (include/bdpt_cu_helper.h:6).  What is computed follows run_cpu_bdpt (reference
 * src/cpu_bdpt.cpp:173-488) wherever it and the CUDA BDPT kernel disagree: the CPU scene
 * model with its one-level group boxes, nl*spl light subpaths carrying illum/spl, every eye vertex
 * connected to every light vertex with the ratio-sum MIS weight.
 *
 * hpt_scene_set_groups hands over the scene file's grouping (kind 0 sphere / 1 triangle, index into
 * the arrays given to hpt_scene_create, group id; insertion order), which decides tie-breaks and the
 * per-group box culls of the CPU model.  Without it: one group, spheres then triangles. */
int hpt_scene_set_groups(hpt_scene *scene, const int32_t *obj_kind, const int32_t *obj_index,
                         const int32_t *obj_group, int num_objects);
int hpt_render_bdpt(hpt_scene *scene, const void *camera, int W, int H, int eye_depth, int light_depth,
                    int spp, int spl, const hpt_params *params, float *host_image);
int hpt_render_bdpt_device(hpt_scene *scene, const void *camera, int W, int H, int eye_depth, int light_depth,
                           int spp, int spl, const hpt_params *params, void *d_local, void *hip_stream);
/* One-shot, argument list of the reference's bdpt_render_wrapper; the lights arrive with illum already
 * divided by light_sample (reference src/bdpt_cu_helper.cpp:60-62), which is undone here. */
int hpt_bdpt_render_wrapper(const void *lights, int num_lights, const void *spheres, int num_spheres,
                            const void *triangles, int num_triangles,
                            const float scene_min[3], const float scene_max[3],
                            const void *camera, float *host_image, int W, int H,
                            int light_depth, int light_sample, int eye_depth, int spp, int spl, int64_t seed);

int hpt_get_stats(const hpt_scene *scene, hpt_stats *out);

/* ---- photon mapping (the reference's PPM integrator) ----------------------------------------------
 * Replaces ppm_render_wrapper (reference include/ppm_cu.cuh:8-15, src/ppm_cu.cu:328-400) and run_cuda_ppm
 * (include/ppm_cu_helper.h).  One pass = an eye pass (a hit point at the first non-delta surface of every pixel,
 * the direct term where a light ball is reached through delta bounces), nl * spl photons of light_depth
 * non-delta bounces each, and for every hit point the sum of flux * f(wo, wi) * throughput over the photon
 * deposits within `radius` (normals agreeing), divided by pi r^2 and clamped to 15.  The reference's float-atomic
 * scatter is replaced by a gather in a fixed order ("PPM"), so an image is a function of the seed.
 * `spp` passes are independent and averaged (HPT_FLAG_OUTPUT_SUM: summed).  eye_depth only has to be >= 1: the
 * eye path ends at its first non-delta hit, delta bounces are free (capped at hpt_params.max_delta) as in the
 * reference.  radius <= 0 -> 0.05 (the reference's PPM_RADIUS; the grid cell is the radius).  scene_min /
 * scene_max NULL -> the scene's bounds as the reference's helper computes them (spheres +- r, triangle vertices,
 * no light balls).  PPM renders on ONE device: params->world must be 0 or 1, and the multi-device fan-out
 * (hpt_multi_*, hpt_wrapper_set_devices) stays PT/BDPT only.  Accepted flags: OUTPUT_SUM, TIME_KERNELS,
 * COUNT_WORK; any other flag, spl < 0, or depths outside [1, 255] return HPT_ERR_INVALID; nl * spl *
 * light_depth deposits that do not fit the device return HPT_ERR_NOMEM (nothing is batched). */
int hpt_render_ppm(hpt_scene *scene, const void *camera, int W, int H, int eye_depth, int light_depth,
                   int spp, int spl, float radius, const float *scene_min, const float *scene_max,
                   const hpt_params *params, float *host_image);

typedef struct hpt_ppm_stats {
    uint64_t photons;         /* photons emitted (all passes of the last render) */
    uint64_t photon_rays;     /* closest-hit rays of the photon paths */
    uint64_t deposits;        /* live photon deposits */
    uint64_t hit_points;      /* eye hit points */
    uint64_t direct_pixels;   /* pixels whose eye path reached a light ball (direct term written) */
    uint64_t candidates;      /* COUNT_WORK: (hit point, deposit) pairs in the 27 cells, exact cell match */
    uint64_t accepted;        /* COUNT_WORK: of those, normals agree and distance < radius */
    uint64_t cand_median, cand_max, acc_median, acc_max;   /* COUNT_WORK: per hit point, last pass */
    uint64_t grid_buckets;    /* bucket table size (power of two) */
    double ms_eye, ms_photon, ms_grid, ms_gather;          /* TIME_KERNELS: device time per phase, all passes */
    double ms_total;          /* device time of the last render */
} hpt_ppm_stats;
int hpt_ppm_get_stats(const hpt_scene *scene, hpt_ppm_stats *out);

/* One-shot, the reference's ppm_render_wrapper argument list plus seed (< 0: clock).  ONE pass whatever spp is
 * (the reference never reads it); scene_min / scene_max are used as given; the scene is kept between calls like
 * the other wrappers' (hpt_wrapper_cache_clear).  Always one device. */
int hpt_ppm_render_wrapper(const void *lights, int num_lights, const void *spheres, int num_spheres,
                           const void *triangles, int num_triangles,
                           const float scene_min[3], const float scene_max[3],
                           const void *camera, float *host_image, int W, int H,
                           int light_depth, int light_sample, int eye_depth, int spp, int64_t seed);

/* ---- progressive photon mapping (per-pixel shrinking radius) ----------------------------------------
 * The progressive step of Hachisuka & Jensen's photon mapping, whose statistics the reference's hit-point record
 * carries (radius2, photon_count, accum_flux in src/ppm_cu.cu) but never uses.  A state holds, per pixel i:
 * R2_i (starts at radius^2), N_i (0), tau_i (0, flux) and D_i (0, the sum of direct terms); K counts the passes.
 * Pass K has the global index sample_offset + K; its eye pass, photons, deposits and grid are those of
 * hpt_render_ppm's pass of that index, with the grid cell = the initial radius for the whole life of the state.
 *   gather   at pixel i's hit point, PPM's cells in PPM's order, a deposit accepted when its cell matches, the
 *            normals agree (> 0.01) and |h - p|^2 < R2_i; for each accepted deposit whose BSDF value f is a valid
 *            colour: Phi += flux * f * throughput, M += 1.  Cells no deposit within R_i can lie in are skipped
 *            ("Progressive photon mapping"): the result is the same bits.
 *   update   pixels with a hit point and M > 0: n = N + alpha M, ratio = n / (N + M), R2 *= ratio,
 *            tau = (tau + Phi) * ratio, N = n.  alpha = 1 keeps the radius (ratio is exactly 1).
 *   direct   D += the direct term of the eye pass (k_resolve's guard).
 *   estimate d = D, p = tau / max(pi R2, 1e-6), both divided by K unless K = 1;
 *            pixel = p a valid colour ? d + clamp(p, 15) : d.
 * One pass with alpha = 1 gives the bytes of hpt_render_ppm with spp = 1 (same seed, offset and radius).
 *
 * hpt_sppm_create takes seed, sample_offset, max_delta and tile from params (flags must be 0, reserved 0, world
 * 0 or 1); radius <= 0 -> 0.05; scene_min / scene_max NULL -> the scene's bounds as for hpt_render_ppm.  alpha
 * outside (0, 1], spl < 0 or depths outside [1, 255] return HPT_ERR_INVALID.  The state lives on the scene's device
 * and the scene must outlive it; renders of any kind on the scene in between do not touch it.
 * hpt_sppm_render advances the state by `passes` (> 0) passes and writes the estimate (W*H*3 floats, row-major)
 * into host_image; flags may hold HPT_FLAG_TIME_KERNELS and HPT_FLAG_COUNT_WORK only, and the scene's
 * hpt_ppm_stats then describe this call (candidates: the pairs examined in the cells visited).  hpt_sppm_reset
 * returns to K = 0 (R2, N, tau and D as at creation) and, where the state was created with scene_min or scene_max NULL,
 * takes that bound from the scene again, as it is now: after a scene update a reset state is a state freshly created
 * on the new scene.  Bounds the caller gave stay as given.  hpt_sppm_read_state copies R2 and N (W*H floats each,
 * row-major; either may be NULL) and K. */
typedef struct hpt_sppm hpt_sppm;
int hpt_sppm_create(hpt_scene *scene, const void *camera, int W, int H, int eye_depth, int light_depth, int spl,
                    float radius, float alpha, const float *scene_min, const float *scene_max,
                    const hpt_params *params, hpt_sppm **out);
int hpt_sppm_render(hpt_sppm *state, int passes, int32_t flags, float *host_image);
int hpt_sppm_reset(hpt_sppm *state);
int hpt_sppm_read_state(const hpt_sppm *state, float *radius2, float *photons, int64_t *passes);
void hpt_sppm_destroy(hpt_sppm *state);

/* ---- multi-device fan-out inside the blocking call -----------------------------------------------
 * The reference's launch API is one blocking call per frame (run_cuda_pt -> pt_render_wrapper, reference
 * src/pt_cu_helper.cpp:66-77, src/pt_cu.cu:255-297, one device).  hpt_multi_* is the same call over the
 * devices of one node, in ONE process: the scene is flattened and its BVH built once and uploaded to every
 * device; every device renders its image tiles (hpt_params.rank/world are set internally) on its own
 * stream, driven by its own host thread; the packed local framebuffers are gathered on device_ids[0] with
 * one ncclGather per device inside one RCCL group (librccl.so is dlopen'ed on first use; each sender uses
 * its own xGMI link to the root), un-tiled there and copied to host_image.  The image is bit-identical to
 * hpt_render_pt's for any number of devices.
 *   device_ids   num_devices HIP device ordinals, NULL = 0 .. num_devices-1; num_devices <= 0 = all visible
 *   exchange     0 = RCCL (distinct devices; fails if RCCL cannot be loaded or initialised)
 *                1 = hipMemcpyPeerAsync into the root's buffer (boxes without RCCL; tests that place
 *                    several ranks on one device, which an RCCL communicator refuses)
 * hpt_wrapper_set_devices(n) (or HPT_DEVICES=n in the environment, read once) makes the two one-shot
 * wrappers -- hence the reference's unmodified run_cuda_pt / run_cuda_bdpt -- render on n devices this way;
 * 0 returns to the environment's value, 1 to a single device.  Photon mapping (hpt_render_ppm,
 * hpt_ppm_render_wrapper) always renders on one device. */
typedef struct hpt_multi hpt_multi;
int hpt_multi_create(const void *lights, int num_lights, const void *spheres, int num_spheres,
                     const void *triangles, int num_triangles,
                     const int *device_ids, int num_devices, int exchange, hpt_multi **out);
void hpt_multi_destroy(hpt_multi *multi);
int hpt_multi_num_devices(const hpt_multi *multi);
int hpt_multi_set_groups(hpt_multi *multi, const int32_t *obj_kind, const int32_t *obj_index,
                         const int32_t *obj_group, int num_objects);
int hpt_multi_render_pt(hpt_multi *multi, const void *camera, int W, int H, int eye_depth, int spp,
                        const hpt_params *params, float *host_image);
int hpt_multi_render_bdpt(hpt_multi *multi, const void *camera, int W, int H, int eye_depth, int light_depth,
                          int spp, int spl, const hpt_params *params, float *host_image);
/* device time of every rank's render (HIP events), of the exchange step, and host wall time of the last call */
int hpt_multi_get_timing(const hpt_multi *multi, double *render_ms_per_device, double *gather_ms, double *total_ms);
int hpt_wrapper_set_devices(int num_devices);

/* Function-level probe of the device BSDF code (tests): evaluates, for n caller-given records, the
 * device versions of bsdf_evaluate / bsdf_pdf / bsdf_sample, FrDielectric, FrSchlick, the GGX D / Lambda / G terms,
 * the visible-normal sample, the local frame, sin/cos(2 pi u), is_valid_color and clamp_radiance (reference
 * include/geometric.cuh:119-235, 419-562) exactly as the shading kernel calls them.  24 floats in and 40 floats out per
 * record; the layout is documented at k_probe_functions (path_tracing_amd/csrc/pt_frame.hip) and mirrored by
 * oracle_function_kats (oracle/pt_oracle.cpp). */
int hpt_probe_functions(const float *records_in, int n, float *results_out);

/* ---- 8-bit output stage on the device -------------------------------------------------------------
 * Replaces the per-pixel loop of the reference CLI, src/main_cli.cpp:225-242: per channel clamp to [0, 1],
 * pow(x, 1/2.2), x 255, truncate.  The device looks the byte up in a table of 255 thresholds that the host
 * computes with its own powf, so the bytes are exactly those of the host loop (hpt_tonemap_reference runs
 * that loop; hpt_tonemap_table returns thresholds[k] = the smallest float whose byte is >= k, [0] = -inf).
 *   d_linear_rgb  3 floats per pixel (the image hpt_untile / hpt_render_* produce), device memory
 *   d_rgb8        3 bytes per pixel, device memory, 4-byte aligned
 *   bgr           non-zero: the reference's cv::Vec3b order (B, G, R); zero: R, G, B
 * hpt_tonemap_host takes and returns host buffers (upload, kernel, download). */
int hpt_tonemap(const void *d_linear_rgb, void *d_rgb8, int64_t num_pixels, int bgr, void *hip_stream);
int hpt_tonemap_host(const float *linear_rgb, unsigned char *rgb8, int64_t num_pixels, int bgr);
void hpt_tonemap_table(float thresholds_out[256]);
void hpt_tonemap_reference(const float *linear_rgb, unsigned char *rgb8, int64_t num_pixels, int bgr);

/* ---- guides and denoiser ----------------------------------------------------------------------------
 * The reference's GUI renders 8 spp per frame and throws its accumulation away whenever the camera moves
 * (src/main.cpp:406-466); it has no denoiser.  These calls add the standard two steps for such sample counts:
 * cheap noise-free guide images of the first rough surface behind every pixel, and an edge-avoiding a-trous wavelet
 * filter (Dammertz et al. 2010) over the noisy radiance, steered by them.  The position and normal guides also steer
 * hpt_history ("history across camera moves", below), which keeps the accumulation when the camera moves.
 *
 * hpt_render_guides: for sample s = 0 .. spp-1, photon mapping's eye pass of pass index (low 32 bits of)
 * sample_offset + s -- streams (seed ^ eye key, pixel, pass), jitter, free delta bounces capped at max_delta, all as
 * in hpt_render_ppm's pass of that index.  A pixel whose pass ends in a hit point (the first non-delta surface) adds
 * the hit material's base colour to A, the ray-facing normal to N, the position to P and one to C, float adds in
 * sample order; pixels that end on a light ball, miss or die add nothing.  Then albedo = A / (float) C, normal =
 * N / (float) C, position = P / (float) C per channel (all zero where C = 0) and coverage = (float) C.  The normal is
 * NOT renormalised: a pixel that straddles an edge gets a shorter normal, which lowers its weight across the edge.
 * Outputs are host images, row-major, row 0 = top: W*H*3 floats (coverage: W*H); any may be NULL, not all four.
 * params: seed, sample_offset, max_delta and tile as for hpt_render_ppm; world other than 0 or 1, a non-zero
 * reserved, any flag but HPT_FLAG_TIME_KERNELS, or spp < 1 return HPT_ERR_INVALID.  One device.  hpt_ppm_stats
 * afterwards holds hit_points and direct_pixels of the call and, under TIME_KERNELS, ms_eye.
 *
 * The filter.  valid(p): coverage[p] > 0.  a(p) = max(albedo[p], 1e-3f) per channel.  c_0(p) = colour[p] / a(p) with
 * HPT_DENOISE_DEMODULATE (valid pixels), else colour[p].  Taps h = {1/16, 1/4, 3/8, 1/4, 1/16}.  Falloff
 * e(x) = q^8, q = fmaxf(0, 1 - x * 0.125f), by three squarings: a polynomial stand-in for exp(-x) (the library calls
 * no device transcendental on a path that is compared bit for bit) with compact support, e(x) = 0 exactly for x >= 8.
 * Level k = 0 .. iterations-1, stride s = 2^k; sc = sigma_color * 2^-k; inv_c = inv(sc), inv_n = inv(sigma_normal),
 * inv_p = inv(sigma_position) with inv(s) = fminf(1.0f / (s * s), FLT_MAX), computed in float on the host.  The clamp acts
 * where s * s is so small (a denormal, or 0) that the quotient is inf: unclamped, the centre tap's x = 0 * inf would be
 * NaN and its weight 0.  With FLT_MAX the centre weighs 9/64 as always and another tap takes part only where its
 * difference squares to (almost) zero, which is the limit of the definition.  A sigma so large that s * s overflows
 * gives inv = 0, every x = 0 and e = 1: the term is as good as off.  An invalid pixel keeps its value.  For a valid p = (x, y):
 * for j = -2..2 (outer), i = -2..2 (inner), q = (x + i s, y + j s), skipped when outside the image or invalid:
 *   xc = (dc.x dc.x + dc.y dc.y + dc.z dc.z) * inv_c with dc = c_k(p) - c_k(q);  xn likewise from normal[p] - normal[q];
 *   t = n(p).x d.x + n(p).y d.y + n(p).z d.z with d = position[q] - position[p] (q's distance from p's tangent plane),
 *   xp = t * t * inv_p;   w = h[j+2] * h[i+2] * e(xc) * e(xn) * e(xp), left to right (a term switched off is 1.0f);
 *   sum += c_k(q) * w per channel, wsum += w;   c_{k+1}(p) = sum / wsum.  The centre tap has x = 0 in every term at every
 *   sigma > 0 (inv is finite), so wsum >= 9/64.
 *   A valid pixel whose 24 other taps are all skipped keeps its value, c_{k+1}(p) = c_k(p): fl(fl(c * 9/64) / (9/64))
 *   is not c for every float, and a level whose stride exceeds the image must hand its input on unchanged.
 * Output c_n(p) * a(p) with DEMODULATE, else c_n(p); an invalid pixel outputs colour[p] exactly.  The tap order is part
 * of the definition; everything is IEEE float, evaluated as written.  Inputs are expected to be finite.
 *
 * hpt_denoiser_create allocates, on the current device, the packed guides and two colour buffers of a W x H image
 * (80 bytes per pixel).  hpt_denoiser_set_guides packs four DEVICE images with the layouts of hpt_render_guides; they
 * stay set for every later run (the GUI sets them when the camera moves and runs once per frame).  hpt_denoiser_run
 * filters d_linear_rgb into d_out (device, W*H*3 floats each, not overlapping); both calls only enqueue on
 * hip_stream, so they compose with hpt_untile before and hpt_tonemap after.  p NULL = all defaults.  Run before
 * set_guides, iterations outside [0, 8], an unknown flag, a NaN sigma or overlapping images return HPT_ERR_INVALID.
 * With HPT_DENOISE_TIME the run is bracketed by HIP events: hpt_denoiser_last_ms waits for it and returns the time of
 * the colour pack and of all levels, hpt_denoiser_level_ms the first `cap` levels' own times (0 past the last level).
 * hpt_denoise_host takes and returns host images (upload, set_guides, run, download). */
typedef struct hpt_denoise_params {
    int32_t iterations;     /* levels, 1..8; 0 -> 5.  Level k samples at stride 2^k */
    float sigma_color;      /* 0 -> 1.0;  < 0 -> colour term off (weight 1) */
    float sigma_normal;     /* 0 -> 0.5;  < 0 -> off */
    float sigma_position;   /* 0 -> 0.05 (the library's one absolute length default, PPM's radius); < 0 -> off */
    int32_t flags;          /* HPT_DENOISE_*; other bits: HPT_ERR_INVALID */
} hpt_denoise_params;
#define HPT_DENOISE_DEMODULATE 1
#define HPT_DENOISE_TIME 2

int hpt_render_guides(hpt_scene *scene, const void *camera, int W, int H, int spp,
                      const hpt_params *params,
                      float *albedo, float *normal, float *position, float *coverage);
/* The same call with four DEVICE output images (any may be NULL, not all four): the same bytes, left on the scene's
 * device; the call returns when they are complete.  A viewer that moves its camera every frame hands them to
 * hpt_history_advance and never brings 40 bytes per pixel to the host and back. */
int hpt_render_guides_device(hpt_scene *scene, const void *camera, int W, int H, int spp,
                             const hpt_params *params,
                             void *d_albedo, void *d_normal, void *d_position, void *d_coverage);

typedef struct hpt_denoiser hpt_denoiser;
int hpt_denoiser_create(int W, int H, hpt_denoiser **out);
int hpt_denoiser_set_guides(hpt_denoiser *d, const void *d_albedo, const void *d_normal,
                            const void *d_position, const void *d_coverage, void *hip_stream);
int hpt_denoiser_run(hpt_denoiser *d, const void *d_linear_rgb, void *d_out,
                     const hpt_denoise_params *p, void *hip_stream);
int hpt_denoiser_last_ms(const hpt_denoiser *d, double *ms_pack, double *ms_filter);
int hpt_denoiser_level_ms(const hpt_denoiser *d, double *ms_levels, int cap);
void hpt_denoiser_destroy(hpt_denoiser *d);
int hpt_denoise_host(const float *linear_rgb, const float *albedo, const float *normal, const float *position,
                     const float *coverage, float *out, int W, int H, const hpt_denoise_params *p);

/* ---- progressive display ----------------------------------------------------------------------------
 * The reference's GUI renders a few samples per frame and, after every frame, runs a host loop over every pixel and
 * channel (src/main.cpp:421-531): running average, clamp / pow(1/2.2) / truncate, row flip into a three-panel
 * framebuffer, and the squared byte differences it plots as "RMS history".  These two objects keep that state on the
 * device, so a frame is hpt_render_*_device, hpt_untile, hpt_accum_add, hpt_display_present on one stream and only
 * two 64-bit sums come back.
 *
 * All images are W*H*3 floats, row-major, row 0 = top, in device memory (the layout hpt_untile writes).  IEEE float,
 * evaluated as written, per value v of the frame:
 *   add       sum = sum + v; with HPT_ACCUM_MOMENTS also sq = sq + v * v.  K, the frame count, is a host counter that
 *             is incremented when the call is enqueued.  d_mean_out, when not NULL, receives sum / (float) K (the
 *             division happens at K = 1 too, as in main.cpp:470); it may be d_frame_rgb itself (in place), any other
 *             overlap of the two is refused.
 *   mean      sum / (float) K; K = 0 returns HPT_ERR_INVALID.
 *   variance  the variance of the MEAN, needs HPT_ACCUM_MOMENTS.  K < 2: all zeros.  Otherwise m = sum / (float) K;
 *             q = sq / (float) K; d = q - m * m; out = fmaxf(d, 0.0f) / (float) (K - 1).  Good for what a progressive
 *             viewer asks of it: Monte-Carlo noise over tens of frames, whose relative variance is 1e-4 and up.  NOT a
 *             general-purpose variance: q and m * m are rounded floats of nearly equal size, so below a relative
 *             variance of about 1e-7 (2^-23) their difference is rounding, not signal (a constant frame gives exactly 0).
 *   reset     zeroes the sums on the stream and sets K = 0; the reference's restart when the camera moves
 *             (main.cpp:453-466) is reset followed by add (hpt_history, below, carries the mean over instead).
 * Every call only enqueues on hip_stream, except hpt_accum_read, which waits for the device and copies the sums to
 * the host (for tests; either image may be NULL).  hpt_accum_create allocates on the current device, sums zeroed.
 * W or H below 1 (or W*H above 2^28), an unknown flag, variance (or a sumsq read) without MOMENTS, a NULL handle, a
 * NULL frame or output, and more than 2^24 adds -- (float) K stops being exact -- return HPT_ERR_INVALID with a
 * message, before anything touches the device. */
#define HPT_ACCUM_MOMENTS 1          /* also keep the per-channel sum of squares */
typedef struct hpt_accum hpt_accum;
int  hpt_accum_create(int W, int H, int32_t flags, hpt_accum **out);
int  hpt_accum_add(hpt_accum *a, const void *d_frame_rgb, void *d_mean_out, void *hip_stream);
int  hpt_accum_mean(hpt_accum *a, void *d_out, void *hip_stream);
int  hpt_accum_variance(hpt_accum *a, void *d_out, void *hip_stream);
int  hpt_accum_reset(hpt_accum *a, void *hip_stream);
int64_t hpt_accum_count(const hpt_accum *a);
int  hpt_accum_read(hpt_accum *a, float *sum, float *sumsq, int64_t *count);
void hpt_accum_destroy(hpt_accum *a);

/* hpt_display_present, the P-th call (P counts from 0), in one launch:
 *   b[r][x][c] = the byte of d_linear_rgb[(r*W + x)*3 + c] under hpt_tonemap's threshold table, i.e. the bytes of
 *                hpt_tonemap_reference(..., bgr = 0): NaN gives 0, anything >= 1 gives 255.
 *   ssd_prev   = the sum over all 3*W*H values of (b - last)^2; 0 when P = 0 (the reference's is_first).
 *   ssd_other  = the same sum against other's `last` (the reference's PPM-BDPT "DIFF RMS"); 0 when other is NULL.
 *                other must be a different display of the same size on the same device that has presented at least
 *                once, else HPT_ERR_INVALID.  The caller orders the two displays' work, as everywhere in this ABI.
 *   d_rgb8, when not NULL:  d_rgb8[(flip ? H-1-r : r) * pitch + x_offset + 3*x + (bgr ? 2-c : c)] = b[r][x][c].
 *                pitch_bytes = 0 means 3*W; pitch < x_offset + 3*W or x_offset < 0 return HPT_ERR_INVALID.  No
 *                alignment is asked of the pointer, the pitch or the offset, and no byte outside the panel's H runs
 *                of 3*W bytes is written, or read and written back: the three panels of one framebuffer are
 *                pitch = 9*W, x_offset = panel*3*W (main.cpp:434-437) and may be presented from different streams.
 *   then last = b and P += 1.  `last` is kept in canonical order (RGB, row 0 = top), so the metrics do not depend on flags.
 * hpt_display_metrics waits for the last present only and returns its numbers: rms = sqrt((double) ssd) / 255.0; any
 * output may be NULL; before any present (or after a reset) it returns HPT_ERR_INVALID.  The sums are exact 64-bit
 * integers, so they do not depend on grid shape, workgroup order or device.
 * Relation to the reference: main.cpp:502-530 adds powf(diff, 2) into a `float` in pixel order.  Every term is an
 * integer <= 65025, so while the sum stays at or below 2^24 every partial sum is an exact integer and the reference's
 * value equals this one; above 2^24 its float sum rounds at every step, and this is the number it approximates.
 * hpt_display_reset sets P = 0 (the next present reports ssd_prev = 0).  hpt_display_create allocates on the current device. */
#define HPT_DISPLAY_BGR    1     /* cv::Vec3b channel order in d_rgb8 */
#define HPT_DISPLAY_FLIP_Y 2     /* image row r goes to output row H-1-r (main.cpp:431) */
typedef struct hpt_display hpt_display;
int  hpt_display_create(int W, int H, hpt_display **out);
int  hpt_display_present(hpt_display *d, const void *d_linear_rgb, const hpt_display *other,
                         void *d_rgb8, int64_t pitch_bytes, int64_t x_offset_bytes, int32_t flags, void *hip_stream);
int  hpt_display_metrics(hpt_display *d, double *rms_prev, double *rms_other,
                         uint64_t *ssd_prev, uint64_t *ssd_other, int64_t *presented);
int  hpt_display_reset(hpt_display *d, void *hip_stream);
void hpt_display_destroy(hpt_display *d);

/* ---- history across camera moves ---------------------------------------------------------------------
 * The reference's GUI discards its running average whenever the camera moves (src/main.cpp:453-466), and hpt_accum can
 * only be reset the same way: every pixel starts again from one noisy frame, even where the same surface point was on
 * screen a frame ago with tens of samples behind it.  hpt_history is a per-pixel running mean that survives the move:
 * it looks up where each pixel's guide point (hpt_render_guides) was in the previous frame and carries that pixel's
 * mean and sample count over when the geometry agrees.
 *
 * Conventions as for hpt_accum / hpt_display: images are device pointers in the layouts hpt_untile and
 * hpt_render_guides write (frame, normal, position, mean: W*H*3 floats; coverage: W*H; row-major, row 0 = top);
 * advance and reset only enqueue on hip_stream; metrics and read wait for the device; create allocates on the current
 * device (96 bytes per pixel, 128 with HPT_HISTORY_MOMENTS).  Every refusal is made, with a message, before anything touches the device.
 *
 * State per pixel: mean (3 floats), history length n (float), and the last frame's guide position, normal and coverage,
 * held in two sets (a pixel reads its neighbours' previous state, so a moved frame writes the other set).  The object
 * also keeps the previous camera record and K, the number of advances since create or reset.
 *
 * Camera constants.  For a camera (eye, UL, dx, dy) the host computes, in float, evaluated as written, with
 * dot(a, b) = a.x*b.x + a.y*b.y + a.z*b.z left to right and cross(a, b) = (a.y*b.z - a.z*b.y, a.z*b.x - a.x*b.z,
 * a.x*b.y - a.y*b.x):
 *   a = UL - eye;  nrm = cross(dx, dy);  an = dot(a, nrm);
 *   cu = cross(dy, nrm);  gu = cu / dot(dx, cu) per component;   cv = cross(nrm, dx);  gv = cv / dot(dy, cv).
 * They are all the kernel reads of a camera.  A camera whose constants (eye included) are not all finite, or whose an
 * is 0, is refused.
 *   project(cam, X):  d = X - eye;  den = dot(d, nrm);  s = an / den;  r = d * s - a (per component: d.x * s - a.x);
 *                     u = dot(r, gu);  v = dot(r, gv);  dist2 = dot(d, d).
 * (u, v) is the continuous pixel coordinate under which the primary ray eye -> UL + u dx + v dy sees X, and s > 0 says
 * that X lies in front of the camera.
 *
 * hpt_history_advance, for pixel p = (x, y) with frame colour c; every comparison below is false for a NaN operand:
 *   1. K = 0: n_r = 0.
 *   2. else, the camera's 84 bytes equal the previous advance's: m = mean[p], n_r = n[p].  No test is applied, so a
 *      still camera is a plain running mean whatever the guides say.
 *   3. else, the guide pointers are NULL or coverage[p] > 0 is false: n_r = 0.
 *   4. else X = position[p], N = normal[p]:
 *      direct view   P = project(this camera, X) must give P.s > 0, |P.u - ((float) x + 0.5f)| <= 1 and
 *                    |P.v - ((float) y + 0.5f)| <= 1.  A pixel whose guide point lies behind a mirror or glass bounce
 *                    does not project onto itself: it restarts rather than inherit history from the wrong place.
 *      range         Q = project(previous camera, X) must give Q.s > 0 and, with up = Q.u - 0.5f, vp = Q.v - 0.5f:
 *                    up >= -1, up < (float) W, vp >= -1, vp < (float) H -- compared in float BEFORE any conversion to
 *                    integer, so NaN and infinity fail here and are never converted.  x0 = floorf(up), fx = up - x0,
 *                    y0 = floorf(vp), fy = vp - y0.
 *      taps          sum = (0, 0, 0), nsum = 0, wsum = 0; for j = 0, 1 (outer), i = 0, 1 (inner), q = (x0 + i, y0 + j),
 *                    skipped when q lies outside the image, when coverage_prev[q] > 0 is false, when (plane test on)
 *                    t = dot(N, position_prev[q] - X) fails t * t <= tol2 * P.dist2 with tol2 = plane_tolerance *
 *                    plane_tolerance computed on the host, or when (normal test on) dot(N, normal_prev[q]) >= normal_min
 *                    is false.  Otherwise w = (i ? fx : 1.0f - fx) * (j ? fy : 1.0f - fy); sum = sum + mean_prev[q] * w per
 *                    channel, nsum = nsum + n_prev[q] * w, wsum = wsum + w.
 *      result        wsum > 0.01f: m = sum / wsum per channel, n_r = nsum / wsum; otherwise n_r = 0 (a history held up
 *                    by a sliver of one tap is extrapolation, and 1 / wsum amplifies its rounding).
 *      Either failed test gives n_r = 0.
 *   5. n_r > 0 is false: mean = c, n = 1.  Otherwise n_c = fminf(n_r, max_history - 1) (the difference computed on the
 *      host), mean = (m * n_c + c) / (n_c + 1.0f) per channel, n = n_c + 1.0f.
 *   6. mean, n and this frame's position, normal and coverage become the pixel's previous state; with NULL guides the
 *      stored guides are kept on an unmoved camera and become coverage 0 otherwise (K = 0 or a moved camera) -- which
 *      makes a moved sequence without guides exactly the reference's restart.  d_mean_out, when not NULL, receives
 *      mean; it may be d_frame_rgb itself, any other overlap among the caller's five images is refused.  The camera is
 *      stored and K incremented when the call is enqueued.
 *   kept counts the pixels with n_r > 0, restarted those without on a frame with K > 0 (so kept + restarted = W*H on
 *   every frame but the first, where both are 0).  Both are exact 64-bit integers and do not depend on the grid.
 * The tap order is part of the definition; everything is IEEE float, evaluated as written.
 *
 * p NULL = all defaults.  The guide pointers are given all three or not at all.  hpt_history_metrics returns the counts
 * of the last advance (any output may be NULL; HPT_ERR_INVALID before the first advance and after a reset);
 * hpt_history_read copies the current mean (W*H*3) and n (W*H) to the host (either may be NULL) and K.  hpt_history_reset
 * zeroes the current state on the stream and sets K = 0.  hpt_history_check runs every argument check of an advance on a
 * W x H history without a handle or a device (a front-end can validate before it allocates; tests).
 *
 * Limits.  A history from hpt_history_create is colour only; hpt_history_create_flags with HPT_HISTORY_MOMENTS adds the
 * second moment ("temporal variance", below).  Without it the variance-guided filter estimates the variance of every
 * frame spatially and divides by hpt_history_length's n.  The guide position is an average
 * over jittered samples, so pixels that straddle an edge mostly fail the direct-view or the plane test and restart.
 * hpt_history_advance has no motion vectors: geometry that moves ("scene updates", below) is followed only by
 * hpt_history_advance_motion with the motion guide ("motion", below); a history that is not given that guide is reset
 * after an update.  Once n reaches max_history the mean turns into an
 * exponential average with weight 1 / max_history for the new frame, which is what lets lighting seen from a new angle
 * (a highlight, a reflection) converge to its new value instead of keeping the old one forever. */
typedef struct hpt_history hpt_history;
typedef struct hpt_history_params {
    float max_history;      /* cap on a pixel's history length; 0 -> 256; < 1 or NaN: HPT_ERR_INVALID */
    float plane_tolerance;  /* 0 -> 0.01: a tap is kept while its stored point lies within this fraction of the
                               eye distance of the pixel's tangent plane; < 0: test off; NaN: HPT_ERR_INVALID */
    float normal_min;       /* 0 -> 0.9: least dot product of the two guide normals; < -1: test off; NaN: HPT_ERR_INVALID */
    int32_t flags;          /* must be 0 */
} hpt_history_params;
int  hpt_history_create(int W, int H, hpt_history **out);
int  hpt_history_advance(hpt_history *h, const void *camera, const void *d_frame_rgb,
                         const void *d_normal, const void *d_position, const void *d_coverage,
                         const hpt_history_params *p, void *d_mean_out, void *hip_stream);
int  hpt_history_metrics(hpt_history *h, uint64_t *kept, uint64_t *restarted, int64_t *frames);
int  hpt_history_read(hpt_history *h, float *mean, float *length, int64_t *frames);
int  hpt_history_reset(hpt_history *h, void *hip_stream);
void hpt_history_destroy(hpt_history *h);
int  hpt_history_check(int W, int H, const void *camera, const void *d_frame_rgb,
                       const void *d_normal, const void *d_position, const void *d_coverage,
                       const hpt_history_params *p, const void *d_mean_out);

/* ---- temporal variance ----------------------------------------------------------------------------------
 * The spatial estimate (hpt_denoiser_estimate_variance, below) looks at the newest frame alone.  A path tracer's noise is
 * not stationary: bright samples are rare, and a pixel whose mean still carries the remnant of one sits in a window where
 * the newest frame has none.  Its estimated variance is small, its colour tolerance tight, and the remnant passes the
 * filter as a speckle.  A history that also carries the running mean of the SQUARED frame values knows each pixel's own
 * variance over time (SVGF's temporal half, Schied et al. 2017).
 *
 * hpt_history_create_flags(W, H, flags, out).  flags = 0 is hpt_history_create; any bit but HPT_HISTORY_MOMENTS returns
 * HPT_ERR_INVALID.  With HPT_HISTORY_MOMENTS each of the two sets holds a fourth 16-byte record per pixel, q.rgb | 0, zeroed
 * by create and by hpt_history_reset like the others: 128 bytes per pixel instead of 96.
 *
 * hpt_history_advance on such a history computes mean, n, kept, restarted and the stored guides exactly as above -- the
 * same bits as a history without the flag -- and carries q through the same steps, per channel, IEEE float, evaluated as
 * written:
 *   2. (unmoved camera)  q_r = q[p].
 *   4. (taps)            qsum = (0, 0, 0) beside sum; a tap that is taken also gives qsum = qsum + q_prev[tap] * w, with the
 *                        same four taps, the same skips, the same w and the same order.  Where m is taken
 *                        (wsum > 0.01f): q_r = qsum / wsum.
 *   5.                   n_r > 0 is false: q = c * c.  Otherwise q = (q_r * n_c + c * c) / (n_c + 1.0f) with the n_c of
 *                        the mean.  (NULL guides on a first or moved frame have n_r = 0, so q = c * c.)
 *
 * hpt_history_variance(h, d_fallback, min_length, d_variance_out, stream): one launch, a map over pixels, enqueues only.
 * L = min_length == 0 ? 4 : min_length; L < 2 or NaN returns HPT_ERR_INVALID, so n - 1 >= 1 wherever the moments are used.
 * For pixel p with the current m, q, n:
 *   n >= L     per channel d = q - m * m; out = fmaxf(d, 0.0f) / (n - 1.0f).  A NaN d (inf - inf) gives 0.
 *   otherwise  out = d_fallback[p] per channel (W*H*3 floats); 0 when d_fallback is NULL.
 * d_fallback may be d_variance_out itself -- the spatial estimate is patched where the history knows better -- any other
 * overlap of the two is refused.  The result is the variance of the MEAN, in the layout hpt_denoiser_run_guided takes.
 *
 * Caveats.  As hpt_accum_variance, this is good for Monte-Carlo noise and NOT a general-purpose variance: q and m * m are
 * rounded floats of nearly equal size, so below a relative variance of about 1e-7 their difference is rounding, not
 * signal.  Past max_history the weights are exponential, not equal, so (q - m * m) / (n - 1) is an approximation of the
 * mean's variance.  After a move q_r - m_r * m_r also contains the spread between the taps' means (the four taps are
 * mixed as if they were one population), which errs on the high side: a pixel is filtered a little more, never less.
 *
 * hpt_history_read_moments copies the current q (W*H*3 floats) to the host and waits for the device (for tests).
 * hpt_history_variance_check runs every argument check of hpt_history_variance on a W x H history created with
 * create_flags, without a handle or a device.  HPT_ERR_INVALID with a message, before anything touches the device: a null
 * handle or output; a history created without HPT_HISTORY_MOMENTS (variance, read_moments); a call before the first
 * advance or after a reset (variance); a bad min_length; a partial overlap; another current device than the history's. */
#define HPT_HISTORY_MOMENTS 1        /* also carry the per-channel running mean of the squared frame values */
int  hpt_history_create_flags(int W, int H, int32_t flags, hpt_history **out);
int  hpt_history_variance(hpt_history *h, const void *d_fallback, float min_length, void *d_variance_out, void *hip_stream);
int  hpt_history_read_moments(hpt_history *h, float *q);
int  hpt_history_variance_check(int W, int H, int32_t create_flags, const void *d_fallback, float min_length,
                                const void *d_variance_out);

/* ---- variance-guided filtering ------------------------------------------------------------------------
 * hpt_denoiser_run uses one sigma_color for the whole image.  After a camera move under hpt_history converged pixels
 * (tens of samples) and restarted ones (n = 1) sit side by side, and no single tolerance serves both.  The guided run
 * takes a per-pixel variance of the image's values and lets it set each pixel's colour tolerance (the variance-guided
 * a-trous of SVGF, Schied et al. 2017; its temporal part is hpt_accum, hpt_history and hpt_history_variance).  It runs on the
 * same hpt_denoiser -- the same packed guides and the same two colour buffers, 80 bytes per pixel as before: the variance
 * is one scalar per pixel and rides in the free fourth word of the colour records.
 *
 * Everything is IEEE float, evaluated as written, left to right; no transcendental, no sqrt, no atomic; the tap order is
 * part of the definition.  valid(p), a(p), the taps h, the falloff e(x), inv_n, inv_p, the skip rules (outside the image,
 * or invalid) and the rule that a pixel whose 24 other taps are all skipped keeps its value are the plain filter's
 * ("The filter", above).
 *
 * hpt_denoiser_run_guided.  d_variance: W*H*3 floats, the per-channel variance of the image's values -- what
 * hpt_accum_variance writes, or hpt_denoiser_estimate_variance.  d_variance_out: W*H floats, may be NULL.
 *   pack      c_0 is the plain filter's.  v_0(p) = fmaxf(vr / (a.x * a.x) + vg / (a.y * a.y) + vb / (a.z * a.z), 0.0f) with
 *             DEMODULATE on a valid pixel, else fmaxf(vr + vg + vb, 0.0f); a NaN sum gives 0.
 *   level k   stride 2^k.  sigma_color is NOT halved per level: the variance shrinks from level to level and does the
 *             narrowing.  s2 = sigma_color * sigma_color, computed on the host.  For a valid p:
 *     prefilter     always at stride 1, g = {1/4, 1/2, 1/4}: num = 0, den = 0; for j = -1..1 (outer), i = -1..1 (inner),
 *                   q = (x + i, y + j) skipped when outside the image or invalid: num = num + v_k(q) * (g[j+1] * g[i+1]),
 *                   den = den + g[j+1] * g[i+1];  vbar = num / den (the centre is always there).
 *     colour scale  inv_c = fminf(1.0f / (s2 * vbar + 1e-12f), FLT_MAX).
 *     taps          the plain filter's 25, with xc = (dc.x dc.x + dc.y dc.y + dc.z dc.z) * inv_c and xn, xp, w as there:
 *                   sum += c_k(q) * w per channel, vsum = vsum + v_k(q) * (w * w), wsum += w.
 *     result        c_{k+1}(p) = sum / wsum, v_{k+1}(p) = vsum / (wsum * wsum).  A pixel whose 24 other taps are all skipped
 *                   keeps both c and v, and so does an invalid pixel.
 *   output    the colour as in the plain filter (re-modulated; an invalid pixel leaves with its input bits).
 *             d_variance_out[p] = v_n(p), in the filter's WORKING SPACE: demodulated when DEMODULATE is set, never
 *             multiplied back by the albedo, and a sum over the three channels.
 * There is no sqrt: the colour term compares a squared difference with a variance, which keeps every operation one a CPU
 * restatement rounds identically.  Zero variance means inv_c = 1e12, so only (almost) equal colours mix: a pixel that
 * claims to be converged passes through.  A sigma_color < 0 switches the colour term off (the variance is still carried).
 *
 * hpt_denoiser_estimate_variance is SVGF's spatial fallback for frames whose temporal variance is unknown (a moved camera,
 * or fewer than 4 frames).  d_frame_rgb is the SINGLE NEW FRAME, not the mean.  For a valid p, over the 7 x 7 window at
 * stride 1, j = -3..3 (outer), i = -3..3 (inner), q skipped when outside the image or invalid; xn and xp are the filter's
 * (a term switched off is 1.0f):  w = e(xn) * e(xp);  per channel s += c(q) * w, t += (c(q) * c(q)) * w;  ws += w.  Then
 * m = s / ws, q2 = t / ws, var = fmaxf(q2 - m * m, 0.0f), and with d_length (W*H floats, a pixel's history length, may be
 * NULL) var = var / fmaxf(len[p], 1.0f), which makes it the variance of the mean.  An invalid pixel gives 0.  Output
 * W*H*3 floats.  Only sigma_normal, sigma_position and the flags' validity are read from p.  As hpt_accum_variance, this
 * is good for Monte-Carlo noise and NOT a general-purpose variance (q2 and m * m are rounded floats of nearly equal size);
 * the weighted estimate is biased low by the factor 1 - sum w^2 / (sum w)^2 (1/49 of the value at equal weights), and
 * image detail inside the window that the guides do not see counts as noise.
 *
 * hpt_history_length writes the current history length n of every pixel (W*H floats), the image read's `length` returns.
 * hpt_guided_check runs every argument check of a guided run on a W x H image without a handle or a device.
 * All calls only enqueue on hip_stream.  HPT_ERR_INVALID with a message, before the device is touched: a null handle,
 * image or variance; d_out overlapping either input; d_variance_out overlapping any other image; a run (or an estimate)
 * before hpt_denoiser_set_guides; iterations outside [0, 8]; an unknown flag; a NaN sigma; hpt_history_length before the
 * first advance.  With HPT_DENOISE_TIME hpt_denoiser_last_ms and hpt_denoiser_level_ms report the guided run. */
typedef struct hpt_guided_params {
    int32_t iterations;     /* 1..8; 0 -> 5 */
    float sigma_color;      /* 0 -> 2.0 (in standard deviations of the pixel's own noise); < 0 -> colour term off */
    float sigma_normal;     /* as hpt_denoise_params */
    float sigma_position;   /* as hpt_denoise_params */
    int32_t flags;          /* HPT_DENOISE_DEMODULATE, HPT_DENOISE_TIME; other bits: HPT_ERR_INVALID */
} hpt_guided_params;
int hpt_denoiser_run_guided(hpt_denoiser *d, const void *d_linear_rgb, const void *d_variance,
                            void *d_out, void *d_variance_out,
                            const hpt_guided_params *p, void *hip_stream);
int hpt_denoiser_estimate_variance(hpt_denoiser *d, const void *d_frame_rgb, const void *d_length,
                                   void *d_variance_out, const hpt_guided_params *p, void *hip_stream);
int hpt_history_length(hpt_history *h, void *d_length_out, void *hip_stream);
int hpt_guided_check(int W, int H, const void *d_linear_rgb, const void *d_variance, const void *d_out,
                     const void *d_variance_out, const hpt_guided_params *p);

/* ---- the acceleration structure, exported (tests) -------------------------------------
 * The reference has no acceleration structure (include/geometric.cuh:293-388 scan every primitive); the tree the
 * kernels walk is this library's own, and the work counts the bench's roofline is built from (hpt_stats.boxes_*,
 * tris_*) are counts of walking it.  These two calls hand the tree out so that an independent walker -- the oracle's
 * host traversal, oracle/pt_oracle.cpp -- can reproduce those counts ray by ray.
 *   qnodes_out  num_nodes records of 32 B: six words of uint16 grid coordinates (coordinate = qorigin + q * qscale) --
 *               per axis x, y, z one word with the lower plane of the left child's box in its low half and of the right
 *               child's in its high half, then one word with the two upper planes the same way -- then the two uint32
 *               child codes: bit 31 set = leaf,
 *               (code & 0x7FFFFFFF) >> 3 = first triangle slot, (code & 7) + 1 = triangle count; 0xFFFFFFFF = no
 *               child; otherwise the index of an inner node.  Node 0 is the root.
 *   tris_out    num_tris records of 48 B in leaf order: v0 | scan ordinal, v1 - v0 | material, v2 - v0 | flags
 * Either output may be NULL (sizes only); the caps are in bytes and must cover what is written.
 * hpt_bvh_export_host builds on the host only (no device needed) exactly what hpt_scene_create would upload;
 * hpt_scene_export_bvh copies back what the scene's device actually holds. */
typedef struct hpt_bvh_info {
    int32_t num_nodes, num_tris, bvh_depth, num_rounds;   /* num_rounds = spheres + light balls: the first triangle ordinal */
    float qorigin[3], qscale[3];
} hpt_bvh_info;
int hpt_bvh_export_host(const void *lights, int num_lights, const void *spheres, int num_spheres,
                        const void *triangles, int num_triangles, hpt_bvh_info *info,
                        void *qnodes_out, size_t qnodes_cap, void *tris_out, size_t tris_cap);
int hpt_scene_export_bvh(const hpt_scene *scene, hpt_bvh_info *info,
                         void *qnodes_out, size_t qnodes_cap, void *tris_out, size_t tris_cap);

/* Ray-level probes of the intersection kernels (tests): n rays, origins/directions as
 * packed float3.  prim is the reference scan ordinal (spheres, then light balls, then
 * triangles in input order), -1 on a miss; t is 1e20f on a miss. */
int hpt_trace_closest(hpt_scene *scene, const float *origins, const float *dirs, int n,
                      int flags, float *t_out, int32_t *prim_out);
/* Shadow segments p1 -> p2 with the reference's (1e-3, dist-1e-3) range; visible_out[i] = 1
 * when no opaque primitive blocks the segment. */
int hpt_trace_visibility(hpt_scene *scene, const float *p1, const float *p2, int n,
                         int flags, int32_t *visible_out);

/* ---- scene updates -----------------------------------------------------------------------------------
 * A live scene's geometry moved in place: the handle, its workspaces and the tree's topology stay, and everything that
 * is a function of the vertex positions -- the leaf records, every node box, the 16-bit grid, both quantised trees and
 * the per-triangle frames -- is recomputed on the device (a refit), to the bytes the host restatement gives
 * (hpt_bvh_refit_host).  The image does not depend on the tree's quality: closest hits break ties by scan ordinal and
 * occlusion is a boolean, so a refitted tree renders what a rebuilt one renders; what a refit costs is traversal work,
 * since boxes refitted to vertices that moved far overlap more than the builder would have let them.
 *
 * hpt_scene_update_triangles takes num_triangles records of HPT_TRIANGLE_BYTES as hpt_scene_create does.  The count
 * must be the scene's, and the 84 bytes of every record behind its three vertices (old material, material, id) must
 * equal the record the scene was created from: an update moves geometry, it does not re-intern materials.  The call is
 * blocking and runs on the null stream, like every blocking entry point: the caller has waited for earlier work on
 * other streams.  Afterwards every integrator on the handle renders the new scene -- PT, BDPT (groups set earlier are
 * kept), photon mapping, the guides and the probes.  Workspaces, the statistics that describe the scene's shape
 * (bvh_nodes, bvh_depth, n_tris, n_materials) and ms_bvh_build are untouched.  Triangles with a non-finite edge are
 * dead, as at creation (no ray hits them, no box holds them), and may come back to life in a later update.
 *
 * hpt_scene_update_rounds replaces the spheres and the lights, which are scanned, not in the tree: the counts must be
 * the scene's and the 84 bytes of every sphere record behind centre and radius must be unchanged; any field of a light
 * may change.
 *
 * Both calls replace the records the handle keeps and invalidate what is derived from them lazily (the bidirectional
 * scene, the photon-mapping bounds).  They return HPT_ERR_INVALID, with a message, before anything touches the device
 * for: a null scene, or a null array with a non-zero count; a count that is not the scene's; changed bytes other than
 * positions (the message names the first record); a current device other than the scene's.  A scene of zero triangles
 * accepts an update of zero triangles.  hpt_scene_update_check makes the refusals of hpt_scene_update_triangles and
 * nothing else: no device work.  After HPT_ERR_DEVICE from an update the scene must be destroyed.
 *
 * What the caller keeps in step: an hpt_sppm state created before an update renders the new scene, but still holds
 * the statistics gathered on the old one and the bounds it took when it was created or last reset -- reset it
 * (hpt_sppm_reset re-reads the bounds the state was created without; bounds handed to hpt_sppm_create are the
 * caller's to keep right) or recreate it (not checked).  hpt_accum has no motion vectors for moving geometry: with a
 * still camera it would average two scenes, so reset it after an update.  hpt_history follows the geometry when it is
 * given the motion guide, in the per-frame call order of "motion" below; without that guide it is reset like hpt_accum.
 *
 * hpt_scene_get_update_info describes the last triangle update of any kind -- hpt_scene_update_triangles or one of the
 * two of "poses" below -- (zeros before the first): how many have been made, how many triangles were live and dead, and
 * the milliseconds of packing the vertices (36 bytes per triangle), of uploading them (the first update also allocates
 * the scratch) and of the device part (HIP events around it).
 *
 * hpt_bvh_refit_host is the definition, on the host alone (no device): it builds from `triangles`, refits to
 * `new_triangles` (same count, same non-vertex bytes) and exports as hpt_bvh_export_host does.  Refitting a tree to the
 * vertices it was built from reproduces the builder's bytes.
 *
 * Out of scope: topology changes and automatic rebuilds (a caller whose geometry has moved far measures the tree with
 * hpt_scene_tree_cost and calls hpt_scene_rebuild, "tree cost" and "rebuild" below);
 * hpt_multi_* and the scene the one-shot wrappers keep, which compare bytes and rebuild as before.  Vertices handed over
 * as a device pointer and per-part transforms are "poses" below.  (pt_cli turns an OBJ's triangles between frames with
 * --spin, "motion" below, and with --spin-device, "poses".) */
typedef struct hpt_update_info {
    uint64_t updates, live_tris, dead_tris;
    double ms_pack, ms_upload, ms_refit;
} hpt_update_info;
int hpt_scene_update_triangles(hpt_scene *scene, const void *triangles, int num_triangles);
int hpt_scene_update_rounds(hpt_scene *scene, const void *lights, int num_lights, const void *spheres, int num_spheres);
int hpt_scene_update_check(const hpt_scene *scene, const void *triangles, int num_triangles);
int hpt_scene_get_update_info(const hpt_scene *scene, hpt_update_info *out);
int hpt_bvh_refit_host(const void *lights, int num_lights, const void *spheres, int num_spheres, const void *triangles,
                       const void *new_triangles, int num_triangles, hpt_bvh_info *info,
                       void *qnodes_out, size_t qnodes_cap, void *tris_out, size_t tris_cap);

/* ---- poses ----------------------------------------------------------------------------------------------------
 * Two more ways for new vertex positions to reach the refit of "scene updates", neither of which has the host touch a
 * triangle: nine floats per triangle that are already on the device, and one 3 x 4 transform per rigid part, applied on
 * the device to a rest pose the scene keeps.  Both end in the same refit and leave the handle as
 * hpt_scene_update_triangles would with records carrying those vertices and the scene's own 84 other bytes: the exported
 * tree equals hpt_bvh_refit_host of those records, every integrator renders them, the previous geometry and the motion
 * guide ("motion") follow them -- they read the device's vertices, whichever call wrote them.  All five calls are blocking
 * and run on the null stream, like every update: the caller has waited for whatever produced d_verts.
 *
 * hpt_scene_update_vertices_device takes num_triangles * 9 floats on the scene's device, in input order v0, v1, v2 per
 * triangle, copies them device to device and refits.  No record is checked, because no non-vertex byte arrives.
 *
 * hpt_scene_set_parts gives every triangle a part: tri_part[i] in [0, num_parts), or tri_part NULL with num_parts == 1
 * for one part that holds every triangle; num_parts lies in [1, 1 << 20] and a part may own no triangle.  The call
 * captures the REST POSE: the nine vertex floats of every triangle as the scene holds them now.  It may be called again,
 * which gives a new map and a new rest pose.  It costs 40 bytes of device memory per triangle, allocated here: a scene
 * that never calls it pays nothing.  The geometry does not change (hpt_scene_has_motion is not set).
 *
 * hpt_scene_pose takes num_parts records of 12 floats, three rows (a, b, c, t) each; num_parts must be the value given to
 * hpt_scene_set_parts.  Poses are absolute: every call is applied to the rest pose, never to the pose before, so rounding
 * does not accumulate.  IEEE float, evaluated as written, left to right, no contraction: a vertex (x, y, z) of a triangle in
 * part k with rows r0, r1, r2 becomes
 *     X = ((r0.a * x + r0.b * y) + r0.c * z) + r0.t     and Y, Z likewise from r1, r2, with two exceptions made on bits:
 *   identity    if the 48 bytes of part k's record are those of (1,0,0,0, 0,1,0,0, 0,0,1,0) with +0 throughout, the vertex
 *               keeps its bits -- a -0 stays -0 (the arithmetic would give +0) and a NaN keeps its payload.  The motion
 *               guide's Y = X rule and step 3' of the history advance compare bytes, so the pixels of a part left at
 *               identity stay exact running means.
 *   non-finite  if X, Y or Z is not finite (exponent bits all ones), all three become 0x7FC00000: processors propagate NaN
 *               signs and payloads differently, and this makes the bytes a function of the inputs alone.  Such a triangle
 *               is dead, as at creation, and a later pose revives it.
 * A non-finite entry of xforms is not refused: it kills the part by the rule above.  After the pose kernel has written
 * the vertices, the refit runs.
 *
 * The rest-pose rule.  Every triangle update that is not a pose -- hpt_scene_update_triangles and
 * hpt_scene_update_vertices_device -- sets the rest pose to the geometry it leaves, which returns every part to identity;
 * the part map is kept.
 *
 * hpt_scene_get_update_info describes these two updates as well: ms_pack is 0, ms_upload is the time of the table's
 * upload or of the device-to-device copy, ms_refit the device part, the pose kernel included.
 *
 * hpt_scene_read_triangles returns the records the handle holds now, num_triangles * HPT_TRIANGLE_BYTES: the scene's 84
 * non-vertex bytes with the current vertices.  After one of the two updates above the handle's host records are behind
 * the device's vertices; they are brought up to date (a download of 36 bytes per triangle) by the first call that reads
 * them -- this one, the bidirectional scene's build, photon mapping's own bounds -- and by nothing else: path tracing,
 * the guides, the probes and further updates never pay for it.
 *
 * hpt_pose_host is the definition, on the host alone (no device): triangles_out gets the records of `triangles` with
 * every vertex posed as above; it may be `triangles` itself.  tri_part NULL with num_parts == 1 as above.
 *
 * Refusals, HPT_ERR_INVALID with a message before anything touches the device: a null scene, or a null array with a
 * non-zero count; a count that is not the scene's; num_parts out of range, or not the value given to
 * hpt_scene_set_parts; a part index out of range (the message names the first triangle); hpt_scene_pose before
 * hpt_scene_set_parts; a current device other than the scene's; tri_part NULL with num_parts != 1.  hpt_pose_host makes
 * those that need no scene.  A scene of zero triangles accepts all of these calls with zero counts.  A refused call leaves
 * the handle as it was.
 *
 * Out of scope: blend-weight skinning (it is "skinning" below); poses for spheres and lights (hpt_scene_update_rounds is a small upload already);
 * a non-blocking or caller-stream variant; hpt_multi_*.
 *
 * pt_cli --frames N --obj mesh.obj --spin-device DEG is --spin through these calls: hpt_scene_set_parts once (part 0:
 * everything that is not the OBJ, left at identity; part 1: the OBJ) and hpt_scene_pose per frame, with the 3 x 4 of
 * --spin's own double-precision rotation about the centroid rounded to float.  No record is copied per frame.  The pose
 * multiplies in float where --spin turns in double and rounds once, so the two images differ in the last bits. */
int hpt_scene_update_vertices_device(hpt_scene *scene, const void *d_verts, int num_triangles);
int hpt_scene_set_parts(hpt_scene *scene, const int32_t *tri_part, int num_triangles, int num_parts);
int hpt_scene_pose(hpt_scene *scene, const float *xforms, int num_parts);
int hpt_scene_read_triangles(hpt_scene *scene, void *triangles_out, int num_triangles);
int hpt_pose_host(const void *triangles, int num_triangles, const int32_t *tri_part,
                  const float *xforms, int num_parts, void *triangles_out);

/* ---- skinning -------------------------------------------------------------------------------------------------
 * A pose moves rigid parts; a skin deforms: every CORNER -- one vertex of one triangle, corner 3 * i + k being v_k of input
 * triangle i (the handle keeps nine floats per triangle, not an indexed mesh) -- follows up to HPT_SKIN_INFLUENCES bones
 * with a weight each, blended over the rest pose on the device.  It ends in the same refit as every update, with the same
 * guarantees as a pose: a definition the host restates byte for byte, static vertices whose bits never change, and
 * everything downstream (the previous geometry, the motion guide, every integrator, the lazy host records) untouched.
 *
 * hpt_scene_set_skin takes corner_bone and corner_weight, num_triangles * 3 * 4 entries each: four (bone, weight)
 * influences per corner, in order; num_bones lies in [1, 65536].  It captures the rest pose exactly as hpt_scene_set_parts
 * does, uploads the influences once (24 bytes per corner: the bones as four 16-bit indices; with the rest pose 108 bytes
 * per triangle, allocated here -- a scene that never calls it pays nothing), is blocking and runs on the null stream.  It
 * may be called again, which gives a new table and a new rest pose.  The geometry does not change (hpt_scene_has_motion is
 * not set).
 *
 * One deformer per scene: a scene holds parts or a skin.  hpt_scene_set_skin drops the parts (hpt_scene_pose is then
 * refused as before hpt_scene_set_parts) and hpt_scene_set_parts drops the skin; the two share the rest pose.  The
 * rest-pose rule of "poses" covers the skin: hpt_scene_update_triangles and hpt_scene_update_vertices_device set the rest
 * pose to the geometry they leave; the influences are kept.
 *
 * hpt_scene_skin takes num_bones records of 12 floats, the rows (a, b, c, t) of hpt_scene_pose; num_bones must be the value
 * given to hpt_scene_set_skin.  It is absolute, like a pose.  hpt_scene_get_update_info reports it as a pose: ms_pack is 0,
 * ms_upload the table's upload, ms_refit the device part, the skin kernel included.  The host records are brought up to date
 * lazily, as after a pose.
 *
 * The definition.  IEEE float, evaluated as written, left to right, no contraction.  A corner has the rest vertex (x, y, z)
 * and influences (b_j, w_j), j = 0..3.  Influence j is ACTIVE if the 32 bits of w_j are not zero.  arith(r) is the three
 * rows of record r, each ((r.a * x + r.b * y) + r.c * z) + r.t, as in a pose.  Three cases, tested in this order:
 *   keep    every active influence's record has the identity's 48 bytes, +0 throughout -- this includes a corner with no
 *           active influence.  The vertex keeps its bits: a -0 stays -0, a NaN keeps its payload.  Static geometry is
 *           given four zero weights and never moves by a bit.
 *   rigid   exactly one influence is active and its weight has the bits of 1.0f: the result is arith of that bone's
 *           record, then the non-finite rule -- the bytes of hpt_scene_pose with that record.  A skin with one-hot
 *           weights IS a pose, byte for byte.
 *   blend   anything else.  For the active influences in index order p_j = arith(record[b_j]) -- plain arithmetic even
 *           for a record that is the identity -- and per component acc = w_j * p_j for the first active influence,
 *           acc = acc + w_j * p_j for each later one; then the non-finite rule.  Weights are not normalised and their sum
 *           is not checked.
 * The non-finite rule is the pose's: if any of the three results has all exponent bits set, all three words become
 * 0x7FC00000; the triangle is dead and a later skin revives it.  An inactive influence is never evaluated: a bone whose
 * record is NaN kills only the corners on which it has weight.  A non-finite entry of xforms is not refused.
 *
 * hpt_skin_host is the definition, on the host alone (no device): triangles_out gets the records of `triangles` with every
 * corner skinned as above; it may be `triangles` itself.
 *
 * Refusals, HPT_ERR_INVALID with a message before anything touches the device: a null scene, or a null array with a
 * non-zero count; a count that is not the scene's; num_bones outside [1, 65536]; a bone index outside [0, num_bones),
 * active or not, and a weight with its sign bit set, NaN or infinite (the message names the first triangle and corner);
 * hpt_scene_skin before hpt_scene_set_skin or with another num_bones; a null xforms; a current device other than the
 * scene's.  hpt_skin_host makes those that need no scene.  A scene of zero triangles accepts all three calls with zero
 * counts.  A refused call leaves the handle as it was.
 *
 * Out of scope: an indexed mesh (shared vertices skinned once); more than four influences; dual-quaternion blending;
 * a non-blocking or caller-stream variant; hpt_multi_*.
 *
 * pt_cli --frames N --obj mesh.obj --twist-device DEG twists the OBJ about the vertical axis through its centroid: two
 * bones, bone 0 at identity and bone 1 --spin-device's turn of f * DEG; an OBJ corner at height y has the weight
 * t = clamp((y - ymin) / (ymax - ymin), 0, 1) on bone 1 and 1 - t on bone 0, every other corner four zero weights. */
#define HPT_SKIN_INFLUENCES 4
int hpt_scene_set_skin(hpt_scene *scene, const int32_t *corner_bone, const float *corner_weight,
                       int num_triangles, int num_bones);
int hpt_scene_skin(hpt_scene *scene, const float *xforms, int num_bones);
int hpt_skin_host(const void *triangles, int num_triangles, const int32_t *corner_bone,
                  const float *corner_weight, const float *xforms, int num_bones, void *triangles_out);

/* ---- morph targets ---------------------------------------------------------------------------------------------
 * The third deformer, and the one that runs before the other two: morph targets (blend shapes; glTF's `targets` and
 * `weights`).  A target is a set of per-corner offsets, a frame carries one scalar weight per target, and the result is
 * rest + sum of w_t * delta_t, computed on the device from a few floats per frame.  It ends in the same refit as every update,
 * with the guarantees of a pose: a definition the host restates byte for byte, geometry no target names never moving by a bit,
 * and everything downstream (the previous geometry, the motion guide, every integrator, the lazy host records) untouched.
 *
 * Targets are sparse.  Target t owns the entries target_begin[t] .. target_begin[t + 1] - 1; target_begin has num_targets + 1
 * values.  Entry e moves corner entry_corner[e] by the three floats entry_delta[3e .. 3e + 2]; corners are numbered as in
 * "skinning": corner 3 * i + k is v_k of input triangle i.  Within one target the corners ascend strictly, so a corner
 * appears at most once per target and the order of the sum is fixed.  A target may be empty and num_entries may be 0.
 *
 * hpt_scene_set_morphs captures the rest pose exactly as hpt_scene_set_parts does, uploads the targets once, is blocking and
 * runs on the null stream.  The geometry does not change (hpt_scene_has_motion is not set).  It may be called again, which
 * gives new targets and a new rest pose.  On the device the targets are kept turned round, one run of entries per corner:
 * 4 bytes per corner (12 per triangle, and 4 more) for the runs' ends and 16 bytes per entry, next to the rest pose's 36
 * bytes per triangle and 4 bytes per target for the weights; all of it is allocated here, and a scene that never calls it
 * pays nothing.
 *
 * The definition.  IEEE float, evaluated as written, no contraction.  Target t is ACTIVE if its weight is neither +0 nor -0
 * ((bits << 1) != 0); negative weights are legitimate here, unlike in a skin.  For a corner with the rest vertex (x, y, z):
 *   keep    no active target has an entry for the corner.  The vertex keeps its bits: a -0 stays -0, a NaN keeps its payload.
 *           Geometry that no target names, and every corner under all-zero weights, never moves by a bit.
 *   morph   otherwise, per component, acc starts as the rest value, and each active target that has an entry for the corner,
 *           in ascending target order, sets acc = acc + w_t * d -- the product is rounded, then the sum.  Then the pose's
 *           non-finite rule: if any of the three results has all exponent bits set, all three words become 0x7FC00000; the
 *           triangle is dead and a later morph revives it.
 * An inactive target is never evaluated: NaN deltas under a zero weight touch nothing.  Weights and deltas are not
 * validated; any bit pattern is accepted, and the non-finite rule makes the bytes a function of the inputs alone.
 *
 * Composition: morph first, then the deformer.  A scene holds at most one deformer (parts or a skin, as before) and,
 * independently, morphs.  Write R for the rest pose and M for the morphed rest pose.  hpt_scene_morph computes
 * M = morph(R, weights); the scene's geometry then becomes the deformer's last table applied to M, and without a deformer
 * M itself.  On a scene with morphs hpt_scene_pose and hpt_scene_skin apply their table to M instead of R; the deformer's
 * stage is exactly its own definition with M as the rest vertex.  Every call that captures a rest pose leaves all weights
 * at zero (M = R, the same bits) and the deformer's table at identity: hpt_scene_set_parts, hpt_scene_set_skin,
 * hpt_scene_set_morphs, and by the rest-pose rule hpt_scene_update_triangles and hpt_scene_update_vertices_device.  Targets,
 * the part map and the influences are kept across such a capture.  hpt_scene_set_parts and hpt_scene_set_skin still replace
 * each other and leave the morphs alone.  On a scene without morphs every earlier call behaves and costs exactly as before.
 * M is a buffer of its own (36 bytes per triangle) only on a scene that has both morphs and a deformer; with morphs alone
 * the kernel writes the scene's vertices directly.
 *
 * hpt_scene_morph takes num_targets weights; num_targets must be the value given to hpt_scene_set_morphs.  It is absolute,
 * blocking, runs on the null stream and ends in the same refit.  hpt_scene_get_update_info reports it as a pose: ms_pack
 * is 0, ms_upload the weights' upload, ms_refit the device part, the morph and deformer kernels included.  The host records
 * go stale and are refreshed lazily.  hpt_scene_rebuild keeps the targets, the weights and M.
 *
 * hpt_morph_host is the definition, on the host alone (no device): triangles_out gets the records of `triangles` with every
 * corner morphed as above; it may be `triangles` itself.  It covers the morph stage only: compose it with hpt_pose_host or
 * hpt_skin_host for the whole chain.
 *
 * Refusals, HPT_ERR_INVALID with a message before anything touches the device: a null scene, or a null array with a
 * non-zero count; a triangle count that is not the scene's; num_targets outside [1, HPT_MORPH_MAX_TARGETS], or
 * num_entries < 0; target_begin[0] != 0, a decreasing target_begin, or target_begin[num_targets] != num_entries; a corner
 * outside [0, 3 * num_triangles), or corners not strictly ascending within a target (the message names the target and the
 * entry); hpt_scene_morph before hpt_scene_set_morphs, with another num_targets, or with null weights; a current device
 * other than the scene's.  hpt_morph_host makes those that need no scene.  A scene of zero triangles accepts all three calls
 * with zero entries.  A refused call leaves the handle as it was.
 *
 * Out of scope: removing morphs from a scene; morphed normals (the renderer derives its normals from the triangle); more
 * than HPT_MORPH_MAX_TARGETS targets; an indexed mesh; a non-blocking or caller-stream variant; hpt_multi_*.
 *
 * pt_cli --frames N --obj mesh.obj --morph-device AMP puts two targets on the OBJ's corners: with h the corner's height in
 * the mesh normalised to [0, 1] and r the OBJ's radius about the vertical axis through its centroid, target 0 pushes the
 * corner away from that axis by h * r / 4 and target 1 lifts it by the same amount.  The weights at frame f are
 * AMP * (1 - cos(2 pi f / 32)) / 2 and AMP * sin(2 pi f / 32), computed in double and rounded to float.  It combines with
 * --spin-device or --twist-device (morph, then the deformer), --reproject and --rebuild-above. */
#define HPT_MORPH_MAX_TARGETS 4096
int hpt_scene_set_morphs(hpt_scene *scene, const int32_t *target_begin, const int32_t *entry_corner,
                         const float *entry_delta, int num_entries, int num_triangles, int num_targets);
int hpt_scene_morph(hpt_scene *scene, const float *weights, int num_targets);
int hpt_morph_host(const void *triangles, int num_triangles, const int32_t *target_begin,
                   const int32_t *entry_corner, const float *entry_delta, int num_entries,
                   int num_targets, const float *weights, void *triangles_out);

/* ---- motion ---------------------------------------------------------------------------------------------
 * hpt_history keeps a viewer's accumulation when the camera moves, and the scene updates move the geometry in place; this
 * is what joins them.  The scene remembers one previous geometry, a fifth guide image says where each pixel's surface
 * point was one frame ago, and a history advance that projects THAT point into the previous camera follows geometry
 * that moves.  A pixel of static geometry under a still camera stays a plain running mean, bit for bit.
 *
 * Per frame, a viewer calls, in this order:
 *   hpt_scene_update_triangles / hpt_scene_update_rounds     this frame's geometry (any number of them, or none)
 *   hpt_render_guides_motion[_device]                        the four guides and prev_position
 *   hpt_render_pt_device (or any integrator), hpt_untile     the frame
 *   hpt_history_advance_motion                               the frame into the history, through prev_position
 *   hpt_scene_keep_previous                                  this frame's geometry becomes the next frame's previous one
 *
 * The previous geometry.  A scene has its current geometry G (what hpt_scene_create and the updates have made it) and a
 * previous geometry G'; at creation G' = G.  The updates change G only.  hpt_scene_keep_previous sets G' := G; it is
 * blocking and runs on the null stream, like the updates.  Several updates inside one frame are all measured against the
 * same G'.  hpt_scene_has_motion returns 1 if any update succeeded since creation or since the last
 * hpt_scene_keep_previous, else 0, and < 0 on a null scene (a host flag, no device work).  G' holds the nine vertex
 * floats of every triangle in input order (36 bytes per triangle) and centre and radius of every sphere (16 bytes); it is
 * allocated by the first update, so a scene that is never updated pays nothing.  Lights and light balls have no previous
 * state: a light ball never becomes a hit point.  A dead triangle (non-finite edge) has non-finite previous vertices.
 * hpt_scene_keep_previous returns HPT_ERR_INVALID with a message, before the device is touched, for a null scene or a
 * current device other than the scene's.
 *
 * The motion guide.  hpt_render_guides_motion and hpt_render_guides_motion_device are hpt_render_guides and
 * hpt_render_guides_device with a fifth output, prev_position (W*H*3 floats).  With prev_position NULL they ARE those
 * calls: the same refusals and the same bytes; "not all outputs NULL" counts five outputs, and the four other images are
 * the same bytes whether or not prev_position is asked for.  IEEE float, evaluated as written, left to right, dot as
 * defined for the history.  Sample s of pixel p that ends in a hit point X on a primitive adds Y to a fifth per-pixel sum
 * Pprev, in sample order beside P:
 *   triangle with input index i, current vertices a0, a1, a2 and previous vertices b0, b1, b2.  If the 36 bytes of the two
 *     sets are equal, Y = X, the same bits.  Otherwise e1 = a1 - a0, e2 = a2 - a0, d = X - a0;
 *     d00 = dot(e1, e1), d01 = dot(e1, e2), d11 = dot(e2, e2), d20 = dot(d, e1), d21 = dot(d, e2);
 *     den = d00 * d11 - d01 * d01;  beta = (d11 * d20 - d01 * d21) / den;  gamma = (d00 * d21 - d01 * d20) / den;
 *     f1 = b1 - b0, f2 = b2 - b0;  Y = (b0 + f1 * beta) + f2 * gamma per component.
 *   sphere j, current centre and radius c, r and previous c', r'.  If the 16 bytes are equal, Y = X.  Otherwise
 *     k = r' / r and Y = c' + (X - c) * k per component.
 * Nothing is special-cased: a zero den, or previous vertices that were dead, give a non-finite Y.  It poisons the pixel's
 * sum, and the history's range test then restarts that pixel (NaN fails every comparison there).
 * prev_position = Pprev / (float) C per channel, zero where C = 0, exactly as position is resolved.  On a scene whose G'
 * equals G byte for byte prev_position therefore equals position bit for bit, at any spp.
 *
 * hpt_history_advance_motion is hpt_history_advance with a sixth image, d_prev_position; hpt_history_motion_check is
 * hpt_history_check with it.  With d_prev_position NULL both ARE those calls, byte for byte.  With it the three guides
 * must be given, and it may not overlap d_mean_out or the frame.  Write X = position[p], Xp = prev_position[p],
 * N = normal[p]; "still": the camera's 84 bytes equal the previous advance's; "same": the three words of Xp equal those of
 * X bitwise.  Steps 1, 5 and 6 of hpt_history_advance, the counts, the second moment (q rides along exactly as in
 * "temporal variance": where m is the pixel's own record, q_r is its own q) and the stored state are unchanged -- the pixel
 * stores X, N and coverage of this frame, never Xp.  Steps 2 to 4 become:
 *   2'. no hit point (coverage[p] > 0 is false): if still and coverage_prev[p] > 0 is also false, m = mean[p], n_r = n[p]
 *       (sky stays sky); otherwise n_r = 0 (something was there a frame ago).
 *   3'. still and same: one tap, the pixel's own previous record, weight 1 and no division.  It is taken when
 *       coverage_prev[p] > 0 holds and the tap passes the plane test t = dot(N, position_prev[p] - X),
 *       t * t <= tol2 * P.dist2 with P = project(this camera, X), and the normal test dot(N, normal_prev[p]) >= normal_min,
 *       each when it is on.  Taken: m = mean_prev[p], n_r = n_prev[p], the same bits; otherwise n_r = 0.  This restarts a
 *       wall pixel the moving object covered one frame ago and keeps every other static pixel an exact running mean.
 *   4'. everything else: the direct-view test as in step 4, with X and this camera; the range test with
 *       Q = project(previous camera, Xp); the taps as in step 4 with the plane test t = dot(N, position_prev[q] - Xp)
 *       against tol2 * P.dist2 and the normal test with the current N; the result rule unchanged (wsum > 0.01f).
 * Limit: both tap tests use the CURRENT normal, so geometry that turns by more than acos(normal_min) per frame (about 25
 * degrees at the default) restarts; a turn of a few degrees does not.  There is no previous-normal guide.  Motion seen
 * through a mirror or glass bounce is not followed: those pixels fail the direct-view test and restart, as before.
 *
 * pt_cli --frames N --obj mesh.obj --spin DEG turns the OBJ's triangles by f * DEG degrees (from the original vertices,
 * so rounding does not accumulate) about the vertical axis through their centroid before frame f and calls
 * hpt_scene_update_triangles; with --reproject the frames go through the call order above, without it the accumulation
 * is reset after every update. */
int hpt_scene_keep_previous(hpt_scene *scene);
int hpt_scene_has_motion(const hpt_scene *scene);
int hpt_render_guides_motion(hpt_scene *scene, const void *camera, int W, int H, int spp, const hpt_params *params,
                             float *albedo, float *normal, float *position, float *coverage, float *prev_position);
int hpt_render_guides_motion_device(hpt_scene *scene, const void *camera, int W, int H, int spp, const hpt_params *params,
                                    void *d_albedo, void *d_normal, void *d_position, void *d_coverage, void *d_prev_position);
int hpt_history_advance_motion(hpt_history *h, const void *camera, const void *d_frame_rgb,
                               const void *d_normal, const void *d_position, const void *d_coverage,
                               const void *d_prev_position, const hpt_history_params *p, void *d_mean_out, void *hip_stream);
int hpt_history_motion_check(int W, int H, const void *camera, const void *d_frame_rgb,
                             const void *d_normal, const void *d_position, const void *d_coverage,
                             const void *d_prev_position, const hpt_history_params *p, const void *d_mean_out);

/* ---- tree cost ------------------------------------------------------------------------------------------------
 * What a refit costs is traversal work ("scene updates"), and until now the only way to see it was a slower frame.
 * These two calls measure the tree itself: the surface-area estimate of a walk of the quantised binary tree, the 32-byte
 * records of "the acceleration structure, exported" that the first trace launch walks (the four-wide twin's boxes come
 * from the same float boxes; its own cost is out of scope).  hpt_scene_tree_cost reduces the tree where it lies, on the
 * device (one streaming kernel over num_nodes * 32 bytes, 96 bytes read back); hpt_bvh_cost_host is the definition, on
 * the host alone, over an exported tree.  The device's struct equals the host's byte for byte.
 *
 * For node i and child c (0 left, 1 right): code = c ? right : left; per axis a the child's planes lo and hi as unsigned
 * integers and d_a = hi >= lo ? hi - lo : 0.
 *   code == 0xFFFFFFFF      empty_children += 1, nothing else
 *   bit 31 set (a leaf)     k = (code & 7) + 1;  leaf_children += 1, leaf_slots += k,
 *                           leaf_xy += k*d_x*d_y, leaf_yz += k*d_y*d_z, leaf_zx += k*d_z*d_x
 *                           (a dead triangle in a leaf counts: it is tested)
 *   otherwise (inner)       inner_children += 1, inner_xy += d_x*d_y, inner_yz += d_y*d_z, inner_zx += d_z*d_x
 * root_extent[a]: the greatest hi minus the least lo over node 0's non-empty children when hi >= lo, else 0; 0 when both
 * children are empty.  num_nodes is the tree's.  A term is below 2^35 (8 * 65535^2) and a tree has fewer than 2^24 nodes
 * (asserted by both calls), so no sum reaches 2^60: every integer is exact, whatever the order of the adds.
 *
 * The doubles, IEEE double, evaluated as written, left to right, by one function both calls share:
 *   Axy = (double) qscale[0] * (double) qscale[1], Ayz and Azx likewise (y z, z x)
 *   root_area = rx*ry*Axy + ry*rz*Ayz + rz*rx*Azx           the extents converted to double first
 *   root_area > 0.0 false:  box_visits = tri_tests = sah = 0  (an empty scene, a point, a grid that is not finite)
 *   box_visits = 1.0 + (inner_xy*Axy + inner_yz*Ayz + inner_zx*Azx) / root_area
 *   tri_tests  = (leaf_xy*Axy + leaf_yz*Ayz + leaf_zx*Azx) / root_area
 *   sah        = 2.0 * box_visits + tri_tests
 * For a random line through the root's box, box_visits is the expected number of inner nodes visited (two slab tests
 * each) and tri_tests the expected number of triangle tests.  The unit costs 2 and 1 are a convention, not a
 * measurement: compare a tree with itself over time; the integer sums are there for any other weights.
 *
 * hpt_scene_tree_cost is blocking and runs on the null stream, like the updates.  Both calls return HPT_ERR_INVALID with a
 * message, before the device is touched, for: a null scene or out; a current device other than the scene's; for the host
 * call a null info or qnodes, qnodes_bytes below num_nodes * 32, or num_nodes < 1. */
typedef struct hpt_tree_cost {
    uint64_t inner_children, leaf_children, empty_children, leaf_slots;
    uint64_t inner_xy, inner_yz, inner_zx, leaf_xy, leaf_yz, leaf_zx;
    uint32_t root_extent[3], num_nodes;
    double box_visits, tri_tests, sah;
} hpt_tree_cost;
int hpt_scene_tree_cost(hpt_scene *scene, hpt_tree_cost *out);
int hpt_bvh_cost_host(const hpt_bvh_info *info, const void *qnodes, size_t qnodes_bytes, hpt_tree_cost *out);

/* ---- rebuild -----------------------------------------------------------------------------------------------------
 * hpt_scene_rebuild gives a live handle a new tree in place.  Afterwards the handle holds the tree that
 * hpt_bvh_export_host(lights, spheres, T) gives, byte for byte, where the lights and spheres are the handle's current
 * records and T is what hpt_scene_read_triangles returns at that moment.  It is blocking and runs on the null stream,
 * like every update: the host records are brought up to date (the lazy download of hpt_scene_read_triangles), the host
 * builder of hpt_scene_create runs on them, and the four tree arrays and the per-triangle frames go into fresh device
 * buffers that replace the old ones only when all of that has succeeded.  A failed allocation (HPT_ERR_NOMEM) leaves the
 * handle exactly as it was; the peak is two trees on the device.  The material table the builder interns equals the
 * handle's (the non-vertex bytes never change); should it ever not, the call returns HPT_ERR_DEVICE with a message and the
 * handle is as it was.  Materials, spheres and lights are not uploaded again.
 *
 * A rebuild is not an update.  Everything in the handle other than the tree is indexed by input triangle, and stays: the
 * current and the previous geometry and hpt_scene_has_motion, hpt_update_info, the rest pose with the part map or skin
 * and the last table, the groups and the bidirectional scene (which has trees of its own), the photon-mapping bounds and
 * every hpt_sppm state, the workspaces.  Every integrator renders the same bytes after the rebuild as before: the image
 * does not depend on the tree, only the work does.  A later update, pose or skin refits the new topology: the exported
 * tree then equals hpt_bvh_refit_host(T, new records) with T the records at the time of the rebuild.  hpt_stats.bvh_nodes,
 * bvh_depth and ms_bvh_build become the new tree's.
 *
 * hpt_scene_get_rebuild_info describes the last rebuild (zeros before the first): how many have been made, the node count
 * and depth before and after, and the milliseconds of bringing the host records up to date, of the host builder, and of
 * the upload with the triangle frames.
 *
 * hpt_scene_rebuild returns HPT_ERR_INVALID with a message, before the device is touched, for a null scene or a current
 * device other than the scene's.  A scene of zero triangles accepts the call and counts it.
 *
 * Out of scope: a rebuild off the calling thread; a partial rebuild (re-splitting subtrees); any
 * automatic policy inside the library (pt_cli --rebuild-above R is a caller's: it rebuilds when sah exceeds R times the
 * cost measured after the last build); hpt_multi_* and the scene the one-shot wrappers keep; the four-wide tree's cost. */
typedef struct hpt_rebuild_info {
    uint64_t rebuilds;
    uint32_t nodes_before, nodes_after, depth_before, depth_after;
    double ms_download, ms_build, ms_upload;
} hpt_rebuild_info;
int hpt_scene_rebuild(hpt_scene *scene);
int hpt_scene_get_rebuild_info(const hpt_scene *scene, hpt_rebuild_info *out);

/* ---- device builds -----------------------------------------------------------------------------------------------
 * hpt_scene_rebuild_device gives a live handle a new tree built on the device from the vertices the device holds now: no
 * download, no host builder, no upload.  It is blocking and runs on the null stream, like every update.  The tree is a
 * linear BVH in Morton order; hpt_bvh_device_build_host is its definition, on the host alone, and the device is held to
 * its bytes (hpt_scene_export_bvh afterwards equals it: info, qnodes, tris).
 *
 * Keys.  Liveness and the box [mn, mx] of a triangle are those of "scene updates" (a non-finite edge: dead).  The cells
 * lie on the box [lo, hi] of the live triangles: per axis ext = hi - lo and scale = 2097152.0f / ext in float, 0 where
 * ext > 0 is false.  A live triangle's centroid is c = 0.5f * (mn + mx) per axis, f = (c - lo) * scale, one float
 * operation at a time, and its cell is f >= 1.0f ? (f < 2097152.0f ? (uint32) f : 2097151) : 0 -- comparisons first, so a
 * NaN lands in cell 0 and nothing out of range is converted.  A key is 64 bits: bit k of the x cell is bit 3k + 2, of the
 * y cell bit 3k + 1, of the z cell bit 3k (k = 0 .. 20); bit 63 is clear.  A dead triangle has the key of all ones.
 * Order.  Ascending by key, ties by input index.  The sorted position is the leaf slot; nothing re-sorts inside a leaf.
 * Topology.  The binary radix tree (Karras 2012) over the sorted pairs: delta(i, j) is the number of leading bits the keys
 * at positions i and j share, and 64 plus the number of leading bits the 32-bit positions share where the keys are equal.
 * A child whose range holds 2 triangles or fewer is the leaf code 0x80000000 | first << 3 | count - 1.  Zero triangles
 * give a root with two empty children, one or two a root with that leaf and an empty right child, as hpt_scene_create does.
 * Numbering.  Breadth-first, as hpt_scene_create: level by level, within a level the inner children in order, left before
 * right.  bvh_depth is the number of levels (0 for an empty scene).
 * Boxes.  Every leaf record, node box, the padding, the grid and qnodes are those of a refit ("scene updates") on this
 * topology; each record carries the ordinal, material and flags of its triangle.
 * The four-wide twin.  The greedy collapse of hpt_scene_create over the float boxes that refit wrote: a node's children
 * are the binary node's (left, then right); while there are fewer than four and an inner one among them, the inner child
 * of the largest half area dx*dy + dy*dz + dz*dx (strict >, first found) is replaced by the last child and its own two
 * are appended.  Wide nodes are numbered breadth-first the same way; wide_depth is their number of levels.
 *
 * The depth of a radix tree is the data's.  When the tree has more than 30 levels, or its four-wide twin is too deep for
 * the resume launch's stack, nothing is swapped: the call runs hpt_scene_rebuild instead, returns its code, and reports
 * fell_back = 1 (hpt_rebuild_info counts that host rebuild; it counts host rebuilds only).  Before the swap the new qnodes
 * are measured by the kernel of "tree cost": leaf_slots must equal the triangle count and inner_children + 1 the node
 * count, else the call returns HPT_ERR_DEVICE with a message and the handle is as it was.  A failed allocation
 * (HPT_ERR_NOMEM) leaves the handle as it was too.  A scene that was never updated gets its device vertices here, exactly
 * as from a first update.
 *
 * A device build is not an update: everything "rebuild" above lists as kept is kept, and every integrator renders the
 * same bytes afterwards.  A later update, pose, skin or morph refits the new topology (the export then equals
 * hpt_bvh_device_build_host with new_triangles).  hpt_stats.bvh_nodes, bvh_depth and ms_bvh_build become the new tree's.
 *
 * hpt_scene_get_device_build_info describes the last call (zeros before the first): how many calls have succeeded, fallen
 * back ones included; whether the last fell back; node count and depth before and after; wide_depth; and the milliseconds
 * between HIP events of the keys and the sort, of the radix tree with the numbering and the permutation, of the refit, and
 * of the collapse with the wide boxes and the frames (zeros after a fallback).  The numbering reads 4 bytes back per level.
 * hpt_bvh_device_build_host fills the fields that describe the tree (builds = 1, fell_back as the device would decide,
 * the after-counts, wide_depth) and zeros the rest; its info may report a bvh_depth above 30.  Its conventions are those
 * of hpt_bvh_refit_host: it builds from `triangles`, refits that topology to new_triangles when they are given (NULL: no
 * refit), and exports as hpt_bvh_export_host does.
 *
 * hpt_scene_rebuild_device returns HPT_ERR_INVALID with a message, before the device is touched, for a null scene or a
 * current device other than the scene's.  A scene of zero triangles accepts the call and counts it.
 *
 * Out of scope: a tree of the host builder's quality (PLOC, treelet optimisation, spatial splits); building at
 * hpt_scene_create; hpt_multi_* and the scene the one-shot wrappers keep; a caller-stream or non-blocking variant;
 * exporting the four-wide tree; any automatic policy inside the library (pt_cli --rebuild-device is a caller's).
 * "Bounded device builds" below bound the depth of this tree; the tree's quality is unchanged by them. */
typedef struct hpt_device_build_info {
    uint64_t builds;
    uint32_t fell_back, nodes_before, nodes_after, depth_before, depth_after, wide_depth;
    double ms_sort, ms_topology, ms_refit, ms_collapse;
} hpt_device_build_info;
int hpt_scene_rebuild_device(hpt_scene *scene);
int hpt_scene_get_device_build_info(const hpt_scene *scene, hpt_device_build_info *out);
int hpt_bvh_device_build_host(const void *lights, int num_lights, const void *spheres, int num_spheres, const void *triangles,
                              const void *new_triangles, int num_triangles, hpt_bvh_info *info, hpt_device_build_info *binfo,
                              void *qnodes_out, size_t qnodes_cap, void *tris_out, size_t tris_cap);

/* ---- bounded device builds ---------------------------------------------------------------------------------------
 * hpt_scene_rebuild_device_bounded is hpt_scene_rebuild_device with a tree of at most max_depth levels, so that the depth
 * of the data's radix tree never sends the call to the host builder.  hpt_bvh_device_build_bounded_host is its
 * definition, on the host alone, and the device is held to its bytes.  Keys, order, leaf codes, numbering, boxes, grid,
 * qnodes and the four-wide twin are those of "device builds"; only the topology differs, and it is made top-down.
 *
 * max_depth.  0 means 30.  Otherwise it must lie in [need(num_triangles), 30], where need(count) is the smallest k >= 1
 * with 2^k >= (count + 1) / 2 (1 up to four triangles): the levels a balanced tree of full leaves takes.
 * A node at level d (the root is level 0) covers the sorted positions [first, first + count), count > 2.  With D the
 * effective max_depth, need(count) <= D - d holds at the root and is kept by both splits:
 *   forced, when need(count) == D - d: the left child gets 2 * ((leaves + 1) / 2) triangles, leaves = (count + 1) / 2,
 *     the right child the rest -- every leaf below is full but possibly the last (the host builder's rule at its limit);
 *   radix, otherwise: with last = first + count - 1 and gamma the largest p in [first, last) for which
 *     delta(first, p) > delta(first, last), the left child gets gamma - first + 1 triangles.  On sorted pairs
 *     delta(first, p) does not increase with p, so gamma is found by bisection, also in ranges below a forced node,
 *     which the radix tree never had.
 * A child of 2 triangles or fewer is a leaf code, any other an inner node at level d + 1.  Two triangles or fewer give
 * the one-node trees of "device builds".
 * What follows: bvh_depth <= D always; and while no node is forced every range is one of the radix tree's and every
 * split the radix tree's, so a build with forced_nodes == 0 equals hpt_bvh_device_build_host byte for byte.
 *
 * The device numbers the tree level by level as before (count, scan, scatter; 4 bytes read back per level), each node
 * carrying its range; the host's loop ends after D levels.  Inner nodes left at that point are impossible by the rule
 * above: the call then returns HPT_ERR_DEVICE ("internal error") and the handle is as it was.  The guard of "device
 * builds" runs unchanged.  The one fallback left is a four-wide twin too deep for the resume launch's stack
 * (wide_depth > 19), handled as there (hpt_scene_rebuild, fell_back = 1).  A wide level spans a binary level at least, so
 * wide_depth <= bvh_depth: a build with max_depth <= 19 can never fall back, and such a depth is accepted up to 2^20
 * triangles.
 *
 * The call fills hpt_device_build_info as hpt_scene_rebuild_device does (hpt_scene_get_device_build_info describes the
 * last device build of either kind) and hpt_bounded_build_info: the effective max_depth, the number of forced nodes and
 * the first level that has one (0xFFFFFFFF when none was forced).  hpt_scene_get_bounded_build_info gives zeros before
 * the first bounded call.  hpt_bvh_device_build_bounded_host takes hpt_bvh_device_build_host's arguments and
 * conventions, then max_depth and the record to fill (may be NULL); its binfo->fell_back is 1 exactly when
 * wide_depth > 19.
 *
 * hpt_scene_rebuild_device_bounded returns HPT_ERR_INVALID with a message, before the device is touched, for a null
 * scene, a max_depth outside the values above, or a current device other than the scene's.
 *
 * Out of scope: a forced split chosen by position or area (it is by count, on the Morton order); raising the
 * traversal's 30 levels; everything "device builds" leaves out. */
typedef struct hpt_bounded_build_info { uint32_t max_depth, forced_nodes, first_forced_level, reserved; } hpt_bounded_build_info;
int hpt_scene_rebuild_device_bounded(hpt_scene *scene, int max_depth);
int hpt_scene_get_bounded_build_info(const hpt_scene *scene, hpt_bounded_build_info *out);
int hpt_bvh_device_build_bounded_host(const void *lights, int num_lights, const void *spheres, int num_spheres, const void *triangles,
                                      const void *new_triangles, int num_triangles, hpt_bvh_info *info, hpt_device_build_info *binfo,
                                      void *qnodes_out, size_t qnodes_cap, void *tris_out, size_t tris_cap, int max_depth,
                                      hpt_bounded_build_info *bbinfo);

#ifdef __cplusplus
}
#endif
#endif /* HPT_H */
