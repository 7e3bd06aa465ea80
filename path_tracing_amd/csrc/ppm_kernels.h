// Launch interface of the photon-mapping kernels (ppm_kernels.hip): the reference's ppm_cu.cu estimator, one pass =
// one eye pass + one photon pass + a gather, with the scatter of the reference replaced by a sorted grid.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include "hpt_scene.h"
#include "pt_kernels.h"

namespace hpt {

// random-stream keys of the two paths (distinct from PT's plain seed and BDPT's 0x4C49474854)
constexpr uint64_t kPpmEyeKey = 0x5050454945ull;       // "PPEIE"
constexpr uint64_t kPpmPhotonKey = 0x50504850484Full;  // "PPHPHO"

// Hit points of one pass, structure of arrays by eye path slot (= local pixel slot).
struct PpmHitBuf {
    float4 *pos_mat;     // position xyz | material index
    float4 *nrm;         // shading normal (faces the eye ray) xyz | unused
    float4 *wo;          // direction back to the camera xyz | unused
    float4 *thr;         // eye throughput xyz | unused
    uint32_t *list;      // compacted slots that hold a hit point
};

// Photon deposits.  dep[4 * slot + k], slot = photon * light_depth + depth:
//   k = 0 position xyz | cell x   1 photon hit normal xyz | cell y   2 direction to the light xyz | cell z   3 flux xyz | 0
// key[slot] = grid bucket of the deposit, or the table size (no deposit in that slot).
struct PpmGrid {
    float4 *dep;
    uint32_t *key, *slot_in, *key_sorted, *slot_sorted;
    float4 *packed;      // dep records in bucket order (ascending slot inside a bucket)
    uint2 *range;        // [bucket]: begin, end in `packed`
    uint32_t buckets;    // power of two
    void *sort_tmp; size_t sort_tmp_bytes;
};

struct PpmCounters {     // device counters, accumulated over the passes of a render
    unsigned long long photon_rays, deposits, hit_points, direct, candidates, accepted;
};

struct PpmFrame {        // what the photon and gather kernels need of the grid
    float smin[3], smax[3];
    float cell, r2;
    uint32_t buckets;
};

// PCG-keyed eye paths: launch_generate with seed ^ kPpmEyeKey, then per iteration launch_trace + this.  Writes the
// direct term into pb.col, hit points into hb (slot-indexed, list compacted through hp_count).
void launch_ppm_eye_shade(hipStream_t s, const SceneDev &sc, PathBuf pb, PpmHitBuf hb, const uint32_t *queue,
                          const uint32_t *qcount, uint32_t max_items, uint32_t *next_queue, uint32_t *next_count,
                          uint32_t *hp_count, int max_delta, PpmCounters *pc);
// photons: one per slot of [0, nl * spl), identity queue of that length in *qcount
void launch_ppm_emit(hipStream_t s, const SceneDev &sc, PathBuf pb, uint32_t *qcount, uint32_t n_photons, int spl,
                     uint64_t seed, uint32_t pass, PpmFrame fr);
void launch_ppm_photon_shade(hipStream_t s, const SceneDev &sc, PathBuf pb, PpmGrid g, const uint32_t *queue,
                             const uint32_t *qcount, uint32_t max_items, uint32_t *next_queue, uint32_t *next_count,
                             int light_depth, int max_delta, PpmFrame fr, PpmCounters *pc);
// grid over the deposits: stable radix sort of the bucket keys (slots ascending inside a bucket), bucket ranges,
// packed records.  sort_tmp_bytes: ppm_sort_tmp_bytes(n_slots, buckets)
size_t ppm_sort_tmp_bytes(uint32_t n_slots, uint32_t buckets);
int launch_ppm_grid(hipStream_t s, PpmGrid g, uint32_t n_slots);
// one lane per hit point: the 27 cells around it, summed in the defined order; resolves into pb.col.
// cand / acc (COUNT_WORK, else null): per hit point slot, the candidate and accepted pair counts
void launch_ppm_gather(hipStream_t s, const SceneDev &sc, PathBuf pb, PpmHitBuf hb, PpmGrid g, const uint32_t *hp_count,
                       uint32_t max_items, PpmFrame fr, uint32_t *cand, uint32_t *acc, PpmCounters *pc);
void launch_ppm_iota(hipStream_t s, uint32_t *p, uint32_t n);

// Progressive photon mapping (hpt_sppm, DESIGN.md "Progressive photon mapping"): per local pixel state that lasts
// across passes and calls.  The passes are PPM's (eye, photon, grid); only the gather and the image differ.
struct SppmState {
    float4 *tau_r2;      // accumulated flux tau xyz | squared radius R2
    float *photons;      // N
    float4 *direct;      // D, the sum of the guarded direct terms xyz | 0
};
// tau = 0, R2 = r2, N = 0, D = 0 for every local pixel
void launch_sppm_init(hipStream_t s, SppmState st, uint32_t n_local, float r2);
// one lane per hit point: the cells its sphere (R2 of its pixel) can reach, summed in PPM's order, and the pixel's
// update (alpha); cand / acc as launch_ppm_gather's.  fr.cell is the grid cell; fr.r2 is not read.
void launch_sppm_gather(hipStream_t s, const SceneDev &sc, PpmHitBuf hb, PpmGrid g, const uint32_t *hp_count, uint32_t max_items,
                        PpmFrame fr, SppmState st, float alpha, uint32_t *cand, uint32_t *acc, PpmCounters *pc);
// d_local[p] = the estimate after `passes` passes (divided when passes != 1)
void launch_sppm_estimate(hipStream_t s, const Tiling &tl, SppmState st, float passes, float *d_local);
// d_local[p] = (R2, N, 0), for launch_untile
void launch_sppm_state(hipStream_t s, const Tiling &tl, SppmState st, float *d_local);

} // namespace hpt
