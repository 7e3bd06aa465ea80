// Launch interface of the temporal-history kernel (history_kernels.hip): the per-pixel running mean that is carried over
// when the camera moves (include/hpt.h, "history across camera moves").
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace hpt {

// The constants project() reads (include/hpt.h), computed by the host in float from a camera (eye, UL, dx, dy).
struct HistoryCamera {
    float eye[3], a[3], nrm[3], gu[3], gv[3];
    float an;
};

// One set of per-pixel state: three 16-byte records per pixel, so a tap is three 16-byte loads.  (A history that keeps
// second moments has a fourth record per set, HistoryArgs::sq_prev / sq_next, and a tap is four loads.)
struct HistorySet {
    float4 *mean_n;      // mean.rgb, n
    float4 *pos_cov;     // position.xyz, coverage
    float4 *nrm;         // normal.xyz, 0
};

// kHistoryMotion: a frame that comes with the motion guide (include/hpt.h, "motion"), whatever the camera did
enum HistoryMode : int { kHistoryFirst = 0, kHistoryIdentity = 1, kHistoryMoved = 2, kHistoryMotion = 3 };

struct HistoryArgs {
    HistorySet prev, next;           // first / identity: the kernel works in place on `next` (prev == next)
    const float *frame;              // 3 W H
    const float *normal, *position;  // 3 W H each, or all three guides null
    const float *coverage;           // W H
    float *mean_out;                 // 3 W H or null; may be `frame`
    unsigned long long *metrics;     // [0] += kept, [1] += restarted; zeroed by the caller before the launch
    HistoryCamera cam, cam_prev;
    int W, H;
    int mode;                        // HistoryMode, the same for every lane
    float max_history_m1;            // max_history - 1
    float tol2;                      // plane_tolerance * plane_tolerance
    float normal_min;
    int plane_on, normal_on;
    // q.rgb, 0 of the two sets: the running mean of the squared frame values; both null without HPT_HISTORY_MOMENTS.  Kept
    // behind everything else, so the kernels without moments read the arguments they always read from where they always were.
    const float4 *sq_prev;
    float4 *sq_next;
    // kHistoryMotion only: where each pixel's guide point was one frame ago (3 W H), and whether the camera's bytes are
    // the previous advance's.  Last, for the same reason.
    const float *prev_position;
    int still;
};
// one lane per pixel; the grid depends on W and H only.  sq_next selects the kernels that carry the second moment.
void launch_history_advance(hipStream_t s, const HistoryArgs &a);

// out[3 p + c] = n[p] >= min_length ? fmaxf(q - m * m, 0) / (n - 1) : fallback ? fallback[3 p + c] : 0, one lane per pixel;
// `out` may be `fallback`
void launch_history_variance(hipStream_t s, const float4 *mean_n, const float4 *sq, const float *fallback, float *out, uint32_t npx,
                             float min_length);

// out[k] = in[3 k] for k < n: the coverage image out of the three-channel image launch_untile writes
void launch_take_first_channel(hipStream_t s, const float *in3, float *out, uint32_t n);

} // namespace hpt
