// Launch interface of the progressive-display kernels (display_kernels.hip): the running sum over frames and the 8-bit
// present with its frame-to-frame metrics (include/hpt.h, "progressive display").
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace hpt {

// sum[i] = sum[i] + frame[i]; with sq, sq[i] = sq[i] + frame[i] * frame[i]; with mean_out, mean_out[i] = sum[i] / k.
// n values; mean_out may be frame itself.  16-byte accesses where frame and mean_out allow them, a scalar tail.
void launch_accum_add(hipStream_t s, float *sum, float *sq, const float *frame, float *mean_out, uint32_t n, float k);
// variance == 0: out[i] = sum[i] / k.  Else m = sum[i] / k, q = sq[i] / k, out[i] = fmaxf(q - m * m, 0) / km1.
void launch_accum_resolve(hipStream_t s, const float *sum, const float *sq, float *out, uint32_t n, float k, float km1, int variance);

struct PresentArgs {
    const float *linear;         // 3 W H canonical values (RGB, row 0 = top)
    const float *thresholds;     // the 256-entry table of hpt_tonemap_table, on the device
    uint32_t *last;              // (3 W H + 3) / 4 packed words; the padding bytes of the final word are kept 0
    const uint32_t *other_last;  // another display's `last`, or null
    unsigned long long *metrics; // [0] += ssd_prev, [1] += ssd_other; zeroed by the caller before the launch
    unsigned char *out;          // the panel's first byte (row 0, x_offset applied), or null
    long long pitch;             // bytes between output rows
    int W, H;
    int has_prev;                // 0: the first present, ssd_prev stays 0
    int bgr, flip;
};
// one lane per word of `last`; the grid depends on W and H only
void launch_present(hipStream_t s, const PresentArgs &a);

} // namespace hpt
