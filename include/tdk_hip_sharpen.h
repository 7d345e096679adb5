/*
 * tdk_hip_sharpen.h -- output sharpening of libtdk_hip.so (unsharp mask with a soft threshold and a halo limit), which the
 * reference does not have.
 *
 * include/tdk_hip.h (the reference's surface), include/tdk_hip_ext.h, include/tdk_hip_denoise.h, include/tdk_hip_resample.h,
 * include/tdk_hip_warp.h and include/tdk_hip_raw.h stay pinned; the sharpener is declared here, with its own version number.  The
 * conventions of tdk_hip.h apply: device pointers, a HIP stream per call, TDK_OK or a tdk_status code with the message in
 * tdk_last_error(), nothing allocates device memory.
 *
 * ---- Specification.  All arithmetic is float32, one rounding per written operation, no contraction (no FMA); parentheses and
 * the stated order give the order of operations.
 *
 * The frame is (height, width, channels), interleaved, channels 1 or 3, dtype TDK_F32, TDK_F16 or TDK_U8 (of tdk_hip_resample.h),
 * the same on both sides.  x[c] is the source value of channel c converted to float32 (exact for all three storage types).
 * scale = 255 for TDK_U8 and 1 for the float types.  An index outside the frame is clamped to the edge (replicate), everywhere.
 *
 * Signal s:
 *   without TDK_SHARPEN_LUMA   s = x[c]: every channel is processed on its own
 *   with TDK_SHARPEN_LUMA      (channels = 3 only)   s = (0.2126729f*r + 0.7151522f*g) + 0.0721750f*b
 *
 * Blur b: symmetric taps w[0..R], 1 <= R <= 12, given by the caller as R + 1 float32 values.
 *   horizontal   h = w[0]*s[0];   for k = 1..R in ascending order:   h = h + w[k]*(s[-k] + s[+k])
 *   vertical     the same formula applied to h along the other axis gives b
 * The intermediate h stays float32.
 *
 * Detail and soft threshold (the rule of darktable's sharpen module):
 *   d  = s - b
 *   t  = threshold_eff = (float)threshold * scale          (formed on the host, in float32)
 *   d' = |d| > t ? copysignf(|d| - t, d) : 0
 *
 * Result:
 *   y[c] = x[c] + amount * d'          (with TDK_SHARPEN_LUMA the same amount * d' is added to all three channels)
 *
 * Halo limit (TDK_SHARPEN_LIMIT): lo[c] and hi[c] are the minimum and maximum of x[c] over the 3x3 neighbourhood;
 *   o = (float)overshoot * scale          (formed on the host, in float32)
 *   y[c] = fminf(fmaxf(y[c], lo[c] - o), hi[c] + o)
 *
 * Store: float32 as it is; binary16 rounded to nearest even; uint8 rint() after clamping to [0, 255].  Float results are not
 * clamped.  amount == 0 stores x[c] itself: the input's bits come back (-0 included).
 *
 * Limits: inputs must be finite; sizes 1..65535 per axis; amount in [0, 16]; threshold and overshoot finite and >= 0 (overshoot is
 * read only with TDK_SHARPEN_LIMIT); weights finite and >= 0; src and dst must not overlap; buffers are contiguous at any element
 * alignment.
 */
#ifndef TDK_HIP_SHARPEN_H
#define TDK_HIP_SHARPEN_H

#include <stddef.h>

#include "tdk_hip.h"
#include "tdk_hip_resample.h" /* TDK_U8 */

#ifdef __cplusplus
extern "C" {
#endif

#define TDK_SHARPEN_ABI_VERSION 1

/* flags of tdk_sharpen */
#define TDK_SHARPEN_LUMA 1
#define TDK_SHARPEN_LIMIT 2

#define TDK_SHARPEN_MAX_RADIUS 12

int tdk_sharpen_abi_version(void);

/* Gaussian taps for tdk_sharpen.  Host only.  sigma in [0.25, 4];  R = ceil(3*sigma), formed in double from the float32 value
 * of sigma (so 1 <= R <= 12);  w_k = exp(-k*k / (2*sigma*sigma)) / (w_0 + 2 * sum_{k >= 1} w_k), computed in double, summed in
 * ascending k, and rounded once to float32.  weights receives TDK_SHARPEN_MAX_RADIUS + 1 values, those beyond R are 0. */
int tdk_sharpen_weights(float sigma, float* weights /* 13 */, int* radius);

/* ---- The unsharp mask (csrc/sharpen.hip).  weights is a HOST pointer to radius + 1 floats, read during the call; the taps and
 * every parameter travel as kernel arguments: one launch, no workspace, no table in device memory, no atomics, no synchronisation
 * -- capturable in a graph from the first call, and deterministic.  Argument errors (null pointers, sizes, channels, dtype, radius,
 * weights, amount, threshold, overshoot, flags, TDK_SHARPEN_LUMA with one channel, overlap) are reported before any HIP call. */
int tdk_sharpen(const void* src, void* dst, int width, int height, int channels, int dtype, const float* weights, int radius, float amount,
                float threshold, float overshoot, int flags, tdk_stream_t stream);

/* LDS bytes one workgroup of tdk_sharpen takes (the signal of the tile with its radius-pixel apron and the horizontally blurred
 * plane); at most 64 KB.  Host query; 0 for arguments tdk_sharpen would reject. */
size_t tdk_sharpen_lds_bytes(int channels, int dtype, int radius, int flags);

#ifdef __cplusplus
}
#endif
#endif
