/*
 * tdk_hip_wavelet.h -- a-trous wavelet-shrinkage denoiser of libtdk_hip.so with a luma/chroma mode, which the reference does not
 * have.
 *
 * include/tdk_hip.h (the reference's surface), include/tdk_hip_ext.h, include/tdk_hip_denoise.h, include/tdk_hip_resample.h,
 * include/tdk_hip_warp.h, include/tdk_hip_raw.h and include/tdk_hip_sharpen.h stay pinned; the wavelet denoiser is declared here,
 * with its own version number.  The conventions of tdk_hip.h apply: device pointers, a HIP stream per call, TDK_OK or a tdk_status
 * code with the message in tdk_last_error(), nothing allocates device memory.
 *
 * ---- Specification.  All arithmetic is float32, one rounding per written operation, no contraction (no FMA); parentheses and
 * the stated order give the order of operations.
 *
 * The frame is (height, width, channels), interleaved, channels 1 or 3, dtype TDK_F32 or TDK_F16, the same on both sides (no
 * uint8: the operator runs on linear data).  x[c] is the source value of channel c converted to float32 (exact).
 *
 * Working space: v[k] is the working value of working-space channel k.
 *   without a flag           v[c] = x[c]                              (k is the frame channel c)
 *   with TDK_WAVELET_YCC     (channels = 3 only; k = 0, 1, 2 is Y, Cb, Cr)
 *                            Y  = (0.25f*r + 0.5f*g) + 0.25f*b
 *                            Cb = b - g
 *                            Cr = r - g
 *   inverse before the store g = Y - 0.25f*(Cb + Cr)
 *                            r = Cr + g
 *                            b = Cb + g
 *
 * Scales: S in 1..TDK_WAVELET_MAX_SCALES.  c_0 = v; for s = 0..S-1, with the step p = 1 << s:
 *   Every index is clamped to the frame (replicate) at EVERY scale: c_s exists only inside the frame, and c_s at a clamped index is
 *   the value at the edge pixel -- not a filter applied to a replicated c_{s-1} beyond the edge.
 *   horizontal   h = (0.0625f*(c_s[-2p] + c_s[+2p]) + 0.25f*(c_s[-p] + c_s[+p])) + 0.375f*c_s[0]
 *   vertical     the same formula applied to h along the other axis gives c_{s+1}
 *   detail       d_s = c_s - c_{s+1}
 *   threshold    t = threshold[s*channels + k], finite and >= 0
 *   shrinkage    d'_s = |d_s| > t ? copysignf(|d_s| - t, d_s) : 0
 *
 * Result, summed finest first:   acc = d'_0;   acc = acc + d'_s for s = 1..S-1;   y = acc + c_S
 *
 * Store: float32 as it is; binary16 rounded to nearest even.  There is no clamp.
 *
 * Limits: inputs must be finite; sizes 1..65535 per axis; src and dst must not overlap; buffers are contiguous at any element
 * alignment.
 */
#ifndef TDK_HIP_WAVELET_H
#define TDK_HIP_WAVELET_H

#include <stddef.h>

#include "tdk_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TDK_WAVELET_ABI_VERSION 1

/* flags of tdk_wavelet */
#define TDK_WAVELET_YCC 1

#define TDK_WAVELET_MAX_SCALES 5

int tdk_wavelet_abi_version(void);

/* Noise gain of each detail band.  Host only.  n_s is the L2 norm of the two-dimensional impulse response of d_s away from the
 * borders (what white noise of sigma 1 in c_0 leaves in d_s), computed in double from the taps and rounded once to float32.
 * scales in 1..5; norms receives TDK_WAVELET_MAX_SCALES values, those beyond scales are 0. */
int tdk_wavelet_band_norms(int scales, float* norms /* 5 */);

/* Bytes of device workspace one call needs: 0 where the first launch finishes the frame (scales <= 2), and 0 for arguments
 * tdk_wavelet would reject.  The workspace holds float32 planes whatever the storage type. */
size_t tdk_wavelet_workspace_bytes(int width, int height, int channels, int scales);

/* ---- The denoiser (csrc/wavelet.hip).  thresholds is a HOST pointer to scales*channels floats, read during the call; they travel
 * as kernel arguments.  At most max(1, scales - 1) launches, no allocation, no atomics, no synchronisation -- capturable in a graph
 * from the first call, and deterministic.  workspace: tdk_wavelet_workspace_bytes bytes of device memory at any alignment, owned by
 * the call until its last launch has finished (one workspace per stream); it may be null where that size is 0.  Argument errors
 * (null pointers, sizes, channels, dtype, scales, thresholds, flags, TDK_WAVELET_YCC with one channel, overlap, a null workspace
 * where one is needed) are reported before any HIP call. */
int tdk_wavelet(const void* src, void* dst, void* workspace, int width, int height, int channels, int dtype, int scales, const float* thresholds,
                int flags, tdk_stream_t stream);

/* The largest LDS use, in bytes, of a workgroup over the launches of such a call; at most 64 KB.  Host query; 0 for arguments
 * tdk_wavelet would reject. */
size_t tdk_wavelet_lds_bytes(int channels, int dtype, int scales, int flags);

#ifdef __cplusplus
}
#endif
#endif
