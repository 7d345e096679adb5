/*
 * tdk_hip_denoise.h -- denoisers of libtdk_hip.so that the reference does not have.
 *
 * include/tdk_hip.h (the reference's surface) and include/tdk_hip_ext.h (the device-resident JPEG encode) stay pinned; the
 * spatial-domain denoiser is declared here, with its own version number.  The conventions of tdk_hip.h apply: device pointers
 * unless named host_*, a HIP stream per call, TDK_OK or a tdk_status code with the message in tdk_last_error(), nothing allocates
 * device memory.
 */
#ifndef TDK_HIP_DENOISE_H
#define TDK_HIP_DENOISE_H

#include "tdk_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TDK_DENOISE_ABI_VERSION 1

int tdk_denoise_abi_version(void);

/* ---- Non-local means (csrc/nlmeans.hip).  image, out: (height, width, channels) interleaved, channels 1 or 3, dtype TDK_F32 or
 * TDK_F16 storage (arithmetic is float32), contiguous at any element alignment; they must not overlap.  With clamp() replicating
 * the frame's edge and n = (2 patch_radius + 1)^2:
 *   D(p, d) = 1/n  sum_{t in [-P,P]^2} sum_c cw[c] (x_c(clamp(p+t)) - x_c(clamp(p+d+t)))^2
 *   w(p, d) = exp(-D(p, d) / h^2) if p+d lies inside the image, else 0
 *   y_c(p)  = sum_{d in [-S,S]^2} w(p,d) x_c(p+d) / sum_d w(p,d)
 * Patch samples are edge-replicated, candidates outside the image are skipped.  search_radius 1..10, patch_radius 1..4, h > 0 and
 * finite, host_channel_weights: `channels` values >= 0 in host memory, not all zero, read during the call (NULL: all 1).  Every
 * parameter travels as a kernel argument: one launch, no workspace, no synchronisation, no copy -- capturable in a graph from the
 * first call.  The result is deterministic (no atomics; a fixed summation order per pixel).  Argument errors are reported before
 * any HIP call. */
int tdk_nlmeans(const void* image, void* out, int width, int height, int channels, int dtype, int search_radius, int patch_radius, float h,
                const float* host_channel_weights, tdk_stream_t stream);

/* LDS bytes one workgroup of tdk_nlmeans stages its tile and halo in (host query; 0 for radii or channels out of range). */
size_t tdk_nlmeans_lds_bytes(int search_radius, int patch_radius, int channels);

#ifdef __cplusplus
}
#endif
#endif
