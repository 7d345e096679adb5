/*
 * tdk_hip_resample.h -- image scaling of libtdk_hip.so, which the reference does not have.
 *
 * include/tdk_hip.h (the reference's surface), include/tdk_hip_ext.h (the device-resident JPEG encode) and
 * include/tdk_hip_denoise.h (non-local means) stay pinned; the scaler is declared here, with its own version number.  The
 * conventions of tdk_hip.h apply: device pointers, a HIP stream per call, TDK_OK or a tdk_status code with the message in
 * tdk_last_error(), nothing allocates device memory.
 */
#ifndef TDK_HIP_RESAMPLE_H
#define TDK_HIP_RESAMPLE_H

#include "tdk_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TDK_RESAMPLE_ABI_VERSION 1

/* storage tag of 8-bit unsigned images, beside TDK_F32 (0) and TDK_F16 (1) of tdk_hip.h; only the entry points below take it */
#define TDK_U8 2

int tdk_resample_abi_version(void);

/* ---- Antialiased bilinear scaling (csrc/resample.hip).  src: (src_height, src_width, channels), dst: (dst_height, dst_width,
 * channels), interleaved, channels 1 or 3, the same dtype TDK_F32, TDK_F16 or TDK_U8 on both sides, contiguous at any element
 * alignment; they must not overlap.  Along one axis with n_in source samples and n_out results, for output index i:
 *   s = n_in / n_out        r = max(s, 1)        c = s (i + 1/2)
 *   w_j = max(0, 1 - |j + 1/2 - c| / r)     for j in [0, n_in)
 *   y_i = sum_j w_j x_j / sum_j w_j
 * The 2-D result is the horizontal pass followed by the vertical pass; the intermediate stays float32 and is not rounded to the
 * storage type.  Arithmetic is float32 with one rounding at the store: binary16 to nearest even, uint8 rint() after clamping to
 * [0, 255].  j + 1/2 - c is formed from integers, (2 n_out j + n_out - (2 i + 1) n_in) / (2 n_out), so positions up to 65535
 * lose nothing; a tap at distance exactly r has weight 0.  n_out == n_in gives weight 1 on j = i: the input's bits come back.
 * Up-scaling (r = 1) is plain bilinear interpolation with the frame's edge replicated.
 * Sizes 1..65535 per axis on both sides; n_in / n_out <= 16 per axis (at most 32 taps); up-scaling is not limited otherwise.
 * Every parameter travels as a kernel argument and the weights are computed in the kernel: one launch, no workspace, no table
 * from the host, no synchronisation, no copy -- capturable in a graph from the first call, and deterministic (a fixed summation
 * order per value).  Argument errors (null pointers, sizes, ratio, channels, dtype, overlap) are reported before any HIP call. */
int tdk_resample(const void* src, void* dst, int src_width, int src_height, int dst_width, int dst_height, int channels, int dtype,
                 tdk_stream_t stream);

/* LDS bytes one workgroup of tdk_resample takes for this geometry (the output tile is sized from the ratio); at most 80 KB.
 * Host query; 0 for arguments tdk_resample would reject. */
size_t tdk_resample_lds_bytes(int src_width, int src_height, int dst_width, int dst_height, int channels, int dtype);

#ifdef __cplusplus
}
#endif
#endif
