/*
 * tdk_hip_temporal.h -- temporal denoiser (libtdk_hip.so): a motion-adaptive recursive filter on raw Bayer mosaics.  Per site it
 * keeps a running average of the frames of a stream and an effective frame count; a window statistic of the squared frame
 * difference against the variance of the noise model of tdk_hip_noise.h tells where the scene moved, and the average restarts
 * there.  A static site averaged over n frames loses a factor n of variance and no detail.  The reference has no counterpart.
 *
 * The filter acts on raw mosaics only, in front of the demosaic: there the noise of neighbouring sites is independent and the model
 * var(x) = a*x + b is exact.
 *
 * include/tdk_hip.h (the reference's surface) and the other tdk_hip_*.h headers stay pinned; the temporal block is declared here,
 * with its own version number.  The conventions of tdk_hip.h apply: device pointers, a HIP stream per call, TDK_OK or a tdk_status
 * code with the message in tdk_last_error(), nothing allocates device memory.
 *
 * ---- Specification (tdk_temporal_denoise).  Per-value arithmetic is float32, one rounding per written operation, no contraction
 * (no FMA), correctly rounded division.  fmaxf and fminf of a NaN and a number give the number.
 *
 * Input.  An (height, width) mosaic, width and height even, 2..65535, float32 or float16, converted exactly to float32, contiguous
 * at any element alignment; the Bayer pattern word of tdk_hip.h.  model: the 12 device floats of tdk_hip_noise.h (per colour a, b,
 * valid, usable bins); gains: 3 device floats or NULL.  Site (i, j) has the CFA position p = 2*(i & 1) + (j & 1) and the colour
 * k = (pattern >> (2*p)) & 3, as in tdk_noise_stabilize; (a, b, valid) is row k of the model.  With g the gain of the row (1 when
 * gains is NULL):
 *   a' = g * a;   b' = (g * g) * b
 * A row is invalid when its valid field is 0.
 *
 * Host parameters, each a float32: radius r is 2 or 3; 0 < t_lo < t_hi, both finite, and inv = fl32(1 / (t_hi - t_lo)) must be
 * finite; c2 = pixel_c2 > 0, the square of the per-site threshold, +inf when the per-site test is off; 1 <= n_max <= 64;
 * v_min > 0, finite.
 *
 * State.  One device buffer of tdk_temporal_state_bytes(width, height, state_dtype) bytes, aligned to 16 bytes.  With
 * PA = align16(width * height * sizeof(state_dtype)) and PC = align16(width * height * 2):
 *   offset 0:                 a head of TDK_TEMPORAL_HEAD_BYTES = 16 bytes; its first word is the frame index idx (uint32), the
 *                             other three words are not used
 *   offset 16:                acc[0]      offset 16 + PA:            acc[1]        (state_dtype: float32 or float16)
 *   offset 16 + 2*PA:         cnt[0]      offset 16 + 2*PA + PC:     cnt[1]        (always binary16)
 *   tdk_temporal_state_bytes = 16 + 2*PA + 2*PC
 * A call with the index idx reads the planes (idx + 1) & 1 and writes the planes idx & 1, then advances the index: idx = idx + 1,
 * and 0xFFFFFFFF -> 2.  idx == 0 means "no history": the planes are not trusted then.  tdk_temporal_reset writes idx = 0 and
 * nothing else; the planes are never cleared.
 *
 * Per site q, x its sample, first = (idx == 0):
 *   A = first ? 0 : (float)acc_src[q]        N = first ? 0 : (float)cnt_src[q]
 *   d = x - A
 *   valid row:    var = fmaxf(a' * fmaxf(A, 0) + b', v_min);   v = var + var / fmaxf(N, 1);   e = d * d
 *   invalid row:  v = 0;  e = 0
 *
 * Window.  The sites of rows i-r..i+r and columns j-r..j+r that lie inside the frame, all CFA colours mixed.  Row sums first, over
 * the in-frame columns in ascending order, starting at 0.0f; then the sum of the row sums over the in-frame rows in ascending
 * order, starting at 0.0f: E (of e) and V (of v).  A sliding sum that adds and subtracts has other bits and is not the
 * specification.  (No e or v is -0, so a sum that also adds +0.0f for the sites outside the frame has the same bits.)
 *   t  = E / V
 *   s  = fminf(fmaxf((t_hi - t) * inv, 0), 1)          (a NaN t gives 0)
 *   if (e > c2 * v) s = 0                               (a false comparison leaves s)
 *   n1 = fminf(s * N + 1, n_max);   invalid row: n1 = 1
 *   y  = (n1 == 1) ? x : A + d / n1
 *   acc_dst[q] = y rounded once to state_dtype;  cnt_dst[q] = n1 rounded to binary16;  out[q] = y rounded once to out_dtype
 * out is float32 or float16 and shares nothing with src or the state.
 *
 * Consequences.  On the first frame out == x.  With n_max == 1 out == x always.  A NaN or infinite sample resets the sites whose
 * window holds it, and the state is finite again one frame later, since y = x whenever n1 == 1.
 *
 * Decisions the issue left open: the valid field is tested against 0, nothing else of the model is checked on the device; the three
 * unused words of the head are never written; pixel_c2 is given squared, so the host squares once in float32; an all-invalid window
 * has t = 0/0 and therefore s = 0.
 */
#ifndef TDK_HIP_TEMPORAL_H
#define TDK_HIP_TEMPORAL_H

#include <stddef.h>

#include "tdk_hip.h"
#include "tdk_hip_noise.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TDK_TEMPORAL_ABI_VERSION 1

/* The output tile of a workgroup of the filter launch: TDK_TEMPORAL_TILE_H rows of TDK_TEMPORAL_TILE_W sites. */
#define TDK_TEMPORAL_TILE_W 64
#define TDK_TEMPORAL_TILE_H 32
#define TDK_TEMPORAL_HEAD_BYTES 16
#define TDK_TEMPORAL_MAX_FRAMES 64

int tdk_temporal_abi_version(void);

/* Bytes of the state buffer (layout above).  0 for arguments tdk_temporal_denoise would reject. */
size_t tdk_temporal_state_bytes(int width, int height, int state_dtype);

/* Static LDS bytes of a workgroup of the filter launch: two staged planes (e, v) of (TILE_H + 2r) x (TILE_W + 8) floats and two
 * planes of row sums of (TILE_H + 2r) x TILE_W floats.  0 for a radius tdk_temporal_denoise would reject. */
size_t tdk_temporal_lds_bytes(int radius);

/* One one-lane launch on `stream`: idx = 0.  Argument errors (null pointer, alignment of state) are reported before any HIP call. */
int tdk_temporal_reset(void* state, tdk_stream_t stream);

/* Exactly two launches on `stream`: the filter (every workgroup reads idx as a uniform value), then a one-lane kernel that advances
 * idx.  No allocation, copy, memset, synchronisation or atomic: capturable in a graph from the first call, replayable any number of
 * times (the parity lives on the device), bit-reproducible.  Argument errors (null pointers, sizes, dtype tags, pattern, radius, the
 * five parameters, the 16-byte alignment of state, overlap of src / out / state / model / gains) are reported before any HIP call. */
int tdk_temporal_denoise(const void* src, int src_dtype, void* out, int out_dtype, void* state, int state_dtype, int width, int height, uint32_t pattern,
                         const float* model, const float* gains, int radius, float t_lo, float t_hi, float pixel_c2, float n_max, float v_min,
                         tdk_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
