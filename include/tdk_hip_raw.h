/*
 * tdk_hip_raw.h -- sensor correction at the head of the chain of libtdk_hip.so (black and white level, defective pixels, lens
 * shading, white balance), which the reference does not have.
 *
 * include/tdk_hip.h (the reference's surface), include/tdk_hip_ext.h, include/tdk_hip_denoise.h, include/tdk_hip_resample.h and
 * include/tdk_hip_warp.h stay pinned; the raw stage is declared here, with its own version number.  The conventions of tdk_hip.h
 * apply: device pointers, a HIP stream per call, TDK_OK or a tdk_status code with the message in tdk_last_error(), nothing
 * allocates device memory.
 *
 * ---- Specification.  All arithmetic is float32, one rounding per written operation, no contraction; parentheses give the order;
 * divisions are correctly rounded.
 *
 * The frame is width x height, both even, 2..65535.  Row i, column j has the CFA position p = 2*(i & 1) + (j & 1); the Bayer
 * pattern word maps p to a colour (0 = R, 1 = G, 2 = B) as everywhere in tdk_hip.h: (pattern >> (2*p)) & 3.
 *
 * Input forms (src_format):
 *   TDK_RAW_PACKED12      12-bit packed bytes, two pixels in three: p0 = ((b1 & 15) << 8) | b0,  p1 = (b2 << 4) | (b1 >> 4)
 *   TDK_RAW_PACKED12_IDS  the same with the IDS nibble order:       p0 = (b0 << 4) | (b2 & 15),  p1 = (b1 << 4) | (b2 >> 4)
 *   TDK_RAW_U16           (height, width) uint16 codes
 *   TDK_RAW_F32, TDK_RAW_F16   (height, width) float32 / binary16
 * raw is the code, or the stored float, converted exactly to float32.  The result is (height, width) float32 or binary16
 * (dst_dtype TDK_F32 / TDK_F16), rounded to nearest even once at the store.
 *
 * Step 1, linearise:
 *   L = (raw - black[p]) * scale[p]
 * black and scale are HOST pointers to four floats each (scale[p] = 1 / (white - black[p]), formed by the caller in float64 and
 * rounded once); their units are code units for the integer forms and the float's own units for the float forms.
 *
 * Step 2, defective pixels (defects = TDK_RAW_HOT | TDK_RAW_DEAD, or 0: step skipped).  Decided on the L values of the uncorrected
 * frame, so the result is a pure function of the input.  n0..n3 are the L values of the same-colour neighbours
 * (i-2, j), (i+2, j), (i, j-2), (i, j+2), visited in this order; a neighbour outside the frame is missing and never counts.
 *   hot rule  (TDK_RAW_HOT):   if L > threshold:  S = { n : n < L*ratio };  if |S| >= min_count:  v = max(S), mask = 1
 *   dead rule (TDK_RAW_DEAD):  only where the hot rule did not fire:
 *                              S = { n : n > threshold and L < n*ratio };  if |S| >= min_count:  v = min(S), mask = 2
 *   otherwise v = L, mask = 0.
 * Comparisons are IEEE as written: a NaN is never corrected and never counts.  max(S) / min(S) start from the first member and
 * replace the held value only where a later member is strictly greater / smaller.
 * mask (optional): (height, width) uint8 of 0, 1, 2.  With mask given and defects = 0 it is written as zeros.
 *
 * Step 3, lens shading (shading != NULL).  shading is (grid_height, grid_width, 4) float32 on the device: a gain per CFA position
 * p at every node.  Node (0, 0) sits on pixel (0, 0) and node (grid_height-1, grid_width-1) on pixel (height-1, width-1) (the
 * semantics of a DNG GainMap).  Positions are integers:
 *   t = j*(gw - 1);  qx = t / (W - 1);  rx = t % (W - 1);  ax = (float)rx / (float)(W - 1);  qx1 = min(qx + 1, gw - 1)
 *   (likewise qy, ay, qy1 from i, gh and H)
 *   g0 = G[qy][qx][p]*(1.0f - ax) + G[qy][qx1][p]*ax
 *   g1 = G[qy1][qx][p]*(1.0f - ax) + G[qy1][qx1][p]*ax
 *   g  = g0*(1.0f - ay) + g1*ay
 *   v  = v*g
 * Limits: gw, gh in 2..257 with 4*(gw - 1) <= W - 1 and 4*(gh - 1) <= H - 1 (nodes at least four pixels apart).
 *
 * Step 4, white balance and clip.  gains is a device pointer to three floats (R, G, B) or NULL, as tdk_apply_white_balance takes
 * it.  With gains:  v = min(max(v*gains[colour], 0.0f), 1.0f)  (fmaxf, fminf: a NaN becomes 0).  With gains NULL and clip != 0:
 * v = min(max(v, 0.0f), 1.0f); with clip = 0 the value is stored as it is.
 *
 * Identity: black = 0, scale = 1.0f/4095.0f, nothing else enabled and clip = 0 gives a packed frame the bits of tdk_decode12_f32
 * (scaled); with gains added, the bits of tdk_apply_white_balance on that.
 *
 * Buffers are contiguous at any element alignment; dst and mask must not overlap each other, src, shading or gains.
 */
#ifndef TDK_HIP_RAW_H
#define TDK_HIP_RAW_H

#include <stddef.h>

#include "tdk_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TDK_RAW_ABI_VERSION 1

/* src_format of tdk_raw_prepare */
#define TDK_RAW_PACKED12 0
#define TDK_RAW_PACKED12_IDS 1
#define TDK_RAW_U16 2
#define TDK_RAW_F32 3
#define TDK_RAW_F16 4

/* defects of tdk_raw_prepare */
#define TDK_RAW_HOT 1
#define TDK_RAW_DEAD 2

int tdk_raw_abi_version(void);

/* ---- The raw stage (csrc/rawprepare.hip).  One launch, no workspace, no atomics, no synchronisation, no table from the host:
 * black, scale and every parameter travel as kernel arguments -- capturable in a graph from the first call, and deterministic.
 * Argument errors (null pointers, sizes, odd width or height, format and dtype tags, pattern, non-finite black or scale, defects,
 * threshold, ratio, min_count, grid limits, clip, overlap) are reported before any HIP call. */
int tdk_raw_prepare(const void* src, int src_format, void* dst, int dst_dtype, unsigned char* mask, int width, int height, uint32_t pattern,
                    const float* black, const float* scale, int defects, float threshold, float ratio, int min_count, const float* shading,
                    int grid_width, int grid_height, const float* gains, int clip, tdk_stream_t stream);

/* LDS bytes one workgroup of tdk_raw_prepare takes: 0 for the plain streaming form (no defects, no mask, no shading), the tile with
 * its apron for defects != 0 (or a mask), the grid records and nodes for shading != 0; at most 64 KB.  Host query. */
size_t tdk_raw_prepare_lds_bytes(int defects, int shading);

#ifdef __cplusplus
}
#endif
#endif
