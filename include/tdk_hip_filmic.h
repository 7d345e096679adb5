/*
 * tdk_hip_filmic.h -- filmic: scene-referred tone mapping, a tone curve over log2 of a pixel norm applied to channel ratios
 * (libtdk_hip.so), which the reference does not have.
 *
 * The other headers under include/ stay pinned; the stage is declared here, with its own version number.  The conventions of
 * tdk_hip.h apply: device pointers unless a parameter says HOST, a HIP stream per call, TDK_OK or a tdk_status code with the message
 * in tdk_last_error(), nothing allocates device memory.
 *
 * A pixel's norm N (its largest channel, a luminance or a power norm) is looked up in a curve T sampled over log2(N); the pixel is
 * the curve's value times its channel ratios x_c / N, pulled towards 1 (grey) by the saturation D that the curve keeps at that
 * exposure, so that chromaticity survives the curve and highlights reach white achromatically.  The tables are the caller's
 * (torch_darktable.Filmic builds darktable's filmic spline and its sigmoid); black, grey, white and contrast live in them.
 *
 * ---- Specification.  All arithmetic is float32, one rounding per written operation, no contraction (no FMA); parentheses give the
 * order; divisions are correctly rounded.  fminf / fmaxf return the other operand for a NaN.  pos(v) = v > 0 ? v : +0 below, so a
 * NaN and -0 become +0.
 *
 * The frame is npix pixels of three interleaved values x_0, x_1, x_2.  The source is TDK_F32 or TDK_F16 (converted exactly); the
 * destination is TDK_F32, TDK_F16 or TDK_U8 (of tdk_hip_resample.h), chosen independently.
 * XMIN = 2^-20; XMAX = 4096 - 2^-12, the largest float32 below 2^12.
 *
 * 1. Exposure.  e = exposure[0], one float32 in device memory, read by every call.
 *      p_c = fminf(pos(x_c * e), XMAX)
 *    +-inf, NaN and negative samples are in the domain (inf * 0 is a NaN and becomes +0).  Denormal x_c, e or x_c * e are not, and
 *    under TDK_FILMIC_POWER neither are samples whose square or cube is denormal.
 *
 * 2. Norm.
 *      TDK_FILMIC_MAX     N = fmaxf(fmaxf(p0, p1), p2)
 *      TDK_FILMIC_LUMA    N = (w0*p0 + w1*p1) + w2*p2
 *      TDK_FILMIC_POWER   q_c = p_c*p_c      k_c = q_c*p_c
 *                         den = (q0 + q1) + q2      num = (k0 + k1) + k2
 *                         N = den > 0 ? num / den : +0
 *      TDK_FILMIC_NONE    every channel is its own norm: step 3 runs per channel with N = p_c, o_c = y, and steps 4 and 5 are skipped
 *
 * 3. Curve.  curve holds T (the display-linear value) in its first TDK_FILMIC_TABLE entries and D (the saturation kept, 0..1) in the
 *    next TDK_FILMIC_TABLE.  The tables cover TDK_FILMIC_EV_MIN .. TDK_FILMIC_EV_MAX in TDK_FILMIC_STEPS nodes per octave, spaced
 *    linearly inside an octave: node j stands at (1 + (j % 32) / 32) * 2^(j / 32 - 20).  The last entry of each table (node 1024, at
 *    2^12) is a guard: it is read with a weight below 1 only.
 *      Nc = fminf(fmaxf(N, XMIN), XMAX)
 *      ex = (bits(Nc) >> 23) - 127      M = bits(Nc) & 0x7FFFFF
 *      i  = (ex + 20)*32 + (M >> 18)    f = (float)(M & 0x3FFFF) / 262144
 *      y  = T[i] + f*(T[i+1] - T[i])
 *      d  = D[i] + f*(D[i+1] - D[i])
 *    No logarithm, power or exponential runs on the device.
 *
 * 4. Ratios.
 *      r_c = p_c / Nc
 *      s_c = 1 + d*(r_c - 1)
 *      o_c = y * s_c
 *
 * 5. Gamut.  m = fmaxf(fmaxf(o0, o1), o2).  Where m > 1:
 *      y >= 1:     o_c = 1
 *      otherwise:  g = (1 - y) / (m - y)      o_c = y + (o_c - y)*g
 *    The pixel is pulled towards the achromatic point of the same curve value until its largest channel is 1 (to within the rounding
 *    of the three operations).  With T <= 1 and D in 0..1 it never fires under TDK_FILMIC_MAX, where no ratio exceeds 1; it does
 *    under the other two norms.
 *
 * 6. Encoding.  encode is null (v_c = o_c) or the table G of TDK_FILMIC_ENC_TABLE values over 2^-16 .. 1, node j at
 *    (1 + (j % 32) / 32) * 2^(j / 32 - 16), the last one at 1:
 *      oc = fminf(pos(o_c), 1 - 2^-24)                      (the largest float32 below 1)
 *      oc <  2^-16:   v_c = (oc * 65536) * G[0]
 *      otherwise:     ex = (bits(oc) >> 23) - 127      M = bits(oc) & 0x7FFFFF
 *                     i  = (ex + 16)*32 + (M >> 18)    f = (float)(M & 0x3FFFF) / 262144
 *                     v_c = G[i] + f*(G[i+1] - G[i])
 *
 * 7. Store.  float32 as it is; binary16 rounded to nearest even, once; uint8 is rintf(fminf(fmaxf(v, 0.0f), 1.0f) * 255.0f), a NaN
 *    stores 0.
 *
 * What follows: under TDK_FILMIC_NONE with T[j] the position of node j, encode null and e = 1 the result has the bits of every source
 * value in [XMIN, XMAX] (the lerp is exact: a node's neighbour is 2^(ex-5) away and f counts 2^-18 of that); with G[512] = 1 the
 * largest encoded value rounds to the uint8 code 255.  Where a float result without an encoding is a NaN (tables that overflow) its
 * payload is not specified.
 *
 * Limits: npix >= 0; the tables are finite float32 values, read as they are; weights are finite and >= 0; curve, encode and exposure
 * are aligned to 4 bytes, src and dst to their elements; dst must not overlap src, curve, encode or exposure (dst == src is refused
 * too); buffers are contiguous.
 */
#ifndef TDK_HIP_FILMIC_H
#define TDK_HIP_FILMIC_H

#include <stddef.h>
#include <stdint.h>

#include "tdk_hip.h"
#include "tdk_hip_resample.h" /* TDK_U8 */

#ifdef __cplusplus
extern "C" {
#endif

#define TDK_FILMIC_ABI_VERSION 1

/* the curve tables: exposures covered, nodes per octave, entries = (EV_MAX - EV_MIN)*STEPS + 1 */
#define TDK_FILMIC_EV_MIN -20
#define TDK_FILMIC_EV_MAX 12
#define TDK_FILMIC_STEPS 32
#define TDK_FILMIC_TABLE 1025
/* the encoding table: from 2^ENC_EV_MIN to 1, entries = -ENC_EV_MIN*STEPS + 1 */
#define TDK_FILMIC_ENC_EV_MIN -16
#define TDK_FILMIC_ENC_TABLE 513

/* norm of tdk_filmic */
#define TDK_FILMIC_MAX 0
#define TDK_FILMIC_LUMA 1
#define TDK_FILMIC_POWER 2
#define TDK_FILMIC_NONE 3

int tdk_filmic_abi_version(void);

/* LDS bytes of one workgroup: static, the same for every call.  The tables are staged once per workgroup with every node next to its
 * successor, so that a lane's T[i], T[i+1], D[i], D[i+1] are one 16-byte read and G[i], G[i+1] one 8-byte read:
 * 16 * (TDK_FILMIC_TABLE - 1) + 8 * (TDK_FILMIC_ENC_TABLE - 1) = 20480. */
size_t tdk_filmic_lds_bytes(void);

/* ---- The stage (csrc/filmic.hip).  One launch: no workspace, no allocation, no copy, no memset, no atomics, no synchronisation --
 * capturable in a graph from the first call, and deterministic.  curve (2 * TDK_FILMIC_TABLE floats), encode (TDK_FILMIC_ENC_TABLE
 * floats, or null) and exposure (one float) are in DEVICE memory and read by every call: a caller may rewrite them between calls,
 * also between the replays of a captured call.  weights is a HOST pointer to three floats, read during the call under every norm.
 * flags is reserved and must be 0.  Argument errors (null pointers, npix < 0, dtype tags, norm, weights, flags, alignment, overlap)
 * are reported before any HIP call.  npix == 0 returns TDK_OK without a launch. */
int tdk_filmic(const void* src, void* dst, const float* curve, const float* encode, const float* exposure, int64_t npix, int src_dtype, int dst_dtype,
               int norm, const float* weights /* host, 3 */, int flags, tdk_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
