/*
 * tdk_hip_lut.h -- colour management of libtdk_hip.so: a 3x3 matrix, shaper curves and a 3D look-up table applied to every pixel
 * in one launch, which the reference does not have.
 *
 * include/tdk_hip.h (the reference's surface) and the other extension headers stay pinned; the colour transform is declared here,
 * with its own version number.  The conventions of tdk_hip.h apply: device pointers unless a parameter says HOST, a HIP stream per
 * call, TDK_OK or a tdk_status code with the message in tdk_last_error(), nothing allocates device memory.
 *
 * ---- Specification.  All arithmetic is float32, one rounding per written operation, no contraction (no FMA); parentheses give the
 * order of operations.  fminf / fmaxf return the other operand for a NaN; fmaxf(-0, +0) is +0.
 *
 * The frame is npix pixels of three interleaved values (r, g, b).  Source and destination storage are independent, each TDK_F32,
 * TDK_F16 or TDK_U8 (of tdk_hip_resample.h).  The three stages are optional and run in this order.
 *
 * Load:     float32 as it is; binary16 converted exactly; uint8 s becomes (float)s * c255, c255 the float32 with the bits
 *           0x3B808081 (0x1.010102p-8f, the float32 nearest 1/255).
 *
 * Matrix (matrix != NULL; m0 .. m8 row-major):
 *   r' = (m0*r + m1*g) + m2*b
 *   g' = (m3*r + m4*g) + m5*b
 *   b' = (m6*r + m7*g) + m8*b
 *
 * Shaper (shaper != NULL; S = shaper_size), per channel c, with the table T = shaper + (shaper_tables == 3 ? c*S : 0):
 *   t = fminf(fmaxf((x - lo) * scale, 0.0f), (float)(S-1))          lo = shaper_lo, scale = shaper_scale
 *   k = min((int)t, S-2)
 *   f = t - (float)k
 *   y = T[k] + f*(T[k+1] - T[k])
 * A NaN has t = 0 and reads T[0]; +inf has t = S-1.
 *
 * 3D LUT (lut != NULL; N = lut_size), per axis c with the value y_c of that channel:
 *   t_c = fminf(fmaxf((y_c - lo_c) * scale_c, 0.0f), (float)(N-1))          lo_c = lut_lo[c], scale_c = lut_scale[c]
 *   k_c = min((int)t_c, N-2)
 *   f_c = t_c - (float)k_c
 * Node (kr, kg, kb) is the three floats L[kr, kg, kb][0..2] at index ((kb*N + kg)*N + kr)*3: red runs fastest, the order of a
 * .cube file.  Every output channel is interpolated on its own, by the same formula.
 *   TDK_LUT_TETRAHEDRAL   Order the three axes by descending f; ties go in the order r, g, b.  Call the axes a, b', c', their
 *       fractions f_a >= f_b' >= f_c' and their unit steps e_a, e_b', e_c'.  Walk P0 = (kr, kg, kb), P1 = P0 + e_a, P2 = P1 + e_b',
 *       P3 = P2 + e_c' (P3 is always (kr+1, kg+1, kb+1)):
 *         out = ((L[P0] + f_a*(L[P1] - L[P0])) + f_b'*(L[P2] - L[P1])) + f_c'*(L[P3] - L[P2])
 *   TDK_LUT_TRILINEAR     with lerp(p, q, f) = p + f*(q - p), along r on the four edges, then along g, then along b:
 *         c00 = lerp(L[kr, kg,   kb  ], L[kr+1, kg,   kb  ], f_r)
 *         c10 = lerp(L[kr, kg+1, kb  ], L[kr+1, kg+1, kb  ], f_r)
 *         c01 = lerp(L[kr, kg,   kb+1], L[kr+1, kg,   kb+1], f_r)
 *         c11 = lerp(L[kr, kg+1, kb+1], L[kr+1, kg+1, kb+1], f_r)
 *         out = lerp(lerp(c00, c10, f_g), lerp(c01, c11, f_g), f_b)
 *
 * Store:    float32 as it is; binary16 rounded to nearest even, once; uint8 is rintf(fminf(fmaxf(v, 0.0f), 1.0f) * 255.0f), a NaN
 *           stores 0.
 *
 * What follows: with no stage and equal storage types the output has the input's bits, for all 256 uint8 values too; a coordinate
 * exactly on a node below the last returns that node's bits (f = 0; the last node is reached with f = 1, within an ulp); grey input
 * to a LUT whose diagonal nodes are grey stays grey under tetrahedral interpolation -- with equal fractions the walk is r, g, b and
 * the two nodes off the diagonal cancel, up to the rounding of the three steps, and to the bit where the channels' steps are equal
 * (per-channel curves, the identity) -- while trilinear interpolation mixes the off-diagonal nodes in.  Where a float result is a NaN
 * (a NaN or an infinity met by a matrix, no table behind it) its payload is not specified.
 *
 * Limits: shaper_size 2..1024; shaper_tables 1 or 3; lut_size 2..65; tables are finite float32 values in device memory, read as they
 * are; matrix, lo and scale values must be finite; dst must not overlap src, the shaper or the LUT (dst == src is refused too);
 * buffers are contiguous at any element alignment.
 */
#ifndef TDK_HIP_LUT_H
#define TDK_HIP_LUT_H

#include <stddef.h>
#include <stdint.h>

#include "tdk_hip.h"
#include "tdk_hip_resample.h" /* TDK_U8 */

#ifdef __cplusplus
extern "C" {
#endif

#define TDK_LUT_ABI_VERSION 1

/* interp of tdk_color_lut */
#define TDK_LUT_TETRAHEDRAL 0
#define TDK_LUT_TRILINEAR 1

/* flags of tdk_color_lut: gather the nodes from global memory whatever the size of the LUT.  For tests and measurement: both ways of
 * reading the nodes give the same bits. */
#define TDK_LUT_GLOBAL 1

#define TDK_LUT_MAX_SHAPER 1024
#define TDK_LUT_MAX_SIZE 65
/* a LUT is staged in LDS when its nodes and the shaper tables together take no more than this: two workgroups share a CU */
#define TDK_LUT_LDS_BUDGET 81920

int tdk_lut_abi_version(void);

/* ---- The colour transform (csrc/colorlut.hip).  A stage whose pointer is NULL is left out, and its other parameters are not read.
 * matrix, lut_lo and lut_scale are HOST pointers, read during the call; they and every scalar travel as kernel arguments: one
 * launch, no workspace, no host-to-device copy, no atomics, no synchronisation -- capturable in a graph from the first call, and
 * deterministic.  Argument errors (null src or dst, npix < 0, dtype tags, shaper_size, shaper_tables, lut_size, a non-finite
 * matrix, lo or scale value, interp, flags, overlap) are reported before any HIP call.  npix == 0 returns TDK_OK without a launch. */
int tdk_color_lut(const void* src, int src_dtype, void* dst, int dst_dtype, int64_t npix, const float* matrix /* HOST, 9 row-major, or NULL */,
                  const float* shaper /* DEVICE, tables*size floats, or NULL */, int shaper_size, int shaper_tables /* 1 or 3 */, float shaper_lo,
                  float shaper_scale, const float* lut /* DEVICE, size^3 * 3 floats, or NULL */, int lut_size, const float* lut_lo /* HOST, 3 */,
                  const float* lut_scale /* HOST, 3 */, int interp, int flags, tdk_stream_t stream);

/* LDS bytes one workgroup of tdk_color_lut takes: the shaper tables (4 * tables * size) and, when the LUT is staged, its nodes
 * (12 * size^3).  shaper_size == 0: no shaper; lut_size == 0: no LUT.  A LUT is staged without TDK_LUT_GLOBAL when both together
 * fit TDK_LUT_LDS_BUDGET (float32 nodes of N <= 17 always do: 58 956 bytes).  Host query; 0 for arguments tdk_color_lut would reject. */
size_t tdk_lut_lds_bytes(int shaper_size, int shaper_tables, int lut_size, int flags);

#ifdef __cplusplus
}
#endif
#endif
