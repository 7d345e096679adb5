/*
 * tdk_hip_hdr.h -- exposure-bracket merge (libtdk_hip.so): 2 to 8 raw Bayer mosaics of one scene at different exposures become one
 * mosaic, per site the inverse-variance weighted mean of the frames under the noise model of tdk_hip_noise.h.  The result has the
 * highlights of the shortest exposure and the shadow noise of the longest.  A frame that disagrees with the anchor frame of a site
 * (something moved between the exposures) loses its weight there, by the window statistic of tdk_hip_temporal.h.  The reference has
 * no counterpart.
 *
 * The merge acts on raw mosaics only, in front of the white balance and the demosaic: there the noise of neighbouring sites is
 * independent and the model var(x) = a*x + b is exact.
 *
 * include/tdk_hip.h (the reference's surface) and the other tdk_hip_*.h headers stay pinned; the merge is declared here, with its
 * own version number.  The conventions of tdk_hip.h apply: device pointers, a HIP stream per call, TDK_OK or a tdk_status code with
 * the message in tdk_last_error(), nothing allocates device memory.
 *
 * ---- Specification (tdk_hdr_merge).  Per-value arithmetic is float32, one rounding per written operation, no contraction (no FMA),
 * correctly rounded division.  fmaxf and fminf of a NaN and a number give the number.
 *
 * Input.  F = num_frames (height, width) mosaics, 2 <= F <= TDK_HDR_MAX_FRAMES, width and height even, 2..65535, all float32 or all
 * float16, converted exactly to float32, each contiguous at any element alignment; the Bayer pattern word of tdk_hip.h.  frames is a
 * HOST array of F device pointers, read at the call.  exposures: F device floats (any unit: only their ratios count); model: the 12
 * device floats of tdk_hip_noise.h (per colour a, b, valid, usable bins).  Both are read on the device by every call.  Site (i, j)
 * has the CFA position p = 2*(i & 1) + (j & 1) and the colour k = (pattern >> (2*p)) & 3, as in tdk_temporal_denoise; (a, b, valid)
 * is row k of the model.  A row is invalid when its valid field is 0; an invalid row uses a = 1, b = 0.  There are no gains.
 *
 * Host parameters, each a float32: radius r is 2 or 3; clip > 0, finite; 0 < t_lo < t_hi, both finite, and
 * inv = fl32(1 / (t_hi - t_lo)) must be finite; c2 = pixel_c2 > 0, the square of the per-site threshold, +inf when the per-site test
 * is off; v_min > 0, finite.  ref is -1 or a frame index.
 *
 * Exposure ratios (the same for every site, computed on the device).  x_f is the sample of frame f.
 *   lo    = the f with the smallest exposures[f], the lowest such f (a later frame replaces an earlier one only when <)
 *   hi    = the f with the largest exposures[f], the lowest such f (only when >)
 *   e_min = exposures[lo];   k_f = exposures[f] / e_min          (every k_f >= 1)
 *   ref == -1 selects ref = hi
 * The result is radiance in the units of frame lo, the shortest: it lies in the range one frame has.
 *
 * Per site q:
 * 1. Clipped sites.
 *   c_f(q)   = !(x_f < clip)                        (a NaN counts as clipped)
 *   sat_f(q) = the OR of c_f over the in-frame sites of the 3 x 3 around q, all colours
 * 2. The anchor frame g(q).
 *   g = ref if !sat_ref(q)
 *   else the frame with the largest k_f among those with !sat_f(q): f ascending, a later frame replaces the choice only when its
 *        k_f is >
 *   else blown(q): g = lo
 *   R = x_g / k_g
 * A blown site has out = R and takes no part in any window.
 * 3. Predicted variance, of any frame f (g included):
 *   m_f = fmaxf(R, 0) * k_f;   var_f = fmaxf(a * m_f + b, v_min);   u_f = var_f / (k_f * k_f)
 * u_f is the predicted variance of r_f = x_f / k_f.
 * 4. Consistency of a frame f != g(q) with the anchor.
 *   d = r_f - R;   eps = d * d;   v = u_f + u_g
 *   a site with sat_f(q), blown(q) or g(q) == f contributes eps = 0, v = 0
 * Window.  The sites of rows i-r..i+r and columns j-r..j+r that lie inside the frame, all CFA colours mixed.  Row sums first, over the
 * in-frame columns in ascending order, starting at 0.0f; then the sum of the row sums over the in-frame rows in ascending order,
 * starting at 0.0f: E (of eps) and V (of v).  This is the rule of tdk_temporal_denoise; a sliding sum has other bits.  (No eps or v
 * is -0, so a sum that also adds +0.0f for the sites outside the frame has the same bits.)
 *   t   = E / V
 *   s_f = fminf(fmaxf((t_hi - t) * inv, 0), 1)       (a NaN t gives 0)
 *   if (eps > c2 * v) s_f = 0                         (eps, v of the site itself; a false comparison leaves s_f)
 *   invalid row: s_f = 1;     s_g = 1
 * 5. Weights and result.
 *   w_f = sat_f(q) ? 0 : s_f / u_f
 *   num = sum of w_f * r_f,  den = sum of w_f,  f ascending from 0.0f, over the frames with w_f > 0
 *   out = (den > 0) ? num / den : R, rounded once to out_dtype
 * 6. Mask, when mask != NULL, a byte per site:  g | (blown ? 8 : 0) | (count of f with w_f > 0) << 4
 * out is float32 or float16 and shares nothing with any input.
 *
 * Consequences.  A site that no frame saturates and no frame contradicts is the inverse-variance mean of all frames.  A site blown in
 * every frame equals x_lo / k_lo = x_lo exactly and has a count of 0.  With finite samples no out is NaN.
 *
 * Decisions the issue left open.  The valid field is tested against 0, nothing else of the model and nothing of exposures is checked
 * on the device (the host checks exposures when it holds the values): a zero, negative, infinite or NaN exposure gives whatever the
 * formulas give.  A frame with w_f == 0 adds nothing to num: with finite samples that is the sum of all w_f * r_f bit for bit (num
 * is never -0), and an infinite sample of a frame without weight cannot turn out into a NaN through 0 * inf.  A +inf sample is
 * clipped like any sample >= clip; a -inf sample is not, and as the anchor it gives out = -inf.  A site whose anchor is f itself
 * tells nothing about the consistency of f, so it is left out of the windows of f like a saturated one.  A site of an invalid row
 * enters the windows of its neighbours with a = 1, b = 0.  A window without any contribution has t = 0/0 and therefore s_f = 0.
 * pixel_c2 is given squared, so the host squares once in float32.  Every address is formed from in-frame coordinates only.
 */
#ifndef TDK_HIP_HDR_H
#define TDK_HIP_HDR_H

#include <stddef.h>

#include "tdk_hip.h"
#include "tdk_hip_noise.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TDK_HDR_ABI_VERSION 1

/* The output tile of a workgroup: TDK_HDR_TILE_H rows of TDK_HDR_TILE_W sites. */
#define TDK_HDR_TILE_W 32
#define TDK_HDR_TILE_H 32
#define TDK_HDR_MAX_FRAMES 8

int tdk_hdr_abi_version(void);

/* Static LDS bytes of a workgroup: two staged planes (eps, v) of (TILE_H + 2r) x (TILE_W + 8) floats, two planes of row sums of
 * (TILE_H + 2r) x TILE_W floats, a plane of clip bits of (TILE_H + 2r + 2) x (TILE_W + 8) bytes and 96 bytes of frame addresses and
 * exposure ratios.  0 for a radius tdk_hdr_merge would reject. */
size_t tdk_hdr_lds_bytes(int radius);

/* Exactly one launch on `stream`: no workspace, no allocation, copy, memset, synchronisation or atomic: capturable in a graph from the
 * first call, bit-reproducible.  The frame addresses travel as kernel arguments.  Argument errors (null pointers, num_frames, sizes,
 * dtype tags, pattern, radius, ref, the five float parameters, clip, overlap of out / mask with frames / exposures / model and with
 * each other) are reported before any HIP call. */
int tdk_hdr_merge(const void* const* frames, int num_frames, int src_dtype, void* out, int out_dtype, unsigned char* mask, int width, int height,
                  uint32_t pattern, const float* exposures, int ref, const float* model, int radius, float clip, float t_lo, float t_hi, float pixel_c2,
                  float v_min, tdk_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
