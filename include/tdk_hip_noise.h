/*
 * tdk_hip_noise.h -- noise profile (libtdk_hip.so): the Poisson-Gaussian noise model var(x) = a*x + b of a sensor, measured on raw
 * mosaics, and the variance-stabilising transform (generalised Anscombe) that puts any denoiser into a domain where the noise is
 * flat.  darktable's "denoise (profiled)" does this with profiles measured off line; the reference has no counterpart.
 *
 * include/tdk_hip.h (the reference's surface) and the other tdk_hip_*.h headers stay pinned; the noise block is declared here, with
 * its own version number.  The conventions of tdk_hip.h apply: device pointers, a HIP stream per call, TDK_OK or a tdk_status code
 * with the message in tdk_last_error(), nothing allocates device memory.  The measured model is a device buffer: it goes from
 * tdk_noise_profile into tdk_noise_stabilize without a copy and without a synchronisation.
 *
 * ---- Specification, estimation (tdk_noise_profile).  Block statistics are integers; the derived values are IEEE double, no
 * contraction (no FMA), rounded once to float32, in i-ascending order where order matters.  Counters are 64-bit integers: no result
 * depends on the order of accumulation.
 *
 * Input.  num_frames (1..TDK_NOISE_MAX_FRAMES) (height, width) mosaics of one geometry, storage type (TDK_F32, TDK_F16, TDK_U16) and
 * Bayer pattern word (tdk_hip.h) pool into one result.  width and height are even, 2..65535; a frame is contiguous at any element
 * alignment.
 *
 * Parameters.  white > 0, finite (float32); the host computes scale = fl32(65535 / white) (must be finite).  Integer clip limits
 * 0 <= clip_lo <= clip_hi <= 65535; intensity bins I in 2..TDK_NOISE_MAX_BINS; min_count >= 1.
 *
 * Per site, x its value converted exactly to float32:
 *   q = (int) rintf(fminf(fmaxf(x * scale, 0), 65535))
 * (uint16 storage with white = 65535 is exact).  A NaN has q = 0 and makes its block a NaN block.
 *
 * Blocks.  Site (i, j) has the CFA position p = 2*(i & 1) + (j & 1); the sites of one position form a plane of (height/2, width/2)
 * samples.  A block is 8 x 8 samples of one plane at block row and column (by, bx): a 16 x 16 mosaic tile holds four blocks, one per
 * CFA position.  Only complete blocks count: (height/2)/8 x (width/2)/8 per plane.  colour k = (pattern >> (2*p)) & 3 (0 = R, 1 = G,
 * 2 = B); the two greens pool.  Per block, q(r, c) its samples, r, c = 0..7:
 *   S = sum of q,  qmin, qmax
 *   h(r, c) = 2*q(r, c) - q(r, c-1) - q(r, c+1)      c = 1..6, every r     (48 values)
 *   v(r, c) = 2*q(r, c) - q(r-1, c) - q(r+1, c)      r = 1..6, every c     (48 values)
 *   E = sum of h*h + sum of v*v                      (64 bits; white noise of variance s2 in q units has the expectation 576 * s2)
 *   all[k] += 1
 *   a NaN block:                                     nan[k] += 1, nothing else
 *   otherwise qmin < clip_lo or qmax > clip_hi:      clipped[k] += 1, nothing else
 *   otherwise (a valid block):
 *     i = ((S >> 6) * I) >> 16
 *     l = level(E):  E < 256: 0;  otherwise e = floor(log2 E), f = (E >> (e - 2)) & 3, l = min(4*(e - 8) + f + 1, 127)
 *     hist[k][i][l] += 1;   sumS[k][i] += S
 * The lower edge of level l >= 1 is E_lo(l) = (4 + ((l-1) & 3)) << (((l-1) >> 2) + 6); TDK_NOISE_LEVELS = 128 levels.
 *
 * Derived values.  kappa = TDK_NOISE_MEDIAN_FACTOR, the median of E / (576 * s2) for white Gaussian noise
 * (profiles/noiseprofile_constants.py re-derives it).  ws = (double)white / 65535.0.  Per (k, i) with n = sum over l of hist[k][i][l]:
 *   n < min_count: the bin is unusable.  Otherwise the median level, as tdk_hip_stats.h takes a percentile at q = 0.5:
 *     r = ceil(0.5 * (double)n) clamped to [1, n]
 *     l* = the smallest l with cum(l) >= r, cum(l) = hist[k][i][0] + ... + hist[k][i][l], cum(-1) = 0
 *     frac = (double)(r - cum(l* - 1)) / (double)hist[k][i][l*]
 *   l* == 0 or l* == 127: the bin is unusable.  Otherwise
 *     E_med = (double)E_lo(l*) + frac * ((double)E_lo(l* + 1) - (double)E_lo(l*))
 *     v_i = (E_med / (576.0 * kappa)) * (ws * ws)
 *     x_i = (((double)sumS[k][i] / (64.0 * (double)n)) / 65535.0) * (double)white
 *     w_i = (double)n / (v_i * v_i)
 * Per colour k, over its usable bins in i-ascending order, every sum starting at 0.0:
 *   Sw = sum w_i;  Swx = sum (w_i * x_i);  Swxx = sum ((w_i * x_i) * x_i);  Swv = sum (w_i * v_i);  Swxv = sum ((w_i * x_i) * v_i)
 *   det = Sw * Swxx - Swx * Swx
 *   fewer than two usable bins, or not det > 0:   valid = 0, a = b = 0
 *   otherwise valid = 1 and
 *     a = (Sw * Swxv - Swx * Swv) / det;   b = (Swxx * Swv - Swx * Swxv) / det
 *     a < 0:        a = 0, b = Swv / Sw
 *     else b < 0:   b = 0, a = Swxv / Swxx
 *
 * Results.  counts (device, 8-byte aligned): 3*I*128 + 3*I + 9 64-bit integers: hist[3][I][128], sumS[3][I], all[3], nan[3],
 * clipped[3].  model (device): 3 x 4 floats, per colour (float)a, (float)b, valid (0 or 1), the number of usable bins.
 * curve (device): 2 x 3 x I floats, (float)x_i then (float)v_i, 0 where the bin is unusable.
 *
 * ---- Specification, transform (tdk_noise_stabilize, tdk_noise_unstabilize).  Per-value arithmetic is float32, one rounding per
 * written operation, no contraction, correctly rounded sqrtf and division.
 *
 * Input.  count elements, float32 or float16 on either side, converted exactly to float32.  Element e takes the model row
 *   pattern != 0 (a mosaic of rows of `width` sites, width even, channels must be 1):  the colour of site (e / width, e % width)
 *   pattern == 0, channels == 3:  e % 3          pattern == 0, channels == 1:  0
 * Per row, with (a, b, valid) of the model, g the gain of the row (1 when gains is NULL) and s = sigma_out > 0:
 *   a' = g * a;   b' = (g * g) * b;   c = 0.375f * (a' * a') + b';   k = (2.0f * s) / a'
 * Forward:
 *   valid == 0, or a' == 0 and b' == 0:    y = x
 *   a' == 0:                               y = (s * x) / sqrtf(b')
 *   otherwise:                             y = k * sqrtf(fmaxf(a' * x + c, 0.0f))
 * Inverse, with d = y / s:
 *   valid == 0, or a' == 0 and b' == 0:    x = y
 *   a' == 0:                               x = d * sqrtf(b')
 *   TDK_NOISE_ALGEBRAIC:                   x = ((a' * (d * d)) * 0.25f) - (c / a')
 *   TDK_NOISE_UNBIASED:                    D = fmaxf(d, 1.2247449f);   D2 = D * D;   sn2 = b' / (a' * a')
 *                                          I = (((((D2 * 0.25f) + (0.30618622f / D)) - (1.375f / D2)) + (0.76546554f / (D2 * D))) - 0.125f) - sn2
 *                                          x = a' * fmaxf(I, 0.0f)
 * (the closed-form unbiased inverse of Makitalo and Foi; 0 at D = sqrt(1.5) when sn2 = 0).  fmaxf of a NaN and a number is the
 * number.  A float16 destination rounds the float32 result once, to nearest even.
 *
 * Decisions the issue left open: the frames of a set share their storage type and one launch gathers the whole set; a NaN block is
 * counted as NaN and not as clipped, whatever else it holds; the Gaussian branch multiplies before it divides; `inverse` is ignored
 * by the two degenerate branches; the model's valid field is tested against 0, nothing else of it is checked on the device.
 */
#ifndef TDK_HIP_NOISE_H
#define TDK_HIP_NOISE_H

#include <stddef.h>

#include "tdk_hip.h"
#include "tdk_hip_stats.h" /* TDK_U16 */

#ifdef __cplusplus
extern "C" {
#endif

#define TDK_NOISE_ABI_VERSION 1

#define TDK_NOISE_MAX_BINS 32
#define TDK_NOISE_MAX_FRAMES 16
#define TDK_NOISE_LEVELS 128
#define TDK_NOISE_MEDIAN_FACTOR 0.9796
/* The gather launch is TDK_NOISE_GRID workgroups whatever the frame size; a workgroup takes a strip of 16 mosaic rows and
 * TDK_NOISE_STRIP_BYTES bytes of each row per step. */
#define TDK_NOISE_GRID 512
#define TDK_NOISE_STRIP_BYTES 512
#define TDK_NOISE_ALGEBRAIC 0
#define TDK_NOISE_UNBIASED 1

int tdk_noise_abi_version(void);

/* Bytes of device workspace of tdk_noise_profile: TDK_NOISE_GRID records, a record being the 3 * bins * 128 uint32 levels of one
 * workgroup, its 3 * bins 64-bit sums and its 9 64-bit counters.  It does not grow with the number of frames.  Every record is
 * written by every call: nothing needs zeroing, nothing survives a call.  0 for a bins tdk_noise_profile would reject. */
size_t tdk_noise_workspace_bytes(int bins);

/* LDS bytes of a workgroup of the gather launch (the largest of the call): the level histograms at TDK_NOISE_MAX_BINS, the sums,
 * the counters and the staged strip, a constant below 64 KB.  0 for a bins tdk_noise_profile would reject. */
size_t tdk_noise_lds_bytes(int bins);

/* One gather launch for the whole set and two small finishing launches (sum the records; derive the floats), all on `stream`.  No
 * global atomics, no float atomics, no memset, no copy, no synchronisation, no allocation: capturable in a graph from the first
 * call, and deterministic.  frames: a HOST array of num_frames device pointers.  workspace: tdk_noise_workspace_bytes(bins) bytes of
 * device memory at any alignment, owned by the call until its last launch has finished (one workspace per stream).  Argument errors
 * (null pointers, counts, sizes, dtype tag, pattern, bins, white, clip limits, min_count, alignment of counts, overlap) are reported
 * before any HIP call. */
int tdk_noise_profile(const void* const* frames, int num_frames, int dtype, void* workspace, int width, int height, uint32_t pattern, int bins,
                      float white, int clip_lo, int clip_hi, int min_count, long long* counts /* device */, float* model /* device */,
                      float* curve /* device */, tdk_stream_t stream);

/* One streaming launch each, out of place: src and dst share nothing.  model: 12 floats,
 * gains: 3 floats or NULL, both device.  Argument errors (null pointers, count, width, channels, dtype tags, pattern, sigma_out,
 * inverse, overlap) are reported before any HIP call. */
int tdk_noise_stabilize(const void* src, int src_dtype, void* dst, int dst_dtype, int64_t count, int width, int channels, uint32_t pattern,
                        const float* model, const float* gains, float sigma_out, tdk_stream_t stream);
int tdk_noise_unstabilize(const void* src, int src_dtype, void* dst, int dst_dtype, int64_t count, int width, int channels, uint32_t pattern,
                          const float* model, const float* gains, float sigma_out, int inverse, tdk_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
