/*
 * tdk_hip_warp.h -- parametric geometric resampling of libtdk_hip.so (lens undistortion, rectification, homographies), which the
 * reference does not have.
 *
 * include/tdk_hip.h (the reference's surface), include/tdk_hip_ext.h (the device-resident JPEG encode), include/tdk_hip_denoise.h
 * (non-local means) and include/tdk_hip_resample.h (the antialiased scaler) stay pinned; the warp is declared here, with its own
 * version number.  The conventions of tdk_hip.h apply: device pointers, a HIP stream per call, TDK_OK or a tdk_status code with
 * the message in tdk_last_error(), nothing allocates device memory.  The storage tag TDK_U8 comes from tdk_hip_resample.h.
 *
 * ---- Specification.  All arithmetic is float32, one rounding per written operation, no contraction; parentheses give the order.
 *
 * The map is 18 floats, m[0..17] = h0..h8, fx, fy, cx, cy, k1, k2, p1, p2, k3 (the distortion coefficients in OpenCV's order).
 * Pixel centres are integers (OpenCV's convention).  Output row i, column j:
 *
 *   u = (float)j;  v = (float)i
 *   X = (h0*u + h1*v) + h2;   Y = (h3*u + h4*v) + h5;   Z = (h6*u + h7*v) + h8
 *   iz = 1.0f / Z             (correctly rounded division)
 *   x = X*iz;  y = Y*iz
 *   x2 = x*x;  y2 = y*y;  r2 = x2 + y2;  xy = x*y
 *   rad = ((k3*r2 + k2)*r2 + k1)*r2 + 1.0f
 *   tx = p1*(xy + xy) + p2*(r2 + (x2 + x2))
 *   ty = p1*(r2 + (y2 + y2)) + p2*(xy + xy)
 *   xd = x*rad + tx;   yd = y*rad + ty
 *   sx = fx*xd + cx;   sy = fy*yd + cy
 *
 * A pixel with !(Z > 0), or with a non-finite sx or sy, is outside: its result is fill for every channel, in both border modes.
 * Otherwise the coordinate is clamped and split, with sw x sh the source size:
 *
 *   sx = min(max(sx, -4), sw + 3)          (likewise sy with sh)
 *   x0 = floorf(sx);  ax = sx - x0;  ix = (int)x0          (likewise y)
 *
 * Interpolation, interp = 0 (bilinear) or 1 (bicubic):
 *   bilinear: taps ix, ix+1 with weights 1.0f - ax, ax;
 *   bicubic:  taps ix-1 .. ix+2 with weights c2(ax + 1), c1(ax), c1(1 - ax), c2(2 - ax), where
 *     c1(t) = ((1.25f*t - 2.25f)*t)*t + 1.0f
 *     c2(t) = ((-0.75f*t + 3.75f)*t - 6.0f)*t + 3.0f
 *   -- the Keys kernel with A = -0.75 of OpenCV's INTER_CUBIC and torch's grid_sample(mode='bicubic'); at ax = 0 the weights are
 *   exactly 0, 1, 0, 0.
 * A row is ((s0*w0 + s1*w1) + s2*w2) + s3*w3, taken left to right (bilinear: the first two terms); the rows combine top to
 * bottom with the y weights in the same shape.  Channels are independent.
 *
 * Border, border = 0 (constant) or 1 (replicate): under constant a tap outside the frame reads fill, under replicate tap indices
 * are clamped into the frame.  fill is in the units of the storage type.
 *
 * Storage: samples convert to float32 exactly.  At the store float32 is written as it is, binary16 rounds to nearest even, uint8
 * is rint() after clamping to [0, 255].
 *
 * Limits: sizes 1..65535 per axis on both sides; channels 1 or 3, interleaved; dtype TDK_F32, TDK_F16 or TDK_U8, the same on both
 * sides; buffers contiguous at any element alignment, and the two must not overlap; all 18 map values and fill finite.
 */
#ifndef TDK_HIP_WARP_H
#define TDK_HIP_WARP_H

#include <stddef.h>

#include "tdk_hip_resample.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TDK_WARP_ABI_VERSION 1

/* flags of tdk_warp: every tile takes its taps from global memory (0: the library picks the sampling path per tile).  Both paths
 * give the same bits; the flag exists for tests and measurement. */
#define TDK_WARP_DIRECT 1

int tdk_warp_abi_version(void);

/* ---- The warp (csrc/warp.hip).  src: (src_height, src_width, channels), dst: (dst_height, dst_width, channels).  map is a HOST
 * pointer to 18 floats; it is read during the call and travels as kernel arguments, like every other parameter: one launch, no
 * workspace, no table from the host, no synchronisation, no copy -- capturable in a graph from the first call, and deterministic.
 * Argument errors (null pointers, sizes, channels, dtype, interp, border, flags, a non-finite map entry or fill, overlap) are
 * reported before any HIP call. */
int tdk_warp(const void* src, void* dst, int src_width, int src_height, int dst_width, int dst_height, int channels, int dtype,
             const float* map, int interp, int border, float fill, int flags, tdk_stream_t stream);

/* xy: (dst_height, dst_width, 2) float32 on the device, sx and sy of every output pixel BEFORE the clamp; outside pixels get NaN
 * in both.  The same arithmetic as tdk_warp; map is a host pointer to 18 floats. */
int tdk_warp_coordinates(float* xy, int dst_width, int dst_height, const float* map, tdk_stream_t stream);

/* LDS bytes one workgroup of tdk_warp takes (a fixed source box and the box reduction); at most 64 KB.  Host query; 0 for
 * arguments tdk_warp would reject. */
size_t tdk_warp_lds_bytes(int channels, int dtype, int interp);

#ifdef __cplusplus
}
#endif
#endif
