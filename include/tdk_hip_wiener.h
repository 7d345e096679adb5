/*
 * tdk_hip_wiener.h -- the Wiener denoiser's entry points with a `flags` argument (libtdk_hip.so), and the host query of the strip
 * kernel's interior rule.
 *
 * The other headers under include/ stay pinned; these are declared here, with their own version number.  The conventions of
 * tdk_hip.h apply: device pointers, a HIP stream per call, TDK_OK or a tdk_status code with the message in tdk_last_error(),
 * nothing allocates device memory.
 *
 * The strip kernel (csrc/tdk_wiener_ystream.h; tile_size 32, overlap_factor 4) gives one workgroup per (strip, segment): a strip
 * is 16 tile columns = 152 sample columns starting at x = 8 (16 strip - 3), a segment is segment_rows tile rows = 8 segment_rows + 24
 * image rows starting at y = 8 (segment_rows segment - 3).  A workgroup none of whose samples lies outside the frame is INTERIOR
 * and runs a second instantiation of the kernel's round loop that carries no bounds test, no reflection and no tile-exists
 * predicate.  The two bodies differ in integer addressing and control flow only: the results are the same bits.
 *
 * Samples outside the usual range (every tile kernel, every tile_size and overlap_factor; tests/test_gpu_denoise_domain.py):
 *   - Footprint.  Two horizontally adjacent tiles -- tile columns 2 m and 2 m + 1, counted from the first tile, whose origin is
 *     x = -(overlap_factor - 1) s with s = tile_size / overlap_factor -- are the real and the imaginary part of ONE complex
 *     transform.  A sample therefore reaches, beyond the tiles that read it (directly or mirrored at a frame edge), the partner
 *     of each of those tiles: its rounding error is relative to the larger of the two tiles' samples, and a NaN or an infinity in
 *     one tile makes both tiles NaN.  The pixels a sample can change are the union of those tiles and partners, cut to the frame:
 *     up to s columns more on either side than the tile union of the reference, the same rows.  Outside that box the result
 *     has the bits it has without the sample (no atomics, a fixed order of additions); a NaN or +-inf sample makes exactly
 *     that box non-finite.
 *   - Gain.  max(1 - sigma^2 / p, 0), p = |X|^2 + 1e-15, is evaluated as max(GS - (4 sigma^2 GS) * rcp(p4), 0) with the
 *     hardware reciprocal.  Where |X|^2 overflows float32 (|X| above 1.8e19: a sample of 1e30), rcp(inf) = 0 and the gain is the
 *     pass-through gain exactly, the value the unrounded expression has; the reference's IEEE division gives inf / inf = NaN
 *     there.  Such a tile returns its samples, within float32 rounding relative to the largest of them.
 *   - Mean.  A tile's mean is a float32 sum of its tile_size^2 samples, a mirrored sample counting once per read.  The result is
 *     finite as long as that sum is: one sample of 3e38 read once is, read twice (within tile_size of a frame edge) it is not,
 *     and the tiles whose sum overflows, with their partners, are NaN.
 *   - The finish kernels multiply by rcp(mask + 1e-15), mask being the analytic sum of the window products over the tiles that
 *     cover a pixel (a positive constant per column and row phase, about 1 / s^2): a factor within 1 ulp, never 0 or inf.
 */
#ifndef TDK_HIP_WIENER_H
#define TDK_HIP_WIENER_H

#include <stddef.h>

#include "tdk_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TDK_WIENER_ABI_VERSION 1

/* flags of tdk_wiener_ex and tdk_wiener_log_luminance_lab_ex */
#define TDK_WIENER_GENERAL_BODY 1u /* every workgroup of the strip kernel takes the general body, the interior ones too */

int tdk_wiener_abi_version(void);

/* tdk_wiener (tdk_hip.h) with flags; flags = 0 is tdk_wiener itself.  Unknown flags are an argument error.  A flag that does not
 * apply to the kernel serving (tile_size, overlap_factor), or to an image it has no interior workgroup for, changes nothing. */
int tdk_wiener_ex(const void* in, void* out, void* workspace, int width, int height, int channels, int tile_size, int overlap_factor,
                  const float* sigmas, int dtype, uint32_t flags, tdk_stream_t stream);

/* tdk_wiener_log_luminance_lab (tdk_hip.h) with flags, in the same way. */
int tdk_wiener_log_luminance_lab_ex(const void* rgb_in, void* workspace, int width, int height, int tile_size, int overlap_factor,
                                    const float* sigma, float eps, const float* bounds, int dtype, float* lum_out, float* ab_out,
                                    uint32_t flags, tdk_stream_t stream);

/* Host query, no device needed: 1 when the strip kernel's workgroup (strip, segment) of a width x height plane cut into segments of
 * segment_rows tile rows is interior, 0 when it is not (also for a strip or segment the plane does not have), -1 for arguments that
 * are no plane of the strip kernel (width or height < 32, segment_rows < 8, a negative index).  It is the rule the kernel itself
 * applies, for a plane it reads with vector loads: width % 4 == 0 (otherwise 0 everywhere), one channel, aligned to 16 bytes.
 *   interior <=> 1 <= strip < width / 128  &&  1 <= segment < height / (8 segment_rows)  &&  width % 4 == 0 */
int tdk_wiener_strip_interior(int width, int height, int segment_rows, int strip, int segment);

/* Host query, no device needed: the (strip, segment) that workgroup number `workgroup` of a plane's launch works on, as
 * segment * strips + strip, or -1 for arguments as above or a number the launch does not have.  The edge workgroups, which keep the
 * general body, get the lowest numbers; a permutation of the plane's strips x segments. */
int tdk_wiener_strip_order(int width, int height, int segment_rows, int workgroup);

#ifdef __cplusplus
}
#endif
#endif
