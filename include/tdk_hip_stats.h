/*
 * tdk_hip_stats.h -- frame statistics (libtdk_hip.so): per-channel histograms, percentiles, means and grey-world gains of a frame or
 * of a set of frames, which the reference computes on the host (scripts/view_raw/histogram_display.py) or not at all.
 *
 * include/tdk_hip.h (the reference's surface) and the other tdk_hip_*.h headers stay pinned; the statistics block is declared here,
 * with its own version number.  The conventions of tdk_hip.h apply: device pointers, a HIP stream per call, TDK_OK or a tdk_status
 * code with the message in tdk_last_error(), nothing allocates device memory.
 *
 * This is the block of an ISP that MEASURES: its results are device buffers, so a measured bound or gain goes into
 * tdk_normalize, tdk_apply_white_balance or tdk_highlights without a copy and without a synchronisation.
 *
 * ---- Specification.  Per-value arithmetic is float32, one rounding per written operation, no contraction (no FMA); the derived
 * values are IEEE double, no contraction, rounded once to float32.  Counters are 64-bit integers: no result depends on the order of
 * accumulation.
 *
 * Input.  num_frames frames (1..TDK_STATS_MAX_FRAMES) of one geometry and storage type pool into one result.  A frame is
 *   pattern == 0:  an (height, width, channels) image, channels = 1 or 3, C = channels;
 *   pattern != 0:  an (height, width) mosaic with that Bayer pattern word (tdk_hip.h), width and height even, channels must be 3:
 *                  site (i, j) has the CFA position p = 2*(i & 1) + (j & 1) and the colour k = (pattern >> (2*p)) & 3
 *                  (0 = R, 1 = G, 2 = B); the two greens pool into channel 1.  C = 3.
 * width and height are 1..65535, the frame is contiguous at any element alignment.  Storage is TDK_F32, TDK_F16, TDK_U8 or
 * TDK_U16, converted exactly to float32: x.  Integer storage is taken at its integer value (a byte histogram is the range
 * [0, 256) with 256 bins).
 *
 * Sampling.  stride s in 1..65535.  Image: pixel (i, j) is sampled when i % s == 0 and j % s == 0; a group is the pixel, its members
 * the C values.  Mosaic: the CFA cell (ci, cj) = (i >> 1, j >> 1) is sampled when ci % s == 0 and cj % s == 0; a group is the cell,
 * its members the four sites.  A member belongs to channel k: the channel index of the image, the colour of the site.
 *
 * Parameters.  bins B in 2..TDK_STATS_MAX_BINS; lo < hi, both finite, with fl32(hi - lo) finite; the host computes
 *   range = fl32(hi - lo)      scale = fl32(fl32(B) / range)        (scale must be finite)
 * min_count >= 1; num_quantiles Q in 0..TDK_STATS_MAX_QUANTILES fractions q in [0, 1] (host pointer, float32).
 *
 * Per sampled member x of channel k:
 *   x is a NaN:   nan[k] += 1, nothing else (a NaN never reaches the index conversion)
 *   otherwise:    t = (x - lo) * scale
 *                 b = (int) fminf(fmaxf(floorf(t), 0.0f), (float)(B - 1))          hist[k][b] += 1
 *                 below[k] += (x < lo);   above[k] += (x >= hi)
 * (+Inf and -Inf land in the last and the first bin through the clamp, and count as above and below.)
 *
 * Per valid group.  A group is valid when every member is not a NaN and has lo <= x < hi.  Each member of a valid group adds
 *   valid[k] += 1
 *   sum[k]   += (long long) rintf(fminf(fmaxf(t, 0.0f), (float)B) * 1048576.0f)
 * (so a mosaic's valid[1] is twice its valid[0]; a pixel with one channel out of range contributes to no mean.)
 *
 * Derived values, with w = (double)range / (double)B:
 *   mean[k] = valid[k] >= min_count ? (float)((double)lo + ((double)sum[k] / ((double)valid[k] * 1048576.0)) * w) : 0.0f
 *   percentile(H, q) of a histogram H -- one per channel, and the pooled one, the sum of the channel histograms:
 *     N = sum of H;  N == 0: the value is lo
 *     r = ceil((double)q * (double)N) clamped to [1, N]
 *     b* = the smallest b with cum(b) >= r, cum(b) = H[0] + ... + H[b], cum(-1) = 0
 *     frac = (double)(r - cum(b* - 1)) / (double)H[b*]
 *     value = (float)((double)lo + ((double)b* + frac) * w)
 *   gain[k] (grey world), channels == 3 with every valid[k] >= min_count and every mean[k] > 0:
 *     gain[k] = fminf(fmaxf(mean[1] / mean[k], 1.0f/64.0f), 64.0f)      (a float32 division; gain[1] is exactly 1)
 *   otherwise gain = (1, 1, 1).
 *
 * Results.  counts (device, 8-byte aligned): C * (B + 5) 64-bit integers, per channel hist[B], below, above, nan, valid, sum.
 * values (device): C + (C + 1) * Q + 3 floats: mean[C], percentile[C + 1][Q] (the last row pooled), gain[3].
 *
 * Decisions the issue left open: the frames of a set share their storage type; below and above are counted on every non-NaN value,
 * sampled groups only; a percentile of an empty histogram is lo for every q; with one channel the three gains are 1.
 */
#ifndef TDK_HIP_STATS_H
#define TDK_HIP_STATS_H

#include <stddef.h>

#include "tdk_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TDK_STATS_ABI_VERSION 1

#define TDK_U16 3 /* storage tag of 16-bit unsigned integers, beside TDK_F32, TDK_F16 (tdk_hip.h) and TDK_U8 (tdk_hip_resample.h) */
#define TDK_STATS_MAX_BINS 1024
#define TDK_STATS_MAX_FRAMES 16
#define TDK_STATS_MAX_QUANTILES 8
/* The gather launch is TDK_STATS_GRID workgroups whatever the frame size; a workgroup takes TDK_STATS_CHUNK pixels (mosaic: sites of
 * one row pair, counted per row) per step, so a frame beyond TDK_STATS_GRID * TDK_STATS_CHUNK pixels makes every workgroup loop. */
#define TDK_STATS_GRID 512
#define TDK_STATS_CHUNK 8192

int tdk_framestats_abi_version(void);

/* Bytes of device workspace of a call with up to max_frames frames: per frame a slot of TDK_STATS_GRID records, a record being the
 * uint32 bins of one workgroup (channels * bins, padded to an even count) and its 5 * channels 64-bit counters.  Every record of a
 * used slot is written by every call: nothing needs zeroing, nothing survives a call.  0 for arguments tdk_framestats would reject. */
size_t tdk_framestats_workspace_bytes(int bins, int channels, int max_frames);

/* LDS bytes of a workgroup of the gather launch (the largest of the call): the replicated histograms and the counters, a constant
 * below 64 KB; the number of replicas follows from bins and channels (16 at 3 x 256 bins, 4 at 3 x 1024).  0 for arguments
 * tdk_framestats would reject. */
size_t tdk_framestats_lds_bytes(int bins, int channels);

/* One gather launch per frame and two small finishing launches (sum the records; derive the floats), all on `stream`.  No global
 * atomics, no float atomics, no memset, no copy, no synchronisation, no allocation: capturable in a graph from the first call, and
 * deterministic.  frames: a HOST array of num_frames device pointers.  workspace: tdk_framestats_workspace_bytes(bins, channels,
 * num_frames) bytes of device memory at any alignment, owned by the call until its last launch has finished (one workspace per
 * stream).  Argument errors (null pointers, counts, sizes, odd mosaic sizes, dtype tag, pattern, channels, stride, bins, range,
 * min_count, quantiles, alignment of counts, overlap) are reported before any HIP call. */
int tdk_framestats(const void* const* frames, int num_frames, int dtype, void* workspace, int width, int height, int channels, uint32_t pattern,
                   int stride, int bins, float lo, float hi, int min_count, const float* quantiles /* host, or NULL with 0 */, int num_quantiles,
                   long long* counts /* device */, float* values /* device */, tdk_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
