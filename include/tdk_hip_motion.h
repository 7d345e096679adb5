/*
 * tdk_hip_motion.h -- motion estimation on raw Bayer mosaics and the motion-compensated temporal denoiser (libtdk_hip.so).
 *
 * tdk_hip_temporal.h averages a mosaic over time per site and restarts where the frame differs from its running average.  Under
 * a panning camera every textured site differs every frame.  This block estimates one displacement per tile of the temporal
 * filter by hierarchical block matching on an 8-bit grey pyramid of the mosaic, and a variant of the filter reads its history
 * where the scene came from.  The reference has no counterpart.
 *
 * include/tdk_hip.h (the reference's surface) and the other tdk_hip_*.h headers stay pinned; the motion block is declared here,
 * with its own version number.  The conventions of tdk_hip.h apply: device pointers, a HIP stream per call, TDK_OK or a tdk_status
 * code with the message in tdk_last_error(), nothing allocates device memory.
 *
 * ---- Specification.  The estimator is integer arithmetic behind one float32 conversion per CFA cell: the order of a reduction
 * cannot change a bit.
 *
 * Grey plane, level 0 (tdk_motion_pyramid).  Input: an (height, width) mosaic, width and height even, 2..65535, float32 or float16
 * converted exactly to float32, contiguous at any element alignment.  The CFA cell (I, J) holds the sites x00 = (2I, 2J),
 * x01 = (2I, 2J + 1), x10 = (2I + 1, 2J), x11 = (2I + 1, 2J + 1) and gives one 8-bit value; float32, one rounding per written
 * operation, no contraction, correctly rounded sqrtf, fmaxf and fminf as in tdk_hip_temporal.h (a NaN and a number give the number):
 *   q = (x00 + x01) + (x10 + x11)
 *   u = fminf(fmaxf(q * scale, 0), 1)                  (a NaN q gives 0)
 *   g = (uint8)(sqrtf(u) * 255 + 0.5f)
 * scale is a host float32, finite and > 0; the Python side passes fl32(1 / (4 * white_level)).  The square root makes shot noise
 * roughly uniform over the grey range; the cell sum makes the plane colour-blind.  Level 0 has h0 = height / 2 rows of
 * w0 = width / 2 values.
 *
 * Pyramid.  Level k + 1 has h(k+1) = ceil(h(k) / 2) rows of w(k+1) = ceil(w(k) / 2) values:
 *   L(k+1)[r][c] = (a + b + c + d + 2) >> 2  over  L(k)[min(2r + {0, 1}, h(k) - 1)][min(2c + {0, 1}, w(k) - 1)]
 * levels K is 1..TDK_MOTION_MAX_LEVELS.
 *
 * Pyramid buffer.  Aligned to 16 bytes.  Level k is a plane of h(k) rows of w(k) bytes without padding between rows; with
 * P(k) = align16(w(k) * h(k)) a slot is the levels 0..K-1 one behind the other and the buffer is TWO slots:
 *   SLOT = P(0) + ... + P(K-1);   level k of slot s at byte offset s * SLOT + P(0) + ... + P(k-1)
 *   tdk_motion_pyramid_bytes = 2 * SLOT
 * The bytes between w(k) * h(k) and P(k) are never written.
 *
 * Tiles (tdk_motion_match).  The tiles of the temporal filter: TDK_MOTION_TILE_W x TDK_MOTION_TILE_H = 64 x 32 sites, 32 x 16 values
 * of level 0; Tx = ceil(width / 64), Ty = ceil(height / 32).  At level k the block of tile (ty, tx) is 16 rows of 32 values of that
 * level, centred at c = ((16 ty + 8) >> k, (32 tx + 16) >> k): rows c.y - 8 .. c.y + 7, columns c.x - 16 .. c.x + 15.  A coarser
 * block sees a wider neighbourhood on the same 512 samples.
 *   cost(d) = sum over the block's positions p of |cur(k)[clamp(p)] - ref(k)[clamp(p + d)]|
 * clamp brings a row into 0..h(k)-1 and a column into 0..w(k)-1; the sum is a uint32 (at most 512 * 255).
 *
 * Search.  Coarse to fine, k = K-1 .. 0.  The candidates of a level are base + (oy, ox):
 *   coarsest level:   base = 0,                    oy, ox in -S..S;   search S is 1..TDK_MOTION_MAX_SEARCH
 *   finer levels:     base = 2 * d(k + 1),         oy, ox in -1..1
 * d(k) = base + the offset that minimises the uint32
 *   key = cost << 14 | (oy*oy + ox*ox) << 8 | (oy + 4) << 4 | (ox + 4)
 * Every candidate has another key: any reduction order gives the same winner, and ties in cost go to the smaller move.
 *
 * Zero preference.  At level 0 cost(0) of the total displacement 0 is evaluated as well.  With w = d(0):
 *   if (cost(w) + zero_bias >= cost(0)) the result is 0, else w;      zero_bias is a uint32, 0..65535
 *
 * Results.  field[ty][tx] = (dy, dx) = 2 * result as two int16, in SITES: always even, so the CFA colours of a site and of its
 * history agree; ref[p + (dy, dx)] ~ cur[p].  |dy|, |dx| <= 2 * ((S + 1) * 2^(K-1) - 1) <= TDK_MOTION_MAX_DISPLACEMENT = 78.
 * costs[ty][tx] = (cost of the result, cost(0)) as two uint32; costs may be NULL.
 *
 * Slots.  index is NULL or a device pointer to a uint32 frame index idx, in practice the first word of a temporal state.
 * tdk_motion_pyramid writes slot `which` when index is NULL, else slot (idx + which) & 1.  tdk_motion_match reads cur from slot
 * which_cur of pyramid_cur and ref from slot which_ref of pyramid_ref (the two may be one buffer), or from (idx + which) & 1 of each
 * when index is not NULL; then idx == 0 means "no history": field and costs are written as 0.
 *
 * ---- The compensated filter (tdk_motion_temporal_denoise).  Everything of tdk_temporal_denoise (tdk_hip_temporal.h: input, model,
 * parameters, state layout, index) holds, with ONE change.  Let (dy, dx) = field[i / 32][j / 64] & ~1 for the OUTPUT site (i, j)
 * (odd values are masked on the device; any int16 is memory-safe).  For every site q that enters the window of that output site,
 * its own included, the history site is h = q + (dy, dx):
 *   h inside the frame and idx != 0:   A = (float)acc_src[h]     N = (float)cnt_src[h]
 *   otherwise:                         A = 0                     N = 0           (the `first` case of tdk_hip_temporal.h)
 * d, e, v, the ordered window sums E and V, t, s, n1 and y are as written there; the three stores go to site q = (i, j) of the
 * destination planes and of out.
 *
 * Consequences.  With a zero field the function is tdk_temporal_denoise bit for bit.  The running average always lives in the
 * coordinates of the newest frame, so the displacement from the previous frame to this one is all a call needs.  A window near
 * a tile seam evaluates the neighbour tile's sites with the OUTPUT tile's displacement: a workgroup loads its whole staged
 * region at one uniform offset.  A state can be handed between tdk_temporal_denoise and this function between frames.
 *
 * Decisions the issue left open: rows of a pyramid plane are not padded; scale must be finite and > 0; costs of a tile without
 * history are (0, 0); tdk_motion_match with index == NULL always matches; the key's cost is that of the offset, the zero
 * preference compares costs only; the field may not overlap out or the state, and is not checked against src.
 */
#ifndef TDK_HIP_MOTION_H
#define TDK_HIP_MOTION_H

#include <stddef.h>

#include "tdk_hip.h"
#include "tdk_hip_temporal.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TDK_MOTION_ABI_VERSION 1

/* The tile of one displacement: the output tile of a workgroup of the temporal filter. */
#define TDK_MOTION_TILE_W 64
#define TDK_MOTION_TILE_H 32
#define TDK_MOTION_MAX_LEVELS 4
#define TDK_MOTION_MAX_SEARCH 4
#define TDK_MOTION_MAX_DISPLACEMENT 78
#define TDK_MOTION_MAX_ZERO_BIAS 65535

int tdk_motion_abi_version(void);

/* Bytes of a pyramid buffer (two slots, layout above).  0 for arguments tdk_motion_pyramid would reject. */
size_t tdk_motion_pyramid_bytes(int width, int height, int levels);

/* One launch on `stream`: the grey plane of src and its coarser levels into one slot of `pyramid`.  A workgroup reduces its own
 * tile of 32 x 16 level-0 values through all levels in LDS.  No allocation, copy, memset, synchronisation or atomic.  Argument
 * errors (null pointers, dtype tag, sizes, scale, levels, which, the 16-byte alignment of pyramid, the 4-byte alignment of index,
 * overlap of src and pyramid) are reported before any HIP call. */
int tdk_motion_pyramid(const void* src, int src_dtype, int width, int height, float scale, int levels, void* pyramid, const uint32_t* index, int which,
                       tdk_stream_t stream);

/* One launch on `stream`: a wave per tile walks the levels coarse to fine and writes field (Ty x Tx x 2 int16) and, when not NULL,
 * costs (Ty x Tx x 2 uint32).  No allocation, copy, memset, synchronisation or atomic.  Argument errors (null pointers, sizes,
 * levels, search, zero_bias, which_cur, which_ref, alignments of the pyramids, of index, field (4 bytes) and costs (8 bytes),
 * overlap of field or costs with a pyramid or each other) are reported before any HIP call. */
int tdk_motion_match(const void* pyramid_cur, int which_cur, const void* pyramid_ref, int which_ref, int width, int height, int levels, int search,
                     uint32_t zero_bias, const uint32_t* index, int16_t* field, uint32_t* costs, tdk_stream_t stream);

/* Exactly two launches on `stream`: the compensated filter, then a one-lane kernel that advances idx by the rule of
 * tdk_temporal_denoise (idx + 1, 0xFFFFFFFF -> 2).  The arguments of tdk_temporal_denoise, its checks and its properties
 * (capturable, replayable, bit-reproducible), and `field`: Ty x Tx x 2 int16 on a 4-byte boundary, not NULL, overlapping neither
 * out nor state.  The LDS of the filter launch is tdk_temporal_lds_bytes(radius). */
int tdk_motion_temporal_denoise(const void* src, int src_dtype, void* out, int out_dtype, void* state, int state_dtype, int width, int height,
                                uint32_t pattern, const float* model, const float* gains, int radius, float t_lo, float t_hi, float pixel_c2, float n_max,
                                float v_min, const int16_t* field, tdk_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
