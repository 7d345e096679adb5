/*
 * tdk_hip_hdralign.h -- exposure brackets of a moving rig (libtdk_hip.so): every frame of a bracket is matched per tile against the
 * anchor frame, and the merge of tdk_hip_hdr.h reads every frame where the scene is.  tdk_hdr_merge assumes that all frames show the
 * same geometry: a frame that disagrees with a site's anchor loses its weight there.  On a bracket whose frames are panned against
 * each other by a few sites every textured site disagrees, the merge falls back to one frame, and where the anchor clips the site is
 * taken from a shorter frame that shows the scene somewhere else.  The reference has no counterpart.
 *
 * include/tdk_hip.h (the reference's surface) and the other tdk_hip_*.h headers stay pinned; this block is declared here, with its own
 * version number.  The conventions of tdk_hip.h apply: device pointers, a HIP stream per call, TDK_OK or a tdk_status code with the
 * message in tdk_last_error(), nothing allocates device memory.
 *
 * The block is three steps, F = num_frames:
 *   1. tdk_hdralign_pyramid, once per frame: the grey pyramid of tdk_hip_motion.h with the frame brought into the units of the longest
 *      frame;
 *   2. tdk_motion_match (tdk_hip_motion.h), unchanged, with index == NULL, once per frame f != ref: cur is the slot of the anchor frame
 *      ref and ref is the slot of frame f.  That gives field_f with frame_f[p + d] ~ anchor[p];
 *   3. tdk_hdralign_merge, once.
 *
 * ---- Specification (tdk_hdralign_pyramid).  Everything of tdk_motion_pyramid with index == NULL holds: the same grey formula, levels,
 * buffer layout and slot `which`.  ONE change: the scale the grey formula uses is computed on the device,
 *   e_hi = the largest of the F device floats exposures[0..F-1], by the rule of tdk_hip_hdr.h (a later frame replaces an earlier one
 *          only when >)
 *   s    = scale * (e_hi / exposures[frame])           (a float32 division, then a float32 product)
 *   q = (x00 + x01) + (x10 + x11);   u = fminf(fmaxf(q * s, 0), 1);   g = (uint8)(sqrtf(u) * 255 + 0.5f)
 * Every frame's grey plane is then in the units of the longest frame and clamps to 255 where that frame clips: clipped regions cost
 * nothing in the match and do not pull it.  Nothing of exposures is checked on the device; a NaN ratio gives grey 0 by the fmaxf rule.
 *
 * ---- Specification (tdk_hdralign_merge).  Everything of tdk_hdr_merge (tdk_hip_hdr.h: input, model, parameters, steps 1 to 6) holds,
 * with these changes.
 * 1. ref is a frame index, 0..F-1; -1 is refused: the host must know which frame the others were matched to.
 * 2. fields is F x Ty x Tx x 2 int16 on a 4-byte boundary, (dy, dx) in sites per tile of tdk_hip_motion.h: TDK_MOTION_TILE_W x
 *    TDK_MOTION_TILE_H = 64 x 32 sites, Tx = ceil(width / 64), Ty = ceil(height / 32).  It may not be NULL and overlaps neither out nor
 *    mask.
 * 3. For the OUTPUT site (i, j):  D_f = fields[f][i / 32][j / 64] & ~1 for f != ref, and D_ref = 0.  The row of ref is never read.  Odd
 *    values are masked on the device; any int16 is memory-safe.
 * 4. For every site q that enters the computation of that output site (its own, the 3 x 3 of the clip test, the windows): the sample
 *    of frame f is the frame's sample at q + D_f if that lies inside the frame, else NaN.  So it counts as clipped and takes its eight
 *    neighbours with it.  "In-frame sites" in the window and 3 x 3 rules keeps meaning q itself inside the frame.
 * 5. A site blown in every frame takes g = lo when q + D_lo lies inside the frame, else g = ref.  The mask byte carries that g.
 *
 * Consequences.  With all-zero fields and ref >= 0 the function is tdk_hdr_merge bit for bit, mask included.  With finite samples no
 * out is NaN (the NaN of rule 4 is clipped wherever it is seen, and rule 5 keeps it from being an anchor).  A 32 x 32 output tile of
 * the merge lies inside one 64 x 32 motion tile: a workgroup reads each frame at one uniform offset, as the compensated temporal filter
 * does, and a window near a motion-tile seam evaluates the neighbour tile's sites with the OUTPUT tile's displacements.  The result
 * lives in the coordinates of ref.
 */
#ifndef TDK_HIP_HDRALIGN_H
#define TDK_HIP_HDRALIGN_H

#include <stddef.h>

#include "tdk_hip.h"
#include "tdk_hip_hdr.h"
#include "tdk_hip_motion.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TDK_HDRALIGN_ABI_VERSION 1

int tdk_hdralign_abi_version(void);

/* Static LDS bytes of a workgroup of the merge launch: tdk_hdr_lds_bytes(radius) and 64 bytes of per-frame displacements.  0 for a
 * radius tdk_hdralign_merge would reject. */
size_t tdk_hdralign_lds_bytes(int radius);

/* One launch on `stream`: the grey plane of frame `frame` of a bracket and its coarser levels into slot `which` of `pyramid`.  No
 * allocation, copy, memset, synchronisation or atomic.  Argument errors (those of tdk_motion_pyramid; a null exposures; num_frames
 * outside 2..TDK_HDR_MAX_FRAMES; frame outside 0..num_frames-1; exposures not on a 4-byte boundary or overlapping pyramid) are reported
 * before any HIP call. */
int tdk_hdralign_pyramid(const void* src, int src_dtype, int width, int height, float scale, int levels, void* pyramid, int which, const float* exposures,
                         int num_frames, int frame, tdk_stream_t stream);

/* Exactly one launch on `stream`: no workspace, no allocation, copy, memset, synchronisation or atomic: capturable in a graph from the
 * first call, bit-reproducible.  Argument errors (those of tdk_hdr_merge; ref == -1; a null or misaligned fields; fields overlapping out
 * or mask) are reported before any HIP call. */
int tdk_hdralign_merge(const void* const* frames, int num_frames, int src_dtype, void* out, int out_dtype, unsigned char* mask, int width, int height,
                       uint32_t pattern, const float* exposures, int ref, const float* model, int radius, float clip, float t_lo, float t_hi, float pixel_c2,
                       float v_min, const int16_t* fields, tdk_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
