/*
 * tdk_bilateral_geometry.h -- host-only view of the bilateral tile kernel's planning (bilateral.hip: plan_tiles and the dispatch
 * of launch_tiles), exported from libtdk_hip.so so that the rule that selects the constant-geometry kernel can be tested without
 * a launch (tests/test_bilateral_geometry.py).  A test hook beside the product surface of include/.
 */
#ifndef TDK_BILATERAL_GEOMETRY_H
#define TDK_BILATERAL_GEOMETRY_H

#include "../../include/tdk_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* words of a geometry record: tile kernel applies (0 / 1), constant-geometry kernel selected (0 / 1), then the LDS grid's
 * sz, rs, plane, usize, lw, lh, ncx, ncy, hx, hy */
#define TDK_BILATERAL_GEOMETRY_WORDS 12

/* planned: the geometry tdk_bilateral_lab would launch its tile kernel with for this image and these sigmas (all zero when the
 * four-kernel path runs), word 1 set when it equals the constant set and the constant-geometry kernel is the one launched for
 * 16-byte aligned planes of a width that is a multiple of 4.  minimal: ncx, ncy, hx, hy, lw, lh as the image's own tiles need
 * them, before the constant shape is considered.  constant: the set the kernel was compiled for (words 0 and 1 are 1). */
int tdk_bilateral_tile_geometry(int width, int height, float sigma_s, float sigma_r, int planned[TDK_BILATERAL_GEOMETRY_WORDS], int minimal[6],
                                int constant[TDK_BILATERAL_GEOMETRY_WORDS]);

/* Which tiles run the interior body of the constant-geometry kernel (csrc/tdk_bilateral_tile.h: tile_is_interior): a tile whose
 * two axis records and sample window are the constant ones, so that no guard against the frame's edge can bind.  The test is
 * separable.  counts: tile columns, tile rows, interior columns, interior rows, interior tiles (their product); all of the last
 * three are 0 where the constant-geometry kernel is not the one planned.  columns / rows (each may be NULL): one byte per tile
 * column / row, 1 = interior. */
#define TDK_BILATERAL_INTERIOR_WORDS 5
int tdk_bilateral_tile_interior(int width, int height, float sigma_s, float sigma_r, int counts[TDK_BILATERAL_INTERIOR_WORDS], unsigned char* columns,
                                unsigned char* rows);

#ifdef __cplusplus
}
#endif
#endif
