/*
 * tdk_hip_tables.h -- entry points of libtdk_hip.so that evaluate a point operator of binary16 pixels through a table over the
 * 65 536 binary16 codes instead of per pixel.
 *
 * The other headers under include/ stay pinned; these are declared here, with their own version number.  The conventions of
 * tdk_hip.h apply: device pointers, a HIP stream per call, TDK_OK or a tdk_status code with the message in tdk_last_error(),
 * nothing allocates device memory.
 *
 * Tone map.  With binary16 storage, the Reinhard mapper and vibrance 0, output byte c of a pixel is a function of input
 * channel c and the per-image constants alone:
 *     mean = light_adapt-lerp of metrics[2 + c] and x_c,  ad = (mean / exposure)^map_key,  g = (x_c / (ad + x_c))^(1 / gamma),
 *     byte = quantise(clip(g)),
 * (nothing crosses channels: Reinhard is bounded, so the overflow rule of the skipped Lab round trip never fires while
 * 1 / gamma <= 2).  tdk_tonemap_ex evaluates that function once per channel and code -- 3 x 65 536 evaluations by the very device
 * function tdk_tonemap runs per sample, 0.5 % of a 12 MP frame's -- into `table`, and the frame's pixels then take their bytes
 * from it: one byte gather per sample, no transcendental.  The bytes are those of tdk_tonemap for every input, special values
 * included, with one exception: when map_key sits on its upper clamp (metrics[0] <= -9.21034: a black frame) and the frame has
 * negative samples, tdk_tonemap's choice between its two arithmetic forms depends on which pixels share a thread, the table
 * chooses per code, and a byte whose pre-quantisation value sits at a rounding tie may differ by 1.
 */
#ifndef TDK_HIP_TABLES_H
#define TDK_HIP_TABLES_H

#include <stddef.h>

#include "tdk_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TDK_TABLES_ABI_VERSION 1

/* bytes of the `table` of tdk_tonemap_ex: one byte per channel and binary16 code */
#define TDK_TONEMAP_TABLE_BYTES (3 * 65536)

/* flags of tdk_tonemap_ex */
#define TDK_TONEMAP_DIRECT 1u /* the kernels of tdk_tonemap also where the table form would run (timer tdk_tonemap(direct)) */

int tdk_tables_abi_version(void);

/* tdk_tonemap (tdk_hip.h) with a table and flags.  The table form runs when `table` is not NULL, TDK_TONEMAP_DIRECT is not set,
 * dtype is TDK_F16, mode is TDK_TONEMAP_REINHARD, vibrance == 0, 0 < 1 / gamma <= 2, and the buffers allow four pixels per
 * thread (rgb 16-byte, out 4-byte aligned, npix >= 4); the npix % 4 pixels past the last group of four go through tdk_tonemap's
 * tail kernel.  Every other call runs the kernels of tdk_tonemap unchanged and does not touch the table.
 *   table: TDK_TONEMAP_TABLE_BYTES bytes, or NULL.  Its contents need not be initialised and mean nothing after the call: build and
 *   use are stream-ordered, so calls on ONE stream may share a table; calls on different streams need one each.
 * Unknown flags are an argument error.  Timers: tdk_tonemap(table) for the build, tdk_tonemap for the pixels; under
 * TDK_TONEMAP_DIRECT tdk_tonemap(direct). */
int tdk_tonemap_ex(const void* rgb, uint8_t* out, int64_t npix, int mode, const float* metrics, float gamma, float intensity,
                   float light_adapt, float vibrance, int dtype, uint8_t* table, uint32_t flags, tdk_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
