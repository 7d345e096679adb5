/*
 * tdk_hip_highlights.h -- white balance that reconstructs clipped highlights (libtdk_hip.so), which the reference does not have.
 *
 * include/tdk_hip.h (the reference's surface), include/tdk_hip_ext.h, include/tdk_hip_denoise.h, include/tdk_hip_resample.h,
 * include/tdk_hip_warp.h, include/tdk_hip_raw.h, include/tdk_hip_sharpen.h and include/tdk_hip_wavelet.h stay pinned; the highlight
 * stage is declared here, with its own version number.  The conventions of tdk_hip.h apply: device pointers, a HIP stream per call,
 * TDK_OK or a tdk_status code with the message in tdk_last_error(), nothing allocates device memory.
 *
 * The stage sits where tdk_apply_white_balance sits: it takes the linear mosaic BEFORE white balance (1.0 = white level) and three
 * gains, and returns the white-balanced mosaic.  A site at or above the threshold has lost its value to the sensor's saturation;
 * mode TDK_HL_OPPOSED rebuilds it from the two other colours around it plus one per-frame colour offset (darktable's "inpaint
 * opposed", with the means taken in the linear domain instead of through a cube root, so that the bits are predictable).  The
 * result is NOT clamped from above.
 *
 * ---- Specification.  All arithmetic is float32, one rounding per written operation, no contraction (no FMA); parentheses give the
 * order; divisions are correctly rounded.
 *
 * The frame is width x height, both even, 2..65535.  Row i, column j has the CFA position p = 2*(i & 1) + (j & 1); the Bayer
 * pattern word maps p to a colour (0 = R, 1 = G, 2 = B) as in tdk_hip_raw.h: c = colour(p) = (pattern >> (2*p)) & 3.
 * g is a DEVICE pointer to three finite gains in (0, 64] (R, G, B), as tdk_apply_white_balance takes it.  The input is (height,
 * width) float32 or binary16 (src_dtype), converted exactly to float32: L.  The output is (height, width) float32 or binary16
 * (dst_dtype), rounded to nearest even once, at the store.
 *
 * Parameters: threshold t in (0, 1]; low in [0, 1); min_count >= 1.
 *
 * For every site:
 *   v       = L * g[c]
 *   clipped = (L >= t)          (a NaN is never clipped)
 *   cl[k]   = t * g[k]
 *
 * Mode TDK_HL_CLIP:
 *   m   = fminf(fminf(cl[0], cl[1]), cl[2])
 *   out = fminf(fmaxf(v, 0.0f), m)
 *
 * Mode TDK_HL_OPPOSED:
 *   Reference value ref(i, j).  Over the 3x3 neighbourhood, for each colour k: S_k is the float32 sum of fmaxf(v', 0.0f) over the
 *   sites v' of colour k and n_k their count.  Sites outside the frame are missing; sites are visited row-major, (i-1, j-1) to
 *   (i+1, j+1); S_k starts from 0 and takes one rounding per addition.  (In a Bayer frame every n_k is at least 1, at corners too.)
 *     mean_k = S_k / (float)n_k
 *     ref = 0.5f * (mean_a + mean_b)        a < b the two colours other than c
 *   Statistics.  A site contributes to colour c when all of these hold:
 *     1. it is not clipped
 *     2. v > low * cl[c]
 *     3. at least one in-frame site of its 5x5 neighbourhood is clipped, of any colour
 *     4. d = v - ref satisfies fabsf(d) <= 64.0f      (a NaN does not contribute)
 *   A contributing site adds q = (long long)rintf(d * 1048576.0f) to sum[c] and 1 to cnt[c], both 64-bit integers: the result
 *   does not depend on the order of accumulation.
 *   Chrominance:
 *     chroma[c] = cnt[c] >= min_count ? (float)((double)sum[c] / ((double)cnt[c] * 1048576.0)) : 0.0f
 *   (int64 -> double and double -> float round to nearest even.)
 *   Result:
 *     clipped site:   out = fmaxf(v, ref + chroma[c])
 *     other sites:    out = fmaxf(v, 0.0f)
 *
 * fmaxf and fminf return the other operand for a NaN: a NaN site becomes 0.  The sign of a zero result is not specified.
 *
 * Identities: with no clipped site, mode TDK_HL_OPPOSED returns fmaxf(L * g[c], 0); where all v <= 1 those are the bits of
 * tdk_apply_white_balance.
 *
 * Buffers are contiguous at any element alignment (stats: 8 bytes); dst must not overlap src, gains, chroma or the workspace.
 */
#ifndef TDK_HIP_HIGHLIGHTS_H
#define TDK_HIP_HIGHLIGHTS_H

#include <stddef.h>

#include "tdk_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TDK_HIGHLIGHTS_ABI_VERSION 1

/* mode of tdk_highlights */
#define TDK_HL_CLIP 0
#define TDK_HL_OPPOSED 1

int tdk_highlights_abi_version(void);

/* Bytes of device workspace a call that gathers the statistics needs: a 48-byte record (sum[3], cnt[3]) per workgroup of the
 * statistics launch, a few KB, the same for every frame size.  Every record is written by every such call: nothing needs zeroing. */
size_t tdk_highlights_workspace_bytes(void);

/* LDS bytes of the largest workgroup over the launches of a call in `mode`: 0 for TDK_HL_CLIP (streaming), the staged tile with
 * its apron for TDK_HL_OPPOSED; at most 64 KB.  Host query; 0 for a mode tdk_highlights would reject. */
size_t tdk_highlights_lds_bytes(int mode);

/* ---- The statistics alone (csrc/highlights.hip): the statistics launch and a small finishing launch.  stats (device, 8-byte
 * aligned) receives sum[3] then cnt[3]; chroma (device) receives the three chrominance values; either may be null, not both.
 * No atomics, no synchronisation, no memset, no allocation: capturable in a graph from the first call, and deterministic.
 * workspace: tdk_highlights_workspace_bytes bytes of device memory at any alignment, owned by the call until its last launch has
 * finished (one workspace per stream).  Argument errors are reported before any HIP call. */
int tdk_highlights_chrominance(const void* src, int src_dtype, void* workspace, int width, int height, uint32_t pattern, const float* gains,
                               float threshold, float low, int min_count, long long* stats /* device, sum[3] then cnt[3] */,
                               float* chroma /* device, 3 */, tdk_stream_t stream);

/* ---- The stage.  mode TDK_HL_CLIP: one streaming launch; workspace and chroma must be null.  mode TDK_HL_OPPOSED with chroma
 * null: the statistics launch and the apply launch (workspace needed).  With chroma given (device, 3 floats): the apply launch
 * only; the three values are used as they are, min_count is not applied again and workspace may be null.  Both ways give the same
 * bits when chroma comes from tdk_highlights_chrominance on the same frame.  At most two launches, no atomics, no synchronisation,
 * no memset, no allocation.  Argument errors (null pointers, sizes, odd width or height, dtype tags, pattern, mode, threshold, low,
 * min_count, overlap) are reported before any HIP call. */
int tdk_highlights(const void* src, int src_dtype, void* dst, int dst_dtype, void* workspace, int width, int height, uint32_t pattern,
                   const float* gains, float threshold, float low, int min_count, int mode, const float* chroma /* device, or NULL */,
                   tdk_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
