/*
 * tdk_hip_toneeq.h -- tone equalizer: dodge and burn by exposure band behind a guided-filter mask (libtdk_hip.so), which the
 * reference does not have.
 *
 * The other headers under include/ stay pinned; the tone equalizer is declared here, with its own version number.  The conventions
 * of tdk_hip.h apply: device pointers, a HIP stream per call, TDK_OK or a tdk_status code with the message in tdk_last_error(),
 * nothing allocates device memory.
 *
 * Every pixel is multiplied by a gain that depends on the brightness of the REGION it lies in: the mask m is the frame's luminance
 * smoothed by a self-guided filter (He et al.) at the resolution of cells of s x s pixels, and the gain is a table over log2(m).
 * The table is the caller's (torch_darktable.ToneEqualizer builds it from nine band gains as darktable does).
 *
 * ---- Specification.  All arithmetic is float32, one rounding per written operation, no contraction (no FMA); parentheses give the
 * order; divisions are correctly rounded.  Inputs are finite.
 *
 * The frame is (height, width, 3), float32 or binary16 (converted exactly to float32); sizes 1..65535 per axis.  The result has the
 * type of the frame.  Parameters: cell s in {2, 4, 8, 16}; radius r in 0..8, in cells; eps > 0, in linear luminance squared;
 * weights w0, w1, w2 finite and >= 0; the table T of TDK_TONEEQ_TABLE float32 values in device memory.
 * pos(v) = v > 0 ? v : +0 below.
 *
 * 1. Luminance.
 *      Y = pos((w0*r + w1*g) + w2*b)
 *
 * 2. Cell means.  The grid is CW = ceil(width / s) by CH = ceil(height / s).  Cell (cy, cx) takes the s x s values
 *    Y[min(cy*s + j, height - 1)][min(cx*s + i, width - 1)]: every cell sums s*s values.  A row is summed as a balanced binary tree
 *    over adjacent pairs ((v0 + v1) + (v2 + v3)) + ...; the s row sums are summed as the same tree over j.
 *      L = tree * (1 / (s*s))             (the factor is a power of two)
 *
 * 3. Coefficients.  box(P)(cy, cx) sums P over the (2r+1) x (2r+1) cells around (cy, cx), indices clamped to the grid:
 *      h(cy, cx)   = (..((P[cy][c(-r)] + P[cy][c(-r+1)]) + P[cy][c(-r+2)]) + ..) + P[cy][c(r)]     c(k) = min(max(cx + k, 0), CW - 1)
 *      box(cy, cx) = (..((h(d(-r), cx) + h(d(-r+1), cx)) + ..) + h(d(r), cx)                        d(k) = min(max(cy + k, 0), CH - 1)
 *    (2r adds per pass: the first tap starts the sum.)  inv = (float)(1.0 / ((2r+1)*(2r+1))), computed in double, rounded once.
 *      mean = box(L)*inv
 *      corr = box(L*L)*inv
 *      var  = pos(corr - mean*mean)
 *      a    = var / (var + eps)
 *      b    = mean - a*mean
 *
 * 4. Second box.
 *      A = box(a)*inv
 *      B = box(b)*inv
 *
 * 5. Upsampling to the pixel (x, y), bilinear between cell centres, in integers:
 *      q  = max(2*x + 1 - s, 0)      x0 = q / (2*s)      fx = (float)(q % (2*s)) / (2*s)      x1 = min(x0 + 1, CW - 1)
 *    and the same along y (y0, y1, fy, CH).  lerp(p0, p1, f) = p0 + f*(p1 - p0).
 *      Au = lerp(lerp(A[y0][x0], A[y0][x1], fx), lerp(A[y1][x0], A[y1][x1], fx), fy)        Bu alike
 *      m  = Au*Y + Bu
 *
 * 6. Gain.  The table covers TDK_TONEEQ_EV_MIN .. TDK_TONEEQ_EV_MAX in TDK_TONEEQ_STEPS steps per octave, the nodes spaced
 *    linearly inside an octave: node j stands at (1 + (j % 32) / 32) * 2^(j / 32 - 16).
 *      mc = fminf(fmaxf(m, 2^-16), 16 - 2^-20)          (the largest float32 below 2^4)
 *      e  = (bits(mc) >> 23) - 127      M = bits(mc) & 0x7FFFFF
 *      i  = (e + 16)*32 + (M >> 18)     f = (float)(M & 0x3FFFF) / 262144
 *      gain = T[i] + f*(T[i+1] - T[i])
 *    No logarithm or exponential runs on the device.
 *
 * 7. Result.
 *      out[c] = x[c] * gain             c = 0, 1, 2; no clamp; binary16 is rounded to nearest even once, at the store
 *    With mask_out (a float32 (height, width) plane) m is stored as well -- m, not mc.  With dst null only the mask is written.
 *
 * Identity: a table of ones returns the bits of the frame.
 *
 * Buffers are contiguous at any element alignment; dst and mask_out must not overlap src, the table, the workspace or each other.
 */
#ifndef TDK_HIP_TONEEQ_H
#define TDK_HIP_TONEEQ_H

#include <stddef.h>

#include "tdk_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TDK_TONEEQ_ABI_VERSION 1

/* the gain table: exposures covered, nodes per octave, entries = (EV_MAX - EV_MIN)*STEPS + 1 */
#define TDK_TONEEQ_EV_MIN -16
#define TDK_TONEEQ_EV_MAX 4
#define TDK_TONEEQ_STEPS 32
#define TDK_TONEEQ_TABLE 641

#define TDK_TONEEQ_MAX_RADIUS 8

int tdk_toneeq_abi_version(void);

/* Bytes of device workspace a call needs: the three float32 cell planes L, a and b of CW x CH values each, plus what aligning them
 * takes.  Every value a launch reads was written by an earlier launch of the same call: nothing needs zeroing.  Host query; 0 for
 * arguments tdk_toneeq would reject. */
size_t tdk_toneeq_workspace_bytes(int width, int height, int cell);

/* LDS bytes of the largest workgroup over the launches of a call; static, at most 64 KB.  Host query; 0 for arguments tdk_toneeq
 * would reject. */
size_t tdk_toneeq_lds_bytes(int dtype, int cell, int radius);

/* ---- The stage (csrc/toneequal.hip).  Three launches: cell means, coefficients, apply.  No allocation, no copy, no memset, no
 * atomics, no synchronisation -- capturable in a graph from the first call, and deterministic.  dst (the frame's type) or mask_out
 * (float32) may be null, not both.  workspace: tdk_toneeq_workspace_bytes bytes of device memory at any alignment, owned by the call
 * until its last launch has finished (one workspace per stream).  table: TDK_TONEEQ_TABLE float32 values in DEVICE memory, read by
 * every call: a caller may rewrite them between calls, also between the replays of a captured call.  weights is a HOST pointer to
 * three floats, read during the call.  flags is reserved and must be 0.  Argument errors (null pointers, sizes, dtype, cell, radius,
 * eps, weights, flags, alignment of mask_out and table, overlap) are reported before any HIP call. */
int tdk_toneeq(const void* src, void* dst, float* mask_out, void* workspace, const float* table, int width, int height, int dtype, int cell,
               int radius, float eps, const float* weights /* host, 3 */, int flags, tdk_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
