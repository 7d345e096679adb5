/*
 * tdk_hip_dehaze.h -- haze removal: He et al.'s dark channel prior with a guided transmission map (libtdk_hip.so), which the
 * reference does not have.
 *
 * The other headers under include/ stay pinned; the haze removal is declared here, with its own version number.  The conventions
 * of tdk_hip.h apply: device pointers, a HIP stream per call, TDK_OK or a tdk_status code with the message in tdk_last_error(),
 * nothing allocates device memory.
 *
 * Haze adds a veil A*(1 - t) to the scene and attenuates it by t, the transmission, which falls with distance:
 * x = J*t + A*(1 - t).  The ambient light A is estimated from the haziest cells of the frame (the largest dark channel), t from the
 * dark channel of x / A at the resolution of cells of s x s pixels, refined by a filter guided by the frame's luminance so that it
 * stops at depth edges, and J = (x - A) / t + A.
 *
 * ---- Specification.  All arithmetic is float32, one rounding per written operation, no contraction (no FMA); parentheses give the
 * order; divisions are correctly rounded.  Inputs are finite.  pos(v) = v > 0 ? v : +0.
 *
 * The frame is (height, width, 3), float32 or binary16 (converted exactly to float32); sizes 1..65535 per axis and CW*CH <= 2^24.
 * The result has the type of the frame.  Parameters: cell s in {2, 4, 8, 16}; dark_radius rd in 0..4, in cells; radius rg in 0..8,
 * in cells; eps > 0; strength in [0, 1]; floor in [2^-6, 1]; weights w0, w1, w2 finite and >= 0; count K in 1..CW*CH.
 *
 * 1. Cells.  The grid is CW = ceil(width / s) by CH = ceil(height / s).  Cell (cy, cx) takes the s x s samples
 *    x[min(cy*s + j, height - 1)][min(cx*s + i, width - 1)]: every cell takes s*s samples.  A row is summed as a balanced binary
 *    tree over adjacent pairs ((v0 + v1) + (v2 + v3)) + ...; the s row sums are summed as the same tree over j.
 *      m_c = minimum of pos(x_c) over the samples                c = 0, 1, 2
 *      M_c = tree(pos(x_c)) * (1 / (s*s))                        (the factor is a power of two)
 *      Y = pos((w0*r + w1*g) + w2*b)
 *      L = tree(Y) * (1 / (s*s))
 *
 * 2. Dark channel (for the estimate only).  minwin_r(P)(cy, cx) is the minimum of P over the (2r+1) x (2r+1) cells around
 *    (cy, cx), indices clamped to the grid.
 *      d = minwin_rd(min(min(m0, m1), m2))
 *
 * 3. Ambient light (for the estimate only).  d >= 0, so bits(d), its pattern as an unsigned integer, is monotone in d.
 *      T = the K-th largest of the CW*CH values bits(d), counted with multiplicity
 *      S = every cell with bits(d) >= T          (all ties are in: the result depends on no order)
 *      n = |S|
 *      fix(v) = (int64)(fminf(v, 65536) * 1048576)          (the product is exact, the conversion truncates)
 *      sum_c = the int64 sum of fix(M_c) over S
 *      ambient[c] = (float)(((double)sum_c / (double)n) * 2^-20)
 *      ambient[3] = (float)n
 *
 * 4. Coefficients.  box(P)(cy, cx) sums P over the (2rg+1) x (2rg+1) cells around (cy, cx), indices clamped to the grid:
 *      h(cy, cx)   = (..((P[cy][c(-rg)] + P[cy][c(-rg+1)]) + P[cy][c(-rg+2)]) + ..) + P[cy][c(rg)]   c(k) = min(max(cx + k, 0), CW - 1)
 *      box(cy, cx) = (..((h(e(-rg), cx) + h(e(-rg+1), cx)) + ..) + h(e(rg), cx)                      e(k) = min(max(cy + k, 0), CH - 1)
 *    (2rg adds per pass: the first tap starts the sum.)  inv = (float)(1.0 / ((2rg+1)*(2rg+1))), computed in double, rounded once.
 *      A_c = fmaxf(ambient[c], 2^-10)            (a NaN or zero ambient cannot divide by zero)
 *      i_c = 1 / A_c
 *      q = fminf(fminf(m0*i0, m1*i1), m2*i2)
 *      t = 1 - strength * fminf(minwin_rd(q), 1)
 *      mL = box(L)*inv
 *      mt = box(t)*inv
 *      cov = box(L*t)*inv - mL*mt
 *      var = pos(box(L*L)*inv - mL*mL)
 *      a = cov / (var + eps)
 *      b = mt - a*mL
 *
 * 5. Apply.
 *      A2 = box(a)*inv
 *      B2 = box(b)*inv
 *    Upsampling to the pixel (x, y), bilinear between cell centres, in integers:
 *      q  = max(2*x + 1 - s, 0)      x0 = q / (2*s)      fx = (float)(q % (2*s)) / (2*s)      x1 = min(x0 + 1, CW - 1)
 *    and the same along y (y0, y1, fy, CH).  lerp(p0, p1, f) = p0 + f*(p1 - p0).
 *      Au = lerp(lerp(A2[y0][x0], A2[y0][x1], fx), lerp(A2[y1][x0], A2[y1][x1], fx), fy)        Bu alike from B2
 *      tp = fminf(fmaxf(Au*Y + Bu, floor), 1)
 *      rt = 1 / tp
 *      out_c = pos((x_c - A_c)*rt + A_c)         no upper clamp; binary16 is rounded to nearest even once, at the store
 *    transmission_out (a float32 (height, width) plane) receives tp.  With dst null only the transmission is written.
 *
 * strength 0 gives t = 1, a = 0, b = 1 up to the rounding of the box means.
 *
 * Buffers are contiguous at any element alignment (ambient and transmission_out at 4 bytes); dst, transmission_out and ambient must
 * not overlap src, the workspace or each other.
 */
#ifndef TDK_HIP_DEHAZE_H
#define TDK_HIP_DEHAZE_H

#include <stddef.h>

#include "tdk_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TDK_DEHAZE_ABI_VERSION 1

#define TDK_DEHAZE_MAX_DARK_RADIUS 4
#define TDK_DEHAZE_MAX_RADIUS 8
/* the largest grid, CW*CH: the int64 sums of step 3 cannot overflow below it */
#define TDK_DEHAZE_MAX_CELLS 16777216
/* float32 cell planes of the workspace: m0 m1 m2, M0 M1 M2, L, d, a, b */
#define TDK_DEHAZE_PLANES 10

int tdk_dehaze_abi_version(void);

/* Bytes of device workspace a call needs: TDK_DEHAZE_PLANES float32 cell planes of CW x CH values each, plus what aligning them
 * takes.  Every value a launch reads was written by an earlier launch of the same call: nothing needs zeroing.  Host query; 0 for
 * arguments tdk_dehaze would reject. */
size_t tdk_dehaze_workspace_bytes(int width, int height, int cell);

/* LDS bytes of the largest workgroup over the launches of a call; static, at most 64 KB.  Host query; 0 for arguments tdk_dehaze
 * would reject. */
size_t tdk_dehaze_lds_bytes(int dtype, int cell, int dark_radius, int radius);

/* ---- The stage (csrc/dehaze.hip).  No allocation, no copy, no memset, no synchronisation, no atomics but integer atomics on LDS
 * -- capturable in a graph from the first call, and deterministic.  workspace: tdk_dehaze_workspace_bytes bytes of device memory
 * at any alignment, owned by the call until its last launch has finished (one workspace per stream).  weights is a HOST pointer to
 * three floats, read during the call.  flags is reserved and must be 0.  Argument errors (null pointers, sizes, dtype, cell, radii,
 * count, eps, strength, floor, weights, flags, alignment, overlap) are reported before any HIP call.
 *
 * tdk_dehaze_ambient: steps 1 to 3, three launches (cells, dark channel, select).  ambient: four float32 values in DEVICE memory,
 * written: A_r, A_g, A_b, n.  count is K, 1..CW*CH. */
int tdk_dehaze_ambient(const void* src, float* ambient, void* workspace, int width, int height, int dtype, int cell, int dark_radius, int count,
                       int flags, tdk_stream_t stream);

/* tdk_dehaze: the frame.  count > 0: steps 1 to 5, five launches (cells, dark channel, select, coefficients, apply); ambient is
 * written by the third and read by the last two.  count == 0: steps 1, 4 and 5, three launches (cells, coefficients, apply);
 * ambient is read on the device by every call: a caller may rewrite it between calls, also between the replays of a captured
 * call.  dst (the frame's type) or transmission_out (float32) may be null, not both. */
int tdk_dehaze(const void* src, void* dst, float* transmission_out, void* workspace, float* ambient, int width, int height, int dtype, int cell,
               int dark_radius, int radius, int count, float eps, float strength, float floor, const float* weights /* host, 3 */, int flags,
               tdk_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
