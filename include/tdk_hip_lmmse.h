/*
 * tdk_hip_lmmse.h -- the demosaic for noisy frames of libtdk_hip.so: Zhang and Wu's directional linear minimum mean-square-error
 * demosaic (IEEE Trans. Image Processing 14 (12), 2005; darktable's "LMMSE"), which the reference does not have.
 *
 * The other headers under include/ stay pinned; this demosaic is declared here, with its own version number.  The conventions of
 * tdk_hip.h apply: device pointers, a HIP stream per call, TDK_OK or a tdk_status code with the message in tdk_last_error(),
 * nothing allocates device memory.
 *
 * Bilinear, PPG and RCD choose a direction per pixel from gradients, and on a noisy mosaic they take noise for structure.  Here
 * the difference "green minus the other colour" is estimated along the row and along the column, each estimate is split into a
 * low-passed part and a residue, a linear estimator weighs the two by their variances over nine sites, and the two directions
 * are fused by the variances of their errors: where the frame holds only noise the result tends to the low pass, where it holds
 * an edge to the direction along it.  By default the arithmetic runs on square roots of the samples, in which shot noise is about
 * uniform over brightness.
 *
 * ---- Specification.  All arithmetic is float32, one rounding per written operation, no contraction (no FMA); parentheses and the
 * stated order give the order of operations; divisions and sqrtf are correctly rounded.  Only + - * /, sqrtf, fminf and fmaxf run on
 * the device.  Inputs are finite.
 *
 * src is a (height, width) mosaic of TDK_F32 or TDK_F16, dst (height, width, 3) interleaved RGB of TDK_F32 or TDK_F16, chosen
 * independently.  m is a sample converted to float32 (exact).  The CFA colour of a site is that of tdk_hip.h's pattern word.
 *
 * Edges: an index outside the frame is reflected about the edge sample without repeating it (-k -> k, n-1+k -> n-1-k), folded
 * until it lies inside (a 2 x 2 frame is legal).  Reflection keeps the parity of an index and so the CFA colour of a site.  Every
 * plane below (t, d, p, D) is defined at a reflected position as its value at the folded index.  (Every formula below is symmetric
 * under reversal of an axis and float32 addition commutes, so evaluating a formula AT a reflected position from reflected operands
 * gives those same bits: an implementation may do either.)
 *
 * Domain:
 *   t = sqrtf(fmaxf(m, 0))                 the default
 *   t = m                                  with TDK_LMMSE_LINEAR
 * (fmaxf(-0, 0) may be either zero: the sign of a zero changes no bit of the output, see Output.)
 *
 * Directional estimates, at every site, for the direction h (offsets along the row) and v (along the column):
 *   e = (0.5*(t[-1] + t[+1]) - 0.25*(t[-2] + t[+2])) + 0.5*t[0]
 *   d = e - t[0]                           at a red or blue site
 *   d = t[0] - e                           at a green site
 * Both are estimates of green minus the other colour of the row (h) or column (v).  A constant mosaic gives d == 0 exactly.
 *
 * Low pass along the same direction, at every site:
 *   p = g0*d[0];   for k = 1..4 in ascending order:   p = p + gk*(d[-k] + d[+k])
 *   gk = exp(-k*k/8) / (g0' + 2*(g1' + g2' + g3' + g4')) with gk' = exp(-k*k/8), formed in double and rounded once to float32:
 *   g0 = 0x1.a22092p-3f (0.20416369)   g1 = 0x1.70fefap-3f (0.18017383)   g2 = 0x1.fb36c8p-4f (0.12383154)
 *   g3 = 0x1.0f7df8p-4f (0.06628224)   g4 = 0x1.c4b2eep-6f (0.02763055)
 *
 * LMMSE per direction, at red and blue sites, over the window k = -4..4 along that direction.  S(a) is a window sum in this order:
 *   S(a) = a[0];   for k = 1..4 in ascending order:   S = S + (a[-k] + a[+k])
 *   mu = S(p) * NINTH                      NINTH = 0x1.c71c72p-4f, 1/9 rounded to float32 (a product, not a division)
 *   vx = EPS + S(a)                        a[k] = (p[k] - mu)*(p[k] - mu);   EPS = 1e-7f = 0x1.ad7f2ap-24f
 *   vn = EPS + S(b)                        b[k] = (d[k] - p[k])*(d[k] - p[k])
 *   x  = (p[0]*vn + d[0]*vx) / (vx + vn)
 *   v  = (vx*vn) / (vx + vn)
 *
 * Fusion, at red and blue sites:
 *   D = (x_h*v_v + x_v*v_h) / (v_h + v_v)  green minus the site's own colour
 *
 * Green:
 *   G = t + D                              at a red or blue site
 *   G = t                                  at a green site
 * Red and blue at a green site: the colour that shares the row from the horizontal neighbours, the other from the vertical ones:
 *   C = G - 0.5*(D[-1] + D[+1])
 * The opposite colour at a red or blue site, with D[dy,dx]:
 *   C = G - 0.25*((D[-1,-1] + D[-1,+1]) + (D[+1,-1] + D[+1,+1]))
 *
 * Output: the site's own colour is the input sample itself (the same dtype on both sides: its bits, negative values and -0
 * included; otherwise converted).  An estimated value c is stored as q*q with q = fmaxf(c, 0) in the square-root domain -- the
 * product is a float32 value -- and as it is, not clamped, with TDK_LMMSE_LINEAR.  binary16 is rounded to nearest even.
 * Refinement by medians of colour differences is not part of this stage: tdk_postprocess does that.
 *
 * Identities:
 *   - the own colour passes through;
 *   - a constant non-negative mosaic comes back bit for bit in all three channels with TDK_LMMSE_LINEAR;
 *   - a horizontal flip of the mosaic with the matching pattern gives the flipped output bit for bit, and so does a vertical flip;
 *   - the result depends neither on the tile size nor on a tile's position.
 *
 * Limits: sizes 2..65535 per axis, odd sizes included; src and dst must not overlap; buffers are contiguous at any element
 * alignment.
 */
#ifndef TDK_HIP_LMMSE_H
#define TDK_HIP_LMMSE_H

#include <stddef.h>
#include <stdint.h>

#include "tdk_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TDK_LMMSE_ABI_VERSION 1

/* flags of tdk_lmmse; the other bits are reserved and must be 0 */
#define TDK_LMMSE_LINEAR 1

/* the output tile of one workgroup, in pixels */
#define TDK_LMMSE_TILE_W 32
#define TDK_LMMSE_TILE_H 32
/* what a stored site depends on, in samples along each axis: D at +-1, p and d at +-4 of that, d at +-4 of p, t at +-2 of d */
#define TDK_LMMSE_APRON 11
#define TDK_LMMSE_MIN_SIZE 2
#define TDK_LMMSE_MAX_SIZE 65535

int tdk_lmmse_abi_version(void);

/* LDS bytes one workgroup of tdk_lmmse takes (t over the tile and its apron, the two d planes, the two p planes and D); static, at
 * most 64 KB, the same for every instantiation.  Host query; 0 for arguments tdk_lmmse would reject. */
size_t tdk_lmmse_lds_bytes(int src_dtype, int dst_dtype, int flags);

/* ---- The stage (csrc/lmmse.hip).  One launch of one kernel; no workspace, no allocation, no copy, no memset, no atomics, no
 * synchronisation -- capturable in a graph from the first call, and deterministic.  Argument errors (null pointers, sizes, pattern,
 * dtypes, unknown flag bits, overlap) are reported before any HIP call. */
int tdk_lmmse(const void* src, void* dst, int width, int height, uint32_t pattern, int src_dtype, int dst_dtype, int flags, tdk_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
