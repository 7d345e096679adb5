/*
 * tdk_hip_scaled.h -- the reduced-size demosaic of libtdk_hip.so: a raw (height, width) Bayer mosaic becomes an (out_height,
 * out_width, 3) RGB frame with out_width <= width / 2 and out_height <= height / 2, in one launch that reads the mosaic once.
 * The reference does not have it.
 *
 * The other headers under include/ stay pinned; this stage is declared here, with its own version number.  The conventions of
 * tdk_hip.h apply: device pointers, a HIP stream per call, TDK_OK or a tdk_status code with the message in tdk_last_error(),
 * nothing allocates device memory.
 *
 * Below half size no direction needs deciding: every output pixel is the weighted average of the sites of each colour under its
 * footprint (darktable's clip_and_zoom_demosaic, every camera ISP's preview path).  The weights are tdk_resample's antialiasing
 * triangle, laid over the sites of ALL colours on the same centres, so the three colours of an output pixel are registered on one
 * point; 2 x 2 binning leaves red and blue one site apart and fringes every edge.
 *
 * ---- Specification.  All arithmetic is float32, one rounding per written operation; fmaf(a, b, c) is a*b + c rounded once; no other
 * contraction; divisions are correctly rounded.
 *
 * Per axis, with n_in sites and n_out results, 2*n_out <= n_in <= 16*n_out, for output i and tap j:
 *   num(i, j) = 2*n_out*j + n_out - (2*i + 1)*n_in        an exact integer (formed in 64 bits; |num| of a tap is below 2^17)
 *   tap j in [0, n_in) takes part in output i   iff   |num| < 2*n_in
 *   w(i, j) = 1 - (float)|num| / (float)(2*n_in)          one rounded division, one rounded subtraction; w > 0
 *   parity of a tap: j & 1
 * This is tdk_resample's triangle of half-width n_in / n_out centred on (n_in / n_out)(i + 1/2).  A tap that does not take part is
 * not visited: an inf or a NaN outside the footprint of a colour does not reach that colour of the output.  Under the limits every
 * output has at least one tap of each parity on both axes, and at most 32 taps take part per axis.
 *
 * Horizontal pass, for source row y, output column i, column parity p; the taps j of parity p in ascending order, x the sample:
 *   A_p[y][i]:   acc = w*x for the first tap;   acc = fmaf(w, x, acc) for every further tap
 *   Sx_p[i]:     s = w for the first tap;       s = s + w for every further tap
 * Vertical pass, for output row o, row parity q; the taps y of parity q in ascending order, v their weights:
 *   B_qp[o][i]:  acc = v*A_p[y][i] for the first tap;   acc = fmaf(v, A_p[y][i], acc) for every further tap
 *   Sy_q[o]:     s = v for the first tap;               s = s + v for every further tap
 * Both passes are pattern-blind.  The combine, with (q, p) the row and column parity of a colour's sites in tdk_hip.h's pattern word:
 *   red, blue:   N = B_qp                    D = Sy_q*Sx_p
 *   green:       N = B_0p1 + B_1p2           D = Sy_0*Sx_p1 + Sy_1*Sx_p2      the site in the even row first; each product rounded,
 *                                                                             then the sum
 *   out = N / D
 * dst is (out_height, out_width, 3) interleaved R, G, B of TDK_F32 or TDK_F16: one round-to-nearest-even at the store, nothing is
 * clamped.
 *
 * The sample x of a site:
 *   TDK_F32 source      the value as it is
 *   TDK_F16 source      the value widened (exact)
 *   packed 12 bits      (float)code * (1.0f / 4095.0f), the bits of tdk_decode12_f32 (scaled), in both nibble orders
 * With gains (3 device floats R, G, B, read on the device by every call) the sample is the value tdk_apply_white_balance writes for
 * the site, bit for bit: fminf(fmaxf(x*g, 0), 1) with g the gain of the site's colour -- and, for a TDK_F16 source, rounded to
 * binary16 as that kernel's store does.  (A NaN sample becomes 0 there, as in that kernel.)  With gains == NULL samples pass
 * unchanged: values above 1, as HdrMerge and Highlights leave them, survive.
 *
 * Identities:
 *   - Pattern swap.  On the same samples (gains == NULL, or equal red and blue gains) TDK_PATTERN_RGGB against TDK_PATTERN_BGGR
 *     swaps channels 0 and 2 bit for bit and leaves green's bits; TDK_PATTERN_GRBG against TDK_PATTERN_GBRG likewise.
 *   - Flat frames.  A mosaic that is a positive constant c per colour (normal numbers, no underflow) returns c in that channel
 *     within the relative error g(n) = n*u / (1 - n*u), u = 2^-24, n = 2*(Tx + Ty + 1), with Tx and Ty the largest number of
 *     taps of one parity an output has along x and along y.  Derivation: the weights w, v are the same float32 values in N and in
 *     D, so their own rounding cancels.  A_p is c * sum(w (1 + t)) with at most Tx roundings on a term (one product or fmaf per
 *     tap), B_qp adds at most Ty, so N = c * sum(v w (1 + t)), |t| <= g(Tx + Ty), plus one rounding for green's sum.  Sx_p carries
 *     Tx - 1 roundings, Sy_q Ty - 1, their product one, green's sum one more: D = sum(v w (1 + t')), |t'| <= g(Tx + Ty).  All
 *     terms are positive, so N / D = c (1 + t) / (1 + t') with one more rounding for the division: at most 2*(Tx + Ty) + 2
 *     roundings in all, and the product of that many factors (1 + d)^(+-1), |d| <= u, lies within g(n) of 1 (Higham, Accuracy and
 *     Stability of Numerical Algorithms, Lemma 3.1).  To first order that is 2*(Tx + Ty + 1) * 2^-24.  A TDK_F16 store adds its
 *     own rounding, 2^-11.
 *   - Fused equals unfused.  tdk_decode12_demosaic_scaled equals tdk_decode12_f32 (scaled) followed by tdk_demosaic_scaled bit
 *     for bit; a call with gains equals tdk_apply_white_balance followed by the call without gains bit for bit.
 * No mirror identity is claimed: a mirrored frame is summed in the opposite order.
 *
 * Limits: mosaic sizes 2..65535 per axis, odd sizes included (the packed form needs an even width: pixel pairs share three bytes);
 * outputs at least 1 x 1; the ratio at least 2 and at most 16 on each axis; src and dst must not overlap; buffers are contiguous at
 * any element alignment (rows that start on 16 bytes are read as 16-byte segments, others element by element: the same bits).
 */
#ifndef TDK_HIP_SCALED_H
#define TDK_HIP_SCALED_H

#include <stddef.h>
#include <stdint.h>

#include "tdk_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TDK_SCALED_ABI_VERSION 1

/* the smallest and the largest ratio n_in / n_out on an axis, and the most taps of an output along one */
#define TDK_SCALED_MIN_RATIO 2
#define TDK_SCALED_MAX_RATIO 16
#define TDK_SCALED_MAX_TAPS 32

int tdk_scaled_abi_version(void);

/* LDS bytes one workgroup takes (static, the same for every geometry and instantiation: the output tile is sized from the ratio
 * to fit it); at most 80 KB, so that two workgroups share a CU.  Host query; 0 for sizes the stage would reject. */
size_t tdk_demosaic_scaled_lds_bytes(int width, int height, int out_width, int out_height);

/* The output tile (columns, rows) of one workgroup for this geometry.  Host query; TDK_OK, or an invalid-argument status for sizes
 * the stage would reject. */
int tdk_demosaic_scaled_tile(int width, int height, int out_width, int out_height, int* tile_width, int* tile_height);

/* ---- The stage (csrc/scaled_demosaic.hip).  One launch of one kernel; no workspace, no allocation, no copy, no memset, no
 * atomics, no synchronisation; every parameter travels as a kernel argument and the weights are computed in the kernel from
 * integers -- capturable in a graph from the first call, and deterministic.  gains may be NULL.  Argument errors (null pointers,
 * sizes, the ratio, the pattern, the dtypes, overlap) are reported before any HIP call. */
int tdk_demosaic_scaled(const void* src, void* dst, const float* gains, int width, int height, int out_width, int out_height, uint32_t pattern,
                        int src_dtype, int dst_dtype, tdk_stream_t stream);

/* The same from the packed 12-bit bytes of the mosaic (width * height * 3 / 2 of them; ids_format: the nibble order of
 * tdk_decode12_f32); width must be even. */
int tdk_decode12_demosaic_scaled(const uint8_t* packed, void* dst, const float* gains, int width, int height, int out_width, int out_height,
                                 uint32_t pattern, int ids_format, int dst_dtype, tdk_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
