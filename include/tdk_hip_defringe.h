/*
 * tdk_hip_defringe.h -- purple-fringe removal of libtdk_hip.so on demosaiced frames: the rule of darktable's "defringe" module with a
 * frame-wide threshold, which the reference does not have.
 *
 * The other headers under include/ stay pinned; this stage is declared here, with its own version number.  The conventions of
 * tdk_hip.h apply: device pointers, a HIP stream per call, TDK_OK or a tdk_status code with the message in tdk_last_error(),
 * nothing allocates device memory.
 *
 * A lens focuses red and blue a little in front of or behind green.  Next to a clipped highlight the defocused channels spill over
 * dark structure as a purple or blue halo a few pixels wide.  No radial model removes it (tdk_ca_correct shifts channels, it does
 * not refocus them).  The halo is chroma that a blur of the chroma planes does not have: the squared distance between a pixel's
 * chroma and the blurred chroma, its "edge chroma" E, is large there.  A pixel whose E exceeds a threshold derived from the frame's
 * average E gets the average chroma of its neighbourhood, each neighbour weighted by the inverse of its own E, so that fringed
 * neighbours count for little.  Lightness is kept.
 *
 * ---- Specification.  All arithmetic is float32, one rounding per written operation, no contraction (no FMA); parentheses and the
 * stated order give the order of operations; divisions and sqrtf are correctly rounded.  An index outside the frame is clamped to
 * the frame's edge (replicate), everywhere.  Inputs are finite.
 *
 * The frame is (height, width, 3), interleaved, dtype TDK_F32 or TDK_F16, the same on both sides.  x_c is the sample of channel c
 * converted to float32 (exact).
 *
 * Working values:
 *   p(v) = v > 0 ? v : +0
 *   t_c = sqrtf(p(x_c))                    the default, the square-root domain
 *   t_c = p(x_c)                           with TDK_DEFRINGE_LINEAR
 *   Y  = (0.25f*t_r + 0.5f*t_g) + 0.25f*t_b
 *   Cb = t_b - t_g
 *   Cr = t_r - t_g
 * (the space of tdk_hip_wavelet.h).
 *
 * Edge chroma: symmetric taps w[0..R], 1 <= R <= 12, given by the caller as R + 1 float32 values.  The blur G(s) is the one of
 * tdk_sharpen and tdk_deconv:
 *   horizontal   h = w[0]*s[0];   for k = 1..R in ascending order:   h = h + w[k]*(s[-k] + s[+k])
 *   vertical     the same formula applied to h along the other axis gives G(s)
 * The intermediate h stays float32.
 *   db = Cb - G(Cb)
 *   dr = Cr - G(Cr)
 *   E  = db*db + dr*dr
 *
 * Frame statistic: every pixel contributes
 *   q = (unsigned long long)floorf(fminf(E, 1024.0f) * 1048576.0f)
 * S is the 64-bit integer sum of q over all pixels (order-free), N = width*height, and
 *   avg = (float)((double)S / ((double)N * 1048576.0))
 * (S converted to double with one rounding, the product is exact, one double division, one rounding to float32).
 *
 * Threshold:
 *   th = fmaxf(floor, strength * avg)      TDK_DEFRINGE_GLOBAL, the default
 *   th = fmaxf(floor, strength)            TDK_DEFRINGE_STATIC
 * floor is finite and > 0, strength finite and >= 0.
 *
 * Correction: a pixel with E > th is fringed.  The samples are all integer offsets (dy, dx) with dx*dx + dy*dy <= S_r*S_r,
 * 1 <= S_r <= 8, visited with dy ascending, then dx ascending; the centre is included; the position is clamped.  The weight of
 * sample s is
 *   wt_s = 1.0f / (E_s + th)
 * Starting from a = b = n = 0, in visiting order:
 *   a = a + wt_s*Cb_s
 *   b = b + wt_s*Cr_s
 *   n = n + wt_s
 * Then
 *   Cb' = a / n
 *   Cr' = b / n
 *   g'  = Y - 0.25f*(Cb' + Cr')
 *   r'  = g' + Cr'
 *   b'  = g' + Cb'
 *   v_c = fmaxf(c', 0)
 *   out_c = v_c*v_c                        in the square-root domain (the product is a float32 value)
 *   out_c = v_c                            with TDK_DEFRINGE_LINEAR
 * Store: float32 as it is; binary16 is rounded once, at the store, to nearest even.
 * A pixel that is not fringed stores x_c itself: the input's bits come back, -0 and negative values included.
 *
 * Optional outputs, each may be null: mask_out, a byte per pixel, 1 where fringed and 0 elsewhere; edge_out, a float32
 * (height, width) plane that receives E; stats_out, a tdk_defringe_stats record that receives S and th.
 *
 * Identities:
 *   - a flat grey frame has E == 0 exactly; a flat coloured one has E = (C - G(C))^2 per plane, the square of the rounding error of
 *     the taps' sum (below 1e-9 for the taps of tdk_defringe_weights and samples up to 64), S == 0 and th == floor: a flat frame
 *     returns its bits for every floor above that, whatever the mode;
 *   - TDK_DEFRINGE_STATIC with a strength >= every E returns the input's bits;
 *   - the result depends neither on the tile size, nor on a tile's position, nor on the number of workgroups that gather S.
 * No mirror identity is claimed: a mirrored frame visits a fringed pixel's samples in the opposite order, and float32 sums in
 * another order are other sums.  E, the mask, S and th of a mirrored frame ARE the mirrored ones (the blur pairs its taps and
 * float32 addition commutes); only the corrected samples may differ.
 *
 * Not part of this stage: an estimate of the per-channel defocus (longitudinal aberration as such), a gate on hue, and darktable's
 * local-average threshold.
 *
 * Limits: sizes 1..65535 per axis; src, dst, the optional outputs and the workspace must not overlap; buffers are contiguous at any
 * element alignment (edge_out at 4 bytes, stats_out at 8).
 */
#ifndef TDK_HIP_DEFRINGE_H
#define TDK_HIP_DEFRINGE_H

#include <stddef.h>
#include <stdint.h>

#include "tdk_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TDK_DEFRINGE_ABI_VERSION 1

/* flags of tdk_defringe: the domain, the mode, and in bits 8..18 a cap on the workgroups of the first launch */
#define TDK_DEFRINGE_GLOBAL 0
#define TDK_DEFRINGE_LINEAR 1
#define TDK_DEFRINGE_STATIC 2
/* bits 8..18 of flags: the largest number of workgroups that gather the statistic, 1..TDK_DEFRINGE_MAX_GROUPS, 0 for
 * TDK_DEFRINGE_MAX_GROUPS.  For tests and measurements: every cap gives the same bits.  The other bits are reserved and must be 0. */
#define TDK_DEFRINGE_GROUPS_SHIFT 8
#define TDK_DEFRINGE_GROUPS_MASK 524032

#define TDK_DEFRINGE_MAX_RADIUS 12
#define TDK_DEFRINGE_MAX_SAMPLE_RADIUS 8
#define TDK_DEFRINGE_MAX_GROUPS 1024
/* the output tile of one workgroup of either launch, in pixels */
#define TDK_DEFRINGE_TILE 32
/* the scale and the cap of a pixel's contribution to S */
#define TDK_DEFRINGE_STAT_SCALE 1048576
#define TDK_DEFRINGE_STAT_CAP 1024

/* stats_out: the frame statistic and the threshold the call used */
typedef struct tdk_defringe_stats {
  uint64_t sum;     /* S */
  float threshold;  /* th */
  uint32_t reserved; /* written as 0 */
} tdk_defringe_stats;

int tdk_defringe_abi_version(void);

/* Gaussian taps for tdk_defringe.  Host only.  sigma in [0.5, 4];  R = ceil(3*sigma), formed in double from the float32 value of
 * sigma (so 2 <= R <= 12);  w_k = exp(-k*k / (2*sigma*sigma)) / (w_0 + 2 * sum_{k >= 1} w_k), computed in double, summed in
 * ascending k, and rounded once to float32: the rule of tdk_sharpen_weights.  weights receives TDK_DEFRINGE_MAX_RADIUS + 1 values,
 * those beyond R are 0. */
int tdk_defringe_weights(float sigma, float* weights /* 13 */, int* radius);

/* Bytes of device workspace a call needs: the float32 plane of E, TDK_DEFRINGE_MAX_GROUPS partial sums of 64 bits, and what
 * aligning them takes.  Every value the second launch reads was written by the first launch of the same call: nothing needs
 * zeroing.  Host query; 0 for a size tdk_defringe would reject. */
size_t tdk_defringe_workspace_bytes(int width, int height);

/* LDS bytes one workgroup takes, the larger of the two launches (the first: Cb and Cr over the tile and its apron of
 * TDK_DEFRINGE_MAX_RADIUS, and their row-blurred planes); static, at most 64 KB.  Host query; 0 for arguments tdk_defringe would
 * reject. */
size_t tdk_defringe_lds_bytes(int dtype, int radius, int sample_radius, int flags);

/* ---- The stage (csrc/defringe.hip).  Two launches: "edge" writes E and one partial sum per workgroup, "correct" sums the partial
 * sums, forms th and rewrites the fringed pixels.  No allocation, no copy, no memset, no atomics, no synchronisation -- capturable
 * in a graph from the first call, and deterministic.  weights is a HOST pointer to radius + 1 floats, read during the call.
 * workspace: tdk_defringe_workspace_bytes bytes of device memory at any alignment, owned by the call until its second launch has
 * finished (one workspace per stream).  With TDK_DEFRINGE_STATIC the second launch takes th from the arguments and reads the
 * partial sums only to fill stats_out.  Argument errors (null pointers, sizes, dtype, radius, taps, sample radius, strength, floor,
 * flags, alignment of edge_out and stats_out, overlap) are reported before any HIP call. */
int tdk_defringe(const void* src, void* dst, unsigned char* mask_out, float* edge_out, tdk_defringe_stats* stats_out, void* workspace, int width, int height,
                 int dtype, const float* weights, int radius, int sample_radius, float strength, float floor, int flags, tdk_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
