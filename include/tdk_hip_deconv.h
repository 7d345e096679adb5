/*
 * tdk_hip_deconv.h -- capture sharpening of libtdk_hip.so: Richardson-Lucy deconvolution of the luminance with a small symmetric
 * PSF and a contrast mask, which the reference does not have.
 *
 * The other headers under include/ stay pinned; the deconvolution is declared here, with its own version number.  The conventions
 * of tdk_hip.h apply: device pointers, a HIP stream per call, TDK_OK or a tdk_status code with the message in tdk_last_error(),
 * nothing allocates device memory.
 *
 * Lens, anti-alias filter and demosaic leave a blur that is roughly a small Gaussian.  Richardson-Lucy (Richardson 1972, Lucy
 * 1974) estimates the frame u whose blur G(u) is the observed frame o by the multiplicative update u <- u * G(o / G(u)); a few
 * iterations on the luminance of the linear frame, held back by a mask where the frame holds nothing but noise, are what raw
 * developers call capture sharpening.  The channels are scaled by the ratio of the new luminance to the old one, so hue stays.
 *
 * ---- Specification.  All arithmetic is float32, one rounding per written operation, no contraction (no FMA); parentheses and the
 * stated order give the order of operations; divisions and sqrtf are correctly rounded.  An index outside the frame is clamped to
 * the frame's edge (replicate), everywhere and in every iteration.  Inputs are finite.
 *
 * The frame is (height, width, channels), interleaved, channels 1 or 3, dtype TDK_F32 or TDK_F16, the same on both sides.  x_c is
 * the sample of channel c converted to float32 (exact).
 *
 * Luminance:
 *   pos(v) = v > 0 ? v : +0
 *   Y = pos((l0*r + l1*g) + l2*b)          three channels; l = the three luma weights, finite and >= 0
 *   Y = pos(x)                             one channel
 *   o = fmaxf(Y, TINY)                     TINY = 2^-20
 *
 * PSF: symmetric taps w[0..R], 1 <= R <= 6, given by the caller as R + 1 float32 values.  The blur G(s) is the one of tdk_sharpen:
 *   horizontal   h = w[0]*s[0];   for k = 1..R in ascending order:   h = h + w[k]*(s[-k] + s[+k])
 *   vertical     the same formula applied to h along the other axis gives G(s)
 * The intermediate h stays float32.
 *
 * Iteration: u_0 = o.  For k = 1..N, N = iterations in 0..50:
 *   b   = G(u_{k-1})
 *   q   = o / fmaxf(b, TINY)
 *   c   = G(q)
 *   u_k = u_{k-1} * c
 * u_k and q are defined on the frame's pixels only: a tap outside the frame reads the value at the clamped index of the same
 * iteration.
 *
 * Contrast mask (TDK_DECONV_MASK; without it m = 1):  hi and lo are the maximum and minimum of o over the 3x3 neighbourhood.
 *   d  = sqrtf(hi) - sqrtf(lo)             (the square root makes shot noise roughly uniform over brightness)
 *   t  = threshold > 0
 *   it = 1 / t                             (formed on the host, in float32)
 *   e  = fminf(fmaxf((d - t) * it, 0), 1)
 *   m  = (e*e) * (3 - 2*e)
 *
 * Result:
 *   Yn = o + m*(u_N - o)
 *   g  = fminf(fmaxf(Yn / o, 1 / G), G)    G = max_gain in [1, 16]; 1 / G is formed on the host, in float32
 *   out_c = x_c * g                        not clamped
 * Store: float32 as it is; binary16 rounded to nearest even.  N == 0 stores x_c itself: the input's bits come back (-0 included).
 * m == 0 gives Yn = o, g = 1 and the input's bits as well.  mask_out, a float32 (height, width) plane, receives m.
 *
 * Limits: sizes 1..65535 per axis; threshold finite and > 0 (read only with TDK_DECONV_MASK); src, dst, mask_out and the workspace
 * must not overlap; buffers are contiguous at any element alignment (mask_out at 4 bytes).
 */
#ifndef TDK_HIP_DECONV_H
#define TDK_HIP_DECONV_H

#include <stddef.h>

#include "tdk_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TDK_DECONV_ABI_VERSION 1

/* flags of tdk_deconv */
#define TDK_DECONV_MASK 1
/* bits 8..11 of flags: the number F of iterations fused per launch, 0 for the library's choice (tdk_deconv_fused_iterations).  A
 * forced F must be one that was built (1, 2 or 4) and must take the radius: R <= 6, 4 and 2.  For tests and measurements: every F
 * gives the same bits. */
#define TDK_DECONV_FUSE_SHIFT 8
#define TDK_DECONV_FUSE_MASK 3840

#define TDK_DECONV_MAX_RADIUS 6
#define TDK_DECONV_MAX_ITERATIONS 50
#define TDK_DECONV_MAX_FUSED 4
/* the output tile of one workgroup, in pixels */
#define TDK_DECONV_TILE 32

int tdk_deconv_abi_version(void);

/* Gaussian taps for tdk_deconv.  Host only.  sigma in [0.3, 2];  R = ceil(3*sigma), formed in double from the float32 value of
 * sigma (so 1 <= R <= 6);  w_k = exp(-k*k / (2*sigma*sigma)) / (w_0 + 2 * sum_{k >= 1} w_k), computed in double, summed in
 * ascending k, and rounded once to float32: the rule of tdk_sharpen_weights.  weights receives TDK_DECONV_MAX_RADIUS + 1 values,
 * those beyond R are 0. */
int tdk_deconv_weights(float sigma, float* weights /* 7 */, int* radius);

/* The number F of iterations one launch of tdk_deconv fuses at this radius when flags forces none; a call of N iterations takes
 * ceil(N / F) launches (one for N == 0).  Host query; 0 for a radius tdk_deconv would reject. */
int tdk_deconv_fused_iterations(int radius);

/* Bytes of device workspace a call needs: the float32 planes u travels in between the launches (none for one launch, one for two,
 * two for more: a launch reads the plane the one before it wrote), plus what aligning them takes.  0 when the whole call is one
 * launch; workspace may then be null.  Every value a launch reads was written by the launch before it: nothing needs zeroing.  A
 * call that forces F needs at most tdk_deconv_workspace_bytes(width, height, TDK_DECONV_MAX_RADIUS, TDK_DECONV_MAX_ITERATIONS).
 * Host query; 0 for arguments tdk_deconv would reject. */
size_t tdk_deconv_workspace_bytes(int width, int height, int radius, int iterations);

/* LDS bytes one workgroup of tdk_deconv takes (u, o, the horizontally blurred plane and q, of the tile with its apron of 2*R*F
 * pixels at the largest radius the instantiation takes); static, at most 64 KB.  Host query; 0 for arguments tdk_deconv would
 * reject. */
size_t tdk_deconv_lds_bytes(int channels, int dtype, int radius, int flags);

/* ---- The stage (csrc/deconv.hip).  ceil(N / F) launches of one kernel; no allocation, no copy, no memset, no atomics, no
 * synchronisation -- capturable in a graph from the first call, and deterministic.  weights is a HOST pointer to radius + 1 floats
 * and luma a HOST pointer to three, both read during the call.  workspace: tdk_deconv_workspace_bytes bytes of device memory at
 * any alignment, owned by the call until its last launch has finished (one workspace per stream).  mask_out may be null.  Argument
 * errors (null pointers, sizes, channels, dtype, radius, weights, iterations, threshold, max_gain, luma, flags, alignment of
 * mask_out, overlap) are reported before any HIP call. */
int tdk_deconv(const void* src, void* dst, float* mask_out, void* workspace, int width, int height, int channels, int dtype, const float* weights,
               int radius, int iterations, float threshold, float max_gain, const float* luma /* host, 3 */, int flags, tdk_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
