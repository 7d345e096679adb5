/*
 * tdk_hip_ca.h -- lateral chromatic aberration on raw Bayer mosaics (libtdk_hip.so): the lens magnifies red and blue a little
 * differently from green, so that towards the corners the colour planes are 0.5 to 3 sites apart.  tdk_ca_correct resamples the red and
 * the blue plane of a mosaic by a radial model, in front of the demosaic (which reads misaligned planes as edges and mixes the damage
 * into all three channels); tdk_ca_estimate fits the model to frames of the camera.  The reference has no counterpart.
 *
 * include/tdk_hip.h (the reference's surface) and the other tdk_hip_*.h headers stay pinned; both entry points are declared here, with
 * their own version number.  The conventions of tdk_hip.h apply: device pointers, a HIP stream per call, TDK_OK or a tdk_status code
 * with the message in tdk_last_error(), nothing allocates device memory.
 *
 * ---- The model.  8 device floats, rows red and blue, columns v, c, b, valid.  Host parameters, each a float32: the optical centre
 * (x0, y0) in site coordinates (site centres are integers) and the normalisation radius rn > 0.  For colour k the sample that belongs
 * at site p is found in the captured plane at
 *   q = c0 + (p - c0) * s_k(rho),   rho = |p - c0| / rn,   s_k = v + c*rho + b*rho^2
 * -- the form and the direction of lensfun's poly3 TCA model (the captured radius as a function of the ideal one): coefficients of a
 * lens database can be used with their own rn.  A row with valid == 0 is the identity.  Site (i, j) has the CFA position
 * p = 2*(i & 1) + (j & 1) and the colour k = (pattern >> (2*p)) & 3 (0 red, 1 green, 2 blue), as everywhere in tdk_hip.h.
 *
 * ---- Specification of tdk_ca_correct.  Per-value arithmetic is float32, one rounding per written operation, no contraction (no FMA),
 * correctly rounded division and sqrtf.  Input: an (height, width) mosaic, float32 or float16 (converted exactly), width and height
 * even, 2..65535, contiguous at any element alignment.  Output float32 or float16, rounded once; it shares nothing with the input.
 *
 * A green site, and a red or blue site whose row has valid == 0: out = the input sample.
 * A red or blue site (i, j) with the row (v, c, b):
 *   px = (float)j - x0;   py = (float)i - y0
 *   r2 = px*px + py*py;   rho = sqrtf(r2) / rn
 *   s = (b*rho + c)*rho + v;   t = s - 1.0f
 *   dx = px*t;   dy = py*t                                      (d = q - p, in sites)
 *   if dx or dy is not finite: dx = dy = 0
 *   dx = fminf(fmaxf(dx, -D), D), likewise dy,  D = TDK_CA_MAX_SHIFT = 8
 *   if dx == 0 and dy == 0: out = the input sample             (the identity returns the input's bits, NaNs included)
 * Otherwise the site's own colour plane, a lattice of spacing 2 with (width/2) x (height/2) samples, is interpolated; the site is plane
 * sample (j >> 1, i >> 1):
 *   u = (float)(j >> 1) + dx*0.5f;   x0f = floorf(u);   ax = u - x0f;   ix = (int)x0f          (likewise w, y0f, ay, iy from i and dy)
 * interp = 0 (bilinear): taps ix, ix+1 with weights 1.0f - ax, ax; interp = 1 (bicubic): taps ix-1 .. ix+2 with weights c2(ax + 1),
 * c1(ax), c1(1 - ax), c2(2 - ax) -- the weight formulas and the summation order of tdk_hip_warp.h: a row is
 * ((s0*w0 + s1*w1) + s2*w2) + s3*w3 left to right (bilinear: the first two terms), the rows combine top to bottom with the y weights in
 * the same shape.  Plane tap indices are clamped into the plane (the edge is replicated).  A NaN or an infinity among the taps spreads
 * as the arithmetic says, also through a zero weight.
 *
 * Why D is fixed.  The model lives on the device (an estimate earlier on the stream feeds a captured correction), so the host cannot
 * size a source box per tile.  With a fixed D every tile's source box is the tile plus a constant apron -- D plus the taps of the
 * interpolation, rounded up to whole 16-byte units of float32: 8 sites left and above, 12 right and below for bilinear (taps j-8 .. j+10),
 * 12 on every side for bicubic (taps j-10 .. j+12).  One staged LDS path serves every tile and there is no global-gather fall-back.
 * Eight sites is more than twice what a poor lens shows at 50 MP (about 3 sites at the corner).
 *
 * Tile shape.  A workgroup of 256 lanes owns TDK_CA_TILE_H = 32 rows of TDK_CA_TILE_W = 64 sites and stages its box as float32 rows of
 * 84 (bilinear) or 88 (bicubic) words, by 16-byte reads of float32 (8-byte reads of float16) where the address allows and per element
 * elsewhere.  A lane owns pairs of one red or blue site and the green site next to it in the row.  A 32-lane half of a wave takes 16
 * pairs of a row and the 16 pairs below them: the red or blue sites of neighbouring rows sit at columns of opposite parity and the
 * row stride is 24 mod 32 words, so that under a displacement that varies slowly the 32 taps of a 4-byte LDS read fall on 32 banks.
 *
 * ---- Specification of tdk_ca_estimate.  F = 1..TDK_CA_MAX_FRAMES mosaics of one camera, all float32 or all float16.  frames is a HOST
 * array of F device pointers.  One gather launch per frame and one finishing launch; the workspace (tdk_ca_workspace_bytes) is owned by
 * the caller per stream and never has to be cleared: the launch of frame 0 writes every record, the later ones add to it, and a record
 * belongs to one workgroup.  No atomic on global memory, no memset, copy or synchronisation.
 *
 * 1. Per block sums -- integers, so the order of addition does not matter.  The frame is cut into blocks of block x block sites from
 * the origin; only complete blocks count (nbx = width / block, nby = height / block; block even, 16..256).  A sample is quantised as
 *   q(x) = (int)fminf(fmaxf(rintf(x * TDK_CA_QSCALE), 0.0f), TDK_CA_QMAX),   TDK_CA_QSCALE = 65535.0f,  TDK_CA_QMAX = 65535
 * With 256 x 256 / 4 sites of a colour per block, 16 frames, |G4| <= 4*QMAX the largest sum is below 2^54: every sum fits an int64 and a
 * float64 takes it with at most one rounding.  (A step of 1/65535 is far below the noise of any sensor; the purpose tests show nothing
 * of it.)  A site (i, j) of colour k in {red, blue} is used when it and its four green neighbours are inside the frame, finite
 * and < clip (1 <= i <= height-2, 1 <= j <= width-2); it belongs to the block its own position is in.  With gl, gr, gu, gd, C the
 * quantised neighbours (left, right, up, down) and the site itself:
 *   G4 = gl + gr + gu + gd;   gx2 = gr - gl;   gy2 = gd - gu
 * A record of (block, k) is TDK_CA_SUMS = 17 int64:  n, sum j, sum i, then the first moments of (G4, gx2, gy2, C) and their ten second
 * moments in the order G4*G4, G4*gx2, G4*gy2, G4*C, gx2*gx2, gx2*gy2, gx2*C, gy2*gy2, gy2*C, C*C.  Records are ordered
 * [block row][block column][k = red, blue] and start the workspace.
 *
 * 2. Per block fit, float64, one rounding per written operation, no contraction; s_a and m_ab are the first and second moments as
 * float64.  The centred moments c_ab = m_ab - (s_a*s_b)/n.  The regression C ~ kappa*Gbar + mx*Gx + my*Gy + const with Gbar = G4/4,
 * Gx = gx2/2, Gy = gy2/2 has the normal matrix and right-hand side
 *   N00 = c11/16  N01 = c12/8  N02 = c13/8  N11 = c22/4  N12 = c23/4  N22 = c33/4     r0 = c14/4  r1 = c24/2  r2 = c34/2
 * With a noise model (tdk_hip_noise.h; row 1, green, valid != 0) the energy that noise puts into the regressors is removed --
 * errors-in-variables with a known variance: nv = (QSCALE*QSCALE) * ((a*((s1/4)/QSCALE)) + b*n), the summed predicted variance of one
 * green sample in quantised units, then N00 -= nv/4, N11 -= nv/2, N22 -= nv/2.  Without it the shift comes out too small by a factor
 * of three on noisy frames.  Cofactors and determinant:
 *   C00 = N11*N22 - N12*N12   C01 = N02*N12 - N01*N22   C02 = N01*N12 - N02*N11
 *   C11 = N00*N22 - N02*N02   C12 = N01*N02 - N00*N12   C22 = N00*N11 - N01*N01
 *   det = (N00*C00 + N01*C01) + N02*C02
 *   kappa = ((C00*r0 + C01*r1) + C02*r2) / det;   mx = ((C01*r0 + C11*r1) + C12*r2) / det;   my = ((C02*r0 + C12*r1) + C22*r2) / det
 *   dx = mx / kappa;   dy = my / kappa;   wx = det / C11;   wy = det / C22       (the reciprocals of the diagonal of N^-1)
 * A block is dropped unless n >= TDK_CA_MIN_SITES = 16 (the minimum-information rule: fewer sites do not determine four parameters
 * with any margin), N00, N11, N22 > 0, det > 0, C11 > 0, C22 > 0, kappa > 0, |dx| <= max_shift and |dy| <= max_shift (every
 * comparison false for a NaN).
 *
 * 3. Global fit per colour, float64.  Sign and order: captured(x) = ideal(x - d) to first order, so the regression finds
 * (dx, dy) = -(q - p), measured at q: each kept block gives -dx = cx*t(rho) and -dy = cy*t(rho) with t = (v-1) + c*rho + b*rho^2,
 * (cx, cy) = (sum j / n - x0, sum i / n - y0) and rho = sqrt(cx*cx + cy*cy) / rn.  The fit is exact to first order in s - 1; the
 * remainder is d^2 / radius, below 0.01 site, and refine() of the Python front-end removes it.  With phi = (1, rho, rho*rho),
 *   g = (wx*cx)*cx + (wy*cy)*cy;   h = -((wx*cx)*dx + (wy*cy)*dy)
 *   A_ab += (g*phi_a)*phi_b  (a <= b);   r_a += h*phi_a        (phi_0 = 1.0 is multiplied like the others)
 * each of the nine sums from 0.0 over the kept blocks in ascending block order.  fit = TDK_CA_LINEAR: e = r_0 / A_00 needs A_00 > 0 and
 * one kept block; fit = TDK_CA_POLY3: (e, c, b) solves the 3 x 3 system by the cofactor formulas above (A for N, r for r), needs three
 * kept blocks and det > 0.  The row is (float)(1.0 + e), (float)c, (float)b, 1; when the system is singular or a result is not finite
 * -- a flat frame, a frame clipped everywhere, a frame too small for any block -- it is (1, 0, 0, 0).
 *
 * Decisions the issue left open.  The quantisation, the tile shape and the minimum-information rule are above.  Partial blocks at the
 * right and bottom edge are left out.  A non-finite displacement zeroes both components.  The valid fields are tested against 0 and
 * nothing else of either model is checked on the device.  The centre is not estimated.  Every address is formed from in-frame
 * coordinates only, and a tap index is clamped into the staged box whatever the model holds.
 */
#ifndef TDK_HIP_CA_H
#define TDK_HIP_CA_H

#include <stddef.h>

#include "tdk_hip.h"
#include "tdk_hip_noise.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TDK_CA_ABI_VERSION 1

#define TDK_CA_MAX_SHIFT 8    /* D: the largest displacement per axis, in sites */
#define TDK_CA_TILE_W 64      /* the output tile of a workgroup of tdk_ca_correct */
#define TDK_CA_TILE_H 32
#define TDK_CA_BILINEAR 0     /* interp of tdk_ca_correct */
#define TDK_CA_BICUBIC 1
#define TDK_CA_LINEAR 0       /* fit of tdk_ca_estimate */
#define TDK_CA_POLY3 1
#define TDK_CA_MAX_FRAMES 16
#define TDK_CA_QSCALE 65535.0f
#define TDK_CA_QMAX 65535
#define TDK_CA_SUMS 17        /* int64 per (block, colour) */
#define TDK_CA_MIN_SITES 16

int tdk_ca_abi_version(void);

/* Static LDS bytes of a workgroup of tdk_ca_correct: the staged box as float32, (32 + 20) x (64 + 20) words for bilinear,
 * (32 + 24) x (64 + 24) for bicubic, whatever the storage type.  0 for arguments tdk_ca_correct would reject. */
size_t tdk_ca_lds_bytes(int interp, int src_dtype);

/* Exactly one launch on `stream`: no workspace, no allocation, copy, memset, synchronisation or atomic: capturable in a graph from the
 * first call, bit-reproducible.  model: 8 device floats, read by every call.  Argument errors (null pointers, dtype tags, sizes,
 * pattern, interp, the centre, rn, overlap of out with src or model) are reported before any HIP call. */
int tdk_ca_correct(const void* src, int src_dtype, void* out, int out_dtype, int width, int height, uint32_t pattern, const float* model, float x0,
                   float y0, float rn, int interp, tdk_stream_t stream);

/* Bytes of the workspace of tdk_ca_estimate: the records of step 1.  0 for arguments tdk_ca_estimate would reject; at least 16. */
size_t tdk_ca_workspace_bytes(int width, int height, int block);

/* num_frames gather launches and one finishing launch on `stream`.  noise_model: the 12 device floats of tdk_hip_noise.h or NULL.
 * model: 8 device floats, written.  Argument errors (null pointers, num_frames, dtype tag, sizes, pattern, fit, clip, block, max_shift,
 * the centre, rn, overlap of workspace or model with the frames and with each other) are reported before any HIP call. */
int tdk_ca_estimate(const void* const* frames, int num_frames, int src_dtype, int width, int height, uint32_t pattern, const float* noise_model, int fit,
                    float clip, int block, float max_shift, float x0, float y0, float rn, void* workspace, float* model, tdk_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
