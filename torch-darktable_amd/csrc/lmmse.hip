// lmmse.hip -- the demosaic for noisy frames: directional linear minimum mean-square-error estimation of green minus the other colour
// (include/tdk_hip_lmmse.h: tdk_lmmse), one launch of one kernel.
//
// The specification is the head comment of include/tdk_hip_lmmse.h.
//
// A workgroup of four waves owns LM_TW x LM_TH = 32 x 32 pixels.  A stored site reads D at +-1, D reads p and d at +-4 along one axis,
// p reads d at +-4 more and d reads t at +-2: the horizontal chain runs over the tile's rows +-1 and its columns +-11, the vertical one
// over its columns +-1 and its rows +-11 -- a cross, not a square.  Six float32 planes in static LDS (39 000 bytes: four workgroups
// per CU), each at the pitch of its own region, so that every pass is one loop over consecutive words (consecutive lanes,
// consecutive banks: the vertical taps of a wave lie in rows of consecutive words as well and conflict no more than the horizontal
// ones).  With (x0, y0) the tile's first pixel:
//   t    rows [-11, 43)  columns [-11, 43)   54 x 54   only the cross is staged: rows [-1, 33) whole, columns [-1, 33) whole
//   dh   rows [ -1, 33)  columns [ -9, 41)   34 x 50   the horizontal estimate of green minus the row's other colour
//   dv   rows [ -9, 41)  columns [ -1, 33)   50 x 34   the vertical one
//   ph   rows [ -1, 33)  columns [ -5, 37)   34 x 42   dh low-passed along the row
//   pv   rows [ -5, 37)  columns [ -1, 33)   42 x 34   dv low-passed along the column
//   D    rows [ -1, 33)  columns [ -1, 33)   34 x 17   the fused difference at the red and blue sites, which are every other site of a
//                                                      row: site (r, c) lies at r * 17 + c / 2
// Staging alone knows about the frame's edges: a staged position holds t of the FOLDED pixel (reflection about the edge sample, as
// often as it takes).  The extension is then symmetric about every edge, reflection keeps the CFA colour, every formula pairs its
// taps (a[-k] + a[+k]) and float32 addition commutes: a plane evaluated at a reflected position from those operands has the bits of
// its value at the folded index, which is the specification's rule.  So the four passes behind staging have no guard at all, and a
// tile inside the frame differs from one on its edge in the staging loop only (it folds nothing).
//   1. t                    the cross, four positions per thread and round in flight
//   2. dh, dv               from t
//   3. ph, pv               from dh, dv
//   4. D                    the red and blue sites of the 34 x 34 region (17 per row), both directions and the fusion per thread
//   5. the tile             four adjacent pixels per thread; whole vectors where the frame has whole groups and dst is aligned
// with a barrier behind 1 to 4.  No pixel's arithmetic depends on the tile, nothing is accumulated across lanes: deterministic.
#include <math.h>

#include "../../include/tdk_hip_lmmse.h"
#include "tdk_frame.h"

namespace {

constexpr int LM_THREADS = 256;
constexpr int LM_TW = TDK_LMMSE_TILE_W, LM_TH = TDK_LMMSE_TILE_H, LM_A = TDK_LMMSE_APRON;
constexpr int LM_PIX = 4, LM_GROUPS = LM_TW / LM_PIX;   // 8 threads per tile row, 32 rows
static_assert(LM_THREADS == LM_GROUPS * LM_TH, "a thread per 4 pixels of the tile");
static_assert(LM_A == 1 + 4 + 4 + 2, "D at +-1, p and d at +-4, d at +-4 of p, t at +-2 of d");

constexpr int LM_TR = LM_TH + 2 * LM_A, LM_TC = LM_TW + 2 * LM_A;      // t
constexpr int LM_DHR = LM_TH + 2, LM_DHC = LM_TW + 2 * 9;              // dh
constexpr int LM_DVR = LM_TH + 2 * 9, LM_DVC = LM_TW + 2;              // dv
constexpr int LM_PHR = LM_TH + 2, LM_PHC = LM_TW + 2 * 5;              // ph
constexpr int LM_PVR = LM_TH + 2 * 5, LM_PVC = LM_TW + 2;              // pv
constexpr int LM_DR = LM_TH + 2, LM_DC = LM_TW + 2;                    // D
constexpr int LM_SITES = LM_DC / 2;                                    // red and blue sites of a row of D
static_assert(LM_DC % 2 == 0, "every row of D holds as many red or blue sites as green ones");

struct LmLds {
  float t[LM_TR * LM_TC], dh[LM_DHR * LM_DHC], dv[LM_DVR * LM_DVC], ph[LM_PHR * LM_PHC], pv[LM_PVR * LM_PVC], D[LM_DR * LM_SITES];
};
static_assert(sizeof(LmLds) <= 40 * 1024, "four workgroups in the 160 KB of a CU");

constexpr int LM_STAGE = 4;   // positions a thread stages per round
constexpr float LM_G0 = 0x1.a22092p-3f, LM_G1 = 0x1.70fefap-3f, LM_G2 = 0x1.fb36c8p-4f, LM_G3 = 0x1.0f7df8p-4f, LM_G4 = 0x1.c4b2eep-6f;
constexpr float LM_NINTH = 0x1.c71c72p-4f, LM_EPS = 1e-7f;

enum : int { LM_VEC_OUT = 1, LM_GREEN_ODD = 2 };   // dst takes whole vectors of four pixels; green sites have an odd row + column

// reflection about the edge sample, folded until the index lies inside; n >= 2
__device__ __forceinline__ int lm_fold(int i, int n) {
  const int period = 2 * (n - 1);
  i = (i < 0 ? -i : i) % period;
  return i < n ? i : period - i;
}

// e = (0.5*(t[-1] + t[+1]) - 0.25*(t[-2] + t[+2])) + 0.5*t[0];  d = green ? t[0] - e : e - t[0]
__device__ __forceinline__ float lm_estimate(const float* __restrict__ q, int step, bool green) {
  const float e = (0.5f * (q[-step] + q[step]) - 0.25f * (q[-2 * step] + q[2 * step])) + 0.5f * q[0];
  return green ? q[0] - e : e - q[0];
}

__device__ __forceinline__ float lm_lowpass(const float* __restrict__ q, int step) {
  float p = LM_G0 * q[0];
  p = p + LM_G1 * (q[-step] + q[step]);
  p = p + LM_G2 * (q[-2 * step] + q[2 * step]);
  p = p + LM_G3 * (q[-3 * step] + q[3 * step]);
  p = p + LM_G4 * (q[-4 * step] + q[4 * step]);
  return p;
}

// S(a) = a[0], then + (a[-k] + a[+k]) for k = 1..4; a[4] is the centre
__device__ __forceinline__ float lm_window(const float a[9]) {
  float s = a[4];
#pragma unroll
  for (int k = 1; k <= 4; k++) s = s + (a[4 - k] + a[4 + k]);
  return s;
}

// the estimate x of one direction at a red or blue site and the variance v of its error; pp and dd point at the site
__device__ __forceinline__ void lm_direction(const float* __restrict__ pp, const float* __restrict__ dd, int step, float& x, float& v) {
  float p[9], d[9], a[9];
#pragma unroll
  for (int k = 0; k < 9; k++) p[k] = pp[(k - 4) * step], d[k] = dd[(k - 4) * step];
  const float mu = lm_window(p) * LM_NINTH;
#pragma unroll
  for (int k = 0; k < 9; k++) a[k] = (p[k] - mu) * (p[k] - mu);
  const float vx = LM_EPS + lm_window(a);
#pragma unroll
  for (int k = 0; k < 9; k++) a[k] = (d[k] - p[k]) * (d[k] - p[k]);
  const float vn = LM_EPS + lm_window(a);
  const float sum = vx + vn;
  x = (p[4] * vn + d[4] * vx) / sum;
  v = (vx * vn) / sum;
}

// an estimated value as it is stored: squared in the square-root domain
template <bool SQRT> __device__ __forceinline__ float lm_finish(float c) {
  if constexpr (SQRT) {
    const float q = fmaxf(c, 0.0f);
    return q * q;
  } else {
    return c;
  }
}

template <typename TI, typename TO, bool SQRT>
__global__ __launch_bounds__(LM_THREADS) void lmmse_kernel(const TI* __restrict__ src, TO* __restrict__ dst, int W, int H, uint32_t pattern, int bits) {
  __shared__ LmLds lds;
  const int tid = (int)threadIdx.x;
  const int x0 = (int)blockIdx.x * LM_TW, y0 = (int)blockIdx.y * LM_TH;
  const int gx0 = x0 - LM_A, gy0 = y0 - LM_A;
  const int gpar = (bits & LM_GREEN_ODD) ? 1 : 0;   // (row + column) & 1 of the green sites

  // ---- 1. t over the cross, of the folded pixel.  LM_STAGE positions of a thread are asked for before the first is looked at.
  {
    const bool inside = gx0 >= 0 && gy0 >= 0 && gx0 + LM_TC <= W && gy0 + LM_TR <= H;   // the same for the whole workgroup
    constexpr int N = LM_TR * LM_TC;
    for (int e0 = tid; e0 < N; e0 += LM_STAGE * LM_THREADS) {
      float m[LM_STAGE];
      bool take[LM_STAGE];
#pragma unroll
      for (int k = 0; k < LM_STAGE; k++) {
        const int e = e0 + k * LM_THREADS;
        const int ty = e / LM_TC, tx = e - ty * LM_TC;
        const bool row_band = ty >= LM_A - 1 && ty < LM_A + LM_TH + 1, col_band = tx >= LM_A - 1 && tx < LM_A + LM_TW + 1;
        take[k] = e < N && (row_band || col_band);
        int gy = gy0 + ty, gx = gx0 + tx;
        if (!inside) gy = lm_fold(gy, H), gx = lm_fold(gx, W);
        m[k] = take[k] ? ld(src, (size_t)gy * W + gx) : 0.0f;
      }
#pragma unroll
      for (int k = 0; k < LM_STAGE; k++)
        if (take[k]) lds.t[e0 + k * LM_THREADS] = SQRT ? sqrtf(fmaxf(m[k], 0.0f)) : m[k];
    }
  }
  __syncthreads();

  // ---- 2. the directional estimates.  dh(r, c) is the site (y0 - 1 + r, x0 - 9 + c), dv(r, c) the site (y0 - 9 + r, x0 - 1 + c);
  // y0 and x0 are even, so the colour of a site follows from r + c alone
  for (int e = tid; e < LM_DHR * LM_DHC; e += LM_THREADS) {
    const int r = e / LM_DHC, c = e - r * LM_DHC;
    lds.dh[e] = lm_estimate(lds.t + (r + LM_A - 1) * LM_TC + (c + 2), 1, ((r + c) & 1) == gpar);
  }
  for (int e = tid; e < LM_DVR * LM_DVC; e += LM_THREADS) {
    const int r = e / LM_DVC, c = e - r * LM_DVC;
    lds.dv[e] = lm_estimate(lds.t + (r + 2) * LM_TC + (c + LM_A - 1), LM_TC, ((r + c) & 1) == gpar);
  }
  __syncthreads();

  // ---- 3. their low pass.  ph(r, c) is the site (y0 - 1 + r, x0 - 5 + c), pv(r, c) the site (y0 - 5 + r, x0 - 1 + c)
  for (int e = tid; e < LM_PHR * LM_PHC; e += LM_THREADS) {
    const int r = e / LM_PHC, c = e - r * LM_PHC;
    lds.ph[e] = lm_lowpass(lds.dh + r * LM_DHC + (c + 4), 1);
  }
  for (int e = tid; e < LM_PVR * LM_PVC; e += LM_THREADS) {
    const int r = e / LM_PVC, c = e - r * LM_PVC;
    lds.pv[e] = lm_lowpass(lds.dv + (r + 4) * LM_DVC + c, LM_DVC);
  }
  __syncthreads();

  // ---- 4. D at the red and blue sites.  D(r, c) is the site (y0 - 1 + r, x0 - 1 + c): green where (r + c) & 1 == gpar
  for (int e = tid; e < LM_DR * LM_SITES; e += LM_THREADS) {
    const int r = e / LM_SITES, j = e - r * LM_SITES;
    const int c = 2 * j + ((r + gpar + 1) & 1);
    float xh, vh, xv, vv;
    lm_direction(lds.ph + r * LM_PHC + (c + 4), lds.dh + r * LM_DHC + (c + 8), 1, xh, vh);
    lm_direction(lds.pv + (r + 4) * LM_PVC + c, lds.dv + (r + 8) * LM_DVC + c, LM_DVC, xv, vv);
    lds.D[e] = (xh * vv + xv * vh) / (vh + vv);   // (e == r * LM_SITES + c / 2)
  }
  __syncthreads();

  // ---- 5. the tile: four adjacent pixels per thread
  const int tr = tid / LM_GROUPS, tc = (tid % LM_GROUPS) * LM_PIX;
  const int y = y0 + tr, x = x0 + tc;
  if (y >= H || x >= W) return;
  const size_t pix = (size_t)y * W + x;
  float out[3 * LM_PIX];
#pragma unroll
  for (int i = 0; i < LM_PIX; i++) {
    const int colour = cfa_color(y & 1, i & 1, pattern);   // (x is even)
    const float own = x + i < W ? ld(src, pix + i) : 0.0f;
    const float t = lds.t[(tr + LM_A) * LM_TC + tc + i + LM_A];
    const int dc = tc + i + 1;   // the pixel's column in D's region; its row is tr + 1
    const float *Dup = lds.D + tr * LM_SITES, *Dmid = Dup + LM_SITES, *Ddn = Dmid + LM_SITES;
    float r, g, b;
    if (colour == 1) {
      // the colour of the row's other sites from the horizontal neighbours, the remaining one from the vertical neighbours
      const float along = lm_finish<SQRT>(t - 0.5f * (Dmid[(dc - 1) >> 1] + Dmid[(dc + 1) >> 1])), across = lm_finish<SQRT>(t - 0.5f * (Dup[dc >> 1] + Ddn[dc >> 1]));
      const bool red_row = cfa_color(y & 1, (i + 1) & 1, pattern) == 0;
      r = red_row ? along : across, g = own, b = red_row ? across : along;
    } else {
      const float G = t + Dmid[dc >> 1];
      const float other = lm_finish<SQRT>(G - 0.25f * ((Dup[(dc - 1) >> 1] + Dup[(dc + 1) >> 1]) + (Ddn[(dc - 1) >> 1] + Ddn[(dc + 1) >> 1])));
      g = lm_finish<SQRT>(G);
      r = colour == 0 ? own : other, b = colour == 0 ? other : own;
    }
    out[3 * i] = r, out[3 * i + 1] = g, out[3 * i + 2] = b;
  }
  // An estimated value is a float32 value and a binary16 store rounds that: two roundings.  The empty asm keeps the value one of its
  // own, so that no instruction that computes and converts in one step (one rounding) can take its place.
  if constexpr (sizeof(TO) == 2) {
#pragma unroll
    for (int i = 0; i < 3 * LM_PIX; i++) asm volatile("" : "+v"(out[i]));
  }
  if (bits & LM_VEC_OUT) {
    rgb4_io<TO>::store(dst + pix * 3, 0, out);   // (width % 4 == 0 and dst on the vector's alignment: the host's check)
  } else {
#pragma unroll
    for (int i = 0; i < 3 * LM_PIX; i++)
      if (x + i / 3 < W) st(dst, pix * 3 + i, out[i]);
  }
}

bool lm_size_ok(int width, int height) {
  return width >= TDK_LMMSE_MIN_SIZE && height >= TDK_LMMSE_MIN_SIZE && width <= TDK_LMMSE_MAX_SIZE && height <= TDK_LMMSE_MAX_SIZE;
}
bool lm_pattern_ok(uint32_t p) { return p == TDK_PATTERN_RGGB || p == TDK_PATTERN_BGGR || p == TDK_PATTERN_GRBG || p == TDK_PATTERN_GBRG; }
bool lm_flags_ok(int flags) { return (flags & ~TDK_LMMSE_LINEAR) == 0; }

template <typename TI, typename TO, bool SQRT>
int lm_run(const void* src, void* dst, int width, int height, uint32_t pattern, int bits, hipStream_t st) {
  const dim3 grid((unsigned)tdk_div_up(width, LM_TW), (unsigned)tdk_div_up(height, LM_TH));
  TDK_LAUNCH("tdk_lmmse", (lmmse_kernel<TI, TO, SQRT>), grid, dim3(LM_THREADS), 0, st, reinterpret_cast<const TI*>(src), reinterpret_cast<TO*>(dst), width, height,
             pattern, bits);
  return TDK_OK;
}

template <typename TI, typename TO>
int lm_domain(bool linear, const void* src, void* dst, int width, int height, uint32_t pattern, int bits, hipStream_t st) {
  if (linear) return lm_run<TI, TO, false>(src, dst, width, height, pattern, bits, st);
  return lm_run<TI, TO, true>(src, dst, width, height, pattern, bits, st);
}

}  // namespace

TDK_EXPORT int tdk_lmmse_abi_version(void) { return TDK_LMMSE_ABI_VERSION; }

TDK_EXPORT size_t tdk_lmmse_lds_bytes(int src_dtype, int dst_dtype, int flags) {
  return tdk_float_dtype_ok(src_dtype) && tdk_float_dtype_ok(dst_dtype) && lm_flags_ok(flags) ? sizeof(LmLds) : 0;
}

TDK_EXPORT int tdk_lmmse(const void* src, void* dst, int width, int height, uint32_t pattern, int src_dtype, int dst_dtype, int flags, tdk_stream_t stream) {
  TDK_REQUIRE(src && dst, "tdk_lmmse: null pointer (src or dst)");
  TDK_REQUIRE(lm_size_ok(width, height), "tdk_lmmse: frame size %dx%d outside %d..%d", width, height, TDK_LMMSE_MIN_SIZE, TDK_LMMSE_MAX_SIZE);
  TDK_REQUIRE(lm_pattern_ok(pattern), "tdk_lmmse: pattern 0x%08x is none of the four Bayer patterns", (unsigned)pattern);
  TDK_REQUIRE(tdk_float_dtype_ok(src_dtype), "tdk_lmmse: unsupported dtype tag %d (src)", src_dtype);
  TDK_REQUIRE(tdk_float_dtype_ok(dst_dtype), "tdk_lmmse: unsupported dtype tag %d (dst)", dst_dtype);
  TDK_REQUIRE(lm_flags_ok(flags), "tdk_lmmse: flags must be 0 or TDK_LMMSE_LINEAR, the other bits are reserved, got %d", flags);
  const size_t n = (size_t)width * height, src_bytes = n * tdk_dtype_bytes(src_dtype), dst_bytes = 3 * n * tdk_dtype_bytes(dst_dtype);
  TDK_REQUIRE(tdk_disjoint(src, src_bytes, dst, dst_bytes), "tdk_lmmse: src and dst overlap (every output reads its neighbours)");

  int bits = cfa_color(0, 0, pattern) == 1 ? 0 : LM_GREEN_ODD;
  // a thread's four pixels as one vector: rows must hold whole groups and start on the vector's alignment
  if (tdk_vec4_ok(width, dst, 4 * tdk_dtype_bytes(dst_dtype))) bits |= LM_VEC_OUT;
  const bool linear = (flags & TDK_LMMSE_LINEAR) != 0;
  hipStream_t st = tdk_stream(stream);
  if (src_dtype == TDK_F32) {
    if (dst_dtype == TDK_F32) return lm_domain<float, float>(linear, src, dst, width, height, pattern, bits, st);
    return lm_domain<float, __half>(linear, src, dst, width, height, pattern, bits, st);
  }
  if (dst_dtype == TDK_F32) return lm_domain<__half, float>(linear, src, dst, width, height, pattern, bits, st);
  return lm_domain<__half, __half>(linear, src, dst, width, height, pattern, bits, st);
}
