// sharpen.hip -- unsharp mask with a soft threshold and a halo limit (include/tdk_hip_sharpen.h: tdk_sharpen), one launch, no
// workspace.
//
// The specification is the head comment of include/tdk_hip_sharpen.h.  The signal s is the channel itself (NS = C signals per pixel)
// or, with TDK_SHARPEN_LUMA, the luminance (NS = 1).
//
// A workgroup of four waves owns SH_TW x SH_TH = 32 x 32 output pixels.  With R the radius, PW = 32 + 2 R:
//   1. stage    the signal of the tile and its R-pixel apron goes to LDS as float32, `sig`: PW rows of PW pixels, the NS signals of
//               a pixel interleaved as in memory.  A lane takes one pixel per step (consecutive lanes, consecutive pixels of a
//               row); the frame index is clamped here, so an apron position outside the frame holds the replicated edge and
//               nothing after this step tests a border.
//   2. rows     the horizontal pass over all PW rows goes to the second plane `hor`: PW rows of 32 NS values, no padding.  A thread
//               owns one value per step and the 256 threads run over them in memory order: consecutive lanes read and write
//               consecutive words (ds_read_b32 / ds_write_b32: conflict-free inside a row; where a wave's 64 values straddle two
//               rows of a 96-value line the two parts may meet on a bank, two-way at worst).
//   3. columns  a thread owns SH_PIX = 4 adjacent pixels of one tile row, 4 NS values: 16 or 48 contiguous bytes of `hor` per tap
//               row, read as 16-byte vectors (lane stride 4 NS words, 3 coprime to 16: each 16-lane group of a ds_read_b128
//               covers the 64 banks once).  The vertical pass, the threshold and the result stay in registers.
// x[c] and the 3x3 extrema of the halo limit: without LUMA the staged signal IS x[c] (the conversion to float32 is exact), so both
// come from `sig`, whose apron (R >= 1) holds the replicated neighbours.  With LUMA the thread re-reads its own four pixels from
// global memory -- the workgroup has just staged these lines, so the reads hit L2 -- and, for the limit, their 3 x 6 neighbourhood
// with clamped indices.
// Global accesses: a thread's four pixels are 4 C elements; where the frame has whole groups (width % 4 == 0) and starts on a
// multiple of four elements they move as C vectors of four elements (16 bytes float32, 8 binary16, 4 uint8), per element otherwise
// (ShArgs::vec_in, vec_out).  Staging is always per element: its runs start R pixels left of the tile, at any alignment.
// Nothing is accumulated across lanes or workgroups: the bits do not depend on scheduling.
#include <math.h>

#include "../../include/tdk_hip_sharpen.h"
#include "tdk_frame.h"

namespace {

constexpr int SH_THREADS = 256;
constexpr int SH_TW = 32, SH_TH = 32, SH_PIX = 4, SH_GROUPS = SH_TW / SH_PIX;   // 8 threads per tile row, 32 rows
constexpr int SH_MAX_R = TDK_SHARPEN_MAX_RADIUS;
constexpr float SH_MAX_AMOUNT = 16.0f;
constexpr size_t SH_LDS_LIMIT = 64 * 1024;   // the dynamic-LDS size a kernel gets without raising its limit; two workgroups per CU
static_assert(SH_THREADS == SH_GROUPS * SH_TH, "a thread per 4 pixels of the tile");

struct ShArgs {
  float w[SH_MAX_R + 1];
  float amount, threshold, overshoot;
  int width, height, radius;
  int limit, vec_in, vec_out;
};

inline size_t sh_lds_bytes(int signals, int radius) {
  const size_t pw = SH_TW + 2 * radius, rows = SH_TH + 2 * radius;
  return (rows * pw + rows * SH_TW) * signals * sizeof(float);
}
static_assert((SH_TH + 2 * SH_MAX_R) * ((SH_TW + 2 * SH_MAX_R) + SH_TW) * 3 * sizeof(float) <= SH_LDS_LIMIT, "LDS of the largest call");

__device__ __forceinline__ float sh_luma(float r, float g, float b) { return (0.2126729f * r + 0.7151522f * g) + 0.0721750f * b; }

template <typename T, int C, bool LUMA>
__global__ __launch_bounds__(SH_THREADS) void sharpen_kernel(const T* __restrict__ src, T* __restrict__ dst, ShArgs a) {
  constexpr int NS = LUMA ? 1 : C;      // signals per pixel
  constexpr int EW = SH_TW * NS;        // values per row of `hor`
  constexpr int N = SH_PIX * NS;        // signal values of a thread
  constexpr int NX = SH_PIX * C;        // elements of a thread
  static_assert(!LUMA || C == 3, "luminance needs three channels");
  extern __shared__ __attribute__((aligned(16))) float sh_lds[];
  const int R = a.radius, W = a.width, H = a.height;
  const int PW = SH_TW + 2 * R, SP = PW * NS;   // staged rows = staged pixels per row = PW (the tile is square)
  float* sig = sh_lds;                 // PW x SP
  float* hor = sh_lds + PW * SP;       // PW x EW; PW * PW = 4 (16 + R)^2: the plane starts on 16 bytes

  const int tid = threadIdx.x;
  const int x0 = (int)blockIdx.x * SH_TW, y0 = (int)blockIdx.y * SH_TH;

  // ---- 1. the signal of the tile and its apron, clamped to the frame
  const float inv_pw = 1.0f / (float)PW;
  for (int it = tid; it < PW * PW; it += SH_THREADS) {
    const int r = (int)(((float)it + 0.5f) * inv_pw), p = it - r * PW;   // it / PW: the quotient is never near an integer
    const int gy = min(max(y0 - R + r, 0), H - 1), gx = min(max(x0 - R + p, 0), W - 1);
    const size_t o = ((size_t)gy * W + gx) * C;
    if constexpr (LUMA) {
      sig[it] = sh_luma(ld(src, o), ld(src, o + 1), ld(src, o + 2));
    } else {
#pragma unroll
      for (int c = 0; c < C; c++) sig[it * C + c] = ld(src, o + c);
    }
  }
  __syncthreads();

  // ---- 2. horizontal pass of every staged row
  for (int it = tid; it < PW * EW; it += SH_THREADS) {
    const int r = it / EW, e = it - r * EW;
    const float* s = sig + r * SP + R * NS + e;
    float h = a.w[0] * s[0];
#pragma unroll
    for (int k = 1; k <= SH_MAX_R; k++)
      if (k <= R) h = h + a.w[k] * (s[-k * NS] + s[k * NS]);   // (R is uniform: a scalar branch per tap)
    hor[it] = h;
  }
  __syncthreads();

  // ---- 3. vertical pass, threshold, result: four adjacent pixels per thread
  const int tr = tid / SH_GROUPS, tc = (tid % SH_GROUPS) * SH_PIX;
  const int y = y0 + tr, x = x0 + tc;
  if (y >= H || x >= W) return;
  const size_t o = ((size_t)y * W + x) * C;
  const float* sp = sig + (tr + R) * SP + (tc + R) * NS;   // the thread's own signal values

  float xv[NX], out[NX];
  if constexpr (LUMA) {
    if (a.vec_in) {
#pragma unroll
      for (int q = 0; q < C; q++) s4_io<T>::load(src + o + 4 * q, 0, xv + 4 * q);   // (aligned to four elements: vec_in)
    } else {
#pragma unroll
      for (int i = 0; i < NX; i++) xv[i] = x + i / C < W ? ld(src, o + i) : 0.0f;
    }
  } else {
#pragma unroll
    for (int i = 0; i < NX; i++) xv[i] = sp[i];
  }

  if (a.amount == 0.0f) {
#pragma unroll
    for (int i = 0; i < NX; i++) out[i] = xv[i];
  } else {
    float b[N];
    {
      const float4* hp = reinterpret_cast<const float4*>(hor + (tr + R) * EW + tc * NS);
      constexpr int ROW4 = EW / 4;
#pragma unroll
      for (int q = 0; q < N / 4; q++) {
        const float4 c = hp[q];
        b[4 * q] = a.w[0] * c.x, b[4 * q + 1] = a.w[0] * c.y, b[4 * q + 2] = a.w[0] * c.z, b[4 * q + 3] = a.w[0] * c.w;
      }
#pragma unroll
      for (int k = 1; k <= SH_MAX_R; k++) {
#pragma unroll
        for (int q = 0; q < N / 4 && k <= R; q++) {
          const float4 u = hp[q - k * ROW4], d = hp[q + k * ROW4];
          b[4 * q] = b[4 * q] + a.w[k] * (u.x + d.x);
          b[4 * q + 1] = b[4 * q + 1] + a.w[k] * (u.y + d.y);
          b[4 * q + 2] = b[4 * q + 2] + a.w[k] * (u.z + d.z);
          b[4 * q + 3] = b[4 * q + 3] + a.w[k] * (u.w + d.w);
        }
      }
    }
    float add[N];
#pragma unroll
    for (int i = 0; i < N; i++) {
      const float d = sp[i] - b[i], ad = fabsf(d);
      const float dp = ad > a.threshold ? copysignf(ad - a.threshold, d) : 0.0f;
      add[i] = a.amount * dp;
    }
#pragma unroll
    for (int i = 0; i < NX; i++) out[i] = xv[i] + add[LUMA ? i / C : i];

    if (a.limit) {
      // minimum and maximum of the three rows in each of the six columns x - 1 .. x + 4, then of three columns per pixel
      float cmin[6 * C], cmax[6 * C];
#pragma unroll
      for (int dy = -1; dy <= 1; dy++) {
        size_t row = 0;
        if constexpr (LUMA) row = (size_t)min(max(y + dy, 0), H - 1) * W;
#pragma unroll
        for (int q = 0; q < 6; q++) {
#pragma unroll
          for (int c = 0; c < C; c++) {
            float v;
            if constexpr (LUMA) v = ld(src, (row + min(max(x - 1 + q, 0), W - 1)) * C + c);
            else v = sp[dy * SP + (q - 1) * C + c];
            cmin[q * C + c] = dy == -1 ? v : fminf(cmin[q * C + c], v);
            cmax[q * C + c] = dy == -1 ? v : fmaxf(cmax[q * C + c], v);
          }
        }
      }
#pragma unroll
      for (int i = 0; i < NX; i++) {
        const float lo = fminf(fminf(cmin[i], cmin[i + C]), cmin[i + 2 * C]);
        const float hi = fmaxf(fmaxf(cmax[i], cmax[i + C]), cmax[i + 2 * C]);
        out[i] = fminf(fmaxf(out[i], lo - a.overshoot), hi + a.overshoot);
      }
    }
  }

  if (a.vec_out) {
#pragma unroll
    for (int q = 0; q < C; q++) s4_io<T>::store(dst + o + 4 * q, 0, out + 4 * q);
  } else {
#pragma unroll
    for (int i = 0; i < NX; i++)
      if (x + i / C < W) st(dst, o + i, out[i]);
  }
}

template <typename T, int C, bool LUMA> int launch(const void* src, void* dst, const ShArgs& a, hipStream_t st) {
  const dim3 grid((unsigned)tdk_div_up(a.width, SH_TW), (unsigned)tdk_div_up(a.height, SH_TH));
  TDK_LAUNCH("tdk_sharpen", (sharpen_kernel<T, C, LUMA>), grid, dim3(SH_THREADS), sh_lds_bytes(LUMA ? 1 : C, a.radius), st, reinterpret_cast<const T*>(src),
             reinterpret_cast<T*>(dst), a);
  return TDK_OK;
}

// luma is set for three channels only (sh_check)
template <typename T, int C> int dispatch(const void* src, void* dst, bool luma, const ShArgs& a, hipStream_t st) {
  if constexpr (C == 3)
    if (luma) return launch<T, 3, true>(src, dst, a, st);
  return launch<T, C, false>(src, dst, a, st);
}

// 0: fine; otherwise which argument is wrong (messages in tdk_sharpen)
int sh_check(int channels, int dtype, int radius, int flags) {
  if (channels != 1 && channels != 3) return 1;
  if (dtype != TDK_F32 && dtype != TDK_F16 && dtype != TDK_U8) return 2;
  if (radius < 1 || radius > SH_MAX_R) return 3;
  if (flags < 0 || (flags & ~(TDK_SHARPEN_LUMA | TDK_SHARPEN_LIMIT)) != 0) return 4;
  if ((flags & TDK_SHARPEN_LUMA) && channels != 3) return 5;
  return 0;
}

}  // namespace

TDK_EXPORT int tdk_sharpen_abi_version(void) { return TDK_SHARPEN_ABI_VERSION; }

TDK_EXPORT int tdk_sharpen_weights(float sigma, float* weights, int* radius) {
  return tdk_gaussian_taps("tdk_sharpen_weights", sigma, 0.25f, 4.0f, SH_MAX_R, weights, radius);
}

TDK_EXPORT size_t tdk_sharpen_lds_bytes(int channels, int dtype, int radius, int flags) {
  if (sh_check(channels, dtype, radius, flags) != 0) return 0;
  return sh_lds_bytes((flags & TDK_SHARPEN_LUMA) ? 1 : channels, radius);
}

TDK_EXPORT int tdk_sharpen(const void* src, void* dst, int width, int height, int channels, int dtype, const float* weights, int radius, float amount,
                           float threshold, float overshoot, int flags, tdk_stream_t stream) {
  TDK_REQUIRE(src && dst, "tdk_sharpen: null pointer (src or dst)");
  TDK_REQUIRE(weights, "tdk_sharpen: null pointer (weights)");
  TDK_REQUIRE(tdk_frame_size_ok(width, height), "tdk_sharpen: frame size %dx%d outside 1..%d", width, height, TDK_FRAME_MAX_SIZE);
  const int bad = sh_check(channels, dtype, radius, flags);
  TDK_REQUIRE(bad != 1, "tdk_sharpen: channels must be 1 or 3, got %d", channels);
  TDK_REQUIRE(bad != 2, "tdk_sharpen: unsupported dtype tag %d", dtype);
  TDK_REQUIRE(bad != 3, "tdk_sharpen: radius must be 1..%d, got %d", SH_MAX_R, radius);
  TDK_REQUIRE(bad != 4, "tdk_sharpen: flags must be a combination of TDK_SHARPEN_LUMA and TDK_SHARPEN_LIMIT, got %d", flags);
  TDK_REQUIRE(bad != 5, "tdk_sharpen: TDK_SHARPEN_LUMA needs three channels, got %d", channels);
  const int bad_tap = tdk_first_bad_weight(weights, radius + 1);
  TDK_REQUIRE(bad_tap < 0, "tdk_sharpen: weights[%d] must be finite and >= 0", bad_tap);
  TDK_REQUIRE(amount >= 0.0f && amount <= SH_MAX_AMOUNT, "tdk_sharpen: amount must lie in [0, %g]", (double)SH_MAX_AMOUNT);
  TDK_REQUIRE(isfinite(threshold) && threshold >= 0.0f, "tdk_sharpen: threshold must be finite and >= 0");
  TDK_REQUIRE(isfinite(overshoot) && overshoot >= 0.0f, "tdk_sharpen: overshoot must be finite and >= 0");
  const size_t esz = tdk_dtype_bytes(dtype), bytes = (size_t)width * height * channels * esz;
  TDK_REQUIRE(tdk_disjoint(src, bytes, dst, bytes), "tdk_sharpen: src and dst overlap (every output reads its neighbours)");

  const float scale = dtype == TDK_U8 ? 255.0f : 1.0f;
  ShArgs a{};
  for (int k = 0; k <= radius; k++) a.w[k] = weights[k];
  a.amount = amount, a.threshold = threshold * scale, a.overshoot = overshoot * scale;
  a.width = width, a.height = height, a.radius = radius;
  a.limit = (flags & TDK_SHARPEN_LIMIT) != 0;
  // a thread's four pixels as whole vectors of four elements: rows must hold whole groups and start on the vector's alignment
  a.vec_in = tdk_vec4_ok(width, src, 4 * esz);
  a.vec_out = tdk_vec4_ok(width, dst, 4 * esz);
  const bool luma = (flags & TDK_SHARPEN_LUMA) != 0;
  hipStream_t st = tdk_stream(stream);
  TDK_DISPATCH_FRAME(dtype, channels, T, C, return dispatch<T, C>(src, dst, luma, a, st));
}
