// warp.hip -- parametric geometric resampling (include/tdk_hip_warp.h: tdk_warp, tdk_warp_coordinates), one launch, no workspace.
//
// The specification is the head comment of include/tdk_hip_warp.h: an output pixel (i, j) goes through a homography, OpenCV's
// radial + tangential distortion and a camera matrix to a source coordinate (sx, sy), evaluated in float32 in a fixed order
// (wp_coord), and is interpolated there bilinearly or bicubically (wp_sample).  The map is 18 floats in the kernel arguments.
//
// A workgroup of four waves owns WP_TW x WP_TH output pixels, WP_PIX per thread.  It
//   1. evaluates the map for its pixels and reduces the bounding box of the taps of those that are not outside -- from the
//      pixels themselves, not from the tile's corners, so any map is handled; tap indices are clamped into the frame first (what
//      replicate reads, and what constant may read: a tap outside the frame is replaced by fill when it is used, because fill
//      need not be a value of the storage type), so the box lies inside the frame and staging is a plain copy.  The reduction is
//      min / max of integers: wave shuffles, then four partial boxes through LDS;
//   2. if the box holds at most WP_BOX source pixels, copies its rows to LDS in the storage type, one element per lane
//      (coalesced, any alignment), and takes the taps from there; otherwise (strong local minification, a horizon) takes them
//      from global memory.  The branch is uniform per workgroup; both paths run wp_sample with another fetch, so they give the
//      same bits.  TDK_WARP_DIRECT forces the second path.
// Nothing is accumulated across lanes or workgroups: the bits do not depend on scheduling.
#include <float.h>
#include <limits.h>
#include <math.h>

#include "../../include/tdk_hip_warp.h"
#include "tdk_frame.h"

namespace {

constexpr int WP_THREADS = 256, WP_WAVES = WP_THREADS / 64;
constexpr int WP_TW = 32, WP_TH = 16, WP_PIX = WP_TW * WP_TH / WP_THREADS, WP_ROWS = WP_TH / WP_PIX;
constexpr int WP_MAX_SIZE = 65535;
constexpr int WP_BOX = 2048;          // source pixels a workgroup stages: a tile at 0.55 x local magnification, or rotated by any angle at 1 x
constexpr int WP_RED_WORDS = 16;      // four partial boxes in front of the staged rows

struct WpMap {
  float m[18];
};
struct WpArgs {
  WpMap map;
  float fill;
  int sw, sh, dw, dh;
  int border, direct;
};

// (sx, sy) of output row i, column j, before the clamp; false: the pixel is outside
__device__ __forceinline__ bool wp_coord(const WpMap& a, int i, int j, float& sx, float& sy) {
  const float* m = a.m;
  const float u = (float)j, v = (float)i;
  const float X = (m[0] * u + m[1] * v) + m[2];
  const float Y = (m[3] * u + m[4] * v) + m[5];
  const float Z = (m[6] * u + m[7] * v) + m[8];
  const float iz = 1.0f / Z;
  const float x = X * iz, y = Y * iz;
  const float x2 = x * x, y2 = y * y, r2 = x2 + y2, xy = x * y;
  const float rad = ((m[17] * r2 + m[14]) * r2 + m[13]) * r2 + 1.0f;
  const float tx = m[15] * (xy + xy) + m[16] * (r2 + (x2 + x2));
  const float ty = m[15] * (r2 + (y2 + y2)) + m[16] * (xy + xy);
  const float xd = x * rad + tx, yd = y * rad + ty;
  sx = m[9] * xd + m[11];
  sy = m[10] * yd + m[12];
  return Z > 0.0f && fabsf(sx) <= FLT_MAX && fabsf(sy) <= FLT_MAX;
}

// clamp and split one coordinate: first tap and the fraction
template <int INTERP> __device__ __forceinline__ void wp_split(float s, int n, int& first, float& frac) {
  s = fminf(fmaxf(s, -4.0f), (float)n + 3.0f);
  const float f = floorf(s);
  frac = s - f;
  first = (int)f - (INTERP ? 1 : 0);
}

__device__ __forceinline__ float wp_c1(float t) { return ((1.25f * t - 2.25f) * t) * t + 1.0f; }
__device__ __forceinline__ float wp_c2(float t) { return ((-0.75f * t + 3.75f) * t - 6.0f) * t + 3.0f; }

template <int INTERP> __device__ __forceinline__ void wp_weights(float a, float* w) {
  if (INTERP == 0) {
    w[0] = 1.0f - a;
    w[1] = a;
  } else {
    w[0] = wp_c2(a + 1.0f);
    w[1] = wp_c1(a);
    w[2] = wp_c1(1.0f - a);
    w[3] = wp_c2(2.0f - a);
  }
}

// One pixel that is not outside.  fetch(x, y, c) returns the sample at an in-frame position.
template <int C, int INTERP, typename Fetch> __device__ __forceinline__ void wp_sample(const WpArgs& a, float sx, float sy, const Fetch& fetch, float* out) {
  constexpr int N = INTERP ? 4 : 2;
  int ix, iy;
  float ax, ay, wx[N], wy[N];
  wp_split<INTERP>(sx, a.sw, ix, ax);
  wp_split<INTERP>(sy, a.sh, iy, ay);
  wp_weights<INTERP>(ax, wx);
  wp_weights<INTERP>(ay, wy);
  int xs[N];
  bool okx[N];
#pragma unroll
  for (int k = 0; k < N; k++) {
    const int x = ix + k;
    okx[k] = a.border != 0 || (x >= 0 && x < a.sw);
    xs[k] = min(max(x, 0), a.sw - 1);
  }
#pragma unroll
  for (int ky = 0; ky < N; ky++) {
    const int y = iy + ky, yc = min(max(y, 0), a.sh - 1);
    const bool oky = a.border != 0 || (y >= 0 && y < a.sh);
    float row[C];
#pragma unroll
    for (int kx = 0; kx < N; kx++) {
#pragma unroll
      for (int c = 0; c < C; c++) {
        const float got = fetch(xs[kx], yc, c);
        const float s = (okx[kx] && oky) ? got : a.fill;
        row[c] = kx == 0 ? s * wx[0] : row[c] + s * wx[kx];
      }
    }
#pragma unroll
    for (int c = 0; c < C; c++) out[c] = ky == 0 ? row[c] * wy[0] : out[c] + row[c] * wy[ky];
  }
}

template <typename T, int C> struct WpGlobal {
  const T* src;
  int sw;
  __device__ __forceinline__ float operator()(int x, int y, int c) const { return ld(src, ((size_t)y * sw + x) * C + c); }
};
template <typename T, int C> struct WpStaged {
  const T* stage;
  int x0, y0, pitch;   // box origin; elements per staged row
  __device__ __forceinline__ float operator()(int x, int y, int c) const { return ld(stage, (size_t)((y - y0) * pitch + (x - x0) * C + c)); }
};

__device__ __forceinline__ int wp_wave_min(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o, 64));
  return v;
}

template <typename T, int C, int INTERP> __global__ __launch_bounds__(WP_THREADS) void warp_kernel(const T* __restrict__ src, T* __restrict__ dst, WpArgs a) {
  extern __shared__ int wp_shared[];
  int* red = wp_shared;                                        // per wave: min x, min y, -max x, -max y
  T* stage = reinterpret_cast<T*>(wp_shared + WP_RED_WORDS);    // the box: bh rows of bw C elements as stored
  constexpr int N = INTERP ? 4 : 2;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int ox = (int)blockIdx.x * WP_TW + (tid & (WP_TW - 1)), oy0 = (int)blockIdx.y * WP_TH + tid / WP_TW;

  // 1. the map, and the box of the taps (clamped into the frame) of the pixels that are not outside
  float sx[WP_PIX], sy[WP_PIX];
  bool live[WP_PIX], inside[WP_PIX];
  int lo_x = INT_MAX, lo_y = INT_MAX, hi_x = INT_MAX, hi_y = INT_MAX;   // hi_* hold the negated maximum: every reduction is a min
#pragma unroll
  for (int p = 0; p < WP_PIX; p++) {
    const int oy = oy0 + p * WP_ROWS;
    live[p] = ox < a.dw && oy < a.dh;
    inside[p] = wp_coord(a.map, oy, ox, sx[p], sy[p]) && live[p];
    if (inside[p]) {
      int ix, iy;
      float ax, ay;
      wp_split<INTERP>(sx[p], a.sw, ix, ax);
      wp_split<INTERP>(sy[p], a.sh, iy, ay);
      lo_x = min(lo_x, min(max(ix, 0), a.sw - 1));
      lo_y = min(lo_y, min(max(iy, 0), a.sh - 1));
      hi_x = min(hi_x, -min(max(ix + N - 1, 0), a.sw - 1));
      hi_y = min(hi_y, -min(max(iy + N - 1, 0), a.sh - 1));
    }
  }
  lo_x = wp_wave_min(lo_x);
  lo_y = wp_wave_min(lo_y);
  hi_x = wp_wave_min(hi_x);
  hi_y = wp_wave_min(hi_y);
  if (lane == 0) {
    red[wave * 4 + 0] = lo_x;
    red[wave * 4 + 1] = lo_y;
    red[wave * 4 + 2] = hi_x;
    red[wave * 4 + 3] = hi_y;
  }
  __syncthreads();
#pragma unroll
  for (int w = 0; w < WP_WAVES; w++) {
    lo_x = min(lo_x, red[w * 4 + 0]);
    lo_y = min(lo_y, red[w * 4 + 1]);
    hi_x = min(hi_x, red[w * 4 + 2]);
    hi_y = min(hi_y, red[w * 4 + 3]);
  }
  // the same in every lane; say so, and the branch below is scalar
  const int bx0 = __builtin_amdgcn_readfirstlane(lo_x), by0 = __builtin_amdgcn_readfirstlane(lo_y);
  const int bx1 = -__builtin_amdgcn_readfirstlane(hi_x), by1 = -__builtin_amdgcn_readfirstlane(hi_y);
  const bool any = bx1 >= bx0;   // false: every pixel of the tile is outside, nothing is read
  const int bw = any ? bx1 - bx0 + 1 : 0, bh = any ? by1 - by0 + 1 : 0;
  const bool staged = a.direct == 0 && bw <= WP_BOX && bh <= WP_BOX && bw * bh <= WP_BOX;

  float out[WP_PIX][C];
  if (staged) {
    // 2a. the rows of the box, one element per lane
    const int pitch = bw * C;
    for (int r = wave; r < bh; r += WP_WAVES) {
      const T* row = src + ((size_t)(by0 + r) * a.sw + bx0) * C;
      T* srow = stage + r * pitch;
#pragma unroll 2
      for (int e = lane; e < pitch; e += 64) srow[e] = row[e];
    }
    __syncthreads();
    const WpStaged<T, C> fetch{stage, bx0, by0, pitch};
#pragma unroll
    for (int p = 0; p < WP_PIX; p++)
      if (inside[p]) wp_sample<C, INTERP>(a, sx[p], sy[p], fetch, out[p]);
  } else {
    // 2b. the taps straight from global memory
    const WpGlobal<T, C> fetch{src, a.sw};
#pragma unroll
    for (int p = 0; p < WP_PIX; p++)
      if (inside[p]) wp_sample<C, INTERP>(a, sx[p], sy[p], fetch, out[p]);
  }

#pragma unroll
  for (int p = 0; p < WP_PIX; p++) {
    if (!live[p]) continue;
    const size_t o = ((size_t)(oy0 + p * WP_ROWS) * a.dw + ox) * C;
#pragma unroll
    for (int c = 0; c < C; c++) st(dst, o + c, inside[p] ? out[p][c] : a.fill);
  }
}

// sx, sy before the clamp; NaN in both for a pixel that is outside.  A wave per 64 columns of a row.
__global__ __launch_bounds__(WP_THREADS) void warp_coordinates_kernel(float* __restrict__ xy, WpMap map, int dw, int dh) {
  const int j = (int)blockIdx.x * 64 + ((int)threadIdx.x & 63), i = (int)blockIdx.y * WP_WAVES + ((int)threadIdx.x >> 6);
  if (j >= dw || i >= dh) return;
  float sx, sy;
  const bool inside = wp_coord(map, i, j, sx, sy);
  const size_t o = ((size_t)i * dw + j) * 2;
  xy[o] = inside ? sx : NAN;
  xy[o + 1] = inside ? sy : NAN;
}

inline size_t wp_lds(int channels, int dtype) { return WP_RED_WORDS * sizeof(int) + (size_t)WP_BOX * channels * tdk_dtype_bytes(dtype); }

template <typename T, int C, int INTERP> int launch(const void* src, void* dst, const WpArgs& a, size_t lds, hipStream_t st) {
  const dim3 grid((unsigned)tdk_div_up(a.dw, WP_TW), (unsigned)tdk_div_up(a.dh, WP_TH));
  TDK_LAUNCH("tdk_warp", (warp_kernel<T, C, INTERP>), grid, dim3(WP_THREADS), lds, st, reinterpret_cast<const T*>(src), reinterpret_cast<T*>(dst), a);
  return TDK_OK;
}

inline bool wp_size_ok(int w, int h) { return w >= 1 && h >= 1 && w <= WP_MAX_SIZE && h <= WP_MAX_SIZE; }
inline bool wp_kind_ok(int channels, int dtype, int interp) {
  return (channels == 1 || channels == 3) && (dtype == TDK_F32 || dtype == TDK_F16 || dtype == TDK_U8) && (interp == 0 || interp == 1);
}
// index of the first map entry that is not finite, or -1
inline int wp_bad_map(const float* map) {
  for (int k = 0; k < 18; k++)
    if (!isfinite(map[k])) return k;
  return -1;
}

}  // namespace

TDK_EXPORT int tdk_warp_abi_version(void) { return TDK_WARP_ABI_VERSION; }

TDK_EXPORT size_t tdk_warp_lds_bytes(int channels, int dtype, int interp) {
  return wp_kind_ok(channels, dtype, interp) ? wp_lds(channels, dtype) : 0;
}

TDK_EXPORT int tdk_warp(const void* src, void* dst, int src_width, int src_height, int dst_width, int dst_height, int channels, int dtype,
                        const float* map, int interp, int border, float fill, int flags, tdk_stream_t stream) {
  TDK_REQUIRE(src && dst, "tdk_warp: null pointer (src or dst)");
  TDK_REQUIRE(map, "tdk_warp: null pointer (map)");
  TDK_REQUIRE(wp_size_ok(src_width, src_height), "tdk_warp: source size %dx%d outside 1..%d", src_width, src_height, WP_MAX_SIZE);
  TDK_REQUIRE(wp_size_ok(dst_width, dst_height), "tdk_warp: destination size %dx%d outside 1..%d", dst_width, dst_height, WP_MAX_SIZE);
  TDK_REQUIRE(channels == 1 || channels == 3, "tdk_warp: channels must be 1 or 3, got %d", channels);
  TDK_REQUIRE(dtype == TDK_F32 || dtype == TDK_F16 || dtype == TDK_U8, "tdk_warp: unsupported dtype tag %d", dtype);
  TDK_REQUIRE(interp == 0 || interp == 1, "tdk_warp: interp must be 0 (bilinear) or 1 (bicubic), got %d", interp);
  TDK_REQUIRE(border == 0 || border == 1, "tdk_warp: border must be 0 (constant) or 1 (replicate), got %d", border);
  TDK_REQUIRE(flags == 0 || flags == TDK_WARP_DIRECT, "tdk_warp: flags must be 0 or TDK_WARP_DIRECT, got %d", flags);
  const int bad = wp_bad_map(map);
  TDK_REQUIRE(bad < 0, "tdk_warp: map[%d] is not finite", bad);
  TDK_REQUIRE(isfinite(fill), "tdk_warp: fill is not finite");
  const size_t esz = tdk_dtype_bytes(dtype);
  const size_t src_bytes = (size_t)src_width * src_height * channels * esz, dst_bytes = (size_t)dst_width * dst_height * channels * esz;
  TDK_REQUIRE(tdk_disjoint(src, src_bytes, dst, dst_bytes), "tdk_warp: src and dst overlap (every output reads other positions)");
  WpArgs a{};
  for (int k = 0; k < 18; k++) a.map.m[k] = map[k];
  a.fill = fill;
  a.sw = src_width, a.sh = src_height, a.dw = dst_width, a.dh = dst_height;
  a.border = border, a.direct = flags & TDK_WARP_DIRECT;
  const size_t lds = wp_lds(channels, dtype);
  hipStream_t st = tdk_stream(stream);
  TDK_DISPATCH_FRAME(dtype, channels, T, C, return interp ? launch<T, C, 1>(src, dst, a, lds, st) : launch<T, C, 0>(src, dst, a, lds, st));
}

TDK_EXPORT int tdk_warp_coordinates(float* xy, int dst_width, int dst_height, const float* map, tdk_stream_t stream) {
  TDK_REQUIRE(xy, "tdk_warp_coordinates: null pointer (xy)");
  TDK_REQUIRE(map, "tdk_warp_coordinates: null pointer (map)");
  TDK_REQUIRE(wp_size_ok(dst_width, dst_height), "tdk_warp_coordinates: destination size %dx%d outside 1..%d", dst_width, dst_height, WP_MAX_SIZE);
  const int bad = wp_bad_map(map);
  TDK_REQUIRE(bad < 0, "tdk_warp_coordinates: map[%d] is not finite", bad);
  WpMap m;
  for (int k = 0; k < 18; k++) m.m[k] = map[k];
  const dim3 grid((unsigned)tdk_div_up(dst_width, 64), (unsigned)tdk_div_up(dst_height, WP_WAVES));
  TDK_LAUNCH("tdk_warp_coordinates", warp_coordinates_kernel, grid, dim3(WP_THREADS), 0, tdk_stream(stream), xy, m, dst_width, dst_height);
  return TDK_OK;
}
