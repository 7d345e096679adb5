// tdk_mosaic_tile.h -- what the tile kernels on raw mosaics share (temporal.hip, motion.hip, hdrmerge.hip): groups of sites in global
// memory and LDS, the rows of the noise model, the geometry of a tile with its apron, the two passes of the (2R + 1)^2 window sums with
// the threshold step that follows them, and the host-side checks of a mosaic and of the thresholds.  It launches nothing: a kernel and
// its launch stay in the file of the operator.
#pragma once

#include <math.h>

#include "tdk_frame.h"

constexpr int MT_THREADS = 256;   // lanes of a workgroup

// ---- storage: M consecutive elements at p, as float32.  One or two 16-byte vectors (8 bytes for four binary16) when p is on such a
// boundary, per element otherwise.
template <typename T, int M> __device__ __forceinline__ bool mt_vector_ok(const T* p) {
  constexpr uintptr_t ALIGN = M * sizeof(T) >= 16 ? 16 : M * sizeof(T);
  return (reinterpret_cast<uintptr_t>(p) & (ALIGN - 1)) == 0;
}

template <int M> __device__ __forceinline__ void mt_load(const float* p, float x[M]) {
#pragma unroll
  for (int k = 0; k < M / 4; k++) {
    const float4 u = reinterpret_cast<const float4*>(p)[k];
    x[4 * k] = u.x, x[4 * k + 1] = u.y, x[4 * k + 2] = u.z, x[4 * k + 3] = u.w;
  }
}
template <int M> __device__ __forceinline__ void mt_load(const __half* p, float x[M]) {
  uint32_t w[M / 2];
  if constexpr (M == 8) {
    const uint4 u = *reinterpret_cast<const uint4*>(p);
    w[0] = u.x, w[1] = u.y, w[2] = u.z, w[3] = u.w;
  } else {
    const uint2 u = *reinterpret_cast<const uint2*>(p);
    w[0] = u.x, w[1] = u.y;
  }
#pragma unroll
  for (int k = 0; k < M; k++) x[k] = __half2float(__ushort_as_half((unsigned short)((w[k / 2] >> (16 * (k % 2))) & 0xffffu)));
}
template <int M> __device__ __forceinline__ void mt_store(float* p, const float y[M]) {
#pragma unroll
  for (int k = 0; k < M / 4; k++) reinterpret_cast<float4*>(p)[k] = make_float4(y[4 * k], y[4 * k + 1], y[4 * k + 2], y[4 * k + 3]);
}
template <int M> __device__ __forceinline__ void mt_store(__half* p, const float y[M]) {
  uint32_t w[M / 2];
#pragma unroll
  for (int k = 0; k < M / 2; k++)
    w[k] = (uint32_t)__half_as_ushort(__float2half_rn(y[2 * k])) | ((uint32_t)__half_as_ushort(__float2half_rn(y[2 * k + 1])) << 16);
  if constexpr (M == 8) *reinterpret_cast<uint4*>(p) = make_uint4(w[0], w[1], w[2], w[3]);
  else *reinterpret_cast<uint2*>(p) = make_uint2(w[0], w[1]);
}

// the elements lo <= m < hi of the M at base[at + m], the others read as 0; `at` is a place in the plane whenever lo < hi covers it.
// M sites of a frame row from an even column of which `live` are inside the frame: lo = 0, hi = live.
template <typename T, int M> __device__ __forceinline__ void mt_fetch(const T* __restrict__ base, int64_t at, int lo, int hi, float x[M]) {
  if (lo == 0 && hi == M && mt_vector_ok<T, M>(base + at)) mt_load<M>(base + at, x);
  else {
#pragma unroll
    for (int m = 0; m < M; m++) x[m] = (m >= lo && m < hi) ? ld<T>(base, (size_t)(at + m)) : 0.0f;
  }
}
template <typename T, int M> __device__ __forceinline__ void mt_put(T* __restrict__ base, size_t at, int live, const float y[M]) {
  if (live == M && mt_vector_ok<T, M>(base + at)) mt_store<M>(base + at, y);
  else {
#pragma unroll
    for (int m = 0; m < M; m++)
      if (m < live) st<T>(base, at + m, y[m]);
  }
}

// ---- a row of the noise model (include/tdk_hip_noise.h): variance a x + b of one colour
struct MtRow {
  float a, b;
  bool valid;
};

// the temporal filters: the row under the white-balance gains, a' and b'
__device__ __forceinline__ MtRow mt_row_gained(const float* __restrict__ model, const float* __restrict__ gains, int row) {
  const float g = gains ? gains[row] : 1.0f;
  MtRow o;
  o.a = g * model[4 * row];
  o.b = (g * g) * model[4 * row + 1];
  o.valid = model[4 * row + 2] != 0.0f;
  return o;
}
// the bracket merge: a row that is not valid reads as variance 1
__device__ __forceinline__ MtRow mt_row_or_unit(const float* __restrict__ model, int row) {
  MtRow o;
  o.valid = model[4 * row + 2] != 0.0f;
  o.a = o.valid ? model[4 * row] : 1.0f;
  o.b = o.valid ? model[4 * row + 1] : 0.0f;
  return o;
}

// row k of three, field by field: values, not addresses, so that the rows stay in registers
__device__ __forceinline__ MtRow mt_pick(int k, const MtRow& r0, const MtRow& r1, const MtRow& r2) {
  MtRow o;
  o.a = k == 0 ? r0.a : k == 1 ? r1.a : r2.a;
  o.b = k == 0 ? r0.b : k == 1 ? r1.b : r2.b;
  o.valid = k == 0 ? r0.valid : k == 1 ? r1.valid : r2.valid;
  return o;
}
// the model rows of the even and the odd columns of frame row i (every unit starts at an even column)
__device__ __forceinline__ void mt_rows_of(uint32_t pattern, int i, const MtRow& r0, const MtRow& r1, const MtRow& r2, MtRow& even, MtRow& odd) {
  const uint32_t pair = (pattern >> (4u * ((uint32_t)i & 1u))) & 15u;
  even = mt_pick((int)(pair & 3u), r0, r1, r2);
  odd = mt_pick((int)(pair >> 2), r0, r1, r2);
}

// ---- the tile of a workgroup: TH rows of TW sites, a lane per GROUP consecutive sites of a row, and around it the apron of the window
// sums, R rows above and below and one unit of four sites left and right
template <int TW_, int TH_, int GROUP_, int R_> struct MtTile {
  static constexpr int TW = TW_, TH = TH_, GROUP = GROUP_, R = R_;
  static constexpr int GROUPS = TW / GROUP;               // lanes of a tile row
  static constexpr int SIDE = 4;                          // staged columns on either side of the tile: one unit of four sites
  static constexpr int SW = TW + 2 * SIDE;                // floats of a staged row
  static constexpr int UNITS = SW / 4;                    // units of four sites of a staged row
  static constexpr int ROWS = TH + 2 * R;                 // staged rows
  static constexpr int APRON = 2 * R * UNITS + 2 * TH;    // units of the apron
  static_assert(TH * GROUPS == MT_THREADS, "a lane per group of the tile");
  static_assert(SIDE >= R, "the apron of the radius");
  static_assert(APRON <= MT_THREADS, "a lane per apron unit");

  struct Lds {
    alignas(16) float e[ROWS * SW];   // staged: tile and apron
    alignas(16) float v[ROWS * SW];
    alignas(16) float re[ROWS * TW];  // row sums of the tile's columns
    alignas(16) float rv[ROWS * TW];
  };
  static_assert(sizeof(Lds) <= 64 * 1024, "LDS of the tile launch");

  // where the group of lane (ty, gx) is staged
  static __device__ __forceinline__ int staged(int ty, int gx) { return (ty + R) * SW + SIDE + GROUP * gx; }
  // the apron unit of lane tid < APRON: R rows above, R rows below (whole staged rows), one unit left and right of each tile row
  static __device__ __forceinline__ void apron_unit(int tid, int& srow, int& unit) {
    if (tid < 2 * R * UNITS) {
      const int band = tid / (R * UNITS), u = tid - band * (R * UNITS);
      srow = band * (R + TH) + u / UNITS;
      unit = u % UNITS;
    } else {
      const int u = tid - 2 * R * UNITS;
      srow = R + (u >> 1);
      unit = (u & 1) ? UNITS - 1 : 0;
    }
  }
};

// ---- the window sums over the staged planes, between two barriers of the caller.  Every sum starts from 0.0f and runs in ascending
// column order, then in ascending row order: the order of the specifications.
// Row sums, four columns of a staged row per step: a lane reads three float4 and writes the four (2R + 1)-term sums of the middle one.
template <typename G> __device__ __forceinline__ void mt_row_sums(typename G::Lds& lds, int tid) {
  constexpr int R = G::R;
#pragma unroll 1
  for (int t = tid; t < G::ROWS * (G::TW / 4); t += MT_THREADS) {
    const int srow = t / (G::TW / 4), cu = t % (G::TW / 4);
    float we[12], wv[12];
    mt_load<12>(lds.e + srow * G::SW + 4 * cu, we);   // staged columns 4 cu .. 4 cu + 11: tile columns 4 cu - 4 .. 4 cu + 7
    mt_load<12>(lds.v + srow * G::SW + 4 * cu, wv);
    float se[4], sv[4];
#pragma unroll
    for (int m = 0; m < 4; m++) {
      float e = 0.0f, v = 0.0f;
#pragma unroll
      for (int k = -R; k <= R; k++) e += we[4 + m + k], v += wv[4 + m + k];
      se[m] = e, sv[m] = v;
    }
    mt_store<4>(lds.re + srow * G::TW + 4 * cu, se);
    mt_store<4>(lds.rv + srow * G::TW + 4 * cu, sv);
  }
}
// Column sums of the group of lane (ty, gx): the 2R + 1 row sums of each of its sites.
template <typename G> __device__ __forceinline__ void mt_column_sums(const typename G::Lds& lds, int ty, int gx, float E[G::GROUP], float V[G::GROUP]) {
#pragma unroll
  for (int m = 0; m < G::GROUP; m++) E[m] = V[m] = 0.0f;
#pragma unroll 1
  for (int dr = 0; dr <= 2 * G::R; dr++) {   // (not unrolled: the loads of all rows at once cost the registers of a fourth wave)
    float pe[G::GROUP], pv[G::GROUP];
    mt_load<G::GROUP>(lds.re + (ty + dr) * G::TW + G::GROUP * gx, pe);
    mt_load<G::GROUP>(lds.rv + (ty + dr) * G::TW + G::GROUP * gx, pv);
#pragma unroll
    for (int m = 0; m < G::GROUP; m++) E[m] += pe[m], V[m] += pv[m];
  }
}
// The threshold step: s of a site from the sums E and V of its window and its own e and v.
__device__ __forceinline__ float mt_similarity(float E, float V, float e, float v, float t_hi, float inv, float c2) {
  const float t = E / V;
  float s = fminf(fmaxf((t_hi - t) * inv, 0.0f), 1.0f);
  if (e > c2 * v) s = 0.0f;
  return s;
}

// ---- host side
static inline bool mt_dtype_ok(int dtype) { return dtype == TDK_F32 || dtype == TDK_F16; }
static inline bool mt_size_ok(int width, int height) { return tdk_mosaic_size_ok(width, height) && width % 2 == 0 && height % 2 == 0; }
static inline size_t mt_plane_bytes(int width, int height, size_t element) { return tdk_align_up((size_t)width * (size_t)height * element, 16); }

// the size of a mosaic, its pattern and the radius of the window
static inline int mt_check_mosaic(const char* who, int width, int height, uint32_t pattern, int radius) {
  TDK_REQUIRE(tdk_mosaic_size_ok(width, height), "%s: frame size %dx%d outside 2..%d", who, width, height, TDK_MOSAIC_MAX_SIZE);
  TDK_REQUIRE(width % 2 == 0 && height % 2 == 0, "%s: mosaic size %dx%d must be even in both axes (whole CFA cells)", who, width, height);
  TDK_REQUIRE(tdk_pattern_ok(pattern), "%s: unknown Bayer pattern 0x%08x", who, pattern);
  TDK_REQUIRE(radius == 2 || radius == 3, "%s: radius must be 2 or 3, got %d", who, radius);
  return TDK_OK;
}
// the thresholds of the threshold step; inv: 1 / (t_hi - t_lo)
static inline int mt_check_thresholds(const char* who, float t_lo, float t_hi, float pixel_c2, float& inv) {
  inv = 1.0f / (t_hi - t_lo);
  TDK_REQUIRE(isfinite(t_lo) && isfinite(t_hi) && t_lo > 0.0f && t_hi > t_lo && isfinite(inv),
              "%s: the thresholds need 0 < t_lo < t_hi, finite, with a finite 1 / (t_hi - t_lo)", who);
  TDK_REQUIRE(pixel_c2 > 0.0f, "%s: pixel_c2 must be > 0 (+inf turns the per-site test off)", who);
  return TDK_OK;
}
