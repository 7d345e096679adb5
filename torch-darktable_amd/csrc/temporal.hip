// temporal.hip -- the motion-adaptive recursive temporal denoiser on raw mosaics (include/tdk_hip_temporal.h: tdk_temporal_denoise: one
// tile launch and a one-lane launch that advances the frame index; tdk_temporal_reset: a one-lane launch).
//
// The specification is the head comment of include/tdk_hip_temporal.h.
//
// Filter, tp_filter<TS, TA, TO, R>: a workgroup of 256 lanes owns an output tile of TP_TH = 32 rows of TP_TW = 64 sites.  Every
// workgroup reads the frame index from the head of the state with one uniform load and derives the source and destination planes
// from its parity: nothing on the host knows which plane is which, so a captured call replays any number of times.
//   1. interior: a lane takes eight consecutive sites of one tile row (32 rows x 8 lanes = 256): the sample, the running average
//      and the count, each as 16-byte vectors when its address allows it and per element otherwise and at the frame's right edge.
//      It forms e and v, stores them as float4 into two LDS planes and keeps x, A and N in registers for step 4.
//   2. apron: the R rows above and below and one unit of four sites left and right of the tile, (36 R + 64) units of four
//      sites, one per lane.  Sites outside the frame are staged as +0.0f: no e or v is -0, so adding them leaves every bit of the
//      sums of the specification (which skip them) as it is.
//   3. row sums: a lane reads three float4 of a staged row and writes the four (2R + 1)-term sums of the middle one, every sum
//      from 0.0f in ascending column order, into two more LDS planes.
//   4. column sums: a lane adds the 2R + 1 row sums of each of its eight sites in ascending row order, applies the update and
//      stores the new average, the new count and the output.
// Advance, tp_advance: one lane writes the next index in plain C++.  Reset, tp_reset: one lane writes 0.
#include <math.h>

#include "../../include/tdk_hip_temporal.h"
#include "tdk_frame.h"

namespace {

constexpr int TP_TW = TDK_TEMPORAL_TILE_W, TP_TH = TDK_TEMPORAL_TILE_H;
constexpr int TP_THREADS = 256;
constexpr int TP_GROUP = 8;                          // sites of a lane in the interior
constexpr int TP_GROUPS = TP_TW / TP_GROUP;          // lanes of a tile row
constexpr int TP_SIDE = 4;                           // staged columns on either side of the tile: one unit of four sites
constexpr int TP_SW = TP_TW + 2 * TP_SIDE;           // floats of a staged row
constexpr int TP_UNITS = TP_SW / 4;                  // units of four sites of a staged row
constexpr int TP_MAX_SIZE = 65535;
static_assert(TP_TH * TP_GROUPS == TP_THREADS, "a lane per group of the tile");
static_assert(TP_SIDE >= 3, "the apron of the largest radius");

template <int R> struct TpLds {
  alignas(16) float e[(TP_TH + 2 * R) * TP_SW];      // staged: tile and apron
  alignas(16) float v[(TP_TH + 2 * R) * TP_SW];
  alignas(16) float re[(TP_TH + 2 * R) * TP_TW];     // row sums of the tile's columns
  alignas(16) float rv[(TP_TH + 2 * R) * TP_TW];
};
static_assert(sizeof(TpLds<3>) <= 64 * 1024, "LDS of the filter launch");
static_assert(36 * 3 + 64 <= TP_THREADS, "a lane per apron unit");
// waves per SIMD the LDS admits (160 KB per compute unit, four waves of a workgroup on four SIMDs): the register budget follows it
#define TP_WAVES(R) ((160 * 1024) / (int)sizeof(TpLds<R>))
static_assert(TP_WAVES(2) == 4 && TP_WAVES(3) == 3, "workgroups per compute unit");

struct TpArgs {
  const void* src;
  void* out;
  unsigned char* state;
  size_t acc_bytes, cnt_bytes;   // PA and PC of the header
  int w, h;
  uint32_t pattern;
  const float* model;
  const float* gains;
  float t_hi, inv, c2, n_max, v_min;
};

struct TpRow {
  float a, b;   // a', b'
  bool valid;
};

__device__ __forceinline__ TpRow tp_row(const float* __restrict__ model, const float* __restrict__ gains, int row) {
  const float g = gains ? gains[row] : 1.0f;
  TpRow o;
  o.a = g * model[4 * row];
  o.b = (g * g) * model[4 * row + 1];
  o.valid = model[4 * row + 2] != 0.0f;
  return o;
}

// row k of three, field by field: values, not addresses, so that the rows stay in registers
__device__ __forceinline__ TpRow tp_pick(int k, const TpRow& r0, const TpRow& r1, const TpRow& r2) {
  TpRow o;
  o.a = k == 0 ? r0.a : k == 1 ? r1.a : r2.a;
  o.b = k == 0 ? r0.b : k == 1 ? r1.b : r2.b;
  o.valid = k == 0 ? r0.valid : k == 1 ? r1.valid : r2.valid;
  return o;
}

// ---- storage: M consecutive elements at p, as float32.  One or two 16-byte vectors (8 bytes for four binary16) when p is on such a
// boundary, per element otherwise.
template <typename T, int M> __device__ __forceinline__ bool tp_vector_ok(const T* p) {
  constexpr uintptr_t ALIGN = M * sizeof(T) >= 16 ? 16 : M * sizeof(T);
  return (reinterpret_cast<uintptr_t>(p) & (ALIGN - 1)) == 0;
}

template <int M> __device__ __forceinline__ void tp_load(const float* p, float x[M]) {
#pragma unroll
  for (int k = 0; k < M / 4; k++) {
    const float4 u = reinterpret_cast<const float4*>(p)[k];
    x[4 * k] = u.x, x[4 * k + 1] = u.y, x[4 * k + 2] = u.z, x[4 * k + 3] = u.w;
  }
}
template <int M> __device__ __forceinline__ void tp_load(const __half* p, float x[M]) {
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
template <int M> __device__ __forceinline__ void tp_store(float* p, const float y[M]) {
#pragma unroll
  for (int k = 0; k < M / 4; k++) reinterpret_cast<float4*>(p)[k] = make_float4(y[4 * k], y[4 * k + 1], y[4 * k + 2], y[4 * k + 3]);
}
template <int M> __device__ __forceinline__ void tp_store(__half* p, const float y[M]) {
  uint32_t w[M / 2];
#pragma unroll
  for (int k = 0; k < M / 2; k++)
    w[k] = (uint32_t)__half_as_ushort(__float2half_rn(y[2 * k])) | ((uint32_t)__half_as_ushort(__float2half_rn(y[2 * k + 1])) << 16);
  if constexpr (M == 8) *reinterpret_cast<uint4*>(p) = make_uint4(w[0], w[1], w[2], w[3]);
  else *reinterpret_cast<uint2*>(p) = make_uint2(w[0], w[1]);
}

// M sites of frame row i from column j0 (even; a multiple of four): `live` sites are inside the frame, the others read as 0
template <typename T, int M> __device__ __forceinline__ void tp_fetch(const T* __restrict__ base, size_t at, int live, float x[M]) {
  if (live == M && tp_vector_ok<T, M>(base + at)) tp_load<M>(base + at, x);
  else {
#pragma unroll
    for (int m = 0; m < M; m++) x[m] = m < live ? ld<T>(base, at + m) : 0.0f;
  }
}
template <typename T, int M> __device__ __forceinline__ void tp_put(T* __restrict__ base, size_t at, int live, const float y[M]) {
  if (live == M && tp_vector_ok<T, M>(base + at)) tp_store<M>(base + at, y);
  else {
#pragma unroll
    for (int m = 0; m < M; m++)
      if (m < live) st<T>(base, at + m, y[m]);
  }
}

// e and v of one site (a site outside the frame is not asked)
__device__ __forceinline__ void tp_site(float x, float A, float N, const TpRow& r, float v_min, float& e, float& v) {
  const float d = x - A;
  const float var = fmaxf(r.a * fmaxf(A, 0.0f) + r.b, v_min);
  v = r.valid ? var + var / fmaxf(N, 1.0f) : 0.0f;
  e = r.valid ? d * d : 0.0f;
}

template <typename TS, typename TA, typename TO, int R>
__global__ __launch_bounds__(TP_THREADS, TP_WAVES(R)) void tp_filter(TpArgs a) {
  __shared__ TpLds<R> lds;
  const int tid = threadIdx.x;
  const int x0 = (int)blockIdx.x * TP_TW, y0 = (int)blockIdx.y * TP_TH;

  // the frame index: the same word for every lane of every workgroup; this launch only reads it
  const uint32_t idx = *reinterpret_cast<const uint32_t*>(a.state);
  const bool first = idx == 0u;
  const size_t to_plane = idx & 1u, from_plane = to_plane ^ 1u;
  unsigned char* planes = a.state + TDK_TEMPORAL_HEAD_BYTES;
  const TA* __restrict__ acc_src = reinterpret_cast<const TA*>(planes + from_plane * a.acc_bytes);
  TA* __restrict__ acc_dst = reinterpret_cast<TA*>(planes + to_plane * a.acc_bytes);
  const __half* __restrict__ cnt_src = reinterpret_cast<const __half*>(planes + 2 * a.acc_bytes + from_plane * a.cnt_bytes);
  __half* __restrict__ cnt_dst = reinterpret_cast<__half*>(planes + 2 * a.acc_bytes + to_plane * a.cnt_bytes);
  const TS* __restrict__ src = reinterpret_cast<const TS*>(a.src);
  TO* __restrict__ out = reinterpret_cast<TO*>(a.out);

  const TpRow r0 = tp_row(a.model, a.gains, 0), r1 = tp_row(a.model, a.gains, 1), r2 = tp_row(a.model, a.gains, 2);
  // the model rows of the even and the odd columns of frame row i (every unit starts at an even column)
  auto rows_of = [&](int i, TpRow& even, TpRow& odd) {
    const uint32_t pair = (a.pattern >> (4u * ((uint32_t)i & 1u))) & 15u;
    even = tp_pick((int)(pair & 3u), r0, r1, r2);
    odd = tp_pick((int)(pair >> 2), r0, r1, r2);
  };

  // ---- 1. interior: eight sites of tile row ty
  const int ty = tid / TP_GROUPS, gx = tid % TP_GROUPS;
  const int i = y0 + ty, j0 = x0 + TP_GROUP * gx;
  const int live = i < a.h ? min(max(a.w - j0, 0), TP_GROUP) : 0;
  const size_t at = (size_t)i * (size_t)a.w + (size_t)j0;   // (not formed into an address unless live > 0)
  float x[TP_GROUP], A[TP_GROUP], N[TP_GROUP];
  TpRow even, odd;
  rows_of(i, even, odd);
  {
#pragma unroll
    for (int m = 0; m < TP_GROUP; m++) x[m] = A[m] = N[m] = 0.0f;
    if (live > 0) {
      tp_fetch<TS, TP_GROUP>(src, at, live, x);
      if (!first) {
        tp_fetch<TA, TP_GROUP>(acc_src, at, live, A);
        tp_fetch<__half, TP_GROUP>(cnt_src, at, live, N);
      }
    }
    float e[TP_GROUP], v[TP_GROUP];
#pragma unroll
    for (int m = 0; m < TP_GROUP; m++) {
      tp_site(x[m], A[m], N[m], (m & 1) ? odd : even, a.v_min, e[m], v[m]);
      if (m >= live) e[m] = v[m] = 0.0f;
    }
    const int to = (ty + R) * TP_SW + TP_SIDE + TP_GROUP * gx;
    tp_store<TP_GROUP>(lds.e + to, e);
    tp_store<TP_GROUP>(lds.v + to, v);
  }

  // ---- 2. apron: R rows above, R rows below (whole staged rows), one unit left and right of each tile row
  if (tid < 2 * R * TP_UNITS + 2 * TP_TH) {
    int srow, unit;
    if (tid < 2 * R * TP_UNITS) {
      const int band = tid / (R * TP_UNITS), u = tid - band * (R * TP_UNITS);
      srow = band * (R + TP_TH) + u / TP_UNITS;
      unit = u % TP_UNITS;
    } else {
      const int u = tid - 2 * R * TP_UNITS;
      srow = R + (u >> 1);
      unit = (u & 1) ? TP_UNITS - 1 : 0;
    }
    const int ai = y0 - R + srow, aj = x0 - TP_SIDE + 4 * unit;
    const int alive = (ai >= 0 && ai < a.h && aj >= 0) ? min(max(a.w - aj, 0), 4) : 0;
    float ax[4] = {0.0f, 0.0f, 0.0f, 0.0f}, aA[4] = {0.0f, 0.0f, 0.0f, 0.0f}, aN[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (alive > 0) {
      const size_t aat = (size_t)ai * (size_t)a.w + (size_t)aj;
      tp_fetch<TS, 4>(src, aat, alive, ax);
      if (!first) {
        tp_fetch<TA, 4>(acc_src, aat, alive, aA);
        tp_fetch<__half, 4>(cnt_src, aat, alive, aN);
      }
    }
    TpRow aeven, aodd;
    rows_of(ai, aeven, aodd);
    float e[4], v[4];
#pragma unroll
    for (int m = 0; m < 4; m++) {
      tp_site(ax[m], aA[m], aN[m], (m & 1) ? aodd : aeven, a.v_min, e[m], v[m]);
      if (m >= alive) e[m] = v[m] = 0.0f;
    }
    tp_store<4>(lds.e + srow * TP_SW + 4 * unit, e);
    tp_store<4>(lds.v + srow * TP_SW + 4 * unit, v);
  }
  __syncthreads();

  // ---- 3. row sums: four columns of a staged row per step
#pragma unroll 1
  for (int t = tid; t < (TP_TH + 2 * R) * (TP_TW / 4); t += TP_THREADS) {
    const int srow = t / (TP_TW / 4), cu = t % (TP_TW / 4);
    float we[12], wv[12];
    tp_load<12>(lds.e + srow * TP_SW + 4 * cu, we);   // staged columns 4 cu .. 4 cu + 11: tile columns 4 cu - 4 .. 4 cu + 7
    tp_load<12>(lds.v + srow * TP_SW + 4 * cu, wv);
    float se[4], sv[4];
#pragma unroll
    for (int m = 0; m < 4; m++) {
      float e = 0.0f, v = 0.0f;
#pragma unroll
      for (int k = -R; k <= R; k++) e += we[4 + m + k], v += wv[4 + m + k];
      se[m] = e, sv[m] = v;
    }
    tp_store<4>(lds.re + srow * TP_TW + 4 * cu, se);
    tp_store<4>(lds.rv + srow * TP_TW + 4 * cu, sv);
  }
  __syncthreads();

  // ---- 4. column sums and the update
  if (live > 0) {
    float E[TP_GROUP], V[TP_GROUP];
#pragma unroll
    for (int m = 0; m < TP_GROUP; m++) E[m] = V[m] = 0.0f;
#pragma unroll 1
    for (int dr = 0; dr <= 2 * R; dr++) {   // (not unrolled: the loads of all rows at once cost the registers of a fourth wave)
      float pe[TP_GROUP], pv[TP_GROUP];
      tp_load<TP_GROUP>(lds.re + (ty + dr) * TP_TW + TP_GROUP * gx, pe);
      tp_load<TP_GROUP>(lds.rv + (ty + dr) * TP_TW + TP_GROUP * gx, pv);
#pragma unroll
      for (int m = 0; m < TP_GROUP; m++) E[m] += pe[m], V[m] += pv[m];
    }
    float e[TP_GROUP], v[TP_GROUP];   // of the lane's own sites, as staged in step 1
    tp_load<TP_GROUP>(lds.e + (ty + R) * TP_SW + TP_SIDE + TP_GROUP * gx, e);
    tp_load<TP_GROUP>(lds.v + (ty + R) * TP_SW + TP_SIDE + TP_GROUP * gx, v);
    float y[TP_GROUP], n1[TP_GROUP];
#pragma unroll
    for (int m = 0; m < TP_GROUP; m++) {
      const TpRow& r = (m & 1) ? odd : even;
      const float d = x[m] - A[m];
      const float t = E[m] / V[m];
      float s = fminf(fmaxf((a.t_hi - t) * a.inv, 0.0f), 1.0f);
      if (e[m] > a.c2 * v[m]) s = 0.0f;
      n1[m] = r.valid ? fminf(s * N[m] + 1.0f, a.n_max) : 1.0f;
      y[m] = n1[m] == 1.0f ? x[m] : A[m] + d / n1[m];
    }
    tp_put<TA, TP_GROUP>(acc_dst, at, live, y);
    tp_put<__half, TP_GROUP>(cnt_dst, at, live, n1);
    tp_put<TO, TP_GROUP>(out, at, live, y);
  }
}

__global__ void tp_advance(uint32_t* head) {
  if (threadIdx.x == 0) {
    const uint32_t idx = *head;
    *head = idx == 0xFFFFFFFFu ? 2u : idx + 1u;
  }
}

__global__ void tp_reset(uint32_t* head) {
  if (threadIdx.x == 0) *head = 0u;
}

bool tp_pattern_ok(uint32_t pattern) {
  return pattern == TDK_PATTERN_RGGB || pattern == TDK_PATTERN_BGGR || pattern == TDK_PATTERN_GRBG || pattern == TDK_PATTERN_GBRG;
}
bool tp_dtype_ok(int dtype) { return dtype == TDK_F32 || dtype == TDK_F16; }
bool tp_size_ok(int width, int height) {
  return width >= 2 && height >= 2 && width <= TP_MAX_SIZE && height <= TP_MAX_SIZE && width % 2 == 0 && height % 2 == 0;
}
size_t tp_plane_bytes(int width, int height, size_t element) { return tdk_align_up((size_t)width * (size_t)height * element, 16); }

template <typename TS, typename TA, typename TO, int R> int tp_launch(const TpArgs& a, hipStream_t st) {
  const dim3 grid((unsigned)tdk_div_up(a.w, TP_TW), (unsigned)tdk_div_up(a.h, TP_TH)), block(TP_THREADS);
  TDK_LAUNCH("tdk_temporal_denoise(filter)", (tp_filter<TS, TA, TO, R>), grid, block, 0, st, a);
  return TDK_OK;
}

template <typename TS, typename TA, typename TO> int tp_launch_radius(const TpArgs& a, int radius, hipStream_t st) {
  return radius == 2 ? tp_launch<TS, TA, TO, 2>(a, st) : tp_launch<TS, TA, TO, 3>(a, st);
}

template <typename TS, typename TA> int tp_launch_out(const TpArgs& a, int out_dtype, int radius, hipStream_t st) {
  return out_dtype == TDK_F32 ? tp_launch_radius<TS, TA, float>(a, radius, st) : tp_launch_radius<TS, TA, __half>(a, radius, st);
}

template <typename TS> int tp_launch_state(const TpArgs& a, int state_dtype, int out_dtype, int radius, hipStream_t st) {
  return state_dtype == TDK_F32 ? tp_launch_out<TS, float>(a, out_dtype, radius, st) : tp_launch_out<TS, __half>(a, out_dtype, radius, st);
}

}  // namespace

TDK_EXPORT int tdk_temporal_abi_version(void) { return TDK_TEMPORAL_ABI_VERSION; }

TDK_EXPORT size_t tdk_temporal_state_bytes(int width, int height, int state_dtype) {
  if (!tp_size_ok(width, height) || !tp_dtype_ok(state_dtype)) return 0;
  return TDK_TEMPORAL_HEAD_BYTES + 2 * tp_plane_bytes(width, height, tdk_dtype_bytes(state_dtype)) + 2 * tp_plane_bytes(width, height, 2);
}

TDK_EXPORT size_t tdk_temporal_lds_bytes(int radius) { return radius == 2 ? sizeof(TpLds<2>) : radius == 3 ? sizeof(TpLds<3>) : 0; }

TDK_EXPORT int tdk_temporal_reset(void* state, tdk_stream_t stream) {
  static const char* const who = "tdk_temporal_reset";
  TDK_REQUIRE(state, "%s: null pointer (state)", who);
  TDK_REQUIRE(tdk_aligned(state, 16), "%s: state must be aligned to 16 bytes", who);
  TDK_LAUNCH("tdk_temporal_reset", tp_reset, dim3(1), dim3(1), 0, tdk_stream(stream), reinterpret_cast<uint32_t*>(state));
  return TDK_OK;
}

TDK_EXPORT int tdk_temporal_denoise(const void* src, int src_dtype, void* out, int out_dtype, void* state, int state_dtype, int width, int height,
                                    uint32_t pattern, const float* model, const float* gains, int radius, float t_lo, float t_hi, float pixel_c2, float n_max,
                                    float v_min, tdk_stream_t stream) {
  static const char* const who = "tdk_temporal_denoise";
  TDK_REQUIRE(src && out && state && model, "%s: null pointer (src, out, state or model)", who);
  TDK_REQUIRE(tp_dtype_ok(src_dtype) && tp_dtype_ok(out_dtype) && tp_dtype_ok(state_dtype), "%s: unsupported dtype tags %d -> %d, state %d", who, src_dtype,
              out_dtype, state_dtype);
  TDK_REQUIRE(width >= 2 && height >= 2 && width <= TP_MAX_SIZE && height <= TP_MAX_SIZE, "%s: frame size %dx%d outside 2..%d", who, width, height, TP_MAX_SIZE);
  TDK_REQUIRE(width % 2 == 0 && height % 2 == 0, "%s: mosaic size %dx%d must be even in both axes (whole CFA cells)", who, width, height);
  TDK_REQUIRE(tp_pattern_ok(pattern), "%s: unknown Bayer pattern 0x%08x", who, pattern);
  TDK_REQUIRE(radius == 2 || radius == 3, "%s: radius must be 2 or 3, got %d", who, radius);
  const float inv = 1.0f / (t_hi - t_lo);
  TDK_REQUIRE(isfinite(t_lo) && isfinite(t_hi) && t_lo > 0.0f && t_hi > t_lo && isfinite(inv),
              "%s: the thresholds need 0 < t_lo < t_hi, finite, with a finite 1 / (t_hi - t_lo)", who);
  TDK_REQUIRE(pixel_c2 > 0.0f, "%s: pixel_c2 must be > 0 (+inf turns the per-site test off)", who);
  TDK_REQUIRE(n_max >= 1.0f && n_max <= (float)TDK_TEMPORAL_MAX_FRAMES, "%s: n_max must be 1..%d", who, TDK_TEMPORAL_MAX_FRAMES);
  TDK_REQUIRE(isfinite(v_min) && v_min > 0.0f, "%s: v_min must be finite and > 0", who);
  TDK_REQUIRE(tdk_aligned(state, 16), "%s: state must be aligned to 16 bytes", who);
  const size_t sites = (size_t)width * (size_t)height;
  const size_t src_bytes = sites * tdk_dtype_bytes(src_dtype), out_bytes = sites * tdk_dtype_bytes(out_dtype);
  const size_t state_bytes = tdk_temporal_state_bytes(width, height, state_dtype);
  TDK_REQUIRE(tdk_disjoint(src, src_bytes, out, out_bytes) && tdk_disjoint(src, src_bytes, state, state_bytes) && tdk_disjoint(out, out_bytes, state, state_bytes),
              "%s: src, out and state overlap", who);
  TDK_REQUIRE(tdk_disjoint(model, 48, out, out_bytes) && tdk_disjoint(model, 48, state, state_bytes) &&
                  (!gains || (tdk_disjoint(gains, 12, out, out_bytes) && tdk_disjoint(gains, 12, state, state_bytes))),
              "%s: the model or the gains overlap out or state", who);

  TpArgs a{};
  a.src = src, a.out = out, a.state = reinterpret_cast<unsigned char*>(state);
  a.acc_bytes = tp_plane_bytes(width, height, tdk_dtype_bytes(state_dtype)), a.cnt_bytes = tp_plane_bytes(width, height, 2);
  a.w = width, a.h = height, a.pattern = pattern, a.model = model, a.gains = gains;
  a.t_hi = t_hi, a.inv = inv, a.c2 = pixel_c2, a.n_max = n_max, a.v_min = v_min;
  hipStream_t st = tdk_stream(stream);
  const int rc = src_dtype == TDK_F32 ? tp_launch_state<float>(a, state_dtype, out_dtype, radius, st) : tp_launch_state<__half>(a, state_dtype, out_dtype, radius, st);
  if (rc != TDK_OK) return rc;
  TDK_LAUNCH("tdk_temporal_denoise(advance)", tp_advance, dim3(1), dim3(1), 0, st, reinterpret_cast<uint32_t*>(state));
  return TDK_OK;
}
