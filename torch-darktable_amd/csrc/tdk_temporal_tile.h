// tdk_temporal_tile.h -- the tile body of the recursive temporal filter (include/tdk_hip_temporal.h), shared by tp_filter of temporal.hip
// and mc_filter of motion.hip, with its arguments and the checks of the two entry points.  The two kernels differ in one place: where the
// history (the running average and the count) of a group of sites is read.  That is a type, so the plain filter pays nothing for the
// compensated one.  The steps of the body are listed at the head of temporal.hip.  It launches nothing.
#pragma once

#include "../../include/tdk_hip_temporal.h"
#include "tdk_mosaic_tile.h"

template <int R> using TtTile = MtTile<TDK_TEMPORAL_TILE_W, TDK_TEMPORAL_TILE_H, 8, R>;   // eight sites of a lane in the interior
// waves per SIMD the LDS admits (160 KB per compute unit, four waves of a workgroup on four SIMDs): the register budget follows it
template <int R> constexpr int TT_WAVES = (160 * 1024) / (int)sizeof(typename TtTile<R>::Lds);
static_assert(TT_WAVES<2> == 4 && TT_WAVES<3> == 3, "workgroups per compute unit");

struct TtArgs {
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

// The history of a group of M sites at element `at` = (i, j0) of which `live` > 0 are in the frame: the elements lo <= m < hi at hat + m,
// lo = hi = 0 when it has none (the first frame has none).  The plain filter reads it where the sites are.  (The flag goes to the policy,
// and the body tests hi > lo, because that is the form the compiler folds: asking `!first && history(...)` costs mc_filter 80 instructions.)
struct TtHistoryInPlace {
  __device__ __forceinline__ void operator()(bool first, int, int, int64_t at, int live, int& lo, int& hi, int64_t& hat) const {
    lo = 0, hi = first ? 0 : live, hat = at;
  }
};

// e and v of one site (a site outside the frame is not asked)
__device__ __forceinline__ void tt_site(float x, float A, float N, const MtRow& r, float v_min, float& e, float& v) {
  const float d = x - A;
  const float var = fmaxf(r.a * fmaxf(A, 0.0f) + r.b, v_min);
  v = r.valid ? var + var / fmaxf(N, 1.0f) : 0.0f;
  e = r.valid ? d * d : 0.0f;
}

template <typename TS, typename TA, typename TO, int R, typename History>
__device__ __forceinline__ void tt_filter_tile(typename TtTile<R>::Lds& lds, const TtArgs& a, const History& history) {
  using G = TtTile<R>;
  constexpr int GROUP = G::GROUP;
  const int tid = threadIdx.x;
  const int x0 = (int)blockIdx.x * G::TW, y0 = (int)blockIdx.y * G::TH;

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

  const MtRow r0 = mt_row_gained(a.model, a.gains, 0), r1 = mt_row_gained(a.model, a.gains, 1), r2 = mt_row_gained(a.model, a.gains, 2);

  // ---- 1. interior: eight sites of tile row ty
  const int ty = tid / G::GROUPS, gx = tid % G::GROUPS;
  const int i = y0 + ty, j0 = x0 + GROUP * gx;
  const int live = i < a.h ? min(max(a.w - j0, 0), GROUP) : 0;
  const size_t at = (size_t)i * (size_t)a.w + (size_t)j0;   // (not formed into an address unless live > 0)
  float x[GROUP], A[GROUP], N[GROUP];
  MtRow even, odd;
  mt_rows_of(a.pattern, i, r0, r1, r2, even, odd);
  {
#pragma unroll
    for (int m = 0; m < GROUP; m++) x[m] = A[m] = N[m] = 0.0f;
    if (live > 0) {
      mt_fetch<TS, GROUP>(src, (int64_t)at, 0, live, x);
      int lo, hi;
      int64_t hat;
      history(first, i, j0, (int64_t)at, live, lo, hi, hat);
      if (hi > lo) {
        mt_fetch<TA, GROUP>(acc_src, hat, lo, hi, A);
        mt_fetch<__half, GROUP>(cnt_src, hat, lo, hi, N);
      }
    }
    float e[GROUP], v[GROUP];
#pragma unroll
    for (int m = 0; m < GROUP; m++) {
      tt_site(x[m], A[m], N[m], (m & 1) ? odd : even, a.v_min, e[m], v[m]);
      if (m >= live) e[m] = v[m] = 0.0f;
    }
    mt_store<GROUP>(lds.e + G::staged(ty, gx), e);
    mt_store<GROUP>(lds.v + G::staged(ty, gx), v);
  }

  // ---- 2. apron (staged through a helper shared with step 1, every instantiation costs 10 to 20 instructions more)
  if (tid < G::APRON) {
    int srow, unit;
    G::apron_unit(tid, srow, unit);
    const int ai = y0 - R + srow, aj = x0 - G::SIDE + 4 * unit;
    const int alive = (ai >= 0 && ai < a.h && aj >= 0) ? min(max(a.w - aj, 0), 4) : 0;
    float ax[4] = {0.0f, 0.0f, 0.0f, 0.0f}, aA[4] = {0.0f, 0.0f, 0.0f, 0.0f}, aN[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (alive > 0) {
      const int64_t aat = (int64_t)ai * (int64_t)a.w + (int64_t)aj;
      mt_fetch<TS, 4>(src, aat, 0, alive, ax);
      int lo, hi;
      int64_t hat;
      history(first, ai, aj, aat, alive, lo, hi, hat);
      if (hi > lo) {
        mt_fetch<TA, 4>(acc_src, hat, lo, hi, aA);
        mt_fetch<__half, 4>(cnt_src, hat, lo, hi, aN);
      }
    }
    MtRow aeven, aodd;
    mt_rows_of(a.pattern, ai, r0, r1, r2, aeven, aodd);
    float e[4], v[4];
#pragma unroll
    for (int m = 0; m < 4; m++) {
      tt_site(ax[m], aA[m], aN[m], (m & 1) ? aodd : aeven, a.v_min, e[m], v[m]);
      if (m >= alive) e[m] = v[m] = 0.0f;
    }
    mt_store<4>(lds.e + srow * G::SW + 4 * unit, e);
    mt_store<4>(lds.v + srow * G::SW + 4 * unit, v);
  }
  __syncthreads();

  // ---- 3. row sums
  mt_row_sums<G>(lds, tid);
  __syncthreads();

  // ---- 4. column sums and the update
  if (live > 0) {
    float E[GROUP], V[GROUP];
    mt_column_sums<G>(lds, ty, gx, E, V);
    float e[GROUP], v[GROUP];   // of the lane's own sites, as staged in step 1
    mt_load<GROUP>(lds.e + G::staged(ty, gx), e);
    mt_load<GROUP>(lds.v + G::staged(ty, gx), v);
    float y[GROUP], n1[GROUP];
#pragma unroll
    for (int m = 0; m < GROUP; m++) {
      const MtRow& r = (m & 1) ? odd : even;
      const float d = x[m] - A[m];
      const float s = mt_similarity(E[m], V[m], e[m], v[m], a.t_hi, a.inv, a.c2);
      n1[m] = r.valid ? fminf(s * N[m] + 1.0f, a.n_max) : 1.0f;
      y[m] = n1[m] == 1.0f ? x[m] : A[m] + d / n1[m];
    }
    mt_put<TA, GROUP>(acc_dst, at, live, y);
    mt_put<__half, GROUP>(cnt_dst, at, live, n1);
    mt_put<TO, GROUP>(out, at, live, y);
  }
}

// the next frame index, by one lane in plain C++
__device__ __forceinline__ void tt_advance(uint32_t* head) {
  if (threadIdx.x == 0) {
    const uint32_t idx = *head;
    *head = idx == 0xFFFFFFFFu ? 2u : idx + 1u;
  }
}

// ---- host side: what tdk_temporal_denoise and tdk_motion_temporal_denoise check alike (null pointers apart), and their arguments
static inline int tt_check(const char* who, const void* src, int src_dtype, void* out, int out_dtype, void* state, int state_dtype, int width, int height,
                           uint32_t pattern, const float* model, const float* gains, int radius, float t_lo, float t_hi, float pixel_c2, float n_max, float v_min,
                           TtArgs& a) {
  TDK_REQUIRE(mt_dtype_ok(src_dtype) && mt_dtype_ok(out_dtype) && mt_dtype_ok(state_dtype), "%s: unsupported dtype tags %d -> %d, state %d", who, src_dtype,
              out_dtype, state_dtype);
  if (const int rc = mt_check_mosaic(who, width, height, pattern, radius)) return rc;
  float inv;
  if (const int rc = mt_check_thresholds(who, t_lo, t_hi, pixel_c2, inv)) return rc;
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
  a.src = src, a.out = out, a.state = reinterpret_cast<unsigned char*>(state);
  a.acc_bytes = mt_plane_bytes(width, height, tdk_dtype_bytes(state_dtype)), a.cnt_bytes = mt_plane_bytes(width, height, 2);
  a.w = width, a.h = height, a.pattern = pattern, a.model = model, a.gains = gains;
  a.t_hi = t_hi, a.inv = inv, a.c2 = pixel_c2, a.n_max = n_max, a.v_min = v_min;
  return TDK_OK;
}
