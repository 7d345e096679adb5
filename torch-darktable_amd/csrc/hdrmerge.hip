// hdrmerge.hip -- the noise-weighted merge of an exposure bracket of raw mosaics (include/tdk_hip_hdr.h: tdk_hdr_merge, one tile launch).
//
// The specification is the head comment of include/tdk_hip_hdr.h.  The storage helpers and the two passes of the window sums are those
// of temporal.hip, duplicated here so that nothing this file needs can change that file's code.
//
// hd_merge<TS, TO, R>: a workgroup of 256 lanes owns an output tile of HD_TH = 32 rows of HD_TW = 32 sites.  A lane takes four
// consecutive sites of one tile row (the interior) and, the first 20 R + 64 lanes, one unit of four sites of the apron: the R rows above
// and below and one unit left and right of the tile.  What a lane knows about its sites stays in its registers through the frame loop.
//   0. every lane finds the shortest and the longest exposure; F lanes write the ratios k_f and one lane the frame addresses into LDS,
//      where a lane can index them with the anchor of a site.
//   1. clip bits: bit f of a byte per site, on the tile and an apron of R + 1 sites, units of four sites round-robin over the lanes
//      (the first read of the frames; the loads of a frame go to addresses clamped into the frame and are all in flight together).
//      Sites outside the frame have no bit set.
//   2. anchors: per interior and apron site the OR of the 3 x 3 clip bytes, the anchor frame g, R = x_g / k_g (one more sample, from the
//      frame the site chose) and u_g.
//   3. per frame f: the lane stages eps and v of its sites (the third read of the frames; a site outside the frame, saturated in f,
//      blown or anchored on f is staged as +0.0f), row sums, column sums, then the weight of f at the four interior sites goes into
//      num and den.
//   4. out = num / den or R, and the mask byte.
#include <math.h>

#include "../../include/tdk_hip_hdr.h"
#include "tdk_frame.h"

namespace {

constexpr int HD_TW = TDK_HDR_TILE_W, HD_TH = TDK_HDR_TILE_H;
constexpr int HD_THREADS = 256;
constexpr int HD_GROUP = 4;                          // sites of a lane in the interior
constexpr int HD_GROUPS = HD_TW / HD_GROUP;          // lanes of a tile row
constexpr int HD_SIDE = 4;                           // staged columns on either side of the tile: one unit of four sites
constexpr int HD_SW = HD_TW + 2 * HD_SIDE;           // sites of a staged row
constexpr int HD_UNITS = HD_SW / 4;                  // units of four sites of a staged row
constexpr int HD_MAX_SIZE = 65535;
constexpr int HD_F = TDK_HDR_MAX_FRAMES;
static_assert(HD_TH * HD_GROUPS == HD_THREADS, "a lane per group of the tile");
static_assert(HD_SIDE >= 3 + 1, "the apron of the largest radius and the rim of the clip bits");
static_assert(HD_F <= 8, "a clip bit per frame in a byte");

template <int R> struct HdLds {
  alignas(16) float e[(HD_TH + 2 * R) * HD_SW];      // staged: tile and apron
  alignas(16) float v[(HD_TH + 2 * R) * HD_SW];
  alignas(16) float re[(HD_TH + 2 * R) * HD_TW];     // row sums of the tile's columns
  alignas(16) float rv[(HD_TH + 2 * R) * HD_TW];
  alignas(16) uint32_t clip[(HD_TH + 2 * R + 2) * HD_UNITS];   // a byte per site, four sites a word: one row more on either side
  alignas(16) const void* frame[HD_F];
  float k[HD_F];
};
static_assert(sizeof(HdLds<3>) <= 64 * 1024, "LDS of the merge launch");
static_assert(2 * 3 * HD_UNITS + 2 * HD_TH <= HD_THREADS, "a lane per apron unit");
// the register budget: four waves per SIMD (128 registers); the LDS would admit six workgroups
constexpr int HD_WAVES = 4;

struct HdArgs {
  const void* frames[HD_F];   // unused entries are null
  void* out;
  unsigned char* mask;
  const float* exposures;
  const float* model;
  int nf, ref, w, h;
  uint32_t pattern;
  float clip, t_hi, inv, c2, v_min;
};

struct HdRow {
  float a, b;
  bool valid;
};

__device__ __forceinline__ HdRow hd_row(const float* __restrict__ model, int row) {
  HdRow o;
  o.valid = model[4 * row + 2] != 0.0f;
  o.a = o.valid ? model[4 * row] : 1.0f;
  o.b = o.valid ? model[4 * row + 1] : 0.0f;
  return o;
}

// row k of three, field by field: values, not addresses, so that the rows stay in registers
__device__ __forceinline__ HdRow hd_pick(int k, const HdRow& r0, const HdRow& r1, const HdRow& r2) {
  HdRow o;
  o.a = k == 0 ? r0.a : k == 1 ? r1.a : r2.a;
  o.b = k == 0 ? r0.b : k == 1 ? r1.b : r2.b;
  o.valid = k == 0 ? r0.valid : k == 1 ? r1.valid : r2.valid;
  return o;
}

// ---- storage: M consecutive elements at p, as float32.  One or two 16-byte vectors (8 bytes for four binary16) when p is on such a
// boundary, per element otherwise.
template <typename T, int M> __device__ __forceinline__ bool hd_vector_ok(const T* p) {
  constexpr uintptr_t ALIGN = M * sizeof(T) >= 16 ? 16 : M * sizeof(T);
  return (reinterpret_cast<uintptr_t>(p) & (ALIGN - 1)) == 0;
}

template <int M> __device__ __forceinline__ void hd_load(const float* p, float x[M]) {
#pragma unroll
  for (int k = 0; k < M / 4; k++) {
    const float4 u = reinterpret_cast<const float4*>(p)[k];
    x[4 * k] = u.x, x[4 * k + 1] = u.y, x[4 * k + 2] = u.z, x[4 * k + 3] = u.w;
  }
}
template <int M> __device__ __forceinline__ void hd_load(const __half* p, float x[M]) {
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
template <int M> __device__ __forceinline__ void hd_store(float* p, const float y[M]) {
#pragma unroll
  for (int k = 0; k < M / 4; k++) reinterpret_cast<float4*>(p)[k] = make_float4(y[4 * k], y[4 * k + 1], y[4 * k + 2], y[4 * k + 3]);
}
template <int M> __device__ __forceinline__ void hd_store(__half* p, const float y[M]) {
  uint32_t w[M / 2];
#pragma unroll
  for (int k = 0; k < M / 2; k++)
    w[k] = (uint32_t)__half_as_ushort(__float2half_rn(y[2 * k])) | ((uint32_t)__half_as_ushort(__float2half_rn(y[2 * k + 1])) << 16);
  if constexpr (M == 8) *reinterpret_cast<uint4*>(p) = make_uint4(w[0], w[1], w[2], w[3]);
  else *reinterpret_cast<uint2*>(p) = make_uint2(w[0], w[1]);
}

// M sites of a frame row from an even column: `live` sites are inside the frame, the others read as 0
template <typename T, int M> __device__ __forceinline__ void hd_fetch(const T* __restrict__ base, size_t at, int live, float x[M]) {
  if (live == M && hd_vector_ok<T, M>(base + at)) hd_load<M>(base + at, x);
  else {
#pragma unroll
    for (int m = 0; m < M; m++) x[m] = m < live ? ld<T>(base, at + m) : 0.0f;
  }
}
template <typename T, int M> __device__ __forceinline__ void hd_put(T* __restrict__ base, size_t at, int live, const float y[M]) {
  if (live == M && hd_vector_ok<T, M>(base + at)) hd_store<M>(base + at, y);
  else {
#pragma unroll
    for (int m = 0; m < M; m++)
      if (m < live) st<T>(base, at + m, y[m]);
  }
}

// byte m of a run of sites packed four to a word
template <int M> __device__ __forceinline__ uint32_t hd_byte(const uint32_t (&w)[M / 4], int m) { return (w[m / 4] >> (8 * (m % 4))) & 0xffu; }

// What a lane keeps of M of its sites: R, u_g, and packed a byte per site the saturation bits and g | blown << 3.
template <int M> struct HdSites {
  float R[M], ug[M];
  uint32_t sat[M / 4], meta[M / 4];
};

// Step 2 for the M sites from staged unit `unit0` of staged row `srow`; `live` of them are inside the frame, from element `at` on.
// A site outside the frame is marked blown: it takes no part in any window.
template <typename TS, int M, int R>
__device__ __forceinline__ void hd_anchor(const HdLds<R>& lds, int nf, int ref, int lo, int srow, int unit0, size_t at, int live, const HdRow& even,
                                          const HdRow& odd, float v_min, HdSites<M>& s) {
  constexpr int W = M / 4;
  // the OR of the three rows around the sites, one word further on either side (a word outside the plane holds no site of the apron)
  uint32_t col[W + 2];
#pragma unroll
  for (int k = 0; k < W + 2; k++) {
    const int u = unit0 - 1 + k;
    const bool in = u >= 0 && u < HD_UNITS;
    const int c = srow * HD_UNITS + (in ? u : 0);   // plane row srow is the row above staged row srow
    const uint32_t three = lds.clip[c] | lds.clip[c + HD_UNITS] | lds.clip[c + 2 * HD_UNITS];
    col[k] = in ? three : 0u;
  }
#pragma unroll
  for (int k = 0; k < W; k++) s.sat[k] = col[k + 1] | (col[k + 1] << 8) | (col[k] >> 24) | (col[k + 1] >> 8) | (col[k + 2] << 24);

  int best[M];
  float bk[M];
#pragma unroll
  for (int m = 0; m < M; m++) best[m] = -1, bk[m] = 0.0f;
#pragma unroll 1
  for (int f = 0; f < nf; f++) {
    const float kf = lds.k[f];
#pragma unroll
    for (int m = 0; m < M; m++) {
      const bool free = ((hd_byte<M>(s.sat, m) >> f) & 1u) == 0u;
      if (free && (best[m] < 0 || kf > bk[m])) best[m] = f, bk[m] = kf;
    }
  }
  const float k_ref = lds.k[ref], k_lo = lds.k[lo];
#pragma unroll
  for (int k = 0; k < W; k++) s.meta[k] = 0u;
  int g[M];
  float kg[M], xg[M];
#pragma unroll
  for (int m = 0; m < M; m++) {
    const bool use_ref = ((hd_byte<M>(s.sat, m) >> ref) & 1u) == 0u;
    g[m] = use_ref ? ref : best[m];
    kg[m] = use_ref ? k_ref : bk[m];
    if (g[m] < 0) {   // blown
      g[m] = lo, kg[m] = k_lo;
      s.meta[m / 4] |= 8u << (8 * (m % 4));
    }
    xg[m] = 0.0f;
  }
  if (live > 0) {
    // one sample per site from the frame it chose; a site outside the frame reads the last one inside, so that the loads do not wait for
    // one another
#pragma unroll
    for (int m = 0; m < M; m++) xg[m] = ld<TS>(reinterpret_cast<const TS*>(lds.frame[g[m]]), at + (size_t)min(m, live - 1));
  }
#pragma unroll
  for (int m = 0; m < M; m++) {
    if (m < live) {
      const HdRow& r = (m & 1) ? odd : even;
      const float Rq = xg[m] / kg[m];
      const float var = fmaxf(r.a * (fmaxf(Rq, 0.0f) * kg[m]) + r.b, v_min);
      s.R[m] = Rq;
      s.ug[m] = var / (kg[m] * kg[m]);
      s.meta[m / 4] |= (uint32_t)g[m] << (8 * (m % 4));
    } else {
      s.R[m] = 0.0f, s.ug[m] = 0.0f;
      s.meta[m / 4] = (s.meta[m / 4] & ~(0xffu << (8 * (m % 4)))) | (8u << (8 * (m % 4)));
    }
  }
}

// Steps 3 and 4 of frame f for M sites: r_f, u_f, and the staged eps and v.  POW2: k_f is a power of two in 1 .. 2^60, so that 1 / k_f and
// 1 / (k_f * k_f) are exact and a product with them is the correctly rounded quotient, bit for bit (subnormal results included): the two
// divisions per site and frame that brackets in whole stops do not need.
template <int M, bool POW2>
__device__ __forceinline__ void hd_site(const float x[M], const HdSites<M>& s, int f, float kf, const HdRow& even, const HdRow& odd, float v_min, float r[M],
                                        float u[M], float e[M], float v[M]) {
  const float kk = kf * kf;
  const float ik = 1.0f / kf, ikk = 1.0f / kk;   // (used when exact)
#pragma unroll
  for (int m = 0; m < M; m++) {
    const HdRow& row = (m & 1) ? odd : even;
    r[m] = POW2 ? x[m] * ik : x[m] / kf;
    const float var = fmaxf(row.a * (fmaxf(s.R[m], 0.0f) * kf) + row.b, v_min);
    u[m] = POW2 ? var * ikk : var / kk;
    const float d = r[m] - s.R[m];
    const uint32_t meta = hd_byte<M>(s.meta, m);
    const bool out = ((hd_byte<M>(s.sat, m) >> f) & 1u) != 0u || (meta & 8u) != 0u || (int)(meta & 7u) == f;
    e[m] = out ? 0.0f : d * d;
    v[m] = out ? 0.0f : u[m] + s.ug[m];
  }
}

template <typename TS, typename TO, int R>
__global__ __launch_bounds__(HD_THREADS, HD_WAVES) void hd_merge(HdArgs a) {
  __shared__ HdLds<R> lds;
  const int tid = threadIdx.x;
  const int x0 = (int)blockIdx.x * HD_TW, y0 = (int)blockIdx.y * HD_TH;
  const int nf = a.nf;
  TO* __restrict__ out = reinterpret_cast<TO*>(a.out);

  // ---- 0. the exposures: the same values for every lane of every workgroup
  int lo = 0, hi = 0;
  float e_lo = a.exposures[0], e_hi = e_lo;
#pragma unroll 1
  for (int f = 1; f < nf; f++) {
    const float e = a.exposures[f];
    if (e < e_lo) lo = f, e_lo = e;
    if (e > e_hi) hi = f, e_hi = e;
  }
  const int ref = a.ref < 0 ? hi : a.ref;
  if (tid < nf) lds.k[tid] = a.exposures[tid] / e_lo;
  if (tid == HD_THREADS - 1) {
#pragma unroll
    for (int f = 0; f < HD_F; f++) lds.frame[f] = a.frames[f];
  }
  __syncthreads();

  // ---- 1. clip bits on the tile and R + 1 sites around it (columns: the whole staged row).  A lane takes CLIP_PER units.  Every address
  // is clamped into the frame and a site outside it is masked afterwards, so that no load hangs on a condition: the loads of a frame are
  // all in flight before the first comparison, one latency per frame instead of one per unit and frame.
  {
    constexpr int CLIP_UNITS = (HD_TH + 2 * R + 2) * HD_UNITS, CLIP_PER = (CLIP_UNITS + HD_THREADS - 1) / HD_THREADS;
    size_t cat[CLIP_PER][4];
    uint32_t inside[CLIP_PER], word[CLIP_PER];
#pragma unroll
    for (int p = 0; p < CLIP_PER; p++) {
      const int t = tid + p * HD_THREADS;
      const int prow = t / HD_UNITS, unit = t % HD_UNITS;
      const int ci = y0 - (R + 1) + prow, cj = x0 - HD_SIDE + 4 * unit;
      const bool row_in = t < CLIP_UNITS && ci >= 0 && ci < a.h;
      const size_t row_at = (size_t)min(max(ci, 0), a.h - 1) * (size_t)a.w;
      inside[p] = word[p] = 0u;
#pragma unroll
      for (int m = 0; m < 4; m++) {
        const int c = cj + m;
        if (row_in && c >= 0 && c < a.w) inside[p] |= 1u << (8 * m);
        cat[p][m] = row_at + (size_t)min(max(c, 0), a.w - 1);
      }
    }
#pragma unroll 1
    for (int f = 0; f < nf; f++) {
      const TS* __restrict__ base = reinterpret_cast<const TS*>(lds.frame[f]);
      float cx[CLIP_PER][4];
#pragma unroll
      for (int p = 0; p < CLIP_PER; p++)
#pragma unroll
        for (int m = 0; m < 4; m++) cx[p][m] = ld<TS>(base, cat[p][m]);
#pragma unroll
      for (int p = 0; p < CLIP_PER; p++) {
        uint32_t clipped = 0u;
#pragma unroll
        for (int m = 0; m < 4; m++) clipped |= (cx[p][m] < a.clip ? 0u : 1u) << (8 * m);
        word[p] |= (clipped & inside[p]) << f;
      }
    }
#pragma unroll
    for (int p = 0; p < CLIP_PER; p++)
      if (tid + p * HD_THREADS < CLIP_UNITS) lds.clip[tid + p * HD_THREADS] = word[p];
  }
  __syncthreads();

  const HdRow r0 = hd_row(a.model, 0), r1 = hd_row(a.model, 1), r2 = hd_row(a.model, 2);
  // the model rows of the even and the odd columns of frame row i (every unit starts at an even column)
  auto rows_of = [&](int i, HdRow& even, HdRow& odd) {
    const uint32_t pair = (a.pattern >> (4u * ((uint32_t)i & 1u))) & 15u;
    even = hd_pick((int)(pair & 3u), r0, r1, r2);
    odd = hd_pick((int)(pair >> 2), r0, r1, r2);
  };

  // ---- 2. anchors: the interior group of the lane ...
  const int ty = tid / HD_GROUPS, gx = tid % HD_GROUPS;
  const int i = y0 + ty, j0 = x0 + HD_GROUP * gx;
  const int live = i < a.h ? min(max(a.w - j0, 0), HD_GROUP) : 0;
  const size_t at = (size_t)i * (size_t)a.w + (size_t)j0;   // (not formed into an address unless live > 0)
  HdRow even, odd;
  rows_of(i, even, odd);
  HdSites<HD_GROUP> in;
  hd_anchor<TS, HD_GROUP, R>(lds, nf, ref, lo, ty + R, (HD_SIDE + HD_GROUP * gx) / 4, at, live, even, odd, a.v_min, in);

  // ... and its apron unit: R rows above, R rows below (whole staged rows), one unit left and right of each tile row
  const bool apron = tid < 2 * R * HD_UNITS + 2 * HD_TH;
  int srow = 0, unit = 0, alive = 0;
  size_t aat = 0;
  HdRow aeven = even, aodd = odd;
  HdSites<4> ap;
  if (apron) {
    if (tid < 2 * R * HD_UNITS) {
      const int band = tid / (R * HD_UNITS), u = tid - band * (R * HD_UNITS);
      srow = band * (R + HD_TH) + u / HD_UNITS;
      unit = u % HD_UNITS;
    } else {
      const int u = tid - 2 * R * HD_UNITS;
      srow = R + (u >> 1);
      unit = (u & 1) ? HD_UNITS - 1 : 0;
    }
    const int ai = y0 - R + srow, aj = x0 - HD_SIDE + 4 * unit;
    alive = (ai >= 0 && ai < a.h && aj >= 0) ? min(max(a.w - aj, 0), 4) : 0;
    aat = (size_t)max(ai, 0) * (size_t)a.w + (size_t)max(aj, 0);   // (not formed into an address unless alive > 0)
    rows_of(ai, aeven, aodd);
    hd_anchor<TS, 4, R>(lds, nf, ref, lo, srow, unit, aat, alive, aeven, aodd, a.v_min, ap);
  }

  // ---- 3. the frames
  float num[HD_GROUP], den[HD_GROUP];
  uint32_t count[HD_GROUP / 4] = {};
#pragma unroll
  for (int m = 0; m < HD_GROUP; m++) num[m] = den[m] = 0.0f;
#pragma unroll 1
  for (int f = 0; f < nf; f++) {
    const float kf = __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(lds.k[f])));   // the same value in every lane: a scalar
    const bool pow2 = (__float_as_uint(kf) & 0x007fffffu) == 0u && kf >= 1.0f && kf <= 0x1p60f;
    const TS* __restrict__ src = reinterpret_cast<const TS*>(lds.frame[f]);
    float r[HD_GROUP], u[HD_GROUP];
    {
      float x[HD_GROUP], e[HD_GROUP], v[HD_GROUP];
#pragma unroll
      for (int m = 0; m < HD_GROUP; m++) x[m] = 0.0f;
      if (live > 0) hd_fetch<TS, HD_GROUP>(src, at, live, x);
      if (pow2) hd_site<HD_GROUP, true>(x, in, f, kf, even, odd, a.v_min, r, u, e, v);
      else hd_site<HD_GROUP, false>(x, in, f, kf, even, odd, a.v_min, r, u, e, v);
      const int to = (ty + R) * HD_SW + HD_SIDE + HD_GROUP * gx;
      hd_store<HD_GROUP>(lds.e + to, e);
      hd_store<HD_GROUP>(lds.v + to, v);
    }
    if (apron) {
      float ax[4] = {0.0f, 0.0f, 0.0f, 0.0f}, ar[4], au[4], e[4], v[4];
      if (alive > 0) hd_fetch<TS, 4>(src, aat, alive, ax);
      if (pow2) hd_site<4, true>(ax, ap, f, kf, aeven, aodd, a.v_min, ar, au, e, v);
      else hd_site<4, false>(ax, ap, f, kf, aeven, aodd, a.v_min, ar, au, e, v);
      hd_store<4>(lds.e + srow * HD_SW + 4 * unit, e);
      hd_store<4>(lds.v + srow * HD_SW + 4 * unit, v);
    }
    __syncthreads();

    // row sums: four columns of a staged row per step
#pragma unroll 1
    for (int t = tid; t < (HD_TH + 2 * R) * (HD_TW / 4); t += HD_THREADS) {
      const int rrow = t / (HD_TW / 4), cu = t % (HD_TW / 4);
      float we[12], wv[12];
      hd_load<12>(lds.e + rrow * HD_SW + 4 * cu, we);   // staged columns 4 cu .. 4 cu + 11: tile columns 4 cu - 4 .. 4 cu + 7
      hd_load<12>(lds.v + rrow * HD_SW + 4 * cu, wv);
      float se[4], sv[4];
#pragma unroll
      for (int m = 0; m < 4; m++) {
        float e = 0.0f, v = 0.0f;
#pragma unroll
        for (int k = -R; k <= R; k++) e += we[4 + m + k], v += wv[4 + m + k];
        se[m] = e, sv[m] = v;
      }
      hd_store<4>(lds.re + rrow * HD_TW + 4 * cu, se);
      hd_store<4>(lds.rv + rrow * HD_TW + 4 * cu, sv);
    }
    __syncthreads();

    // column sums and the weight of frame f
    if (live > 0) {
      float E[HD_GROUP], V[HD_GROUP];
#pragma unroll
      for (int m = 0; m < HD_GROUP; m++) E[m] = V[m] = 0.0f;
#pragma unroll 1
      for (int dr = 0; dr <= 2 * R; dr++) {
        float pe[HD_GROUP], pv[HD_GROUP];
        hd_load<HD_GROUP>(lds.re + (ty + dr) * HD_TW + HD_GROUP * gx, pe);
        hd_load<HD_GROUP>(lds.rv + (ty + dr) * HD_TW + HD_GROUP * gx, pv);
#pragma unroll
        for (int m = 0; m < HD_GROUP; m++) E[m] += pe[m], V[m] += pv[m];
      }
      float e[HD_GROUP], v[HD_GROUP];   // of the lane's own sites, as staged
      hd_load<HD_GROUP>(lds.e + (ty + R) * HD_SW + HD_SIDE + HD_GROUP * gx, e);
      hd_load<HD_GROUP>(lds.v + (ty + R) * HD_SW + HD_SIDE + HD_GROUP * gx, v);
#pragma unroll
      for (int m = 0; m < HD_GROUP; m++) {
        const HdRow& row = (m & 1) ? odd : even;
        const uint32_t meta = hd_byte<HD_GROUP>(in.meta, m);
        const float t = E[m] / V[m];
        float s = fminf(fmaxf((a.t_hi - t) * a.inv, 0.0f), 1.0f);
        if (e[m] > a.c2 * v[m]) s = 0.0f;
        if (!row.valid || (int)(meta & 7u) == f) s = 1.0f;
        const bool sat = ((hd_byte<HD_GROUP>(in.sat, m) >> f) & 1u) != 0u;
        const float w = sat ? 0.0f : s / u[m];
        if (w > 0.0f) {
          num[m] += w * r[m];
          den[m] += w;
          count[m / 4] += 1u << (8 * (m % 4));
        }
      }
    }
    // (no barrier here: after the second barrier above a lane reads of e and v only what it staged itself, and the next frame's row
    // sums are written behind that frame's first barrier, which every lane reaches with its column sums done)
  }

  // ---- 4. the result
  if (live > 0) {
    float y[HD_GROUP];
#pragma unroll
    for (int m = 0; m < HD_GROUP; m++) y[m] = den[m] > 0.0f ? num[m] / den[m] : in.R[m];
    hd_put<TO, HD_GROUP>(out, at, live, y);
    if (a.mask) {
      static_assert(HD_GROUP == 4, "the mask bytes of a lane are one word");
      const uint32_t bytes = in.meta[0] | (count[0] << 4);
      unsigned char* p = a.mask + at;
      if (live == HD_GROUP && (reinterpret_cast<uintptr_t>(p) & 3u) == 0) *reinterpret_cast<uint32_t*>(p) = bytes;
      else {
#pragma unroll
        for (int m = 0; m < HD_GROUP; m++)
          if (m < live) p[m] = (unsigned char)((bytes >> (8 * m)) & 0xffu);
      }
    }
  }
}

bool hd_pattern_ok(uint32_t pattern) {
  return pattern == TDK_PATTERN_RGGB || pattern == TDK_PATTERN_BGGR || pattern == TDK_PATTERN_GRBG || pattern == TDK_PATTERN_GBRG;
}
bool hd_dtype_ok(int dtype) { return dtype == TDK_F32 || dtype == TDK_F16; }

template <typename TS, typename TO, int R> int hd_launch(const HdArgs& a, hipStream_t st) {
  const dim3 grid((unsigned)tdk_div_up(a.w, HD_TW), (unsigned)tdk_div_up(a.h, HD_TH)), block(HD_THREADS);
  TDK_LAUNCH("tdk_hdr_merge", (hd_merge<TS, TO, R>), grid, block, 0, st, a);
  return TDK_OK;
}

template <typename TS, typename TO> int hd_launch_radius(const HdArgs& a, int radius, hipStream_t st) {
  return radius == 2 ? hd_launch<TS, TO, 2>(a, st) : hd_launch<TS, TO, 3>(a, st);
}

template <typename TS> int hd_launch_out(const HdArgs& a, int out_dtype, int radius, hipStream_t st) {
  return out_dtype == TDK_F32 ? hd_launch_radius<TS, float>(a, radius, st) : hd_launch_radius<TS, __half>(a, radius, st);
}

}  // namespace

TDK_EXPORT int tdk_hdr_abi_version(void) { return TDK_HDR_ABI_VERSION; }

TDK_EXPORT size_t tdk_hdr_lds_bytes(int radius) { return radius == 2 ? sizeof(HdLds<2>) : radius == 3 ? sizeof(HdLds<3>) : 0; }

TDK_EXPORT int tdk_hdr_merge(const void* const* frames, int num_frames, int src_dtype, void* out, int out_dtype, unsigned char* mask, int width, int height,
                             uint32_t pattern, const float* exposures, int ref, const float* model, int radius, float clip, float t_lo, float t_hi,
                             float pixel_c2, float v_min, tdk_stream_t stream) {
  static const char* const who = "tdk_hdr_merge";
  TDK_REQUIRE(frames && out && exposures && model, "%s: null pointer (frames, out, exposures or model)", who);
  TDK_REQUIRE(num_frames >= 2 && num_frames <= HD_F, "%s: num_frames must be 2..%d, got %d", who, HD_F, num_frames);
  for (int f = 0; f < num_frames; f++) TDK_REQUIRE(frames[f], "%s: null pointer (frame %d)", who, f);
  TDK_REQUIRE(hd_dtype_ok(src_dtype) && hd_dtype_ok(out_dtype), "%s: unsupported dtype tags %d -> %d", who, src_dtype, out_dtype);
  TDK_REQUIRE(width >= 2 && height >= 2 && width <= HD_MAX_SIZE && height <= HD_MAX_SIZE, "%s: frame size %dx%d outside 2..%d", who, width, height, HD_MAX_SIZE);
  TDK_REQUIRE(width % 2 == 0 && height % 2 == 0, "%s: mosaic size %dx%d must be even in both axes (whole CFA cells)", who, width, height);
  TDK_REQUIRE(hd_pattern_ok(pattern), "%s: unknown Bayer pattern 0x%08x", who, pattern);
  TDK_REQUIRE(radius == 2 || radius == 3, "%s: radius must be 2 or 3, got %d", who, radius);
  TDK_REQUIRE(ref >= -1 && ref < num_frames, "%s: ref must be -1 or a frame index below %d, got %d", who, num_frames, ref);
  TDK_REQUIRE(isfinite(clip) && clip > 0.0f, "%s: clip must be finite and > 0", who);
  const float inv = 1.0f / (t_hi - t_lo);
  TDK_REQUIRE(isfinite(t_lo) && isfinite(t_hi) && t_lo > 0.0f && t_hi > t_lo && isfinite(inv),
              "%s: the thresholds need 0 < t_lo < t_hi, finite, with a finite 1 / (t_hi - t_lo)", who);
  TDK_REQUIRE(pixel_c2 > 0.0f, "%s: pixel_c2 must be > 0 (+inf turns the per-site test off)", who);
  TDK_REQUIRE(isfinite(v_min) && v_min > 0.0f, "%s: v_min must be finite and > 0", who);
  const size_t sites = (size_t)width * (size_t)height;
  const size_t src_bytes = sites * tdk_dtype_bytes(src_dtype), out_bytes = sites * tdk_dtype_bytes(out_dtype);
  const size_t exp_bytes = (size_t)num_frames * sizeof(float);
  for (int f = 0; f < num_frames; f++)
    TDK_REQUIRE(tdk_disjoint(frames[f], src_bytes, out, out_bytes) && (!mask || tdk_disjoint(frames[f], src_bytes, mask, sites)),
                "%s: out or mask overlaps frame %d", who, f);
  TDK_REQUIRE(tdk_disjoint(exposures, exp_bytes, out, out_bytes) && tdk_disjoint(model, 48, out, out_bytes) &&
                  (!mask || (tdk_disjoint(exposures, exp_bytes, mask, sites) && tdk_disjoint(model, 48, mask, sites))),
              "%s: the exposures or the model overlap out or mask", who);
  TDK_REQUIRE(!mask || tdk_disjoint(out, out_bytes, mask, sites), "%s: out and mask overlap", who);

  HdArgs a{};
  for (int f = 0; f < num_frames; f++) a.frames[f] = frames[f];
  a.out = out, a.mask = mask, a.exposures = exposures, a.model = model;
  a.nf = num_frames, a.ref = ref, a.w = width, a.h = height, a.pattern = pattern;
  a.clip = clip, a.t_hi = t_hi, a.inv = inv, a.c2 = pixel_c2, a.v_min = v_min;
  hipStream_t st = tdk_stream(stream);
  return src_dtype == TDK_F32 ? hd_launch_out<float>(a, out_dtype, radius, st) : hd_launch_out<__half>(a, out_dtype, radius, st);
}
