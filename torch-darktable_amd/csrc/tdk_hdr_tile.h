// tdk_hdr_tile.h -- the tile body of the exposure-bracket merge (include/tdk_hip_hdr.h), shared by hd_merge of hdrmerge.hip and
// ha_merge of hdralign.hip (include/tdk_hip_hdralign.h), with its arguments and the checks of the two entry points.  The two kernels
// differ in one thing: where the sample of a frame at a site is read.  That is a type (HdInPlace, HdDisplaced), so the plain merge pays
// nothing for the aligned one.  The steps of the body are listed at the head of hdrmerge.hip.  It launches nothing.
#pragma once

#include "../../include/tdk_hip_hdr.h"
#include "tdk_mosaic_tile.h"

template <int R> using HdTile = MtTile<TDK_HDR_TILE_W, TDK_HDR_TILE_H, 4, R>;   // four sites of a lane in the interior
constexpr int HD_F = TDK_HDR_MAX_FRAMES;
static_assert(HdTile<3>::SIDE >= 3 + 1, "the apron of the largest radius and the rim of the clip bits");
static_assert(HD_F <= 8, "a clip bit per frame in a byte");

template <int R> struct HdLds {
  typename HdTile<R>::Lds t;                                                   // the staged planes and their row sums
  alignas(16) uint32_t clip[(HdTile<R>::ROWS + 2) * HdTile<R>::UNITS];         // a byte per site, four sites a word: one row more on either side
  alignas(16) const void* frame[HD_F];
  float k[HD_F];
};
static_assert(sizeof(HdLds<3>) <= 64 * 1024, "LDS of the merge launch");
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

// ---- where the sample of frame f at a site is read.  The plain merge reads it at the site.
struct HdInPlace {
  static constexpr bool ALIGNED = false;
};
// The aligned merge reads it (dy[f], dx[f]) further on, the displacement of the output tile of the workgroup: the same for every site
// the workgroup touches, so a frame is still fetched at one uniform offset.  dy and dx are LDS arrays of HD_F entries that step 0 of the
// body fills from the fields (tdk_hip_hdralign.h: (dy, dx) of a motion tile as one word, dy in the low half; odd values masked; the row
// of ref reads as 0 and is not read).
struct HdDisplaced {
  static constexpr bool ALIGNED = true;
  static constexpr int TILE_W = 64, TILE_H = 32;   // the motion tile (hdralign.hip holds them to tdk_hip_motion.h): whole output tiles
  static_assert(TILE_W % TDK_HDR_TILE_W == 0 && TILE_H % TDK_HDR_TILE_H == 0, "an output tile lies inside one motion tile");
  int* dy;
  int* dx;
  const uint32_t* fields;
  int tiles_x, tiles_y;   // motion tiles of the frame
};

// byte m of a run of sites packed four to a word
template <int M> __device__ __forceinline__ uint32_t hd_byte(const uint32_t (&w)[M / 4], int m) { return (w[m / 4] >> (8 * (m % 4))) & 0xffu; }

// What a lane keeps of M of its sites: R, u_g, and packed a byte per site the saturation bits and g | blown << 3.
template <int M> struct HdSites {
  float R[M], ug[M];
  uint32_t sat[M / 4], meta[M / 4];
};

// The elements lo <= m < hi of the `live` sites from (i, j0) whose sample of a frame displaced by (dy, dx) lies inside the frame, and
// the element `fat` of the first site's sample (a place in the plane for lo <= m < hi only).
__device__ __forceinline__ void hd_displaced(int i, int j0, size_t at, int live, int dy, int dx, int w, int h, int& lo, int& hi, int64_t& fat) {
  const int row = i + dy, col = j0 + dx;
  lo = hi = 0;
  fat = 0;
  if (live <= 0 || row < 0 || row >= h) return;
  lo = max(0, -col), hi = min(live, w - col);
  if (hi <= lo) {
    lo = hi = 0;
    return;
  }
  fat = (int64_t)at + (int64_t)dy * (int64_t)w + (int64_t)dx;
}

// Step 2 for the M sites from staged unit `unit0` of staged row `srow`; `live` of them are inside the frame, from element `at` on, which
// is site (i, j0).  A site outside the frame is marked blown: it takes no part in any window.
template <typename TS, int M, int R, typename D>
__device__ __forceinline__ void hd_anchor(const HdLds<R>& lds, const D& disp, int nf, int ref, int lo, int srow, int unit0, size_t at, int i, int j0, int w, int h,
                                          int live, const MtRow& even, const MtRow& odd, float v_min, HdSites<M>& s) {
  constexpr int W = M / 4, UNITS = HdTile<R>::UNITS;
  // the OR of the three rows around the sites, one word further on either side (a word outside the plane holds no site of the apron)
  uint32_t col[W + 2];
#pragma unroll
  for (int k = 0; k < W + 2; k++) {
    const int u = unit0 - 1 + k;
    const bool in = u >= 0 && u < UNITS;
    const int c = srow * UNITS + (in ? u : 0);   // plane row srow is the row above staged row srow
    const uint32_t three = lds.clip[c] | lds.clip[c + UNITS] | lds.clip[c + 2 * UNITS];
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
  // the aligned merge: a blown site takes frame lo where its displaced sample is inside the frame, else ref (which is not displaced)
  int blown_row = 0, blown_col = 0;   // of the sample of frame lo at element 0
  if constexpr (D::ALIGNED) blown_row = i + disp.dy[lo], blown_col = j0 + disp.dx[lo];
#pragma unroll
  for (int m = 0; m < M; m++) {
    const bool use_ref = ((hd_byte<M>(s.sat, m) >> ref) & 1u) == 0u;
    g[m] = use_ref ? ref : best[m];
    kg[m] = use_ref ? k_ref : bk[m];
    if (g[m] < 0) {   // blown
      g[m] = lo, kg[m] = k_lo;
      if constexpr (D::ALIGNED) {
        const bool inside = blown_row >= 0 && blown_row < h && blown_col + m >= 0 && blown_col + m < w;
        if (!inside) g[m] = ref, kg[m] = k_ref;
      }
      s.meta[m / 4] |= 8u << (8 * (m % 4));
    }
    xg[m] = 0.0f;
  }
  if (live > 0) {
    // one sample per site from the frame it chose; a site outside the frame reads the last one inside, so that the loads do not wait for
    // one another
    if constexpr (D::ALIGNED) {
      // (the anchor of a site inside the frame is not clipped there, or is the frame rule 5 found inside: its displaced sample is a place
      // in the plane; a site outside the frame reads the last one inside as frame ref has it)
#pragma unroll
      for (int m = 0; m < M; m++) {
        const int gl = m < live ? g[m] : ref;
        const int64_t off = (int64_t)disp.dy[gl] * (int64_t)w + (int64_t)disp.dx[gl];
        xg[m] = ld<TS>(reinterpret_cast<const TS*>(lds.frame[gl]), (size_t)((int64_t)at + (int64_t)min(m, live - 1) + off));
      }
    } else {
#pragma unroll
      for (int m = 0; m < M; m++) xg[m] = ld<TS>(reinterpret_cast<const TS*>(lds.frame[g[m]]), at + (size_t)min(m, live - 1));
    }
  }
#pragma unroll
  for (int m = 0; m < M; m++) {
    if (m < live) {
      const MtRow& r = (m & 1) ? odd : even;
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
__device__ __forceinline__ void hd_site(const float x[M], const HdSites<M>& s, int f, float kf, const MtRow& even, const MtRow& odd, float v_min, float r[M],
                                        float u[M], float e[M], float v[M]) {
  const float kk = kf * kf;
  const float ik = 1.0f / kf, ikk = 1.0f / kk;   // (used when exact)
#pragma unroll
  for (int m = 0; m < M; m++) {
    const MtRow& row = (m & 1) ? odd : even;
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

template <typename TS, typename TO, int R, typename D> __device__ __forceinline__ void hd_merge_tile(HdLds<R>& lds, const HdArgs& a, const D& disp) {
  using G = HdTile<R>;
  constexpr int GROUP = G::GROUP;
  const int tid = threadIdx.x;
  const int x0 = (int)blockIdx.x * G::TW, y0 = (int)blockIdx.y * G::TH;
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
  if constexpr (D::ALIGNED) {
    // the displacement of every frame at this output tile: the motion tile it lies in
    if (tid < HD_F) {
      int dy = 0, dx = 0;
      if (tid < nf && tid != ref) {
        const size_t tile = ((size_t)tid * (size_t)disp.tiles_y + (size_t)(y0 / D::TILE_H)) * (size_t)disp.tiles_x + (size_t)(x0 / D::TILE_W);
        const uint32_t word = disp.fields[tile];
        dy = (int)(int16_t)(word & 0xffffu) & ~1, dx = (int)(int16_t)(word >> 16) & ~1;
      }
      disp.dy[tid] = dy, disp.dx[tid] = dx;
    }
  }
  if (tid == MT_THREADS - 1) {
#pragma unroll
    for (int f = 0; f < HD_F; f++) lds.frame[f] = a.frames[f];
  }
  __syncthreads();

  // ---- 1. clip bits on the tile and R + 1 sites around it (columns: the whole staged row).  A lane takes CLIP_PER units.  Every address
  // is clamped into the frame and a site outside it is masked afterwards, so that no load hangs on a condition: the loads of a frame are
  // all in flight before the first comparison, one latency per frame instead of one per unit and frame.
  {
    constexpr int CLIP_UNITS = (G::ROWS + 2) * G::UNITS, CLIP_PER = (CLIP_UNITS + MT_THREADS - 1) / MT_THREADS;
    if constexpr (D::ALIGNED) {
      // the sample of frame f is the one (dy, dx) further on, clamped into the frame like the site; a sample outside the frame counts as
      // clipped: the predicate is a bit beside the comparison
      int ci[CLIP_PER], cj[CLIP_PER];
      uint32_t inside[CLIP_PER], word[CLIP_PER];
#pragma unroll
      for (int p = 0; p < CLIP_PER; p++) {
        const int t = tid + p * MT_THREADS;
        const int prow = t / G::UNITS, unit = t % G::UNITS;
        ci[p] = y0 - (R + 1) + prow, cj[p] = x0 - G::SIDE + 4 * unit;
        const bool row_in = t < CLIP_UNITS && ci[p] >= 0 && ci[p] < a.h;
        inside[p] = word[p] = 0u;
#pragma unroll
        for (int m = 0; m < 4; m++)
          if (row_in && cj[p] + m >= 0 && cj[p] + m < a.w) inside[p] |= 1u << (8 * m);
      }
#pragma unroll 1
      for (int f = 0; f < nf; f++) {
        const TS* __restrict__ base = reinterpret_cast<const TS*>(lds.frame[f]);
        const int dy = __builtin_amdgcn_readfirstlane(disp.dy[f]), dx = __builtin_amdgcn_readfirstlane(disp.dx[f]);
        float cx[CLIP_PER][4];
        uint32_t away[CLIP_PER];
#pragma unroll
        for (int p = 0; p < CLIP_PER; p++) {
          const int row = ci[p] + dy;
          const bool row_in = row >= 0 && row < a.h;
          const size_t row_at = (size_t)min(max(row, 0), a.h - 1) * (size_t)a.w;
          away[p] = 0u;
#pragma unroll
          for (int m = 0; m < 4; m++) {
            const int c = cj[p] + m + dx;
            if (!(row_in && c >= 0 && c < a.w)) away[p] |= 1u << (8 * m);
            cx[p][m] = ld<TS>(base, row_at + (size_t)min(max(c, 0), a.w - 1));
          }
        }
#pragma unroll
        for (int p = 0; p < CLIP_PER; p++) {
          uint32_t clipped = away[p];
#pragma unroll
          for (int m = 0; m < 4; m++) clipped |= (cx[p][m] < a.clip ? 0u : 1u) << (8 * m);
          word[p] |= (clipped & inside[p]) << f;
        }
      }
#pragma unroll
      for (int p = 0; p < CLIP_PER; p++)
        if (tid + p * MT_THREADS < CLIP_UNITS) lds.clip[tid + p * MT_THREADS] = word[p];
    } else {
      size_t cat[CLIP_PER][4];
      uint32_t inside[CLIP_PER], word[CLIP_PER];
#pragma unroll
      for (int p = 0; p < CLIP_PER; p++) {
        const int t = tid + p * MT_THREADS;
        const int prow = t / G::UNITS, unit = t % G::UNITS;
        const int ci = y0 - (R + 1) + prow, cj = x0 - G::SIDE + 4 * unit;
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
        if (tid + p * MT_THREADS < CLIP_UNITS) lds.clip[tid + p * MT_THREADS] = word[p];
    }
  }
  __syncthreads();

  const MtRow r0 = mt_row_or_unit(a.model, 0), r1 = mt_row_or_unit(a.model, 1), r2 = mt_row_or_unit(a.model, 2);

  // ---- 2. anchors: the interior group of the lane ...
  const int ty = tid / G::GROUPS, gx = tid % G::GROUPS;
  const int i = y0 + ty, j0 = x0 + GROUP * gx;
  const int live = i < a.h ? min(max(a.w - j0, 0), GROUP) : 0;
  const size_t at = (size_t)i * (size_t)a.w + (size_t)j0;   // (not formed into an address unless live > 0)
  MtRow even, odd;
  mt_rows_of(a.pattern, i, r0, r1, r2, even, odd);
  HdSites<GROUP> in;
  hd_anchor<TS, GROUP, R>(lds, disp, nf, ref, lo, ty + R, (G::SIDE + GROUP * gx) / 4, at, i, j0, a.w, a.h, live, even, odd, a.v_min, in);

  // ... and its apron unit: R rows above, R rows below (whole staged rows), one unit left and right of each tile row
  const bool apron = tid < G::APRON;
  int srow = 0, unit = 0, alive = 0, ai = 0, aj = 0;
  size_t aat = 0;
  MtRow aeven = even, aodd = odd;
  HdSites<4> ap;
  if (apron) {
    G::apron_unit(tid, srow, unit);
    ai = y0 - R + srow, aj = x0 - G::SIDE + 4 * unit;
    alive = (ai >= 0 && ai < a.h && aj >= 0) ? min(max(a.w - aj, 0), 4) : 0;
    aat = (size_t)max(ai, 0) * (size_t)a.w + (size_t)max(aj, 0);   // (not formed into an address unless alive > 0)
    mt_rows_of(a.pattern, ai, r0, r1, r2, aeven, aodd);
    hd_anchor<TS, 4, R>(lds, disp, nf, ref, lo, srow, unit, aat, ai, aj, a.w, a.h, alive, aeven, aodd, a.v_min, ap);
  }

  // ---- 3. the frames
  float num[GROUP], den[GROUP];
  uint32_t count[GROUP / 4] = {};
#pragma unroll
  for (int m = 0; m < GROUP; m++) num[m] = den[m] = 0.0f;
#pragma unroll 1
  for (int f = 0; f < nf; f++) {
    const float kf = __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(lds.k[f])));   // the same value in every lane: a scalar
    const bool pow2 = (__float_as_uint(kf) & 0x007fffffu) == 0u && kf >= 1.0f && kf <= 0x1p60f;
    const TS* __restrict__ src = reinterpret_cast<const TS*>(lds.frame[f]);
    int dy = 0, dx = 0;
    if constexpr (D::ALIGNED) dy = __builtin_amdgcn_readfirstlane(disp.dy[f]), dx = __builtin_amdgcn_readfirstlane(disp.dx[f]);
    float r[GROUP], u[GROUP];
    {
      float x[GROUP], e[GROUP], v[GROUP];
#pragma unroll
      for (int m = 0; m < GROUP; m++) x[m] = 0.0f;
      if constexpr (D::ALIGNED) {
        // (a site whose sample lies outside the frame is saturated in f: what it reads as is never used)
        int flo, fhi;
        int64_t fat;
        hd_displaced(i, j0, at, live, dy, dx, a.w, a.h, flo, fhi, fat);
        if (fhi > flo) mt_fetch<TS, GROUP>(src, fat, flo, fhi, x);
      } else {
        if (live > 0) mt_fetch<TS, GROUP>(src, (int64_t)at, 0, live, x);
      }
      if (pow2) hd_site<GROUP, true>(x, in, f, kf, even, odd, a.v_min, r, u, e, v);
      else hd_site<GROUP, false>(x, in, f, kf, even, odd, a.v_min, r, u, e, v);
      mt_store<GROUP>(lds.t.e + G::staged(ty, gx), e);
      mt_store<GROUP>(lds.t.v + G::staged(ty, gx), v);
    }
    if (apron) {
      float ax[4] = {0.0f, 0.0f, 0.0f, 0.0f}, ar[4], au[4], e[4], v[4];
      if constexpr (D::ALIGNED) {
        int flo, fhi;
        int64_t fat;
        hd_displaced(ai, aj, aat, alive, dy, dx, a.w, a.h, flo, fhi, fat);
        if (fhi > flo) mt_fetch<TS, 4>(src, fat, flo, fhi, ax);
      } else {
        if (alive > 0) mt_fetch<TS, 4>(src, (int64_t)aat, 0, alive, ax);
      }
      if (pow2) hd_site<4, true>(ax, ap, f, kf, aeven, aodd, a.v_min, ar, au, e, v);
      else hd_site<4, false>(ax, ap, f, kf, aeven, aodd, a.v_min, ar, au, e, v);
      mt_store<4>(lds.t.e + srow * G::SW + 4 * unit, e);
      mt_store<4>(lds.t.v + srow * G::SW + 4 * unit, v);
    }
    __syncthreads();

    // row sums: mt_row_sums of tdk_mosaic_tile.h, written out.  Behind any call, a local lambda included, the compiler builds this kernel
    // otherwise: the selects of hd_site become branches, 56 to 62 instructions more per instantiation, and the binary16 rows of
    // profiles/hdrmerge_bench.py take 1 to 2 % longer (profiles/r23/tile_layer_bench.txt).
#pragma unroll 1
    for (int t = tid; t < G::ROWS * (G::TW / 4); t += MT_THREADS) {
      const int rrow = t / (G::TW / 4), cu = t % (G::TW / 4);
      float we[12], wv[12];
      mt_load<12>(lds.t.e + rrow * G::SW + 4 * cu, we);   // staged columns 4 cu .. 4 cu + 11: tile columns 4 cu - 4 .. 4 cu + 7
      mt_load<12>(lds.t.v + rrow * G::SW + 4 * cu, wv);
      float se[4], sv[4];
#pragma unroll
      for (int m = 0; m < 4; m++) {
        float e = 0.0f, v = 0.0f;
#pragma unroll
        for (int k = -R; k <= R; k++) e += we[4 + m + k], v += wv[4 + m + k];
        se[m] = e, sv[m] = v;
      }
      mt_store<4>(lds.t.re + rrow * G::TW + 4 * cu, se);
      mt_store<4>(lds.t.rv + rrow * G::TW + 4 * cu, sv);
    }
    __syncthreads();

    // column sums and the weight of frame f
    if (live > 0) {
      float E[GROUP], V[GROUP];
      mt_column_sums<G>(lds.t, ty, gx, E, V);
      float e[GROUP], v[GROUP];   // of the lane's own sites, as staged
      mt_load<GROUP>(lds.t.e + G::staged(ty, gx), e);
      mt_load<GROUP>(lds.t.v + G::staged(ty, gx), v);
#pragma unroll
      for (int m = 0; m < GROUP; m++) {
        const MtRow& row = (m & 1) ? odd : even;
        const uint32_t meta = hd_byte<GROUP>(in.meta, m);
        float s = mt_similarity(E[m], V[m], e[m], v[m], a.t_hi, a.inv, a.c2);
        if (!row.valid || (int)(meta & 7u) == f) s = 1.0f;
        const bool sat = ((hd_byte<GROUP>(in.sat, m) >> f) & 1u) != 0u;
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
    float y[GROUP];
#pragma unroll
    for (int m = 0; m < GROUP; m++) y[m] = den[m] > 0.0f ? num[m] / den[m] : in.R[m];
    mt_put<TO, GROUP>(out, at, live, y);
    if (a.mask) {
      static_assert(GROUP == 4, "the mask bytes of a lane are one word");
      const uint32_t bytes = in.meta[0] | (count[0] << 4);
      unsigned char* p = a.mask + at;
      if (live == GROUP && (reinterpret_cast<uintptr_t>(p) & 3u) == 0) *reinterpret_cast<uint32_t*>(p) = bytes;
      else {
#pragma unroll
        for (int m = 0; m < GROUP; m++)
          if (m < live) p[m] = (unsigned char)((bytes >> (8 * m)) & 0xffu);
      }
    }
  }
}

// ---- host side: the checks of tdk_hdr_merge, which tdk_hdralign_merge shares (it refuses ref == -1: ref_min is 0), and the arguments
static inline int hd_check(const char* who, const void* const* frames, int num_frames, int src_dtype, void* out, int out_dtype, unsigned char* mask, int width,
                           int height, uint32_t pattern, const float* exposures, int ref, int ref_min, const float* model, int radius, float clip, float t_lo,
                           float t_hi, float pixel_c2, float v_min, HdArgs& a) {
  TDK_REQUIRE(frames && out && exposures && model, "%s: null pointer (frames, out, exposures or model)", who);
  TDK_REQUIRE(num_frames >= 2 && num_frames <= HD_F, "%s: num_frames must be 2..%d, got %d", who, HD_F, num_frames);
  for (int f = 0; f < num_frames; f++) TDK_REQUIRE(frames[f], "%s: null pointer (frame %d)", who, f);
  TDK_REQUIRE(mt_dtype_ok(src_dtype) && mt_dtype_ok(out_dtype), "%s: unsupported dtype tags %d -> %d", who, src_dtype, out_dtype);
  if (const int rc = mt_check_mosaic(who, width, height, pattern, radius)) return rc;
  if (ref_min < 0) TDK_REQUIRE(ref >= -1 && ref < num_frames, "%s: ref must be -1 or a frame index below %d, got %d", who, num_frames, ref);
  else TDK_REQUIRE(ref >= 0 && ref < num_frames, "%s: ref must be a frame index below %d (the host says which frame the others follow), got %d", who, num_frames, ref);
  TDK_REQUIRE(isfinite(clip) && clip > 0.0f, "%s: clip must be finite and > 0", who);
  float inv;
  if (const int rc = mt_check_thresholds(who, t_lo, t_hi, pixel_c2, inv)) return rc;
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

  for (int f = 0; f < num_frames; f++) a.frames[f] = frames[f];
  a.out = out, a.mask = mask, a.exposures = exposures, a.model = model;
  a.nf = num_frames, a.ref = ref, a.w = width, a.h = height, a.pattern = pattern;
  a.clip = clip, a.t_hi = t_hi, a.inv = inv, a.c2 = pixel_c2, a.v_min = v_min;
  return TDK_OK;
}
