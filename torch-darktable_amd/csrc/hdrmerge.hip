// hdrmerge.hip -- the noise-weighted merge of an exposure bracket of raw mosaics (include/tdk_hip_hdr.h: tdk_hdr_merge, one tile launch).
//
// The specification is the head comment of include/tdk_hip_hdr.h.  The storage helpers, the rows of the noise model, the tile geometry
// with its apron mapping and staged LDS planes, the column sums and the threshold step are those of the temporal filters:
// tdk_mosaic_tile.h, with a tile of 32 x 32 sites and four sites per lane.  The row sums are that header's too, but written out in the
// frame loop (the reason stands there).  Steps 0 to 2 and 4 and the arithmetic of a site in a frame are this file's own.
//
// hd_merge<TS, TO, R>: a workgroup of 256 lanes owns an output tile of 32 rows of 32 sites (HdTile<R>).  A lane takes four
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
#include "../../include/tdk_hip_hdr.h"
#include "tdk_mosaic_tile.h"

namespace {

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
__device__ __forceinline__ void hd_anchor(const HdLds<R>& lds, int nf, int ref, int lo, int srow, int unit0, size_t at, int live, const MtRow& even,
                                          const MtRow& odd, float v_min, HdSites<M>& s) {
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

template <typename TS, typename TO, int R>
__global__ __launch_bounds__(MT_THREADS, HD_WAVES) void hd_merge(HdArgs a) {
  using G = HdTile<R>;
  constexpr int GROUP = G::GROUP;
  __shared__ HdLds<R> lds;
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
  hd_anchor<TS, GROUP, R>(lds, nf, ref, lo, ty + R, (G::SIDE + GROUP * gx) / 4, at, live, even, odd, a.v_min, in);

  // ... and its apron unit: R rows above, R rows below (whole staged rows), one unit left and right of each tile row
  const bool apron = tid < G::APRON;
  int srow = 0, unit = 0, alive = 0;
  size_t aat = 0;
  MtRow aeven = even, aodd = odd;
  HdSites<4> ap;
  if (apron) {
    G::apron_unit(tid, srow, unit);
    const int ai = y0 - R + srow, aj = x0 - G::SIDE + 4 * unit;
    alive = (ai >= 0 && ai < a.h && aj >= 0) ? min(max(a.w - aj, 0), 4) : 0;
    aat = (size_t)max(ai, 0) * (size_t)a.w + (size_t)max(aj, 0);   // (not formed into an address unless alive > 0)
    mt_rows_of(a.pattern, ai, r0, r1, r2, aeven, aodd);
    hd_anchor<TS, 4, R>(lds, nf, ref, lo, srow, unit, aat, alive, aeven, aodd, a.v_min, ap);
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
    float r[GROUP], u[GROUP];
    {
      float x[GROUP], e[GROUP], v[GROUP];
#pragma unroll
      for (int m = 0; m < GROUP; m++) x[m] = 0.0f;
      if (live > 0) mt_fetch<TS, GROUP>(src, (int64_t)at, 0, live, x);
      if (pow2) hd_site<GROUP, true>(x, in, f, kf, even, odd, a.v_min, r, u, e, v);
      else hd_site<GROUP, false>(x, in, f, kf, even, odd, a.v_min, r, u, e, v);
      mt_store<GROUP>(lds.t.e + G::staged(ty, gx), e);
      mt_store<GROUP>(lds.t.v + G::staged(ty, gx), v);
    }
    if (apron) {
      float ax[4] = {0.0f, 0.0f, 0.0f, 0.0f}, ar[4], au[4], e[4], v[4];
      if (alive > 0) mt_fetch<TS, 4>(src, (int64_t)aat, 0, alive, ax);
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

template <typename TS, typename TO, int R> int hd_launch(const HdArgs& a, hipStream_t st) {
  const dim3 grid((unsigned)tdk_div_up(a.w, HdTile<R>::TW), (unsigned)tdk_div_up(a.h, HdTile<R>::TH)), block(MT_THREADS);
  TDK_LAUNCH("tdk_hdr_merge", (hd_merge<TS, TO, R>), grid, block, 0, st, a);
  return TDK_OK;
}

template <typename TS, typename TO> int hd_launch_radius(const HdArgs& a, int radius, hipStream_t st) {
  return radius == 2 ? hd_launch<TS, TO, 2>(a, st) : hd_launch<TS, TO, 3>(a, st);
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
  TDK_REQUIRE(mt_dtype_ok(src_dtype) && mt_dtype_ok(out_dtype), "%s: unsupported dtype tags %d -> %d", who, src_dtype, out_dtype);
  if (const int rc = mt_check_mosaic(who, width, height, pattern, radius)) return rc;
  TDK_REQUIRE(ref >= -1 && ref < num_frames, "%s: ref must be -1 or a frame index below %d, got %d", who, num_frames, ref);
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

  HdArgs a{};
  for (int f = 0; f < num_frames; f++) a.frames[f] = frames[f];
  a.out = out, a.mask = mask, a.exposures = exposures, a.model = model;
  a.nf = num_frames, a.ref = ref, a.w = width, a.h = height, a.pattern = pattern;
  a.clip = clip, a.t_hi = t_hi, a.inv = inv, a.c2 = pixel_c2, a.v_min = v_min;
  hipStream_t st = tdk_stream(stream);
  TDK_DISPATCH_DTYPE(src_dtype, TS, TDK_DISPATCH_DTYPE(out_dtype, TO, return hd_launch_radius<TS, TO>(a, radius, st)));
  return TDK_OK;
}
