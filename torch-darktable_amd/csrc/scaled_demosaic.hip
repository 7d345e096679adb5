// scaled_demosaic.hip -- raw mosaic -> reduced-size RGB frame (include/tdk_hip_scaled.h: tdk_demosaic_scaled,
// tdk_decode12_demosaic_scaled), one launch, no workspace.
//
// Along an axis tap j takes part in output i iff |N| < D with N = 2 n_out j + n_out - (2 i + 1) n_in and D = 2 n_in, and its weight
// is 1 - |N| / D.  N is formed in 64-bit once per output and stepped in 32-bit over its taps (|N| < D < 2^17), as resample.hip does.
//
// A workgroup of four waves owns TW x TH output pixels; TW is 64 (32 beyond 8:1) and TH follows from the vertical ratio, so that the
// source rows under the tile fit the LDS (sd_plan()).  It
//   1. builds the tap tables of its TW columns and TH rows in LDS: first tap, tap count, weights, and the weight sums Sx_0, Sx_1;
//   2. walks down its source footprint SD_SR rows at a time: the bytes of the rows are copied to LDS as they are stored -- as aligned
//      16-byte segments when the rows start on 16 bytes, element by element otherwise, the packed form included -- then every
//      (row, parity, column) chain A_p[y][i] is run over them into the float32 intermediate, FH x 2 x TW in LDS; neighbouring lanes
//      own neighbouring columns and write neighbouring words;
//   3. runs the four vertical chains B_qp of every output pixel over the intermediate (neighbouring lanes read neighbouring words),
//      combines them by the pattern and stores the three channels.
// The sample conversion (widening, 12-bit decode, white balance) happens where a chain reads its tap, with the expressions of
// codec.hip and postprocess.hip: the fused forms give the bits of the separate calls.
// Nothing is accumulated across lanes or workgroups: the bits do not depend on scheduling, on the tile or on the staging path.
#include "../../include/tdk_hip_scaled.h"
#include "tdk_frame.h"

namespace {

constexpr int SD_THREADS = 256;
constexpr int SD_SR = 8;                   // source rows staged per step
constexpr int SD_STAGE_SEGS = 136;         // 16-byte segments of a staged row: 529 float32 samples and the alignment slack on both sides
constexpr int SD_INTER_WORDS = 8192;       // A_0 and A_1 of the rows under a tile
constexpr int SD_MAX_TW = 64, SD_MAX_TH = 32;
constexpr int SD_WX_WORDS = 1024;          // 64 columns x 16 taps, or 32 x 32
constexpr int SD_WY_WORDS = 512;
enum { SD_F32 = 0, SD_F16 = 1, SD_P12 = 2, SD_P12_IDS = 3 };   // how the sites are stored

struct SdLds {
  uint4 stage[SD_SR][SD_STAGE_SEGS];
  float inter[SD_INTER_WORDS];
  float wx[SD_WX_WORDS], wy[SD_WY_WORDS];
  float sumx[2][SD_MAX_TW];
  int jx[SD_MAX_TW], cx[SD_MAX_TW];
  int jy[SD_MAX_TH], cy[SD_MAX_TH];
};
static_assert(sizeof(SdLds) <= 64 * 1024, "two workgroups per CU, and no raised LDS limit");

struct SdArgs {
  int sw, sh, dw, dh;
  int TW, TH;      // the output tile
  int KX, KY;      // tap-table depth
  int vec;         // rows start on 16 bytes: staged as 16-byte segments
  uint32_t pattern;
};

// The taps of output i: first source index, count, and N of the first tap (N steps by 2 n_out per tap, |N| < D = 2 n_in for every tap).
__host__ __device__ __forceinline__ void sd_taps(int i, int n_in, int n_out, int& j0, int& cnt, int& n0) {
  const int64_t two = 2 * (int64_t)n_out, D = 2 * (int64_t)n_in;
  const int64_t A = (2 * (int64_t)i + 1) * n_in - n_out;
  // first j with N > -D: floor((A - D) / two) + 1; D <= 32 n_out = 16 two, so 17 two keeps the dividend positive
  int64_t lo = (int64_t)((uint64_t)(A - D + 17 * two) / (uint64_t)two) - 16;
  int64_t hi = (int64_t)((uint64_t)(A + D - 1) / (uint64_t)two);   // last j with N < D
  if (lo < 0) lo = 0;
  if (hi > n_in - 1) hi = n_in - 1;
  j0 = (int)lo;
  cnt = (int)(hi - lo + 1);
  n0 = (int)(two * lo - A);
}

// most taps of any output, and most source samples under T consecutive outputs
inline int sd_max_taps(int n_in, int n_out) { return (2 * n_in + n_out - 1) / n_out; }
inline int sd_span(int T, int n_in, int n_out) {
  return (int)(((int64_t)(T - 1) * n_in + 2 * (int64_t)n_in) / n_out + 1);   // (not capped by n_in: the tile follows from the ratio alone)
}

// The tile: 64 columns up to 8:1 and 32 beyond (the staged row and the weight table hold either), and as many rows as the
// intermediate and the vertical weight table hold.
inline SdArgs sd_plan(int sw, int sh, int dw, int dh) {
  SdArgs a{sw, sh, dw, dh, 0, 0, sd_max_taps(sw, dw), sd_max_taps(sh, dh), 0, 0u};
  a.TW = (int64_t)sw <= 8 * (int64_t)dw ? 64 : 32;
  const int rows = SD_INTER_WORDS / (2 * a.TW);
  a.TH = 1;
  for (int th = SD_MAX_TH; th > 1; th--)
    if (sd_span(th, sh, dh) <= rows && a.KY * th <= SD_WY_WORDS) {
      a.TH = th;
      break;
    }
  return a;
}

// ---- how a site is stored: bytes of a row, the byte range of columns [c0, c1), the byte of a column, the unit of the scalar copy
template <int SRC> struct SdSrc;
template <> struct SdSrc<SD_F32> {
  using unit = uint32_t;
  static __host__ __device__ int64_t row_bytes(int w) { return 4 * (int64_t)w; }
  static __device__ int lo(int c0) { return 4 * c0; }
  static __device__ int hi(int c1) { return 4 * c1; }
  static __device__ float sample(const unsigned char* row, int a0, int c) { return *reinterpret_cast<const float*>(row + (4 * c - a0)); }
};
template <> struct SdSrc<SD_F16> {
  using unit = uint16_t;
  static __host__ __device__ int64_t row_bytes(int w) { return 2 * (int64_t)w; }
  static __device__ int lo(int c0) { return 2 * c0; }
  static __device__ int hi(int c1) { return 2 * c1; }
  static __device__ float sample(const unsigned char* row, int a0, int c) { return __half2float(*reinterpret_cast<const __half*>(row + (2 * c - a0))); }
};
template <bool IDS> struct SdPacked {
  using unit = uint8_t;
  static __host__ __device__ int64_t row_bytes(int w) { return 3 * (int64_t)(w / 2); }
  static __device__ int lo(int c0) { return 3 * (c0 >> 1); }
  static __device__ int hi(int c1) { return 3 * ((c1 + 1) >> 1); }
  static __device__ float sample(const unsigned char* row, int a0, int c) {   // codec.hip: unpack() and the scaled float32 conversion
    const unsigned char* b = row + (3 * (c >> 1) - a0);
    const uint32_t b0 = b[0], b1 = b[1], b2 = b[2];
    uint32_t p;
    if (IDS) p = (c & 1) ? ((b1 << 4) | (b2 >> 4)) : ((b0 << 4) | (b2 & 0xfu));
    else p = (c & 1) ? ((b2 << 4) | (b1 >> 4)) : (((b1 & 0xfu) << 8) | b0);
    return (float)p * (1.0f / 4095.0f);
  }
};
template <> struct SdSrc<SD_P12> : SdPacked<false> {};
template <> struct SdSrc<SD_P12_IDS> : SdPacked<true> {};

// the value tdk_apply_white_balance writes for a sample (postprocess.hip: white_balance_kernel), as a later kernel reads it back
template <int SRC> __device__ __forceinline__ float sd_balanced(float x, float g) {
  const float v = clampf(x * g, 0.0f, 1.0f);
  return SRC == SD_F16 ? as_stored<__half>(v) : v;
}

__device__ __forceinline__ float sd_gain(int r, int c, uint32_t pattern, float gr, float gg, float gb) {
  const int k = cfa_color(r, c, pattern);
  return (k == 0) ? gr : (k == 2 ? gb : gg);
}

template <int SRC, typename TO>
__global__ __launch_bounds__(SD_THREADS) void scaled_demosaic_kernel(const unsigned char* __restrict__ src, TO* __restrict__ dst, const float* __restrict__ gains,
                                                                      SdArgs a) {
  using S = SdSrc<SRC>;
  using unit = typename S::unit;
  __shared__ SdLds lds;
  const int tid = threadIdx.x;
  const int TW = a.TW, TH = a.TH;
  const int ox0 = (int)blockIdx.x * TW, oy0 = (int)blockIdx.y * TH;
  const int tw = min(TW, a.dw - ox0), th = min(TH, a.dh - oy0);

  // 1. tap tables: wave 0 the columns, wave 1 the rows
  if (tid < tw) {
    int j0, cnt, n0;
    sd_taps(ox0 + tid, a.sw, a.dw, j0, cnt, n0);
    const float D = (float)(2 * a.sw);
    float s0 = 0.0f, s1 = 0.0f;   // (0 + w is w: the first weight starts its sum)
    for (int k = 0; k < cnt; k++) {
      const float w = 1.0f - (float)abs(n0 + k * 2 * a.dw) / D;
      lds.wx[k * TW + tid] = w;
      if ((j0 + k) & 1) s1 = s1 + w;
      else s0 = s0 + w;
    }
    lds.jx[tid] = j0;
    lds.cx[tid] = cnt;
    lds.sumx[0][tid] = s0;
    lds.sumx[1][tid] = s1;
  } else if (tid >= 64 && tid - 64 < th) {
    const int t = tid - 64;
    int j0, cnt, n0;
    sd_taps(oy0 + t, a.sh, a.dh, j0, cnt, n0);
    const float D = (float)(2 * a.sh);
    for (int k = 0; k < cnt; k++) lds.wy[t * a.KY + k] = 1.0f - (float)abs(n0 + k * 2 * a.dh) / D;
    lds.jy[t] = j0;
    lds.cy[t] = cnt;
  }
  __syncthreads();

  // the tile's source footprint (the first tap moves right / down with the output index): columns [c0, c1), rows [sy0, sy0 + fh)
  const int c0 = lds.jx[0], c1 = lds.jx[tw - 1] + lds.cx[tw - 1];
  const int sy0 = lds.jy[0], fh = lds.jy[th - 1] + lds.cy[th - 1] - sy0;
  const int b0 = S::lo(c0), b1 = S::hi(c1);   // bytes of a row
  const int a0 = a.vec ? (b0 & ~15) : b0;      // the byte of a row that byte 0 of its staged copy holds
  const int64_t row_bytes = S::row_bytes(a.sw);
  const bool wb = gains != nullptr;
  // the gain of (row parity, column parity)
  float g00 = 1.0f, g01 = 1.0f, g10 = 1.0f, g11 = 1.0f;
  if (wb) {
    const float gr = gains[0], gg = gains[1], gb = gains[2];
    g00 = sd_gain(0, 0, a.pattern, gr, gg, gb), g01 = sd_gain(0, 1, a.pattern, gr, gg, gb);
    g10 = sd_gain(1, 0, a.pattern, gr, gg, gb), g11 = sd_gain(1, 1, a.pattern, gr, gg, gb);
  }
  const float inv_2tw = 1.0f / (float)(2 * tw), inv_tw = 1.0f / (float)tw;

  // 2. SD_SR source rows at a time: stage the bytes, then the horizontal chains
  for (int y0 = 0; y0 < fh; y0 += SD_SR) {
    const int rows = min(SD_SR, fh - y0);
    if (a.vec) {
      const int nseg = (b1 - a0 + 15) >> 4;
      const float inv = 1.0f / (float)nseg;
      for (int it = tid; it < rows * nseg; it += SD_THREADS) {
        int r, s;
        tdk_split_rc(it, nseg, inv, r, s);
        lds.stage[r][s] = *reinterpret_cast<const uint4*>(src + (int64_t)(sy0 + y0 + r) * row_bytes + a0 + 16 * s);
      }
    } else {
      const int nu = (b1 - b0) / (int)sizeof(unit);
      const float inv = 1.0f / (float)nu;
      for (int it = tid; it < rows * nu; it += SD_THREADS) {
        int r, e;
        tdk_split_rc(it, nu, inv, r, e);
        reinterpret_cast<unit*>(lds.stage[r])[e] = reinterpret_cast<const unit*>(src + (int64_t)(sy0 + y0 + r) * row_bytes + b0)[e];
      }
    }
    __syncthreads();
    for (int it = tid; it < rows * 2 * tw; it += SD_THREADS) {
      int r, e;
      tdk_split_rc(it, 2 * tw, inv_2tw, r, e);
      const int p = e >= tw ? 1 : 0, i = e - p * tw;
      const int y = sy0 + y0 + r;
      const float g = (y & 1) ? (p ? g11 : g10) : (p ? g01 : g00);
      const unsigned char* row = reinterpret_cast<const unsigned char*>(lds.stage[r]);
      const int j0 = lds.jx[i], cnt = lds.cx[i];
      int k = ((j0 & 1) == p) ? 0 : 1;   // the first tap of parity p
      float acc = 0.0f;
      if (k < cnt) {
        float x = S::sample(row, a0, j0 + k);
        if (wb) x = sd_balanced<SRC>(x, g);
        acc = lds.wx[k * TW + i] * x;
        for (k += 2; k < cnt; k += 2) {
          x = S::sample(row, a0, j0 + k);
          if (wb) x = sd_balanced<SRC>(x, g);
          acc = fmaf(lds.wx[k * TW + i], x, acc);
        }
      }
      lds.inter[((y0 + r) * 2 + p) * TW + i] = acc;
    }
    __syncthreads();
  }

  // 3. the vertical chains, the combine and the store
  const int c00 = cfa_color(0, 0, a.pattern), c01 = cfa_color(0, 1, a.pattern);
  for (int it = tid; it < th * tw; it += SD_THREADS) {
    int o, i;
    tdk_split_rc(it, tw, inv_tw, o, i);
    const int j0 = lds.jy[o], cnt = lds.cy[o];
    const float* wy = lds.wy + o * a.KY;
    // the taps at even k have the row parity of j0, those at odd k the other
    float e0 = 0.0f, e1 = 0.0f, es = 0.0f, f0 = 0.0f, f1 = 0.0f, fs = 0.0f;
    {
      const float* col = lds.inter + ((j0 - sy0) * 2) * TW + i;
      float v = wy[0];
      e0 = v * col[0], e1 = v * col[TW], es = v;
      for (int k = 2; k < cnt; k += 2) {
        v = wy[k];
        e0 = fmaf(v, col[2 * k * TW], e0), e1 = fmaf(v, col[(2 * k + 1) * TW], e1), es = es + v;
      }
    }
    if (cnt > 1) {
      const float* col = lds.inter + ((j0 - sy0) * 2) * TW + i;
      float v = wy[1];
      f0 = v * col[2 * TW], f1 = v * col[3 * TW], fs = v;
      for (int k = 3; k < cnt; k += 2) {
        v = wy[k];
        f0 = fmaf(v, col[2 * k * TW], f0), f1 = fmaf(v, col[(2 * k + 1) * TW], f1), fs = fs + v;
      }
    }
    const bool odd = j0 & 1;
    const float B00 = odd ? f0 : e0, B01 = odd ? f1 : e1, B10 = odd ? e0 : f0, B11 = odd ? e1 : f1;
    const float Sy0 = odd ? fs : es, Sy1 = odd ? es : fs;
    const float Sx0 = lds.sumx[0][i], Sx1 = lds.sumx[1][i];
    const float d00 = Sy0 * Sx0, d01 = Sy0 * Sx1, d10 = Sy1 * Sx0, d11 = Sy1 * Sx1;
    float R, G, B;
    if (c00 == 1) {   // green at (0, 0) and (1, 1): GRBG, GBRG
      G = (B00 + B11) / (d00 + d11);
      const float u = B01 / d01, l = B10 / d10;
      R = c01 == 0 ? u : l;
      B = c01 == 0 ? l : u;
    } else {          // green at (0, 1) and (1, 0): RGGB, BGGR
      G = (B01 + B10) / (d01 + d10);
      const float u = B00 / d00, l = B11 / d11;
      R = c00 == 0 ? u : l;
      B = c00 == 0 ? l : u;
    }
    const size_t at = ((size_t)(oy0 + o) * a.dw + (ox0 + i)) * 3;
    st<TO>(dst, at, R);
    st<TO>(dst, at + 1, G);
    st<TO>(dst, at + 2, B);
  }
}

template <int SRC, typename TO> int sd_launch(const void* src, void* dst, const float* gains, const SdArgs& a, hipStream_t st) {
  const dim3 grid((unsigned)tdk_div_up(a.dw, a.TW), (unsigned)tdk_div_up(a.dh, a.TH));
  TDK_LAUNCH("tdk_demosaic_scaled", (scaled_demosaic_kernel<SRC, TO>), grid, dim3(SD_THREADS), 0, st, reinterpret_cast<const unsigned char*>(src),
             reinterpret_cast<TO*>(dst), gains, a);
  return TDK_OK;
}

// 0: fine; otherwise which argument is wrong (the messages are with the entry points)
int sd_check_sizes(int w, int h, int ow, int oh) {
  if (!tdk_mosaic_size_ok(w, h)) return 1;
  if (ow < 1 || oh < 1) return 2;
  if ((int64_t)TDK_SCALED_MIN_RATIO * ow > w || (int64_t)TDK_SCALED_MIN_RATIO * oh > h) return 3;
  if ((int64_t)w > (int64_t)TDK_SCALED_MAX_RATIO * ow || (int64_t)h > (int64_t)TDK_SCALED_MAX_RATIO * oh) return 4;
  return 0;
}

int sd_run(const char* who, const void* src, void* dst, const float* gains, int w, int h, int ow, int oh, uint32_t pattern, bool packed, int src_tag, int dst_dtype,
           tdk_stream_t stream) {
  TDK_REQUIRE(src && dst, "%s: null pointer (src or dst)", who);
  const int bad = sd_check_sizes(w, h, ow, oh);
  TDK_REQUIRE(bad != 1, "%s: mosaic size %dx%d outside 2..%d", who, w, h, TDK_MOSAIC_MAX_SIZE);
  TDK_REQUIRE(bad != 2, "%s: output size %dx%d below 1x1", who, ow, oh);
  TDK_REQUIRE(bad != 3, "%s: ratio %dx%d -> %dx%d below %d:1 on an axis (a full-size demosaic serves that)", who, w, h, ow, oh, TDK_SCALED_MIN_RATIO);
  TDK_REQUIRE(bad != 4, "%s: ratio %dx%d -> %dx%d beyond %d:1 on an axis", who, w, h, ow, oh, TDK_SCALED_MAX_RATIO);
  TDK_REQUIRE(!packed || (w & 1) == 0, "%s: width must be even (pixel pairs share three bytes), got %d", who, w);
  TDK_REQUIRE(tdk_pattern_ok(pattern), "%s: invalid Bayer pattern 0x%08x", who, pattern);
  TDK_REQUIRE(packed || tdk_float_dtype_ok(src_tag), "%s: unsupported src dtype tag %d", who, src_tag);
  TDK_REQUIRE(tdk_float_dtype_ok(dst_dtype), "%s: unsupported dst dtype tag %d", who, dst_dtype);
  const int src_kind = packed ? (src_tag ? SD_P12_IDS : SD_P12) : src_tag;   // (TDK_F32 and TDK_F16 are SD_F32 and SD_F16)
  const int64_t row_bytes = src_kind == SD_F32 ? SdSrc<SD_F32>::row_bytes(w) : src_kind == SD_F16 ? SdSrc<SD_F16>::row_bytes(w) : SdSrc<SD_P12>::row_bytes(w);
  const size_t src_bytes = (size_t)row_bytes * h, dst_bytes = (size_t)ow * oh * 3 * tdk_dtype_bytes(dst_dtype);
  TDK_REQUIRE(tdk_disjoint(src, src_bytes, dst, dst_bytes), "%s: src and dst overlap (every output reads a neighbourhood)", who);
  TDK_REQUIRE(!gains || tdk_disjoint(gains, 12, dst, dst_bytes), "%s: gains and dst overlap", who);
  SdArgs a = sd_plan(w, h, ow, oh);
  a.pattern = pattern;
  a.vec = tdk_aligned(src, 16) && row_bytes % 16 == 0;
  hipStream_t st = tdk_stream(stream);
  if (dst_dtype == TDK_F32) {
    switch (src_kind) {
      case SD_F32: return sd_launch<SD_F32, float>(src, dst, gains, a, st);
      case SD_F16: return sd_launch<SD_F16, float>(src, dst, gains, a, st);
      case SD_P12: return sd_launch<SD_P12, float>(src, dst, gains, a, st);
      default: return sd_launch<SD_P12_IDS, float>(src, dst, gains, a, st);
    }
  }
  switch (src_kind) {
    case SD_F32: return sd_launch<SD_F32, __half>(src, dst, gains, a, st);
    case SD_F16: return sd_launch<SD_F16, __half>(src, dst, gains, a, st);
    case SD_P12: return sd_launch<SD_P12, __half>(src, dst, gains, a, st);
    default: return sd_launch<SD_P12_IDS, __half>(src, dst, gains, a, st);
  }
}

}  // namespace

static_assert(SD_F32 == TDK_F32 && SD_F16 == TDK_F16, "the float kinds are the dtype tags");

TDK_EXPORT int tdk_scaled_abi_version(void) { return TDK_SCALED_ABI_VERSION; }

TDK_EXPORT size_t tdk_demosaic_scaled_lds_bytes(int width, int height, int out_width, int out_height) {
  return sd_check_sizes(width, height, out_width, out_height) == 0 ? sizeof(SdLds) : 0;
}

TDK_EXPORT int tdk_demosaic_scaled_tile(int width, int height, int out_width, int out_height, int* tile_width, int* tile_height) {
  TDK_REQUIRE(tile_width && tile_height, "tdk_demosaic_scaled_tile: null pointer");
  TDK_REQUIRE(sd_check_sizes(width, height, out_width, out_height) == 0, "tdk_demosaic_scaled_tile: sizes %dx%d -> %dx%d are not a legal call", width, height,
              out_width, out_height);
  const SdArgs a = sd_plan(width, height, out_width, out_height);
  *tile_width = a.TW;
  *tile_height = a.TH;
  return TDK_OK;
}

TDK_EXPORT int tdk_demosaic_scaled(const void* src, void* dst, const float* gains, int width, int height, int out_width, int out_height, uint32_t pattern,
                                   int src_dtype, int dst_dtype, tdk_stream_t stream) {
  return sd_run("tdk_demosaic_scaled", src, dst, gains, width, height, out_width, out_height, pattern, false, src_dtype, dst_dtype, stream);
}

TDK_EXPORT int tdk_decode12_demosaic_scaled(const uint8_t* packed, void* dst, const float* gains, int width, int height, int out_width, int out_height,
                                            uint32_t pattern, int ids_format, int dst_dtype, tdk_stream_t stream) {
  return sd_run("tdk_decode12_demosaic_scaled", packed, dst, gains, width, height, out_width, out_height, pattern, true, ids_format != 0, dst_dtype, stream);
}
