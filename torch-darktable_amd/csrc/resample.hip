// resample.hip -- antialiased bilinear scaling (include/tdk_hip_resample.h: tdk_resample), one launch, no workspace.
//
// Along an axis the weight of source sample j for output i is max(0, 1 - |j + 1/2 - c| / r).  With N = 2 n_out j + n_out -
// (2 i + 1) n_in and D = 2 max(n_in, n_out) that is (D - |N|) / D: the taps of an output are the integers M = D - |N| > 0, at most
// 2^17 each and below 2^23 in sum, so M and the sum S are exact in float32 and the normalised weight M / S carries one rounding.
// N is formed in 64-bit once per output and stepped in 32-bit over its taps; nothing about a position ever passes through float32.
//
// A workgroup of four waves owns TW x TH output pixels, both powers of two picked on the host from the ratio (plan()).  It
//   1. builds the tap tables of its TW columns and TH rows in LDS: first tap, tap count, normalised weights;
//   2. walks down its source footprint SR rows at a time: the rows are copied to LDS in the storage type with one element per
//      lane (coalesced, any alignment), then filtered horizontally into the float32 intermediate, FH x (TW C) in LDS -- a thread
//      owns one (row, column, channel), the 256 threads run over them in memory order, so neighbouring lanes write
//      neighbouring words;
//   3. filters the intermediate vertically and stores: a thread owns one (row, column, channel) again, neighbouring lanes read
//      neighbouring words of LDS and the store of a tile row is one contiguous run.
// The first product initialises each sum (no 0 + ...), so the identity scale returns the bits it read, -0 included.
// Nothing is accumulated across lanes or workgroups: the bits do not depend on scheduling.
#include <math.h>

#include "tdk_frame.h"

namespace {

constexpr int RS_THREADS = 256, RS_WAVES = RS_THREADS / 64;
constexpr int RS_MAX_SIZE = 65535, RS_MAX_RATIO = 16;
constexpr size_t RS_LDS_LIMIT = 64 * 1024;      // the dynamic-LDS size a kernel gets without raising its limit; two workgroups per CU
constexpr size_t RS_LDS_TARGET = 40 * 1024;     // four, where some tile gets there
constexpr double RS_MIN_GROUPS = 1024.0;        // four workgroups for each of 256 compute units

// The taps of output i: first source index, count, and N of the first tap (N steps by 2 n_out per tap, |N| < D for every tap).
__host__ __device__ inline void rs_taps(int i, int n_in, int n_out, int& j0, int& cnt, int& n0) {
  const int64_t two = 2 * (int64_t)n_out, D = 2 * (int64_t)(n_in > n_out ? n_in : n_out);
  const int64_t A = (2 * (int64_t)i + 1) * n_in - n_out;
  // first j with N > -D: floor((A - D) / two) + 1; D <= 32 n_out, so 17 two keeps the dividend positive
  int64_t lo = (int64_t)((uint64_t)(A - D + 17 * two) / (uint64_t)two) - 16;
  int64_t hi = (int64_t)((uint64_t)(A + D - 1) / (uint64_t)two);   // last j with N < D
  if (lo < 0) lo = 0;
  if (hi > n_in - 1) hi = n_in - 1;
  j0 = (int)lo;
  cnt = (int)(hi - lo + 1);
  n0 = (int)(two * lo - A);
}

// most taps of any output, and most source samples under T consecutive outputs
inline int rs_max_taps(int n_in, int n_out) { return (2 * (n_in > n_out ? n_in : n_out) + n_out - 1) / n_out; }
inline int rs_span(int T, int n_in, int n_out) {
  const int64_t D = 2 * (int64_t)(n_in > n_out ? n_in : n_out);
  const int64_t v = ((int64_t)(T - 1) * n_in + D) / n_out + 1;
  return (int)(v < n_in ? v : n_in);
}

struct RsArgs {
  int sw, sh, dw, dh;
  int lw, lh;        // log2 of the tile
  int SR, FW, FH;    // staged rows per step; source columns / rows under a tile (LDS extents)
  int KX, KY;        // tap-table depth
  size_t lds;
};

inline size_t rs_lds(const RsArgs& a, int C, size_t esz) {
  const size_t TW = (size_t)1 << a.lw, TH = (size_t)1 << a.lh;
  const size_t words = (size_t)a.FH * TW * C + (size_t)a.KX * TW + (size_t)a.KY * TH + 4 * (TW + TH);
  return words * 4 + tdk_align_up((size_t)a.SR * a.FW * C * esz, 4);
}

// The tile with the least re-read halo (weighed against the number of workgroups, below) among those whose LDS leaves four
// workgroups per CU; if none does, among those that leave two.
inline RsArgs rs_plan(int sw, int sh, int dw, int dh, int C, size_t esz) {
  RsArgs best{};
  double best_cost = 0.0;
  for (size_t limit : {RS_LDS_TARGET, RS_LDS_LIMIT}) {
    for (int lw = 6; lw >= 3; lw--) {
      for (int lh = 5; lh >= 0; lh--) {
        RsArgs a{sw, sh, dw, dh, lw, lh, 8, 0, 0, rs_max_taps(sw, dw), rs_max_taps(sh, dh), 0};
        const int tw = (1 << lw) < dw ? (1 << lw) : dw, th = (1 << lh) < dh ? (1 << lh) : dh;
        a.FW = rs_span(tw, sw, dw);
        a.FH = rs_span(th, sh, dh);
        if (rs_lds(a, C, esz) > limit) a.SR = 4;
        a.lds = rs_lds(a, C, esz);
        if (a.lds > limit) continue;
        // source samples staged per output pixel, and times what is missing to RS_MIN_GROUPS workgroups: a tile that leaves
        // compute units without work costs more than its smaller halo saves
        const double groups = (double)tdk_div_up(dw, 1 << lw) * tdk_div_up(dh, 1 << lh);
        const double cost = (double)a.FW * a.FH / ((double)tw * th) * (groups < RS_MIN_GROUPS ? RS_MIN_GROUPS / groups : 1.0);
        if (best.lds == 0 || cost < best_cost) {
          best = a;
          best_cost = cost;
        }
      }
    }
    if (best.lds) break;
  }
  return best;
}

template <typename T, int C> __global__ __launch_bounds__(RS_THREADS) void resample_kernel(const T* __restrict__ src, T* __restrict__ dst, RsArgs a) {
  extern __shared__ float lds[];
  const int TW = 1 << a.lw, TH = 1 << a.lh, EW = TW * C;
  float* inter = lds;                   // FH x EW, horizontally filtered rows
  float* wx = inter + a.FH * EW;        // KX x TW normalised weights, tap-major
  float* wy = wx + a.KX * TW;           // KY x TH
  float* sumx = wy + a.KY * TH;
  float* sumy = sumx + TW;
  int* jx = reinterpret_cast<int*>(sumy + TH);   // first tap, tap count, N of the first tap
  int *cx = jx + TW, *nx = cx + TW;
  int *jy = nx + TW, *cy = jy + TH, *ny = cy + TH;
  T* stage = reinterpret_cast<T*>(ny + TH);      // SR x (FW C) source rows as stored
  const int SWC = a.FW * C;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int ox0 = (int)blockIdx.x * TW, oy0 = (int)blockIdx.y * TH;
  const int tw = min(TW, a.dw - ox0), th = min(TH, a.dh - oy0);
  const int Dx = 2 * max(a.sw, a.dw), Dy = 2 * max(a.sh, a.dh);

  // 1. tap tables: wave 0 the columns, wave 1 the rows
  if (wave < 2) {
    const bool isx = wave == 0;
    const int t = lane, n = isx ? tw : th;
    if (t < n) {
      int j0, cnt, n0;
      rs_taps((isx ? ox0 : oy0) + t, isx ? a.sw : a.sh, isx ? a.dw : a.dh, j0, cnt, n0);
      const int step = 2 * (isx ? a.dw : a.dh), D = isx ? Dx : Dy;
      int sum = 0;
      for (int k = 0; k < cnt; k++) sum += D - abs(n0 + k * step);
      (isx ? jx : jy)[t] = j0;
      (isx ? cx : cy)[t] = cnt;
      (isx ? nx : ny)[t] = n0;
      (isx ? sumx : sumy)[t] = (float)sum;
    }
  }
  __syncthreads();
  for (int idx = tid; idx < a.KX * TW; idx += RS_THREADS) {
    const int k = idx >> a.lw, t = idx & (TW - 1);
    if (t < tw && k < cx[t]) wx[idx] = (float)(Dx - abs(nx[t] + k * 2 * a.dw)) / sumx[t];
  }
  for (int idx = tid; idx < a.KY * TH; idx += RS_THREADS) {
    const int k = idx >> a.lh, t = idx & (TH - 1);
    if (t < th && k < cy[t]) wy[idx] = (float)(Dy - abs(ny[t] + k * 2 * a.dh)) / sumy[t];
  }
  __syncthreads();

  // the tile's source footprint (the first tap moves right / down with the output index); the min() only restate rs_span
  const int sx0 = jx[0], sy0 = jy[0];
  const int fw = min(jx[tw - 1] + cx[tw - 1] - sx0, a.FW), fh = min(jy[th - 1] + cy[th - 1] - sy0, a.FH);
  const int fwc = fw * C, twc = tw * C;
  const float inv_twc = 1.0f / (float)twc;

  // 2. SR source rows at a time: stage, then filter horizontally
  for (int y0 = 0; y0 < fh; y0 += a.SR) {
    const int rows = min(a.SR, fh - y0);
    for (int r = wave; r < rows; r += RS_WAVES) {
      const T* row = src + ((size_t)(sy0 + y0 + r) * a.sw + sx0) * C;
      T* srow = stage + r * SWC;
#pragma unroll 4
      for (int e = lane; e < fwc; e += 64) srow[e] = row[e];
    }
    __syncthreads();
    for (int it = tid; it < rows * twc; it += RS_THREADS) {
      const int r = (int)(((float)it + 0.5f) * inv_twc), e = it - r * twc;   // it / twc: the quotient is never near an integer
      const T* srow = stage + r * SWC;
      const int ox = e / C, c = e - ox * C;
      const int n = cx[ox], base = (jx[ox] - sx0) * C + c;
      float acc = wx[ox] * ld(srow, (size_t)base);
      for (int k = 1; k < n; k++) acc = fmaf(wx[k * TW + ox], ld(srow, (size_t)(base + k * C)), acc);
      inter[(y0 + r) * EW + e] = acc;
    }
    __syncthreads();
  }

  // 3. vertical pass and store
  for (int it = tid; it < th * twc; it += RS_THREADS) {
    const int oy = (int)(((float)it + 0.5f) * inv_twc), e = it - oy * twc;
    const int n = cy[oy];
    const float* col = inter + (jy[oy] - sy0) * EW + e;
    float acc = wy[oy] * col[0];
    for (int k = 1; k < n; k++) acc = fmaf(wy[k * TH + oy], col[k * EW], acc);
    st(dst, ((size_t)(oy0 + oy) * a.dw + ox0) * C + e, acc);
  }
}

template <typename T, int C> int launch(const void* src, void* dst, const RsArgs& a, hipStream_t st) {
  const dim3 grid((unsigned)tdk_div_up(a.dw, 1 << a.lw), (unsigned)tdk_div_up(a.dh, 1 << a.lh));
  TDK_LAUNCH("tdk_resample", (resample_kernel<T, C>), grid, dim3(RS_THREADS), a.lds, st, reinterpret_cast<const T*>(src), reinterpret_cast<T*>(dst), a);
  return TDK_OK;
}

// 0: fine; otherwise which argument is wrong (messages in tdk_resample)
int rs_check(int sw, int sh, int dw, int dh, int channels, int dtype) {
  if (sw < 1 || sh < 1 || sw > RS_MAX_SIZE || sh > RS_MAX_SIZE) return 1;
  if (dw < 1 || dh < 1 || dw > RS_MAX_SIZE || dh > RS_MAX_SIZE) return 2;
  if (channels != 1 && channels != 3) return 3;
  if (dtype != TDK_F32 && dtype != TDK_F16 && dtype != TDK_U8) return 4;
  if ((int64_t)sw > (int64_t)RS_MAX_RATIO * dw || (int64_t)sh > (int64_t)RS_MAX_RATIO * dh) return 5;
  return 0;
}

}  // namespace

TDK_EXPORT int tdk_resample_abi_version(void) { return TDK_RESAMPLE_ABI_VERSION; }

TDK_EXPORT size_t tdk_resample_lds_bytes(int src_width, int src_height, int dst_width, int dst_height, int channels, int dtype) {
  if (rs_check(src_width, src_height, dst_width, dst_height, channels, dtype) != 0) return 0;
  return rs_plan(src_width, src_height, dst_width, dst_height, channels, tdk_dtype_bytes(dtype)).lds;
}

TDK_EXPORT int tdk_resample(const void* src, void* dst, int src_width, int src_height, int dst_width, int dst_height, int channels, int dtype,
                            tdk_stream_t stream) {
  TDK_REQUIRE(src && dst, "tdk_resample: null pointer");
  const int bad = rs_check(src_width, src_height, dst_width, dst_height, channels, dtype);
  TDK_REQUIRE(bad != 1, "tdk_resample: source size %dx%d outside 1..%d", src_width, src_height, RS_MAX_SIZE);
  TDK_REQUIRE(bad != 2, "tdk_resample: destination size %dx%d outside 1..%d", dst_width, dst_height, RS_MAX_SIZE);
  TDK_REQUIRE(bad != 3, "tdk_resample: channels must be 1 or 3, got %d", channels);
  TDK_REQUIRE(bad != 4, "tdk_resample: unsupported dtype tag %d", dtype);
  TDK_REQUIRE(bad != 5, "tdk_resample: ratio %dx%d -> %dx%d beyond %d:1 on an axis", src_width, src_height, dst_width, dst_height, RS_MAX_RATIO);
  const size_t esz = tdk_dtype_bytes(dtype);
  const size_t src_bytes = (size_t)src_width * src_height * channels * esz, dst_bytes = (size_t)dst_width * dst_height * channels * esz;
  TDK_REQUIRE(tdk_disjoint(src, src_bytes, dst, dst_bytes), "tdk_resample: src and dst overlap (every output reads its neighbours)");
  const RsArgs a = rs_plan(src_width, src_height, dst_width, dst_height, channels, esz);
  if (a.lds == 0 || a.lds > RS_LDS_LIMIT) {
    tdk_set_error("tdk_resample: no tile fits %zu bytes of LDS", RS_LDS_LIMIT);
    return TDK_ERR_INVALID_ARGUMENT;
  }
  hipStream_t st = tdk_stream(stream);
  TDK_DISPATCH_FRAME(dtype, channels, T, C, return launch<T, C>(src, dst, a, st));
}
