// toneequal.hip -- tone equalizer: dodge and burn by exposure band behind a guided-filter mask (include/tdk_hip_toneeq.h:
// tdk_toneeq), three launches.
//
// The specification is the head comment of include/tdk_hip_toneeq.h; the steps named below are its steps.
//
// A lane moves 48 bytes of a frame row as three 16-byte accesses: TE_PX = 4 pixels of float32, 8 of binary16 (te_load / te_store).
// A group that hangs over the row's end, or does not start on 16 bytes (an odd width, an offset view), goes element by element.
//
// Cells, te_cells<T, S> (steps 1, 2): a wave owns a band of 16 pixel rows, 16 / S rows of cells, and 64 * TE_PX columns; the four
// waves of a workgroup take four bands one below the other.  The lanes of a wave lie side by side on ONE row.  The row tree over
// adjacent pairs is lane-local up to TE_PX values and goes on by xor-shuffles where a cell is wider than a lane's group (S = 16,
// and S = 8 of float32): both partners form the same sum.  The S row sums of a cell stay in the lane and are summed as the same
// tree.  Coordinates are clamped, not guarded: lanes past the frame re-read its last column, so every lane of a wave takes part in
// the shuffles.
// Coefficients, te_coeff (step 3): a tile of 32 x 32 cells with an apron of r cells, staged by clamped coordinates, in LDS; the
// horizontal sums of L and L*L over the staged rows, then the vertical sums, mean, corr, var, a and b per cell.
// Apply, te_apply<T, S> (steps 4 to 7): a tile of 128 x 32 pixels.  It stages the cells its pixels touch (128 / S + 2 by
// 32 / S + 2: a bilinear tap each side) plus the apron r of a and b, sums them horizontally and vertically in LDS to A and B, copies
// the table to LDS, and then every lane upsamples A and B for its pixels, looks the gain up and scales them.
// No value is summed into by more than one thread and every sum has a fixed order: the bits do not depend on scheduling.
#include <math.h>

#include "../../include/tdk_hip_toneeq.h"
#include "tdk_frame.h"

namespace {

constexpr int TE_THREADS = 256;
constexpr int TE_RMAX = TDK_TONEEQ_MAX_RADIUS;
constexpr int TE_BAND = 16;                       // pixel rows of a wave of te_cells
constexpr int TE_CT = 32;                         // te_coeff: a tile of TE_CT x TE_CT cells
constexpr int TE_CS = TE_CT + 2 * TE_RMAX;        // ... staged with the largest apron
constexpr int TE_TW = 128, TE_TH = 32;            // te_apply: a tile of pixels
constexpr size_t TE_WS_ALIGN = 16;
static_assert(TDK_TONEEQ_TABLE == (TDK_TONEEQ_EV_MAX - TDK_TONEEQ_EV_MIN) * TDK_TONEEQ_STEPS + 1, "table");
static_assert(TDK_TONEEQ_STEPS == 32, "the index takes five mantissa bits");

template <typename T> struct TePx {
  static constexpr int N = 16 / (int)sizeof(T);   // pixels of a lane: 48 bytes
};

struct TeArgs {
  int w, h, cw, ch;
  int r;
  float inv, eps;
  float w0, w1, w2;
};

__device__ __forceinline__ float te_lum(const TeArgs& a, float r, float g, float b) { return tdk_pos((a.w0 * r + a.w1 * g) + a.w2 * b); }

// TE_PX pixels of a row from column x0 on as v[3 * i + c]; columns past the row's end repeat its last pixel
template <typename T> __device__ __forceinline__ void te_load(const T* __restrict__ row, int x0, int w, float* v);
template <> __device__ __forceinline__ void te_load<float>(const float* __restrict__ row, int x0, int w, float* v) {
  const float* p = row + (size_t)x0 * 3;
  if (x0 + 4 <= w && (reinterpret_cast<uintptr_t>(p) & 15) == 0) {
    const float4* q = reinterpret_cast<const float4*>(p);
    const float4 a = q[0], b = q[1], c = q[2];
    v[0] = a.x, v[1] = a.y, v[2] = a.z, v[3] = a.w, v[4] = b.x, v[5] = b.y, v[6] = b.z, v[7] = b.w, v[8] = c.x, v[9] = c.y, v[10] = c.z, v[11] = c.w;
  } else {
#pragma unroll
    for (int i = 0; i < 4; i++) {
      const size_t o = (size_t)min(x0 + i, w - 1) * 3;
      v[3 * i] = row[o], v[3 * i + 1] = row[o + 1], v[3 * i + 2] = row[o + 2];
    }
  }
}
template <> __device__ __forceinline__ void te_load<__half>(const __half* __restrict__ row, int x0, int w, float* v) {
  const __half* p = row + (size_t)x0 * 3;
  if (x0 + 8 <= w && (reinterpret_cast<uintptr_t>(p) & 15) == 0) {
    const uint4* q = reinterpret_cast<const uint4*>(p);
#pragma unroll
    for (int k = 0; k < 3; k++) {
      const uint4 u = q[k];
      const __half2* h = reinterpret_cast<const __half2*>(&u);
#pragma unroll
      for (int j = 0; j < 4; j++) {
        const float2 f = __half22float2(h[j]);
        v[8 * k + 2 * j] = f.x, v[8 * k + 2 * j + 1] = f.y;
      }
    }
  } else {
#pragma unroll
    for (int i = 0; i < 8; i++) {
      const size_t o = (size_t)min(x0 + i, w - 1) * 3;
      v[3 * i] = __half2float(row[o]), v[3 * i + 1] = __half2float(row[o + 1]), v[3 * i + 2] = __half2float(row[o + 2]);
    }
  }
}

// ... and back: only the columns inside the row are written
template <typename T> __device__ __forceinline__ void te_store(T* __restrict__ row, int x0, int w, const float* v);
template <> __device__ __forceinline__ void te_store<float>(float* __restrict__ row, int x0, int w, const float* v) {
  float* p = row + (size_t)x0 * 3;
  if (x0 + 4 <= w && (reinterpret_cast<uintptr_t>(p) & 15) == 0) {
    float4* q = reinterpret_cast<float4*>(p);
    q[0] = make_float4(v[0], v[1], v[2], v[3]);
    q[1] = make_float4(v[4], v[5], v[6], v[7]);
    q[2] = make_float4(v[8], v[9], v[10], v[11]);
  } else {
#pragma unroll
    for (int i = 0; i < 4; i++)
      if (x0 + i < w) p[3 * i] = v[3 * i], p[3 * i + 1] = v[3 * i + 1], p[3 * i + 2] = v[3 * i + 2];
  }
}
template <> __device__ __forceinline__ void te_store<__half>(__half* __restrict__ row, int x0, int w, const float* v) {
  __half* p = row + (size_t)x0 * 3;
  if (x0 + 8 <= w && (reinterpret_cast<uintptr_t>(p) & 15) == 0) {
    uint4* q = reinterpret_cast<uint4*>(p);
#pragma unroll
    for (int k = 0; k < 3; k++) {
      uint4 u;
      __half2* h = reinterpret_cast<__half2*>(&u);
#pragma unroll
      for (int j = 0; j < 4; j++) h[j] = __floats2half2_rn(v[8 * k + 2 * j], v[8 * k + 2 * j + 1]);
      q[k] = u;
    }
  } else {
#pragma unroll
    for (int i = 0; i < 8; i++)
      if (x0 + i < w) p[3 * i] = __float2half_rn(v[3 * i]), p[3 * i + 1] = __float2half_rn(v[3 * i + 1]), p[3 * i + 2] = __float2half_rn(v[3 * i + 2]);
  }
}

// N values of the mask plane, a float32 row, from column x0 on
template <int N> __device__ __forceinline__ void te_store_mask(float* __restrict__ row, int x0, int w, const float* m) {
  float* p = row + x0;
  if (x0 + N <= w && (reinterpret_cast<uintptr_t>(p) & 15) == 0) {
#pragma unroll
    for (int k = 0; k < N / 4; k++) reinterpret_cast<float4*>(p)[k] = make_float4(m[4 * k], m[4 * k + 1], m[4 * k + 2], m[4 * k + 3]);
  } else {
#pragma unroll
    for (int i = 0; i < N; i++)
      if (x0 + i < w) p[i] = m[i];
  }
}

// v[0 .. N) summed as a balanced tree over adjacent pairs, in place: the sum is v[0]
template <int N> __device__ __forceinline__ void te_tree(float* v) {
#pragma unroll
  for (int step = 1; step < N; step *= 2)
#pragma unroll
    for (int i = 0; i < N; i += 2 * step) v[i] = v[i] + v[i + step];
}

// ---- steps 1 and 2
template <typename T, int S>
__global__ __launch_bounds__(TE_THREADS) void te_cells(const T* __restrict__ src, float* __restrict__ cells, TeArgs a) {
  constexpr int PX = TePx<T>::N;
  constexpr int CPL = PX >= S ? PX / S : 1;   // cells of a lane's group
  constexpr int LPC = S > PX ? S / PX : 1;    // lanes a cell is spread over
  constexpr int SUB = PX / CPL;               // values of one cell in a lane's group
  const int lane = (int)threadIdx.x & 63, band = (int)blockIdx.y * (TE_THREADS / 64) + (int)threadIdx.x / 64;
  const int x0 = ((int)blockIdx.x * 64 + lane) * PX;
#pragma unroll 1
  for (int k = 0; k < TE_BAND / S; k++) {
    const int cy = band * (TE_BAND / S) + k;
    if (cy >= a.ch) break;   // (the whole wave)
    float rows[CPL][S];
#pragma unroll
    for (int j = 0; j < S; j++) {
      const int y = min(cy * S + j, a.h - 1);
      float v[3 * PX], lum[PX];
      te_load<T>(src + (size_t)y * a.w * 3, x0, a.w, v);
#pragma unroll
      for (int i = 0; i < PX; i++) lum[i] = te_lum(a, v[3 * i], v[3 * i + 1], v[3 * i + 2]);
#pragma unroll
      for (int c = 0; c < CPL; c++) {
        te_tree<SUB>(lum + c * SUB);
        float t = lum[c * SUB];
#pragma unroll
        for (int o = 1; o < LPC; o *= 2) t = t + __shfl_xor(t, o, 64);
        rows[c][j] = t;
      }
    }
#pragma unroll
    for (int c = 0; c < CPL; c++) {
      te_tree<S>(rows[c]);
      const int cx = x0 / S + c;
      if (lane % LPC == 0 && cx < a.cw) cells[(size_t)cy * a.cw + cx] = rows[c][0] * (1.0f / (S * S));
    }
  }
}

// ---- step 3
struct TeCoeffLds {
  float l[TE_CS * TE_CS];        // the staged cells, pitch = TE_CT + 2r
  float h1[TE_CS * TE_CT];       // horizontal sums of L ...
  float h2[TE_CS * TE_CT];       // ... and of L*L, a row per staged row
};
static_assert(sizeof(TeCoeffLds) <= 64 * 1024, "LDS of te_coeff");

__global__ __launch_bounds__(TE_THREADS) void te_coeff(const float* __restrict__ cells, float* __restrict__ ca, float* __restrict__ cb, TeArgs a) {
  __shared__ TeCoeffLds lds;
  const int tid = (int)threadIdx.x;
  const int r = a.r, taps = 2 * r + 1, pitch = TE_CT + 2 * r;
  const int cx0 = (int)blockIdx.x * TE_CT, cy0 = (int)blockIdx.y * TE_CT;
  for (int e = tid; e < pitch * pitch; e += TE_THREADS) {
    const int sy = e / pitch, sx = e - sy * pitch;
    const int gy = min(max(cy0 - r + sy, 0), a.ch - 1), gx = min(max(cx0 - r + sx, 0), a.cw - 1);
    lds.l[e] = cells[(size_t)gy * a.cw + gx];
  }
  __syncthreads();
  for (int e = tid; e < pitch * TE_CT; e += TE_THREADS) {
    const int sy = e / TE_CT, ox = e - sy * TE_CT;
    const float* p = lds.l + sy * pitch + ox;
    float s1 = p[0], s2 = p[0] * p[0];
    for (int t = 1; t < taps; t++) {
      const float v = p[t];
      s1 = s1 + v;
      s2 = s2 + v * v;
    }
    lds.h1[e] = s1, lds.h2[e] = s2;
  }
  __syncthreads();
  for (int e = tid; e < TE_CT * TE_CT; e += TE_THREADS) {
    const int oy = e / TE_CT, ox = e - oy * TE_CT;
    const int cy = cy0 + oy, cx = cx0 + ox;
    if (cy >= a.ch || cx >= a.cw) continue;
    const int at = oy * TE_CT + ox;
    float s1 = lds.h1[at], s2 = lds.h2[at];
    for (int t = 1; t < taps; t++) {
      s1 = s1 + lds.h1[at + t * TE_CT];
      s2 = s2 + lds.h2[at + t * TE_CT];
    }
    const float mean = s1 * a.inv, corr = s2 * a.inv;
    const float var = tdk_pos(corr - mean * mean);
    const float ga = var / (var + a.eps);
    const size_t o = (size_t)cy * a.cw + cx;
    ca[o] = ga;
    cb[o] = mean - ga * mean;
  }
}

// ---- steps 4 to 7
template <int S> struct TeApplyLds {
  static constexpr int NX = TE_TW / S + 2, NY = TE_TH / S + 2;   // the cells the tile's pixels touch
  static constexpr int SX = NX + 2 * TE_RMAX, SY = NY + 2 * TE_RMAX;
  float sa[SY * SX], sb[SY * SX];   // a and b staged, pitch = NX + 2r
  float ha[SY * NX], hb[SY * NX];   // horizontal sums, a row per staged row
  float fa[NY * NX], fb[NY * NX];   // A and B
  float table[TDK_TONEEQ_TABLE];
};
static_assert(sizeof(TeApplyLds<2>) <= 64 * 1024, "LDS of te_apply");

__device__ __forceinline__ float te_lerp(float p0, float p1, float f) { return p0 + f * (p1 - p0); }

// the two taps of an axis: cell indices relative to `origin`, and the weight of the second
template <int S> __device__ __forceinline__ void te_taps(int x, int cells, int origin, int& i0, int& i1, float& f) {
  const int q = max(2 * x + 1 - S, 0);
  const int c0 = q / (2 * S);
  f = (float)(q % (2 * S)) * (1.0f / (2 * S));
  i0 = c0 - origin;
  i1 = min(c0 + 1, cells - 1) - origin;
}

template <typename T, int S>
__global__ __launch_bounds__(TE_THREADS) void te_apply(const T* __restrict__ src, T* __restrict__ dst, float* __restrict__ mask_out, const float* __restrict__ ca,
                                                       const float* __restrict__ cb, const float* __restrict__ table, TeArgs a) {
  using Lds = TeApplyLds<S>;
  constexpr int PX = TePx<T>::N, NX = Lds::NX, NY = Lds::NY;
  constexpr int LPR = TE_TW / PX, RPP = TE_THREADS / LPR;   // lanes of a tile row, tile rows of a pass
  __shared__ Lds lds;
  const int tid = (int)threadIdx.x;
  const int r = a.r, taps = 2 * r + 1, pitch = NX + 2 * r, srows = NY + 2 * r;
  const int px0 = (int)blockIdx.x * TE_TW, py0 = (int)blockIdx.y * TE_TH;
  const int ox = px0 / S - 1, oy = py0 / S - 1;   // the cell of fa[0]; -1 in the first tile, never read there
  for (int e = tid; e < TDK_TONEEQ_TABLE; e += TE_THREADS) lds.table[e] = table[e];
  for (int e = tid; e < srows * pitch; e += TE_THREADS) {
    const int sy = e / pitch, sx = e - sy * pitch;
    const int gy = min(max(oy - r + sy, 0), a.ch - 1), gx = min(max(ox - r + sx, 0), a.cw - 1);
    const size_t o = (size_t)gy * a.cw + gx;
    lds.sa[e] = ca[o], lds.sb[e] = cb[o];
  }
  __syncthreads();
  for (int e = tid; e < srows * NX; e += TE_THREADS) {
    const int sy = e / NX, x = e - sy * NX;
    const float *pa = lds.sa + sy * pitch + x, *pb = lds.sb + sy * pitch + x;
    float s1 = pa[0], s2 = pb[0];
    for (int t = 1; t < taps; t++) s1 = s1 + pa[t], s2 = s2 + pb[t];
    lds.ha[e] = s1, lds.hb[e] = s2;
  }
  __syncthreads();
  for (int e = tid; e < NY * NX; e += TE_THREADS) {
    float s1 = lds.ha[e], s2 = lds.hb[e];
    for (int t = 1; t < taps; t++) s1 = s1 + lds.ha[e + t * NX], s2 = s2 + lds.hb[e + t * NX];
    lds.fa[e] = s1 * a.inv, lds.fb[e] = s2 * a.inv;
  }
  __syncthreads();

  const int x0 = px0 + (tid % LPR) * PX;
  if (x0 >= a.w) return;
  int i0[PX], i1[PX];
  float fx[PX];
#pragma unroll
  for (int i = 0; i < PX; i++) te_taps<S>(min(x0 + i, a.w - 1), a.cw, ox, i0[i], i1[i], fx[i]);
#pragma unroll 1
  for (int pass = 0; pass < TE_TH / RPP; pass++) {
    const int y = py0 + pass * RPP + tid / LPR;
    if (y >= a.h) break;
    int j0, j1;
    float fy;
    te_taps<S>(y, a.ch, oy, j0, j1, fy);
    const float *a0 = lds.fa + j0 * NX, *a1 = lds.fa + j1 * NX, *b0 = lds.fb + j0 * NX, *b1 = lds.fb + j1 * NX;
    float v[3 * PX], m[PX];
    te_load<T>(src + (size_t)y * a.w * 3, x0, a.w, v);
#pragma unroll
    for (int i = 0; i < PX; i++) {
      const float lum = te_lum(a, v[3 * i], v[3 * i + 1], v[3 * i + 2]);
      const float au = te_lerp(te_lerp(a0[i0[i]], a0[i1[i]], fx[i]), te_lerp(a1[i0[i]], a1[i1[i]], fx[i]), fy);
      const float bu = te_lerp(te_lerp(b0[i0[i]], b0[i1[i]], fx[i]), te_lerp(b1[i0[i]], b1[i1[i]], fx[i]), fy);
      m[i] = au * lum + bu;
      const float mc = fminf(fmaxf(m[i], 0x1p-16f), 0x1.fffffep+3f);
      const uint32_t bits = __float_as_uint(mc), mant = bits & 0x7fffffu;
      const int at = ((int)(bits >> 23) - 127 - TDK_TONEEQ_EV_MIN) * TDK_TONEEQ_STEPS + (int)(mant >> 18);
      const float f = (float)(mant & 0x3ffffu) * (1.0f / 262144.0f);
      const float t0 = lds.table[at], t1 = lds.table[at + 1];
      const float gain = t0 + f * (t1 - t0);
      v[3 * i] = v[3 * i] * gain, v[3 * i + 1] = v[3 * i + 1] * gain, v[3 * i + 2] = v[3 * i + 2] * gain;
      // The product is a float32 value and the store rounds that to binary16: two roundings.  Left alone, the compiler may fold product
      // and conversion into one v_fma_mixlo_f16, which rounds once: the empty asm keeps the float32 product a value of its own.
      if constexpr (sizeof(T) == 2) asm volatile("" : "+v"(v[3 * i]), "+v"(v[3 * i + 1]), "+v"(v[3 * i + 2]));
    }
    if (dst != nullptr) te_store<T>(dst + (size_t)y * a.w * 3, x0, a.w, v);
    if (mask_out != nullptr) te_store_mask<PX>(mask_out + (size_t)y * a.w, x0, a.w, m);
  }
}

bool te_cell_ok(int cell) { return cell == 2 || cell == 4 || cell == 8 || cell == 16; }

// Run a statement with the cell size S as a constant; the caller has checked `cell`.
#define TE_DISPATCH_CELL(cell, S, ...)                       \
  do {                                                       \
    if ((cell) == 2) { constexpr int S = 2; __VA_ARGS__; }   \
    else if ((cell) == 4) { constexpr int S = 4; __VA_ARGS__; } \
    else if ((cell) == 8) { constexpr int S = 8; __VA_ARGS__; } \
    else { constexpr int S = 16; __VA_ARGS__; }              \
  } while (0)

template <int S> size_t te_apply_lds() { return sizeof(TeApplyLds<S>); }

template <typename T, int S>
int te_launch(const void* src, void* dst, float* mask_out, float* planes, const float* table, const TeArgs& a, hipStream_t st) {
  constexpr int PX = TePx<T>::N;
  const size_t n = (size_t)a.cw * a.ch;
  float *cells = planes, *ca = planes + n, *cb = planes + 2 * n;
  const dim3 block(TE_THREADS);
  const dim3 cells_grid((unsigned)tdk_div_up(a.cw * S, 64 * PX), (unsigned)tdk_div_up(a.ch, (TE_THREADS / 64) * (TE_BAND / S)));
  TDK_LAUNCH("tdk_toneeq(cells)", (te_cells<T, S>), cells_grid, block, 0, st, reinterpret_cast<const T*>(src), cells, a);
  const dim3 coeff_grid((unsigned)tdk_div_up(a.cw, TE_CT), (unsigned)tdk_div_up(a.ch, TE_CT));
  TDK_LAUNCH("tdk_toneeq(coefficients)", te_coeff, coeff_grid, block, 0, st, cells, ca, cb, a);
  const dim3 apply_grid((unsigned)tdk_div_up(a.w, TE_TW), (unsigned)tdk_div_up(a.h, TE_TH));
  TDK_LAUNCH("tdk_toneeq(apply)", (te_apply<T, S>), apply_grid, block, 0, st, reinterpret_cast<const T*>(src), reinterpret_cast<T*>(dst), mask_out, ca, cb, table, a);
  return TDK_OK;
}

}  // namespace

TDK_EXPORT int tdk_toneeq_abi_version(void) { return TDK_TONEEQ_ABI_VERSION; }

TDK_EXPORT size_t tdk_toneeq_workspace_bytes(int width, int height, int cell) {
  if (!tdk_frame_size_ok(width, height) || !te_cell_ok(cell)) return 0;
  return (size_t)3 * tdk_div_up(width, cell) * tdk_div_up(height, cell) * sizeof(float) + TE_WS_ALIGN;
}

TDK_EXPORT size_t tdk_toneeq_lds_bytes(int dtype, int cell, int radius) {
  if (!tdk_float_dtype_ok(dtype) || !te_cell_ok(cell) || radius < 0 || radius > TE_RMAX) return 0;
  size_t apply = 0;
  TE_DISPATCH_CELL(cell, S, apply = te_apply_lds<S>());
  return apply > sizeof(TeCoeffLds) ? apply : sizeof(TeCoeffLds);
}

TDK_EXPORT int tdk_toneeq(const void* src, void* dst, float* mask_out, void* workspace, const float* table, int width, int height, int dtype, int cell,
                          int radius, float eps, const float* weights, int flags, tdk_stream_t stream) {
  static const char* const who = "tdk_toneeq";
  TDK_REQUIRE(src, "%s: null pointer (src)", who);
  TDK_REQUIRE(dst || mask_out, "%s: null pointer (dst and mask_out: one of them is needed)", who);
  TDK_REQUIRE(workspace, "%s: null pointer (workspace)", who);
  TDK_REQUIRE(table, "%s: null pointer (table)", who);
  TDK_REQUIRE(weights, "%s: null pointer (weights)", who);
  TDK_REQUIRE(tdk_frame_size_ok(width, height), "%s: frame size %dx%d outside 1..%d", who, width, height, TDK_FRAME_MAX_SIZE);
  TDK_REQUIRE(tdk_float_dtype_ok(dtype), "%s: unsupported dtype tag %d", who, dtype);
  TDK_REQUIRE(te_cell_ok(cell), "%s: cell must be 2, 4, 8 or 16, got %d", who, cell);
  TDK_REQUIRE(radius >= 0 && radius <= TE_RMAX, "%s: radius must be 0..%d, got %d", who, TE_RMAX, radius);
  TDK_REQUIRE(eps > 0.0f && isfinite(eps), "%s: eps must be finite and > 0", who);
  const int bad_weight = tdk_first_bad_weight(weights, 3);
  TDK_REQUIRE(bad_weight < 0, "%s: weights must be finite and >= 0 (weights[%d])", who, bad_weight);
  TDK_REQUIRE(flags == 0, "%s: flags is reserved and must be 0, got %d", who, flags);
  TDK_REQUIRE(tdk_aligned(table, 4), "%s: table must be aligned to 4 bytes", who);
  TDK_REQUIRE(tdk_aligned(mask_out, 4), "%s: mask_out must be aligned to 4 bytes", who);
  const size_t n = (size_t)width * height, frame_bytes = n * 3 * tdk_dtype_bytes(dtype), mask_bytes = n * sizeof(float);
  const size_t ws_bytes = tdk_toneeq_workspace_bytes(width, height, cell), table_bytes = TDK_TONEEQ_TABLE * sizeof(float);
  TDK_REQUIRE(!dst || tdk_disjoint(src, frame_bytes, dst, frame_bytes), "%s: src and dst overlap", who);
  TDK_REQUIRE(!mask_out || (tdk_disjoint(mask_out, mask_bytes, src, frame_bytes) && (!dst || tdk_disjoint(mask_out, mask_bytes, dst, frame_bytes))),
              "%s: mask_out overlaps src or dst", who);
  TDK_REQUIRE((!dst || tdk_disjoint(table, table_bytes, dst, frame_bytes)) && (!mask_out || tdk_disjoint(table, table_bytes, mask_out, mask_bytes)),
              "%s: the table overlaps dst or mask_out", who);
  TDK_REQUIRE(tdk_disjoint(workspace, ws_bytes, src, frame_bytes) && (!dst || tdk_disjoint(workspace, ws_bytes, dst, frame_bytes)) &&
                  (!mask_out || tdk_disjoint(workspace, ws_bytes, mask_out, mask_bytes)) && tdk_disjoint(workspace, ws_bytes, table, table_bytes),
              "%s: the workspace overlaps src, dst, mask_out or the table", who);

  TeArgs a{};
  a.w = width, a.h = height, a.cw = tdk_div_up(width, cell), a.ch = tdk_div_up(height, cell);
  a.r = radius;
  a.inv = (float)(1.0 / (double)((2 * radius + 1) * (2 * radius + 1)));
  a.eps = eps;
  a.w0 = weights[0], a.w1 = weights[1], a.w2 = weights[2];
  float* planes = reinterpret_cast<float*>(tdk_align_up(reinterpret_cast<uintptr_t>(workspace), TE_WS_ALIGN));
  hipStream_t st = tdk_stream(stream);
  TDK_DISPATCH_DTYPE(dtype, T, TE_DISPATCH_CELL(cell, S, return (te_launch<T, S>(src, dst, mask_out, planes, table, a, st))));
}
