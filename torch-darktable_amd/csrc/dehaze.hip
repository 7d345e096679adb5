// dehaze.hip -- haze removal: dark channel prior with a guided transmission map (include/tdk_hip_dehaze.h: tdk_dehaze,
// tdk_dehaze_ambient), five launches with the estimate of the ambient light, three without.
//
// The specification is the head comment of include/tdk_hip_dehaze.h; the steps named below are its steps.  The cell grid, the box
// sums and the upsampling follow the rules of the tone equalizer (csrc/toneequal.hip), restated here.
//
// A lane moves 48 bytes of a frame row as three 16-byte accesses: 4 pixels of float32, 8 of binary16 (dh_load / dh_store).  A group
// that hangs over the row's end, or does not start on 16 bytes (an odd width, an offset view), goes element by element.
//
// Cells, dh_cells<T, S> (step 1): a wave owns a band of 16 pixel rows and 64 lane groups of columns; the lanes of a wave lie side by
// side on ONE row.  Minimum and row tree are lane-local up to a lane's group and go on by xor-shuffles where a cell is wider: both
// partners form the same value.  Coordinates are clamped, not guarded, so every lane of a wave takes part in the shuffles.  Seven
// planes per cell: m0 m1 m2, M0 M1 M2, L.
// Dark channel, dh_dark (step 2): a tile of 32 x 32 cells with an apron of rd cells in LDS, the minimum along x, then along y.
// Select, dh_select (step 3): ONE workgroup of 1024 threads.  A radix select over the 32-bit keys, the most significant byte first:
// four passes, each a histogram of 256 bins in LDS over the keys that carry the prefix found so far, then 256 threads find the bin the
// K-th largest key lies in.  The first bytes of a frame's keys are nearly all the same: a thread adds a run of equal digits at once,
// and the histogram is kept in 32 copies, a lane adding to its own.  A fifth pass sums fix(M_c) over the keys >= T in int64 per thread and then into LDS.  Integer sums: no order matters.
// Coefficients, dh_coeff (step 4): a tile of 32 x 32 cells.  q is staged with an apron of rd + rg cells, its windowed minimum gives t
// on the tile plus rg -- the window centred on the CLAMPED cell of a staged position, since box() reads t at clamped cells -- L is
// staged alike, and the horizontal and vertical sums of L, t, L*t and L*L follow in the LDS that q has left.
// Apply, dh_apply<T, S> (step 5): a tile of 128 x 32 pixels.  It stages the cells its pixels touch (a bilinear tap each side) plus the
// apron rg of a and b, sums them to A2 and B2 in LDS, and every lane upsamples them for its pixels.
// No float is summed into by more than one thread and every float sum has a fixed order: the bits do not depend on scheduling.
#include <math.h>

#include "../../include/tdk_hip_dehaze.h"
#include "tdk_frame.h"

namespace {

constexpr int DH_THREADS = 256;
constexpr int DH_SEL_THREADS = 1024;
constexpr int DH_RD = TDK_DEHAZE_MAX_DARK_RADIUS, DH_RG = TDK_DEHAZE_MAX_RADIUS;
constexpr int DH_BAND = 16;                        // pixel rows of a wave of dh_cells
constexpr int DH_CT = 32;                          // dh_dark, dh_coeff: a tile of DH_CT x DH_CT cells
constexpr int DH_DS = DH_CT + 2 * DH_RD;           // dh_dark: staged with the largest apron
constexpr int DH_TS = DH_CT + 2 * DH_RG;           // dh_coeff: t and L, the tile plus rg
constexpr int DH_QS = DH_TS + 2 * DH_RD;           // dh_coeff: q, the tile plus rg + rd
constexpr int DH_TW = 128, DH_TH = 32;             // dh_apply: a tile of pixels
constexpr size_t DH_WS_ALIGN = 16;
constexpr float DH_MIN_AMBIENT = 0x1p-10f;
static_assert(DH_RD + DH_RG == 12, "the apron of dh_coeff");

template <typename T> struct DhPx {
  static constexpr int N = 16 / (int)sizeof(T);   // pixels of a lane: 48 bytes
};

struct DhArgs {
  int w, h, cw, ch;
  int rd, rg;
  float inv, eps, strength, floor;
  float w0, w1, w2;
};

__device__ __forceinline__ float dh_lum(const DhArgs& a, float r, float g, float b) { return tdk_pos((a.w0 * r + a.w1 * g) + a.w2 * b); }

// PX pixels of a row from column x0 on as v[3 * i + c]; columns past the row's end repeat its last pixel
template <typename T> __device__ __forceinline__ void dh_load(const T* __restrict__ row, int x0, int w, float* v);
template <> __device__ __forceinline__ void dh_load<float>(const float* __restrict__ row, int x0, int w, float* v) {
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
template <> __device__ __forceinline__ void dh_load<__half>(const __half* __restrict__ row, int x0, int w, float* v) {
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
template <typename T> __device__ __forceinline__ void dh_store(T* __restrict__ row, int x0, int w, const float* v);
template <> __device__ __forceinline__ void dh_store<float>(float* __restrict__ row, int x0, int w, const float* v) {
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
template <> __device__ __forceinline__ void dh_store<__half>(__half* __restrict__ row, int x0, int w, const float* v) {
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

// N values of the transmission plane, a float32 row, from column x0 on
template <int N> __device__ __forceinline__ void dh_store_plane(float* __restrict__ row, int x0, int w, const float* m) {
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
template <int N> __device__ __forceinline__ void dh_tree(float* v) {
#pragma unroll
  for (int step = 1; step < N; step *= 2)
#pragma unroll
    for (int i = 0; i < N; i += 2 * step) v[i] = v[i] + v[i + step];
}

// ---- step 1.  planes: m0 m1 m2 M0 M1 M2 L, n = cw*ch values each
template <typename T, int S>
__global__ __launch_bounds__(DH_THREADS) void dh_cells(const T* __restrict__ src, float* __restrict__ planes, DhArgs a) {
  constexpr int PX = DhPx<T>::N;
  constexpr int CPL = PX >= S ? PX / S : 1;   // cells of a lane's group
  constexpr int LPC = S > PX ? S / PX : 1;    // lanes a cell is spread over
  constexpr int SUB = PX / CPL;               // values of one cell in a lane's group
  const int lane = (int)threadIdx.x & 63, band = (int)blockIdx.y * (DH_THREADS / 64) + (int)threadIdx.x / 64;
  const int x0 = ((int)blockIdx.x * 64 + lane) * PX;
  const size_t n = (size_t)a.cw * a.ch;
#pragma unroll 1
  for (int k = 0; k < DH_BAND / S; k++) {
    const int cy = band * (DH_BAND / S) + k;
    if (cy >= a.ch) break;   // (the whole wave)
    float sums[4][CPL][S];   // the row sums of pos(x_0), pos(x_1), pos(x_2) and Y
    float lows[3][CPL];
#pragma unroll
    for (int c = 0; c < CPL; c++) lows[0][c] = lows[1][c] = lows[2][c] = INFINITY;
#pragma unroll
    for (int j = 0; j < S; j++) {
      const int y = min(cy * S + j, a.h - 1);
      float v[3 * PX];
      dh_load<T>(src + (size_t)y * a.w * 3, x0, a.w, v);
#pragma unroll
      for (int c = 0; c < CPL; c++) {
        float p[4][SUB];
#pragma unroll
        for (int i = 0; i < SUB; i++) {
          const float* px = v + 3 * (c * SUB + i);
          p[0][i] = tdk_pos(px[0]), p[1][i] = tdk_pos(px[1]), p[2][i] = tdk_pos(px[2]);
          p[3][i] = dh_lum(a, px[0], px[1], px[2]);
        }
#pragma unroll
        for (int q = 0; q < 3; q++) {
          float lo = p[q][0];
#pragma unroll
          for (int i = 1; i < SUB; i++) lo = fminf(lo, p[q][i]);
#pragma unroll
          for (int o = 1; o < LPC; o *= 2) lo = fminf(lo, __shfl_xor(lo, o, 64));
          lows[q][c] = fminf(lows[q][c], lo);
        }
#pragma unroll
        for (int q = 0; q < 4; q++) {
          dh_tree<SUB>(p[q]);
          float t = p[q][0];
#pragma unroll
          for (int o = 1; o < LPC; o *= 2) t = t + __shfl_xor(t, o, 64);
          sums[q][c][j] = t;
        }
      }
    }
#pragma unroll
    for (int c = 0; c < CPL; c++) {
#pragma unroll
      for (int q = 0; q < 4; q++) dh_tree<S>(sums[q][c]);
      const int cx = x0 / S + c;
      if (lane % LPC == 0 && cx < a.cw) {
        const size_t o = (size_t)cy * a.cw + cx;
#pragma unroll
        for (int q = 0; q < 3; q++) planes[q * n + o] = lows[q][c];
#pragma unroll
        for (int q = 0; q < 4; q++) planes[(3 + q) * n + o] = sums[q][c][0] * (1.0f / (S * S));
      }
    }
  }
}

// ---- step 2
struct DhDarkLds {
  float q[DH_DS * DH_DS];   // min(m0, m1, m2) staged, pitch = DH_CT + 2rd
  float h[DH_DS * DH_CT];   // the minimum along x, a row per staged row
};

__global__ __launch_bounds__(DH_THREADS) void dh_dark(const float* __restrict__ lows, float* __restrict__ dark, DhArgs a) {
  __shared__ DhDarkLds lds;
  const int tid = (int)threadIdx.x;
  const int r = a.rd, taps = 2 * r + 1, pitch = DH_CT + 2 * r;
  const int cx0 = (int)blockIdx.x * DH_CT, cy0 = (int)blockIdx.y * DH_CT;
  const size_t n = (size_t)a.cw * a.ch;
  for (int e = tid; e < pitch * pitch; e += DH_THREADS) {
    const int sy = e / pitch, sx = e - sy * pitch;
    const int gy = min(max(cy0 - r + sy, 0), a.ch - 1), gx = min(max(cx0 - r + sx, 0), a.cw - 1);
    const size_t o = (size_t)gy * a.cw + gx;
    lds.q[e] = fminf(fminf(lows[o], lows[n + o]), lows[2 * n + o]);
  }
  __syncthreads();
  for (int e = tid; e < pitch * DH_CT; e += DH_THREADS) {
    const int sy = e / DH_CT, ox = e - sy * DH_CT;
    const float* p = lds.q + sy * pitch + ox;
    float m = p[0];
    for (int t = 1; t < taps; t++) m = fminf(m, p[t]);
    lds.h[e] = m;
  }
  __syncthreads();
  for (int e = tid; e < DH_CT * DH_CT; e += DH_THREADS) {
    const int oy = e / DH_CT, ox = e - oy * DH_CT;
    const int cy = cy0 + oy, cx = cx0 + ox;
    if (cy >= a.ch || cx >= a.cw) continue;
    float m = lds.h[e];
    for (int t = 1; t < taps; t++) m = fminf(m, lds.h[e + t * DH_CT]);
    dark[(size_t)cy * a.cw + cx] = m;
  }
}

// ---- step 3: one workgroup
// f(e, key) over the keys of a thread, DH_SEL_UNROLL of them asked for before the first is looked at: with one load in flight per
// thread a pass over 196 608 keys waits 192 times for memory
constexpr int DH_SEL_UNROLL = 32;
template <typename F> __device__ __forceinline__ void dh_for_keys(const unsigned* __restrict__ keys, int n, int tid, F&& f) {
  constexpr int ROUND = DH_SEL_UNROLL * DH_SEL_THREADS;
  int start = 0;
  for (; start + ROUND <= n; start += ROUND) {   // (the same for every thread: no guard per key)
    unsigned k[DH_SEL_UNROLL];
#pragma unroll
    for (int u = 0; u < DH_SEL_UNROLL; u++) k[u] = keys[start + u * DH_SEL_THREADS + tid];
#pragma unroll
    for (int u = 0; u < DH_SEL_UNROLL; u++) f(start + u * DH_SEL_THREADS + tid, k[u]);
  }
  for (int e = start + tid; e < n; e += DH_SEL_THREADS) f(e, keys[e]);
}

constexpr int DH_SEL_COPIES = 32;    // histograms side by side, a lane adds to copy lane % 32: the keys of a frame share their first bytes,
                                     // and 64 lanes adding to one address are served one after the other
struct DhSelectLds {
  unsigned hist[256 * DH_SEL_COPIES];   // bin b of copy c at b * DH_SEL_COPIES + c: the copies of a bin lie in different banks
  alignas(16) unsigned total[256];
  unsigned prefix, remaining;        // the bytes of T found so far; the rank of T among the keys that carry them
  unsigned long long sums[3];
  unsigned count;
};

__global__ __launch_bounds__(DH_SEL_THREADS) void dh_select(const float* __restrict__ dark, const float* __restrict__ means, float* __restrict__ ambient, int n, int count) {
  __shared__ DhSelectLds lds;
  const int tid = (int)threadIdx.x;
  const unsigned* keys = reinterpret_cast<const unsigned*>(dark);
  if (tid == 0) {
    lds.prefix = 0u, lds.remaining = (unsigned)count;
    lds.sums[0] = lds.sums[1] = lds.sums[2] = 0ull, lds.count = 0u;
  }
  __syncthreads();
#pragma unroll 1
  for (int shift = 24; shift >= 0; shift -= 8) {
    const unsigned prefix = lds.prefix, remaining = lds.remaining;
    const unsigned mask = shift == 24 ? 0u : 0xffffffffu << (shift + 8);
    for (int e = tid; e < 256 * DH_SEL_COPIES; e += DH_SEL_THREADS) lds.hist[e] = 0u;
    __syncthreads();
    unsigned* const copy = lds.hist + (tid & (DH_SEL_COPIES - 1));
    int last = -1;
    unsigned run = 0u;
    dh_for_keys(keys, n, tid, [&](int, unsigned key) {
      if ((key & mask) != prefix) return;
      const int digit = (int)((key >> shift) & 255u);
      if (digit != last) {
        if (run) atomicAdd(&copy[last * DH_SEL_COPIES], run);
        last = digit, run = 0u;
      }
      run++;
    });
    if (run) atomicAdd(&copy[last * DH_SEL_COPIES], run);
    __syncthreads();
    if (tid < 256) {   // (copy c + tid first: the lanes of a wave start in different banks)
      unsigned sum = 0u;
#pragma unroll
      for (int c = 0; c < DH_SEL_COPIES; c++) sum += lds.hist[tid * DH_SEL_COPIES + ((c + tid) & (DH_SEL_COPIES - 1))];
      lds.total[tid] = sum;
    }
    __syncthreads();
    if (tid < 256) {   // the one bin with: keys above it < remaining <= keys above it + its own
      unsigned above = 0u;   // (every lane reads every total, four at a time, the same address: a loop from tid + 1 on waits for LDS once per bin)
#pragma unroll 8
      for (int b = 0; b < 256; b += 4) {
        const uint4 v = *reinterpret_cast<const uint4*>(&lds.total[b]);
        above += (b > tid ? v.x : 0u) + (b + 1 > tid ? v.y : 0u) + (b + 2 > tid ? v.z : 0u) + (b + 3 > tid ? v.w : 0u);
      }
      if (above < remaining && remaining <= above + lds.total[tid]) lds.prefix = prefix | ((unsigned)tid << shift), lds.remaining = remaining - above;
    }
    __syncthreads();
  }
  const unsigned threshold = lds.prefix;
  long long s0 = 0, s1 = 0, s2 = 0;
  unsigned mine = 0u;
  dh_for_keys(keys, n, tid, [&](int e, unsigned key) {
    if (key < threshold) return;
    s0 += (long long)(fminf(means[e], 65536.0f) * 1048576.0f);
    s1 += (long long)(fminf(means[(size_t)n + e], 65536.0f) * 1048576.0f);
    s2 += (long long)(fminf(means[2 * (size_t)n + e], 65536.0f) * 1048576.0f);
    mine++;
  });
  if (mine) {
    atomicAdd(&lds.sums[0], (unsigned long long)s0), atomicAdd(&lds.sums[1], (unsigned long long)s1), atomicAdd(&lds.sums[2], (unsigned long long)s2);
    atomicAdd(&lds.count, mine);
  }
  __syncthreads();
  if (tid < 3) ambient[tid] = (float)(((double)(long long)lds.sums[tid] / (double)lds.count) * 0x1p-20);
  if (tid == 3) ambient[3] = (float)lds.count;
}

// ---- step 4
constexpr int DH_U_FIRST = DH_QS * DH_QS + DH_QS * DH_TS, DH_U_THEN = 4 * DH_TS * DH_CT;
struct DhCoeffLds {
  float u[DH_U_FIRST > DH_U_THEN ? DH_U_FIRST : DH_U_THEN];   // q (pitch DH_CT + 2(rg + rd)) and its minimum along x; then the four horizontal sums
  float t[DH_TS * DH_TS], l[DH_TS * DH_TS];  // t and L on the tile plus rg, pitch DH_CT + 2rg
};
static_assert(sizeof(DhCoeffLds) <= 64 * 1024, "LDS of dh_coeff");

__global__ __launch_bounds__(DH_THREADS) void dh_coeff(const float* __restrict__ planes, const float* __restrict__ ambient, float* __restrict__ ca, float* __restrict__ cb,
                                                       DhArgs a) {
  __shared__ DhCoeffLds lds;
  const int tid = (int)threadIdx.x;
  const int r = a.rg, rd = a.rd, taps = 2 * r + 1, dtaps = 2 * rd + 1, tp = DH_CT + 2 * r, qp = tp + 2 * rd;
  const int cx0 = (int)blockIdx.x * DH_CT, cy0 = (int)blockIdx.y * DH_CT;
  const size_t n = (size_t)a.cw * a.ch;
  const float i0 = 1.0f / fmaxf(ambient[0], DH_MIN_AMBIENT), i1 = 1.0f / fmaxf(ambient[1], DH_MIN_AMBIENT), i2 = 1.0f / fmaxf(ambient[2], DH_MIN_AMBIENT);
  float *q = lds.u, *hm = lds.u + qp * qp;
  for (int e = tid; e < qp * qp; e += DH_THREADS) {
    const int sy = e / qp, sx = e - sy * qp;
    const int gy = min(max(cy0 - r - rd + sy, 0), a.ch - 1), gx = min(max(cx0 - r - rd + sx, 0), a.cw - 1);
    const size_t o = (size_t)gy * a.cw + gx;
    q[e] = fminf(fminf(planes[o] * i0, planes[n + o] * i1), planes[2 * n + o] * i2);
  }
  for (int e = tid; e < tp * tp; e += DH_THREADS) {
    const int sy = e / tp, sx = e - sy * tp;
    const int gy = min(max(cy0 - r + sy, 0), a.ch - 1), gx = min(max(cx0 - r + sx, 0), a.cw - 1);
    lds.l[e] = planes[6 * n + (size_t)gy * a.cw + gx];
  }
  __syncthreads();
  // the window of a staged position is centred on its clamped cell gx: column gx - rd of the grid is column gx - cx0 + r of q
  for (int e = tid; e < qp * tp; e += DH_THREADS) {
    const int sy = e / tp, sx = e - sy * tp;
    const int gx = min(max(cx0 - r + sx, 0), a.cw - 1);
    const float* p = q + sy * qp + (gx - cx0 + r);
    float m = p[0];
    for (int t = 1; t < dtaps; t++) m = fminf(m, p[t]);
    hm[e] = m;
  }
  __syncthreads();
  for (int e = tid; e < tp * tp; e += DH_THREADS) {
    const int sy = e / tp, sx = e - sy * tp;
    const int gy = min(max(cy0 - r + sy, 0), a.ch - 1);
    const float* p = hm + (gy - cy0 + r) * tp + sx;
    float m = p[0];
    for (int t = 1; t < dtaps; t++) m = fminf(m, p[t * tp]);
    lds.t[e] = 1.0f - a.strength * fminf(m, 1.0f);
  }
  __syncthreads();   // q and hm are done with
  float *h1 = lds.u, *h2 = h1 + tp * DH_CT, *h3 = h2 + tp * DH_CT, *h4 = h3 + tp * DH_CT;
  for (int e = tid; e < tp * DH_CT; e += DH_THREADS) {
    const int sy = e / DH_CT, ox = e - sy * DH_CT;
    const float *pl = lds.l + sy * tp + ox, *pt = lds.t + sy * tp + ox;
    float s1 = pl[0], s2 = pt[0], s3 = pl[0] * pt[0], s4 = pl[0] * pl[0];
    for (int t = 1; t < taps; t++) {
      const float vl = pl[t], vt = pt[t];
      s1 = s1 + vl;
      s2 = s2 + vt;
      s3 = s3 + vl * vt;
      s4 = s4 + vl * vl;
    }
    h1[e] = s1, h2[e] = s2, h3[e] = s3, h4[e] = s4;
  }
  __syncthreads();
  for (int e = tid; e < DH_CT * DH_CT; e += DH_THREADS) {
    const int oy = e / DH_CT, ox = e - oy * DH_CT;
    const int cy = cy0 + oy, cx = cx0 + ox;
    if (cy >= a.ch || cx >= a.cw) continue;
    float s1 = h1[e], s2 = h2[e], s3 = h3[e], s4 = h4[e];
    for (int t = 1; t < taps; t++) {
      s1 = s1 + h1[e + t * DH_CT];
      s2 = s2 + h2[e + t * DH_CT];
      s3 = s3 + h3[e + t * DH_CT];
      s4 = s4 + h4[e + t * DH_CT];
    }
    const float ml = s1 * a.inv, mt = s2 * a.inv;
    const float cov = s3 * a.inv - ml * mt;
    const float var = tdk_pos(s4 * a.inv - ml * ml);
    const float ga = cov / (var + a.eps);
    const size_t o = (size_t)cy * a.cw + cx;
    ca[o] = ga;
    cb[o] = mt - ga * ml;
  }
}

// ---- step 5
template <int S> struct DhApplyLds {
  static constexpr int NX = DH_TW / S + 2, NY = DH_TH / S + 2;   // the cells the tile's pixels touch
  static constexpr int SX = NX + 2 * DH_RG, SY = NY + 2 * DH_RG;
  float sa[SY * SX], sb[SY * SX];   // a and b staged, pitch = NX + 2rg
  float ha[SY * NX], hb[SY * NX];   // horizontal sums, a row per staged row
  float fa[NY * NX], fb[NY * NX];   // A2 and B2
};
static_assert(sizeof(DhApplyLds<2>) <= 64 * 1024, "LDS of dh_apply");

__device__ __forceinline__ float dh_lerp(float p0, float p1, float f) { return p0 + f * (p1 - p0); }

// the two taps of an axis: cell indices relative to `origin`, and the weight of the second
template <int S> __device__ __forceinline__ void dh_taps(int x, int cells, int origin, int& i0, int& i1, float& f) {
  const int q = max(2 * x + 1 - S, 0);
  const int c0 = q / (2 * S);
  f = (float)(q % (2 * S)) * (1.0f / (2 * S));
  i0 = c0 - origin;
  i1 = min(c0 + 1, cells - 1) - origin;
}

template <typename T, int S>
__global__ __launch_bounds__(DH_THREADS) void dh_apply(const T* __restrict__ src, T* __restrict__ dst, float* __restrict__ t_out, const float* __restrict__ ca,
                                                       const float* __restrict__ cb, const float* __restrict__ ambient, DhArgs a) {
  using Lds = DhApplyLds<S>;
  constexpr int PX = DhPx<T>::N, NX = Lds::NX, NY = Lds::NY;
  constexpr int LPR = DH_TW / PX, RPP = DH_THREADS / LPR;   // lanes of a tile row, tile rows of a pass
  __shared__ Lds lds;
  const int tid = (int)threadIdx.x;
  const int r = a.rg, taps = 2 * r + 1, pitch = NX + 2 * r, srows = NY + 2 * r;
  const int px0 = (int)blockIdx.x * DH_TW, py0 = (int)blockIdx.y * DH_TH;
  const int ox = px0 / S - 1, oy = py0 / S - 1;   // the cell of fa[0]; -1 in the first tile, never read there
  for (int e = tid; e < srows * pitch; e += DH_THREADS) {
    const int sy = e / pitch, sx = e - sy * pitch;
    const int gy = min(max(oy - r + sy, 0), a.ch - 1), gx = min(max(ox - r + sx, 0), a.cw - 1);
    const size_t o = (size_t)gy * a.cw + gx;
    lds.sa[e] = ca[o], lds.sb[e] = cb[o];
  }
  __syncthreads();
  for (int e = tid; e < srows * NX; e += DH_THREADS) {
    const int sy = e / NX, x = e - sy * NX;
    const float *pa = lds.sa + sy * pitch + x, *pb = lds.sb + sy * pitch + x;
    float s1 = pa[0], s2 = pb[0];
    for (int t = 1; t < taps; t++) s1 = s1 + pa[t], s2 = s2 + pb[t];
    lds.ha[e] = s1, lds.hb[e] = s2;
  }
  __syncthreads();
  for (int e = tid; e < NY * NX; e += DH_THREADS) {
    float s1 = lds.ha[e], s2 = lds.hb[e];
    for (int t = 1; t < taps; t++) s1 = s1 + lds.ha[e + t * NX], s2 = s2 + lds.hb[e + t * NX];
    lds.fa[e] = s1 * a.inv, lds.fb[e] = s2 * a.inv;
  }
  __syncthreads();

  const int x0 = px0 + (tid % LPR) * PX;
  if (x0 >= a.w) return;
  const float amb[3] = {fmaxf(ambient[0], DH_MIN_AMBIENT), fmaxf(ambient[1], DH_MIN_AMBIENT), fmaxf(ambient[2], DH_MIN_AMBIENT)};
  int i0[PX], i1[PX];
  float fx[PX];
#pragma unroll
  for (int i = 0; i < PX; i++) dh_taps<S>(min(x0 + i, a.w - 1), a.cw, ox, i0[i], i1[i], fx[i]);
#pragma unroll 1
  for (int pass = 0; pass < DH_TH / RPP; pass++) {
    const int y = py0 + pass * RPP + tid / LPR;
    if (y >= a.h) break;
    int j0, j1;
    float fy;
    dh_taps<S>(y, a.ch, oy, j0, j1, fy);
    const float *a0 = lds.fa + j0 * NX, *a1 = lds.fa + j1 * NX, *b0 = lds.fb + j0 * NX, *b1 = lds.fb + j1 * NX;
    float v[3 * PX], m[PX];
    dh_load<T>(src + (size_t)y * a.w * 3, x0, a.w, v);
#pragma unroll
    for (int i = 0; i < PX; i++) {
      const float lum = dh_lum(a, v[3 * i], v[3 * i + 1], v[3 * i + 2]);
      const float au = dh_lerp(dh_lerp(a0[i0[i]], a0[i1[i]], fx[i]), dh_lerp(a1[i0[i]], a1[i1[i]], fx[i]), fy);
      const float bu = dh_lerp(dh_lerp(b0[i0[i]], b0[i1[i]], fx[i]), dh_lerp(b1[i0[i]], b1[i1[i]], fx[i]), fy);
      m[i] = fminf(fmaxf(au * lum + bu, a.floor), 1.0f);
      const float rt = 1.0f / m[i];
#pragma unroll
      for (int c = 0; c < 3; c++) v[3 * i + c] = tdk_pos((v[3 * i + c] - amb[c]) * rt + amb[c]);
      // The sum is a float32 value and the store rounds that to binary16: two roundings.  Left alone, the compiler may fold the add
      // and the conversion into one v_fma_mixlo_f16, which rounds once: the empty asm keeps the float32 sum a value of its own.
      if constexpr (sizeof(T) == 2) asm volatile("" : "+v"(v[3 * i]), "+v"(v[3 * i + 1]), "+v"(v[3 * i + 2]));
    }
    if (dst != nullptr) dh_store<T>(dst + (size_t)y * a.w * 3, x0, a.w, v);
    if (t_out != nullptr) dh_store_plane<PX>(t_out + (size_t)y * a.w, x0, a.w, m);
  }
}

bool dh_cell_ok(int cell) { return cell == 2 || cell == 4 || cell == 8 || cell == 16; }
size_t dh_cells_of(int width, int height, int cell) { return (size_t)tdk_div_up(width, cell) * tdk_div_up(height, cell); }

// Run a statement with the cell size S as a constant; the caller has checked `cell`.
#define DH_DISPATCH_CELL(cell, S, ...)                       \
  do {                                                       \
    if ((cell) == 2) { constexpr int S = 2; __VA_ARGS__; }   \
    else if ((cell) == 4) { constexpr int S = 4; __VA_ARGS__; } \
    else if ((cell) == 8) { constexpr int S = 8; __VA_ARGS__; } \
    else { constexpr int S = 16; __VA_ARGS__; }              \
  } while (0)

template <int S> size_t dh_apply_lds() { return sizeof(DhApplyLds<S>); }

// The launches of a call: cells; with count > 0 dark channel and select; with `apply` coefficients and apply.
template <typename T, int S>
int dh_launch(const void* src, void* dst, float* t_out, float* planes, float* ambient, const DhArgs& a, int count, bool apply, hipStream_t st) {
  constexpr int PX = DhPx<T>::N;
  const size_t n = (size_t)a.cw * a.ch;
  float *dark = planes + 7 * n, *ca = planes + 8 * n, *cb = planes + 9 * n;
  const dim3 block(DH_THREADS);
  const dim3 cells_grid((unsigned)tdk_div_up(a.cw * S, 64 * PX), (unsigned)tdk_div_up(a.ch, (DH_THREADS / 64) * (DH_BAND / S)));
  const dim3 tile_grid((unsigned)tdk_div_up(a.cw, DH_CT), (unsigned)tdk_div_up(a.ch, DH_CT));
  TDK_LAUNCH("tdk_dehaze(cells)", (dh_cells<T, S>), cells_grid, block, 0, st, reinterpret_cast<const T*>(src), planes, a);
  if (count > 0) {
    TDK_LAUNCH("tdk_dehaze(dark)", dh_dark, tile_grid, block, 0, st, planes, dark, a);
    TDK_LAUNCH("tdk_dehaze(select)", dh_select, dim3(1), dim3(DH_SEL_THREADS), 0, st, dark, planes + 3 * n, ambient, (int)n, count);
  }
  if (apply) {
    TDK_LAUNCH("tdk_dehaze(coefficients)", dh_coeff, tile_grid, block, 0, st, planes, ambient, ca, cb, a);
    const dim3 apply_grid((unsigned)tdk_div_up(a.w, DH_TW), (unsigned)tdk_div_up(a.h, DH_TH));
    TDK_LAUNCH("tdk_dehaze(apply)", (dh_apply<T, S>), apply_grid, block, 0, st, reinterpret_cast<const T*>(src), reinterpret_cast<T*>(dst), t_out, ca, cb, ambient, a);
  }
  return TDK_OK;
}

// What both entry points ask of the arguments they share.
int dh_check_common(const char* who, const void* src, const void* workspace, const float* ambient, int width, int height, int dtype, int cell, int dark_radius,
                    int flags) {
  TDK_REQUIRE(src, "%s: null pointer (src)", who);
  TDK_REQUIRE(workspace, "%s: null pointer (workspace)", who);
  TDK_REQUIRE(ambient, "%s: null pointer (ambient)", who);
  TDK_REQUIRE(tdk_frame_size_ok(width, height), "%s: frame size %dx%d outside 1..%d", who, width, height, TDK_FRAME_MAX_SIZE);
  TDK_REQUIRE(tdk_float_dtype_ok(dtype), "%s: unsupported dtype tag %d", who, dtype);
  TDK_REQUIRE(dh_cell_ok(cell), "%s: cell must be 2, 4, 8 or 16, got %d", who, cell);
  TDK_REQUIRE(dh_cells_of(width, height, cell) <= (size_t)TDK_DEHAZE_MAX_CELLS, "%s: the grid of %zu cells is larger than %d", who, dh_cells_of(width, height, cell),
              TDK_DEHAZE_MAX_CELLS);
  TDK_REQUIRE(dark_radius >= 0 && dark_radius <= DH_RD, "%s: dark_radius must be 0..%d, got %d", who, DH_RD, dark_radius);
  TDK_REQUIRE(flags == 0, "%s: flags is reserved and must be 0, got %d", who, flags);
  TDK_REQUIRE(tdk_aligned(ambient, 4), "%s: ambient must be aligned to 4 bytes", who);
  return TDK_OK;
}

}  // namespace

TDK_EXPORT int tdk_dehaze_abi_version(void) { return TDK_DEHAZE_ABI_VERSION; }

TDK_EXPORT size_t tdk_dehaze_workspace_bytes(int width, int height, int cell) {
  if (!tdk_frame_size_ok(width, height) || !dh_cell_ok(cell) || dh_cells_of(width, height, cell) > (size_t)TDK_DEHAZE_MAX_CELLS) return 0;
  return (size_t)TDK_DEHAZE_PLANES * dh_cells_of(width, height, cell) * sizeof(float) + DH_WS_ALIGN;
}

TDK_EXPORT size_t tdk_dehaze_lds_bytes(int dtype, int cell, int dark_radius, int radius) {
  if (!tdk_float_dtype_ok(dtype) || !dh_cell_ok(cell) || dark_radius < 0 || dark_radius > DH_RD || radius < 0 || radius > DH_RG) return 0;
  size_t most = 0;
  DH_DISPATCH_CELL(cell, S, most = dh_apply_lds<S>());
  for (size_t other : {sizeof(DhCoeffLds), sizeof(DhDarkLds), sizeof(DhSelectLds)}) most = other > most ? other : most;
  return most;
}

TDK_EXPORT int tdk_dehaze_ambient(const void* src, float* ambient, void* workspace, int width, int height, int dtype, int cell, int dark_radius, int count, int flags,
                                  tdk_stream_t stream) {
  static const char* const who = "tdk_dehaze_ambient";
  if (const int rc = dh_check_common(who, src, workspace, ambient, width, height, dtype, cell, dark_radius, flags)) return rc;
  const size_t cells = dh_cells_of(width, height, cell);
  TDK_REQUIRE(count >= 1 && (size_t)count <= cells, "%s: count must be 1..%zu (the cells of the grid), got %d", who, cells, count);
  const size_t frame_bytes = (size_t)width * height * 3 * tdk_dtype_bytes(dtype), ws_bytes = tdk_dehaze_workspace_bytes(width, height, cell);
  const size_t amb_bytes = 4 * sizeof(float);
  TDK_REQUIRE(tdk_disjoint(ambient, amb_bytes, src, frame_bytes), "%s: ambient overlaps src", who);
  TDK_REQUIRE(tdk_disjoint(workspace, ws_bytes, src, frame_bytes) && tdk_disjoint(workspace, ws_bytes, ambient, amb_bytes), "%s: the workspace overlaps src or ambient", who);

  DhArgs a{};
  a.w = width, a.h = height, a.cw = tdk_div_up(width, cell), a.ch = tdk_div_up(height, cell);
  a.rd = dark_radius;
  float* planes = reinterpret_cast<float*>(tdk_align_up(reinterpret_cast<uintptr_t>(workspace), DH_WS_ALIGN));
  hipStream_t st = tdk_stream(stream);
  TDK_DISPATCH_DTYPE(dtype, T, DH_DISPATCH_CELL(cell, S, return (dh_launch<T, S>(src, nullptr, nullptr, planes, ambient, a, count, false, st))));
}

TDK_EXPORT int tdk_dehaze(const void* src, void* dst, float* transmission_out, void* workspace, float* ambient, int width, int height, int dtype, int cell,
                          int dark_radius, int radius, int count, float eps, float strength, float floor, const float* weights, int flags, tdk_stream_t stream) {
  static const char* const who = "tdk_dehaze";
  TDK_REQUIRE(dst || transmission_out, "%s: null pointer (dst and transmission_out: one of them is needed)", who);
  TDK_REQUIRE(weights, "%s: null pointer (weights)", who);
  if (const int rc = dh_check_common(who, src, workspace, ambient, width, height, dtype, cell, dark_radius, flags)) return rc;
  const size_t cells = dh_cells_of(width, height, cell);
  TDK_REQUIRE(radius >= 0 && radius <= DH_RG, "%s: radius must be 0..%d, got %d", who, DH_RG, radius);
  TDK_REQUIRE(count >= 0 && (size_t)count <= cells, "%s: count must be 0..%zu (the cells of the grid), got %d", who, cells, count);
  TDK_REQUIRE(eps > 0.0f && isfinite(eps), "%s: eps must be finite and > 0", who);
  TDK_REQUIRE(strength >= 0.0f && strength <= 1.0f, "%s: strength must be in 0..1", who);
  TDK_REQUIRE(floor >= 0x1p-6f && floor <= 1.0f, "%s: floor must be in 2^-6..1", who);
  const int bad_weight = tdk_first_bad_weight(weights, 3);
  TDK_REQUIRE(bad_weight < 0, "%s: weights must be finite and >= 0 (weights[%d])", who, bad_weight);
  TDK_REQUIRE(tdk_aligned(transmission_out, 4), "%s: transmission_out must be aligned to 4 bytes", who);
  const size_t n = (size_t)width * height, frame_bytes = n * 3 * tdk_dtype_bytes(dtype), plane_bytes = n * sizeof(float);
  const size_t ws_bytes = tdk_dehaze_workspace_bytes(width, height, cell), amb_bytes = 4 * sizeof(float);
  float* const t_out = transmission_out;
  TDK_REQUIRE(!dst || tdk_disjoint(src, frame_bytes, dst, frame_bytes), "%s: src and dst overlap", who);
  TDK_REQUIRE(!t_out || (tdk_disjoint(t_out, plane_bytes, src, frame_bytes) && (!dst || tdk_disjoint(t_out, plane_bytes, dst, frame_bytes))),
              "%s: transmission_out overlaps src or dst", who);
  TDK_REQUIRE(tdk_disjoint(ambient, amb_bytes, src, frame_bytes) && (!dst || tdk_disjoint(ambient, amb_bytes, dst, frame_bytes)) &&
                  (!t_out || tdk_disjoint(ambient, amb_bytes, t_out, plane_bytes)),
              "%s: ambient overlaps src, dst or transmission_out", who);
  TDK_REQUIRE(tdk_disjoint(workspace, ws_bytes, src, frame_bytes) && (!dst || tdk_disjoint(workspace, ws_bytes, dst, frame_bytes)) &&
                  (!t_out || tdk_disjoint(workspace, ws_bytes, t_out, plane_bytes)) && tdk_disjoint(workspace, ws_bytes, ambient, amb_bytes),
              "%s: the workspace overlaps src, dst, transmission_out or ambient", who);

  DhArgs a{};
  a.w = width, a.h = height, a.cw = tdk_div_up(width, cell), a.ch = tdk_div_up(height, cell);
  a.rd = dark_radius, a.rg = radius;
  a.inv = (float)(1.0 / (double)((2 * radius + 1) * (2 * radius + 1)));
  a.eps = eps, a.strength = strength, a.floor = floor;
  a.w0 = weights[0], a.w1 = weights[1], a.w2 = weights[2];
  float* planes = reinterpret_cast<float*>(tdk_align_up(reinterpret_cast<uintptr_t>(workspace), DH_WS_ALIGN));
  hipStream_t st = tdk_stream(stream);
  TDK_DISPATCH_DTYPE(dtype, T, DH_DISPATCH_CELL(cell, S, return (dh_launch<T, S>(src, dst, t_out, planes, ambient, a, count, true, st))));
}
