// cacorrect.hip -- lateral chromatic aberration on raw mosaics (include/tdk_hip_ca.h): tdk_ca_correct, one tile launch, and
// tdk_ca_estimate, one gather launch per frame and one finishing launch.
//
// The specification is the head comment of include/tdk_hip_ca.h.
//
// ca_correct<TS, TO, CUBIC>: a workgroup of 256 lanes owns CA_TH = 32 rows of CA_TW = 64 sites.
//   1. the box -- the tile and its apron of LO sites left and above, HI right and below -- is staged as float32, units of four sites
//      round-robin over the lanes; only sites inside the frame are read, the others are staged as 0 and never used (tap indices are
//      clamped into the plane, that is into the frame).
//   2. a lane takes pairs (a red or blue site, the green site next to it): a 32-lane half of a wave takes 16 pairs of a row and the 16
//      pairs below them, so that its taps alternate between even and odd LDS banks (the header: Tile shape).
// ca_gather<TS>: a workgroup per block; a lane walks CFA cells, keeps the 17 sums of one colour in registers (the colours one after the
//      other), the waves reduce them by shuffles and 17 lanes write or add to the record.
// ca_finish: one workgroup, chunks of 256 blocks: a lane per block for the fit of step 2 writes the block's terms of step 3 into LDS,
//      then 20 lanes add them in ascending block order, one sum each (a walk over LDS whose only chain is the float64 addition), and
//      two lanes solve.
#include <math.h>

#include "../../include/tdk_hip_ca.h"
#include "tdk_frame.h"

namespace {

constexpr int CA_TW = TDK_CA_TILE_W, CA_TH = TDK_CA_TILE_H;
constexpr int CA_THREADS = 256;
constexpr int CA_D = TDK_CA_MAX_SHIFT;
constexpr int CA_SUMS = TDK_CA_SUMS;
constexpr int CA_TERMS = 10;   // per colour the nine sums of step 3 and the number of kept blocks

template <bool CUBIC> struct CaBox {
  static constexpr int LO = CUBIC ? 12 : 8, HI = 12;   // sites of apron: D + the taps, in whole units of four
  static constexpr int SW = CA_TW + LO + HI, SH = CA_TH + LO + HI;
  static constexpr int UNITS = SW / 4;
  static constexpr int T_LO = CUBIC ? -1 : 0, T_HI = CUBIC ? 2 : 1;   // taps around the floor, in plane samples
  static_assert(LO % 4 == 0 && HI % 4 == 0, "whole units");
  static_assert(2 * (CA_D / 2 - T_LO) <= LO && 2 * (CA_D / 2 + T_HI) <= HI, "the apron holds D and the taps");
  static_assert(SW % 32 == 24 || SW % 32 == 20, "rows of opposite column parity fall on banks of opposite parity (the stride is even)");
};
template <bool CUBIC> struct CaLds {
  alignas(16) float box[CaBox<CUBIC>::SH * CaBox<CUBIC>::SW];
};
static_assert(sizeof(CaLds<true>) <= 64 * 1024, "LDS of the correction launch");

struct CaArgs {
  const void* src;
  void* out;
  const float* model;
  int w, h;
  uint32_t pattern;
  float x0, y0, rn;
};

template <typename T> __device__ __forceinline__ bool ca_aligned(const T* p, uintptr_t bytes) { return (reinterpret_cast<uintptr_t>(p) & (bytes - 1)) == 0; }

// four consecutive elements at p as float32: one 16-byte (float32) or 8-byte (binary16) read when p is on such a boundary
__device__ __forceinline__ void ca_load4(const float* p, float x[4]) {
  if (ca_aligned(p, 16)) {
    const float4 u = *reinterpret_cast<const float4*>(p);
    x[0] = u.x, x[1] = u.y, x[2] = u.z, x[3] = u.w;
  } else {
#pragma unroll
    for (int m = 0; m < 4; m++) x[m] = p[m];
  }
}
__device__ __forceinline__ void ca_load4(const __half* p, float x[4]) {
  if (ca_aligned(p, 8)) {
    const uint2 u = *reinterpret_cast<const uint2*>(p);
    x[0] = __half2float(__ushort_as_half((unsigned short)(u.x & 0xffffu))), x[1] = __half2float(__ushort_as_half((unsigned short)(u.x >> 16)));
    x[2] = __half2float(__ushort_as_half((unsigned short)(u.y & 0xffffu))), x[3] = __half2float(__ushort_as_half((unsigned short)(u.y >> 16)));
  } else {
#pragma unroll
    for (int m = 0; m < 4; m++) x[m] = __half2float(p[m]);
  }
}
// two consecutive elements
__device__ __forceinline__ void ca_store2(float* p, float a, float b) {
  if (ca_aligned(p, 8)) *reinterpret_cast<float2*>(p) = make_float2(a, b);
  else p[0] = a, p[1] = b;
}
__device__ __forceinline__ void ca_store2(__half* p, float a, float b) {
  const uint32_t w = (uint32_t)__half_as_ushort(__float2half_rn(a)) | ((uint32_t)__half_as_ushort(__float2half_rn(b)) << 16);
  if (ca_aligned(p, 4)) *reinterpret_cast<uint32_t*>(p) = w;
  else p[0] = __float2half_rn(a), p[1] = __float2half_rn(b);
}

// the weights of tdk_hip_warp.h
__device__ __forceinline__ float ca_c1(float t) { return ((1.25f * t - 2.25f) * t) * t + 1.0f; }
__device__ __forceinline__ float ca_c2(float t) { return ((-0.75f * t + 3.75f) * t - 6.0f) * t + 3.0f; }
template <bool CUBIC> __device__ __forceinline__ void ca_weights(float a, float w[4]) {
  if constexpr (CUBIC) w[0] = ca_c2(a + 1.0f), w[1] = ca_c1(a), w[2] = ca_c1(1.0f - a), w[3] = ca_c2(2.0f - a);
  else w[0] = 1.0f - a, w[1] = a, w[2] = 0.0f, w[3] = 0.0f;
}

template <typename TS, typename TO, bool CUBIC>
__global__ __launch_bounds__(CA_THREADS) void ca_correct(CaArgs a) {
  using B = CaBox<CUBIC>;
  __shared__ CaLds<CUBIC> lds;
  const int tid = threadIdx.x;
  const int tx0 = (int)blockIdx.x * CA_TW, ty0 = (int)blockIdx.y * CA_TH;
  const TS* __restrict__ src = reinterpret_cast<const TS*>(a.src);
  TO* __restrict__ out = reinterpret_cast<TO*>(a.out);

  // ---- 1. the box
#pragma unroll 1
  for (int t = tid; t < B::SH * B::UNITS; t += CA_THREADS) {
    const int brow = t / B::UNITS, unit = t % B::UNITS;
    const int i = ty0 - B::LO + brow, j = tx0 - B::LO + 4 * unit;
    float x[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (i >= 0 && i < a.h && j >= 0 && j < a.w) {   // (j is even and so is the width: two or four sites of the unit are inside)
      const size_t at = (size_t)i * (size_t)a.w + (size_t)j;
      if (j + 4 <= a.w) ca_load4(src + at, x);
      else x[0] = ld<TS>(src, at), x[1] = ld<TS>(src, at + 1);
    }
    *reinterpret_cast<float4*>(lds.box + brow * B::SW + 4 * unit) = make_float4(x[0], x[1], x[2], x[3]);
  }
  __syncthreads();

  // ---- 2. the pairs.  Lane: wave, half (a segment of 32 columns), the row of a pair of rows, 16 pairs of that row.
  const int wave = tid >> 6, seg = (tid >> 5) & 1, sub = (tid >> 4) & 1, pair = tid & 15;
  const int pw = a.w >> 1, ph = a.h >> 1;
#pragma unroll 1
  for (int pass = 0; pass < CA_TH / 8; pass++) {
    const int ty = 8 * pass + 2 * wave + sub, tx = 32 * seg + 2 * pair;
    const int i = ty0 + ty, j = tx0 + tx;   // the even column of the pair
    if (i >= a.h || j >= a.w) continue;
    const float* centre = lds.box + (ty + B::LO) * B::SW + (tx + B::LO);
    const float2 both = *reinterpret_cast<const float2*>(centre);
    const int k0 = cfa_color(i, j, a.pattern);
    const int par = k0 == 1 ? 1 : 0;                       // the column parity of the red or blue site of this row
    const int k = k0 == 1 ? cfa_color(i, j + 1, a.pattern) : k0;
    const float* row = a.model + (k == 0 ? 0 : 4);
    const float v = row[0], c = row[1], b = row[2];
    const bool valid = row[3] != 0.0f;
    const int jj = j + par;
    float value = par ? both.y : both.x;
    if (valid) {
      const float px = (float)jj - a.x0, py = (float)i - a.y0;
      const float r2 = px * px + py * py;
      const float rho = sqrtf(r2) / a.rn;
      const float s = (b * rho + c) * rho + v;
      const float t = s - 1.0f;
      float dx = px * t, dy = py * t;
      if (!(isfinite(dx) && isfinite(dy))) dx = dy = 0.0f;
      dx = fminf(fmaxf(dx, -(float)CA_D), (float)CA_D);
      dy = fminf(fmaxf(dy, -(float)CA_D), (float)CA_D);
      if (!(dx == 0.0f && dy == 0.0f)) {
        const int pj = jj >> 1, pi = i >> 1;
        const float u = (float)pj + dx * 0.5f, w = (float)pi + dy * 0.5f;
        const float xf = floorf(u), yf = floorf(w);
        const float ax = u - xf, ay = w - yf;
        // (|d| <= D puts the floors within D / 2 samples of the site; the integer clamp states it for the LDS addresses)
        const int ix = min(max((int)xf, pj - CA_D / 2), pj + CA_D / 2), iy = min(max((int)yf, pi - CA_D / 2), pi + CA_D / 2);
        float wx[4], wy[4];
        ca_weights<CUBIC>(ax, wx);
        ca_weights<CUBIC>(ay, wy);
        constexpr int TAPS = B::T_HI - B::T_LO + 1;
        int col[TAPS];
#pragma unroll
        for (int n = 0; n < TAPS; n++) col[n] = 2 * min(max(ix + B::T_LO + n, 0), pw - 1) + par - (tx0 - B::LO);   // box column
        float acc = 0.0f;
#pragma unroll
        for (int m = 0; m < TAPS; m++) {
          const int brow = 2 * min(max(iy + B::T_LO + m, 0), ph - 1) + (i & 1) - (ty0 - B::LO);
          const float* line = lds.box + brow * B::SW;
          float r = line[col[0]] * wx[0] + line[col[1]] * wx[1];
          if constexpr (CUBIC) r = (r + line[col[2]] * wx[2]) + line[col[3]] * wx[3];
          acc = m == 0 ? r * wy[0] : acc + r * wy[m];
        }
        value = acc;
      }
    }
    const size_t at = (size_t)i * (size_t)a.w + (size_t)j;
    ca_store2(out + at, par ? both.x : value, par ? value : both.y);
  }
}

template <typename TS, typename TO> int ca_launch_correct(const CaArgs& a, int interp, hipStream_t st) {
  const dim3 grid((unsigned)tdk_div_up(a.w, CA_TW), (unsigned)tdk_div_up(a.h, CA_TH)), block(CA_THREADS);
  if (interp == TDK_CA_BICUBIC) TDK_LAUNCH("tdk_ca_correct", (ca_correct<TS, TO, true>), grid, block, 0, st, a);
  else TDK_LAUNCH("tdk_ca_correct", (ca_correct<TS, TO, false>), grid, block, 0, st, a);
  return TDK_OK;
}

// ---------------------------------------------------------------- the estimator
struct CaGatherArgs {
  const void* frame;
  long long* sums;
  int w, h, block, nbx;
  uint32_t pattern;
  float clip;
  int first;
};

__device__ __forceinline__ bool ca_usable(float x, float clip) { return isfinite(x) && x < clip; }
__device__ __forceinline__ int ca_quantise(float x) { return (int)fminf(fmaxf(rintf(x * TDK_CA_QSCALE), 0.0f), (float)TDK_CA_QMAX); }

template <typename TS>
__global__ __launch_bounds__(CA_THREADS) void ca_gather(CaGatherArgs a) {
  __shared__ long long part[CA_THREADS / 64][CA_SUMS];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const TS* __restrict__ src = reinterpret_cast<const TS*>(a.frame);
  const int bx = (int)blockIdx.x, by = (int)blockIdx.y;
  const int cells = a.block >> 1;   // CFA cells per block side
#pragma unroll 1
  for (int kk = 0; kk < 2; kk++) {
    const int colour = 2 * kk;   // red, blue
    // where the colour sits in a CFA cell
    int oy = 0, ox = 0;
#pragma unroll
    for (int p = 0; p < 4; p++)
      if ((int)((a.pattern >> (2 * p)) & 3u) == colour) oy = p >> 1, ox = p & 1;
    long long s[CA_SUMS];
#pragma unroll
    for (int n = 0; n < CA_SUMS; n++) s[n] = 0;
#pragma unroll 1
    for (int t = tid; t < cells * cells; t += CA_THREADS) {
      const int i = by * a.block + 2 * (t / cells) + oy, j = bx * a.block + 2 * (t % cells) + ox;
      if (i < 1 || j < 1 || i > a.h - 2 || j > a.w - 2) continue;
      const size_t at = (size_t)i * (size_t)a.w + (size_t)j;
      const float xc = ld<TS>(src, at), xl = ld<TS>(src, at - 1), xr = ld<TS>(src, at + 1), xu = ld<TS>(src, at - (size_t)a.w), xd = ld<TS>(src, at + (size_t)a.w);
      if (!(ca_usable(xc, a.clip) && ca_usable(xl, a.clip) && ca_usable(xr, a.clip) && ca_usable(xu, a.clip) && ca_usable(xd, a.clip))) continue;
      const int gl = ca_quantise(xl), gr = ca_quantise(xr), gu = ca_quantise(xu), gd = ca_quantise(xd);
      const long long C = ca_quantise(xc), G4 = (gl + gr) + (gu + gd), gx = gr - gl, gy = gd - gu;
      s[0] += 1, s[1] += j, s[2] += i;
      s[3] += G4, s[4] += gx, s[5] += gy, s[6] += C;
      s[7] += G4 * G4, s[8] += G4 * gx, s[9] += G4 * gy, s[10] += G4 * C;
      s[11] += gx * gx, s[12] += gx * gy, s[13] += gx * C;
      s[14] += gy * gy, s[15] += gy * C, s[16] += C * C;
    }
#pragma unroll
    for (int n = 0; n < CA_SUMS; n++) {
      long long v = s[n];
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
      if (lane == 0) part[wave][n] = v;
    }
    __syncthreads();
    if (tid < CA_SUMS) {
      long long* rec = a.sums + ((size_t)(by * a.nbx + bx) * 2 + kk) * CA_SUMS;
      long long v = a.first ? 0 : rec[tid];
#pragma unroll
      for (int wv = 0; wv < CA_THREADS / 64; wv++) v += part[wv][tid];
      rec[tid] = v;
    }
    __syncthreads();
  }
}

struct CaFinishArgs {
  const long long* sums;
  const float* noise;
  float* model;
  int blocks, fit;
  double max_shift, x0, y0, rn;
};

struct CaSolve {
  double det, x0, x1, x2, C11, C22;
};
// the cofactor formulas of the header for the symmetric N and the right-hand side r
__device__ __forceinline__ CaSolve ca_solve(double N00, double N01, double N02, double N11, double N12, double N22, double r0, double r1, double r2) {
  const double C00 = N11 * N22 - N12 * N12, C01 = N02 * N12 - N01 * N22, C02 = N01 * N12 - N02 * N11;
  const double C11 = N00 * N22 - N02 * N02, C12 = N01 * N02 - N00 * N12, C22 = N00 * N11 - N01 * N01;
  CaSolve o;
  o.det = (N00 * C00 + N01 * C01) + N02 * C02;
  o.x0 = ((C00 * r0 + C01 * r1) + C02 * r2) / o.det;
  o.x1 = ((C01 * r0 + C11 * r1) + C12 * r2) / o.det;
  o.x2 = ((C02 * r0 + C12 * r1) + C22 * r2) / o.det;
  o.C11 = C11, o.C22 = C22;
  return o;
}

__global__ __launch_bounds__(CA_THREADS) void ca_finish(CaFinishArgs a) {
  // terms of step 3 of one chunk of CA_THREADS blocks: per colour the nine sums of the header and, tenth, the kept flag
  __shared__ double term[2 * CA_TERMS][CA_THREADS];
  __shared__ double acc[2 * CA_TERMS];
  const int tid = threadIdx.x;
  const bool noisy = a.noise != nullptr && a.noise[4 + 2] != 0.0f;
  const double na = noisy ? (double)a.noise[4] : 0.0, nb = noisy ? (double)a.noise[4 + 1] : 0.0;
  double sum = 0.0;   // of lane tid < 2 * CA_TERMS: sum tid % CA_TERMS of colour tid / CA_TERMS
#pragma unroll 1
  for (int base = 0; base < a.blocks; base += CA_THREADS) {
    // ---- step 2: a lane per block of the chunk, the colours one after the other
    const int blk = base + tid;
#pragma unroll 1
    for (int kk = 0; kk < 2; kk++) {
      bool kept = false;
      double g = 0.0, h = 0.0, rho = 0.0;
      if (blk < a.blocks) {
        const long long* rec = a.sums + ((size_t)blk * 2 + kk) * CA_SUMS;
        const double n = (double)rec[0];
        if (rec[0] >= TDK_CA_MIN_SITES) {
          const double s1 = (double)rec[3], s2 = (double)rec[4], s3 = (double)rec[5], s4 = (double)rec[6];
          const double c11 = (double)rec[7] - (s1 * s1) / n, c12 = (double)rec[8] - (s1 * s2) / n, c13 = (double)rec[9] - (s1 * s3) / n;
          const double c14 = (double)rec[10] - (s1 * s4) / n, c22 = (double)rec[11] - (s2 * s2) / n, c23 = (double)rec[12] - (s2 * s3) / n;
          const double c24 = (double)rec[13] - (s2 * s4) / n, c33 = (double)rec[14] - (s3 * s3) / n, c34 = (double)rec[15] - (s3 * s4) / n;
          double N00 = c11 / 16.0, N01 = c12 / 8.0, N02 = c13 / 8.0, N11 = c22 / 4.0, N12 = c23 / 4.0, N22 = c33 / 4.0;
          const double r0 = c14 / 4.0, r1 = c24 / 2.0, r2 = c34 / 2.0;
          if (noisy) {
            const double Q = (double)TDK_CA_QSCALE;
            const double nv = (Q * Q) * ((na * ((s1 / 4.0) / Q)) + nb * n);
            N00 -= nv / 4.0, N11 -= nv / 2.0, N22 -= nv / 2.0;
          }
          const CaSolve f = ca_solve(N00, N01, N02, N11, N12, N22, r0, r1, r2);
          const double kappa = f.x0, dx = f.x1 / kappa, dy = f.x2 / kappa;
          kept = N00 > 0.0 && N11 > 0.0 && N22 > 0.0 && f.det > 0.0 && f.C11 > 0.0 && f.C22 > 0.0 && kappa > 0.0 && fabs(dx) <= a.max_shift && fabs(dy) <= a.max_shift;
          if (kept) {
            const double wx = f.det / f.C11, wy = f.det / f.C22;
            const double cx = (double)rec[1] / n - a.x0, cy = (double)rec[2] / n - a.y0;
            rho = sqrt(cx * cx + cy * cy) / a.rn;
            g = (wx * cx) * cx + (wy * cy) * cy;
            h = -((wx * cx) * dx + (wy * cy) * dy);
          }
        }
      }
      // a dropped block adds +0.0 to every sum: no sum that starts at +0.0 is ever -0.0, so that is the sum without it, bit for bit
      const double phi1 = rho, phi2 = rho * rho;
      double (*t)[CA_THREADS] = term + CA_TERMS * kk;
      t[0][tid] = kept ? (g * 1.0) * 1.0 : 0.0, t[1][tid] = kept ? (g * 1.0) * phi1 : 0.0, t[2][tid] = kept ? (g * 1.0) * phi2 : 0.0;
      t[3][tid] = kept ? (g * phi1) * phi1 : 0.0, t[4][tid] = kept ? (g * phi1) * phi2 : 0.0, t[5][tid] = kept ? (g * phi2) * phi2 : 0.0;
      t[6][tid] = kept ? h * 1.0 : 0.0, t[7][tid] = kept ? h * phi1 : 0.0, t[8][tid] = kept ? h * phi2 : 0.0;
      t[9][tid] = kept ? 1.0 : 0.0;
    }
    __syncthreads();
    // ---- step 3: a lane per sum, the blocks of the chunk in ascending order
    if (tid < 2 * CA_TERMS) {
      const double* mine = term[tid];
#pragma unroll 8
      for (int n = 0; n < CA_THREADS; n++) sum += mine[n];
    }
    __syncthreads();
  }
  if (tid < 2 * CA_TERMS) acc[tid] = sum;
  __syncthreads();
  if (tid < 2) {
    const double* A = acc + CA_TERMS * tid;
    const double count = A[9];   // (an integer below 2^53: exact)
    double e = 0.0, c = 0.0, b = 0.0;
    bool ok;
    if (a.fit == TDK_CA_LINEAR) {
      e = A[6] / A[0];
      ok = count >= 1.0 && A[0] > 0.0;
    } else {
      const CaSolve f = ca_solve(A[0], A[1], A[2], A[3], A[4], A[5], A[6], A[7], A[8]);
      e = f.x0, c = f.x1, b = f.x2;
      ok = count >= 3.0 && f.det > 0.0;
    }
    const float v32 = (float)(1.0 + e), c32 = (float)c, b32 = (float)b;
    ok = ok && isfinite(v32) && isfinite(c32) && isfinite(b32);
    float* row = a.model + 4 * tid;
    row[0] = ok ? v32 : 1.0f, row[1] = ok ? c32 : 0.0f, row[2] = ok ? b32 : 0.0f, row[3] = ok ? 1.0f : 0.0f;
  }
}

template <typename TS> int ca_launch_gather(const CaGatherArgs& a, int nby, hipStream_t st) {
  const dim3 grid((unsigned)a.nbx, (unsigned)nby), block(CA_THREADS);
  TDK_LAUNCH("tdk_ca_gather", (ca_gather<TS>), grid, block, 0, st, a);
  return TDK_OK;
}

int ca_launch_finish(const CaFinishArgs& a, hipStream_t st) {
  TDK_LAUNCH("tdk_ca_finish", ca_finish, dim3(1), dim3(CA_THREADS), 0, st, a);
  return TDK_OK;
}

bool ca_dtype_ok(int dtype) { return dtype == TDK_F32 || dtype == TDK_F16; }
bool ca_block_ok(int block) { return block >= 16 && block <= 256 && block % 2 == 0; }

}  // namespace

TDK_EXPORT int tdk_ca_abi_version(void) { return TDK_CA_ABI_VERSION; }

TDK_EXPORT size_t tdk_ca_lds_bytes(int interp, int src_dtype) {
  if (!ca_dtype_ok(src_dtype)) return 0;
  return interp == TDK_CA_BILINEAR ? sizeof(CaLds<false>) : interp == TDK_CA_BICUBIC ? sizeof(CaLds<true>) : 0;
}

TDK_EXPORT int tdk_ca_correct(const void* src, int src_dtype, void* out, int out_dtype, int width, int height, uint32_t pattern, const float* model, float x0,
                              float y0, float rn, int interp, tdk_stream_t stream) {
  static const char* const who = "tdk_ca_correct";
  TDK_REQUIRE(src && out && model, "%s: null pointer (src, out or model)", who);
  TDK_REQUIRE(ca_dtype_ok(src_dtype) && ca_dtype_ok(out_dtype), "%s: unsupported dtype tags %d -> %d", who, src_dtype, out_dtype);
  TDK_REQUIRE(tdk_mosaic_size_ok(width, height), "%s: frame size %dx%d outside 2..%d", who, width, height, TDK_MOSAIC_MAX_SIZE);
  TDK_REQUIRE(width % 2 == 0 && height % 2 == 0, "%s: mosaic size %dx%d must be even in both axes (whole CFA cells)", who, width, height);
  TDK_REQUIRE(tdk_pattern_ok(pattern), "%s: unknown Bayer pattern 0x%08x", who, pattern);
  TDK_REQUIRE(interp == TDK_CA_BILINEAR || interp == TDK_CA_BICUBIC, "%s: interp must be 0 (bilinear) or 1 (bicubic), got %d", who, interp);
  TDK_REQUIRE(isfinite(x0) && isfinite(y0), "%s: the centre must be finite", who);
  TDK_REQUIRE(isfinite(rn) && rn > 0.0f, "%s: rn must be finite and > 0", who);
  const size_t sites = (size_t)width * (size_t)height;
  const size_t src_bytes = sites * tdk_dtype_bytes(src_dtype), out_bytes = sites * tdk_dtype_bytes(out_dtype);
  TDK_REQUIRE(tdk_disjoint(src, src_bytes, out, out_bytes), "%s: out overlaps src", who);
  TDK_REQUIRE(tdk_disjoint(model, 32, out, out_bytes), "%s: out overlaps the model", who);

  CaArgs a{};
  a.src = src, a.out = out, a.model = model, a.w = width, a.h = height, a.pattern = pattern, a.x0 = x0, a.y0 = y0, a.rn = rn;
  hipStream_t st = tdk_stream(stream);
  if (src_dtype == TDK_F32) return out_dtype == TDK_F32 ? ca_launch_correct<float, float>(a, interp, st) : ca_launch_correct<float, __half>(a, interp, st);
  return out_dtype == TDK_F32 ? ca_launch_correct<__half, float>(a, interp, st) : ca_launch_correct<__half, __half>(a, interp, st);
}

TDK_EXPORT size_t tdk_ca_workspace_bytes(int width, int height, int block) {
  if (!tdk_mosaic_size_ok(width, height) || width % 2 || height % 2 || !ca_block_ok(block)) return 0;
  const size_t blocks = (size_t)(width / block) * (size_t)(height / block);
  const size_t bytes = blocks * 2 * CA_SUMS * sizeof(long long);
  return bytes < 16 ? 16 : bytes;
}

TDK_EXPORT int tdk_ca_estimate(const void* const* frames, int num_frames, int src_dtype, int width, int height, uint32_t pattern, const float* noise_model,
                               int fit, float clip, int block, float max_shift, float x0, float y0, float rn, void* workspace, float* model,
                               tdk_stream_t stream) {
  static const char* const who = "tdk_ca_estimate";
  TDK_REQUIRE(frames && workspace && model, "%s: null pointer (frames, workspace or model)", who);
  TDK_REQUIRE(num_frames >= 1 && num_frames <= TDK_CA_MAX_FRAMES, "%s: num_frames must be 1..%d, got %d", who, TDK_CA_MAX_FRAMES, num_frames);
  for (int f = 0; f < num_frames; f++) TDK_REQUIRE(frames[f], "%s: null pointer (frame %d)", who, f);
  TDK_REQUIRE(ca_dtype_ok(src_dtype), "%s: unsupported dtype tag %d", who, src_dtype);
  TDK_REQUIRE(tdk_mosaic_size_ok(width, height), "%s: frame size %dx%d outside 2..%d", who, width, height, TDK_MOSAIC_MAX_SIZE);
  TDK_REQUIRE(width % 2 == 0 && height % 2 == 0, "%s: mosaic size %dx%d must be even in both axes (whole CFA cells)", who, width, height);
  TDK_REQUIRE(tdk_pattern_ok(pattern), "%s: unknown Bayer pattern 0x%08x", who, pattern);
  TDK_REQUIRE(fit == TDK_CA_LINEAR || fit == TDK_CA_POLY3, "%s: fit must be 0 (linear) or 1 (poly3), got %d", who, fit);
  TDK_REQUIRE(isfinite(clip) && clip > 0.0f, "%s: clip must be finite and > 0", who);
  TDK_REQUIRE(ca_block_ok(block), "%s: block must be even, 16..256, got %d", who, block);
  TDK_REQUIRE(isfinite(max_shift) && max_shift > 0.0f && max_shift <= (float)CA_D, "%s: max_shift must be in (0, %d]", who, CA_D);
  TDK_REQUIRE(isfinite(x0) && isfinite(y0), "%s: the centre must be finite", who);
  TDK_REQUIRE(isfinite(rn) && rn > 0.0f, "%s: rn must be finite and > 0", who);
  const size_t src_bytes = (size_t)width * (size_t)height * tdk_dtype_bytes(src_dtype);
  const size_t ws_bytes = tdk_ca_workspace_bytes(width, height, block);
  for (int f = 0; f < num_frames; f++)
    TDK_REQUIRE(tdk_disjoint(frames[f], src_bytes, workspace, ws_bytes) && tdk_disjoint(frames[f], src_bytes, model, 32), "%s: workspace or model overlaps frame %d",
                who, f);
  TDK_REQUIRE(tdk_disjoint(workspace, ws_bytes, model, 32), "%s: workspace and model overlap", who);
  TDK_REQUIRE(!noise_model || (tdk_disjoint(noise_model, 48, workspace, ws_bytes) && tdk_disjoint(noise_model, 48, model, 32)),
              "%s: the noise model overlaps workspace or model", who);

  const int nbx = width / block, nby = height / block;
  const int blocks = nbx * nby;
  long long* sums = reinterpret_cast<long long*>(workspace);
  hipStream_t st = tdk_stream(stream);
  if (blocks > 0) {
    for (int f = 0; f < num_frames; f++) {
      CaGatherArgs g{};
      g.frame = frames[f], g.sums = sums, g.w = width, g.h = height, g.block = block, g.nbx = nbx, g.pattern = pattern, g.clip = clip, g.first = f == 0;
      const int rc = src_dtype == TDK_F32 ? ca_launch_gather<float>(g, nby, st) : ca_launch_gather<__half>(g, nby, st);
      if (rc != TDK_OK) return rc;
    }
  }
  CaFinishArgs fa{};
  fa.sums = sums, fa.noise = noise_model, fa.model = model;
  fa.blocks = blocks, fa.fit = fit, fa.max_shift = (double)max_shift, fa.x0 = (double)x0, fa.y0 = (double)y0, fa.rn = (double)rn;
  return ca_launch_finish(fa, st);
}
