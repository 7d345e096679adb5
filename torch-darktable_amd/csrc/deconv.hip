// deconv.hip -- capture sharpening: Richardson-Lucy deconvolution of the luminance with a contrast mask (include/tdk_hip_deconv.h:
// tdk_deconv), ceil(N / F) launches of one kernel.
//
// The specification is the head comment of include/tdk_hip_deconv.h.
//
// A workgroup of four waves owns DC_T x DC_T = 32 x 32 pixels and runs nf <= F whole iterations for them inside LDS.  With R the
// radius and A = 2 R nf the apron, PW = 32 + 2 A; four float32 planes of PW x PW values, all at the pitch PW:
//   u   the estimate, staged from the workspace plane the launch before wrote (the first launch: u = o)
//   o   fmaxf(Y, TINY), recomputed from src by every launch: the frame is read anyway by the last launch, its lines are shared
//       through L2 by neighbouring tiles, and a plane of o would cost a write of 4 bytes per pixel and a third workspace plane
//   h   a horizontally blurred plane (of u, then of q)
//   q   o / fmaxf(G(u), TINY)
// Every staged position holds the value of the CLAMPED pixel, and every blur of a staged position is centred on the clamped
// pixel's place in LDS: a position outside the frame thereby holds exactly what the pixel on the edge holds, in every iteration,
// which is the specification's rule for taps outside the frame.  A clamped pixel lies between the position and the tile, so its
// taps stay inside the region the pass before made valid.
// One iteration, with [lo, hi) the rows and columns of u that are valid (lo = 2 R j in iteration j, hi = PW - lo):
//   1. h = rows of u        rows [lo, hi)           columns [lo + R, hi - R)
//   2. q = o / max(cols of h, TINY)                 rows and columns [lo + R, hi - R)
//   3. h = rows of q        rows [lo + R, hi - R)   columns [lo + 2R, hi - 2R)
//   4. u = u * cols of h                            rows and columns [lo + 2R, hi - 2R)
// each a pass of the 256 threads over the region in row order (consecutive lanes, consecutive words of LDS) with a barrier behind
// it.  A workgroup whose staged region lies inside the frame clamps nothing and runs the passes four columns per thread (dc_rows4,
// dc_cols4 below: the same operations per valid position).  After nf iterations the tile itself is valid.  A launch that is not the last stores u of its tile to the other workspace
// plane; the last forms the mask from the 3x3 neighbourhood of o in LDS (A >= 2 > 1), the gain, and scales the pixels.
// The epilogue gives a thread DC_PIX = 4 adjacent pixels of a tile row: where the frame has whole groups (width % 4 == 0) and a
// buffer starts on the vector's alignment they move as vectors of four elements, per element otherwise (DC_VEC_*).  Staging is
// always per element: its runs start A pixels left of the tile, at any alignment.
// No pixel's arithmetic depends on the tile or on F, nothing is accumulated across lanes: the bits depend on neither F nor scheduling.
#include <math.h>

#include "../../include/tdk_hip_deconv.h"
#include "tdk_frame.h"

namespace {

constexpr int DC_THREADS = 256;
constexpr int DC_T = TDK_DECONV_TILE, DC_PIX = 4, DC_GROUPS = DC_T / DC_PIX;   // 8 threads per tile row, 32 rows
constexpr int DC_MAX_R = TDK_DECONV_MAX_RADIUS;
constexpr float DC_TINY = 0x1p-20f;
constexpr float DC_MAX_GAIN = 16.0f;
constexpr size_t DC_WS_ALIGN = 16;
constexpr int DC_STAGE = 4;              // positions a thread stages per round
static_assert(DC_THREADS == DC_GROUPS * DC_T, "a thread per 4 pixels of the tile");

// The instantiation that fuses F iterations takes radii up to RMAX: its apron 2 * RMAX * F keeps four planes within 64 KB.
template <int F> struct DcGeom {
  static constexpr int RMAX = F == 1 ? 6 : F == 2 ? 4 : 2;
  static constexpr int APRON = 2 * RMAX * F;
  static constexpr int P = DC_T + 2 * APRON;
};
template <int F> struct DcLds {
  static constexpr int N = DcGeom<F>::P * DcGeom<F>::P;
  alignas(16) float u[N], o[N], h[N], q[N];   // (N * 4 is a multiple of 16: every plane and, PW being a multiple of 4, every row starts on 16 bytes)
};
static_assert(sizeof(DcLds<1>) <= 64 * 1024 && sizeof(DcLds<2>) <= 64 * 1024 && sizeof(DcLds<4>) <= 64 * 1024, "LDS of the largest call");

struct DcArgs {
  float w[DC_MAX_R + 1];
  float l0, l1, l2;
  float t, it, gain, inv_gain;
  int width, height, radius;
  int nf;                  // iterations of this launch, 0..F
  int bits;                // DC_* below, in one word: the kernel keeps its arguments in scalar registers
};
enum : int {
  DC_FIRST = 1, DC_LAST = 2,     // u = o instead of a plane read; mask, gain and store instead of a plane written
  DC_MASK = 4, DC_COPY = 8,      // TDK_DECONV_MASK; N == 0: the input's samples are stored
  DC_VEC_IN = 16, DC_VEC_OUT = 32, DC_VEC_U = 64, DC_VEC_M = 128,   // whole vectors of four elements for src, dst, the planes of u, mask_out
};

// d = the horizontal blur of s on rows [r0, r1), columns [c0, c1), each centred on the column of its clamped pixel
__device__ __forceinline__ void dc_rows(const float* __restrict__ s, float* __restrict__ d, int r0, int r1, int c0, int c1, int PW, int gx0, const DcArgs& a, int tid) {
  const int cols = c1 - c0, n = (r1 - r0) * cols, R = a.radius;
  const float inv = 1.0f / (float)cols;
  for (int e = tid; e < n; e += DC_THREADS) {
    int r, c;
    tdk_split_rc(e, cols, inv, r, c);
    const int sy = r0 + r, sx = c0 + c;
    const float* p = s + sy * PW + (min(max(gx0 + sx, 0), a.width - 1) - gx0);
    float h = a.w[0] * p[0];
#pragma unroll
    for (int k = 1; k <= DC_MAX_R; k++)
      if (k <= R) h = h + a.w[k] * (p[-k] + p[k]);   // (R is uniform: a scalar branch per tap)
    d[sy * PW + sx] = h;
  }
}

// The vertical blur v of h on rows [r0, r1), columns [c0, c1), each centred on the row of its clamped pixel.
// QUOTIENT: out = o / fmaxf(v, TINY); otherwise out = out * v.
template <bool QUOTIENT>
__device__ __forceinline__ void dc_cols(const float* __restrict__ h, float* __restrict__ out, const float* __restrict__ o, int r0, int r1, int c0, int c1, int PW, int gy0, const DcArgs& a, int tid) {
  const int cols = c1 - c0, n = (r1 - r0) * cols, R = a.radius;
  const float inv = 1.0f / (float)cols;
  for (int e = tid; e < n; e += DC_THREADS) {
    int r, c;
    tdk_split_rc(e, cols, inv, r, c);
    const int sy = r0 + r, sx = c0 + c;
    const float* p = h + (min(max(gy0 + sy, 0), a.height - 1) - gy0) * PW + sx;
    float v = a.w[0] * p[0];
#pragma unroll
    for (int k = 1; k <= DC_MAX_R; k++)
      if (k <= R) v = v + a.w[k] * (p[-k * PW] + p[k * PW]);
    const int i = sy * PW + sx;
    if constexpr (QUOTIENT) out[i] = o[i] / fmaxf(v, DC_TINY);
    else out[i] = out[i] * v;
  }
}

// ---- The same two passes for a workgroup whose staged region lies inside the frame (nothing is clamped, the centre of a position is
// the position): a thread owns four adjacent columns that start on a multiple of four, reads 16 bytes at a time and keeps the taps'
// operands in registers.  The columns [c0, c1) are widened to whole groups; what the widening adds is computed from values that are
// not valid and lands in positions that are not valid either -- no valid position reads them, in this pass or a later one, because
// a valid position's taps lie inside the region the pass before made valid.  The arithmetic of a valid position is that of dc_rows
// and dc_cols, operation for operation.
// NCH: the 16-byte chunks around a group, 3 take R <= 4 (larger radii stay with dc_rows and dc_cols).  A chunk index is clamped to the row: only positions that
// are not valid would have read past it.
template <int NCH>
__device__ __forceinline__ void dc_rows4(const float* __restrict__ s, float* __restrict__ d, int r0, int r1, int c0, int c1, int PW, const DcArgs& a, int tid) {
  constexpr int SIDE = NCH / 2, KMAX = 4 * SIDE > DC_MAX_R ? DC_MAX_R : 4 * SIDE;
  const int c0a = c0 & ~3, groups = (((c1 + 3) & ~3) - c0a) >> 2, n = (r1 - r0) * groups, R = a.radius;
  const float inv = 1.0f / (float)groups;
  for (int e = tid; e < n; e += DC_THREADS) {
    int r, g;
    tdk_split_rc(e, groups, inv, r, g);
    const int x = c0a + 4 * g, row = (r0 + r) * PW;
    float v[4 * NCH];
#pragma unroll
    for (int q = 0; q < NCH; q++) {
      const float4 t = *reinterpret_cast<const float4*>(s + row + min(max(x + 4 * (q - SIDE), 0), PW - 4));
      v[4 * q] = t.x, v[4 * q + 1] = t.y, v[4 * q + 2] = t.z, v[4 * q + 3] = t.w;
    }
    float h[4];
#pragma unroll
    for (int i = 0; i < 4; i++) {
      constexpr int C0 = 4 * SIDE;
      h[i] = a.w[0] * v[C0 + i];
#pragma unroll
      for (int k = 1; k <= KMAX; k++)
        if (k <= R) h[i] = h[i] + a.w[k] * (v[C0 + i - k] + v[C0 + i + k]);
    }
    *reinterpret_cast<float4*>(d + row + x) = make_float4(h[0], h[1], h[2], h[3]);
  }
}

template <bool QUOTIENT>
__device__ __forceinline__ void dc_cols4(const float* __restrict__ h, float* __restrict__ out, const float* __restrict__ o, int r0, int r1, int c0, int c1, int PW,
                                         const DcArgs& a, int tid) {
  const int c0a = c0 & ~3, groups = (((c1 + 3) & ~3) - c0a) >> 2, n = (r1 - r0) * groups, R = a.radius;
  const float inv = 1.0f / (float)groups;
  for (int e = tid; e < n; e += DC_THREADS) {
    int r, g;
    tdk_split_rc(e, groups, inv, r, g);
    const int i = (r0 + r) * PW + c0a + 4 * g;
    const float4* p = reinterpret_cast<const float4*>(h + i);
    const int row4 = PW / 4;
    const float4 c = p[0];
    float v[4] = {a.w[0] * c.x, a.w[0] * c.y, a.w[0] * c.z, a.w[0] * c.w};
#pragma unroll
    for (int k = 1; k <= DC_MAX_R; k++)
      if (k <= R) {
        const float4 up = p[-k * row4], dn = p[k * row4];
        v[0] = v[0] + a.w[k] * (up.x + dn.x);
        v[1] = v[1] + a.w[k] * (up.y + dn.y);
        v[2] = v[2] + a.w[k] * (up.z + dn.z);
        v[3] = v[3] + a.w[k] * (up.w + dn.w);
      }
    if constexpr (QUOTIENT) {
      const float4 t = *reinterpret_cast<const float4*>(o + i);
      *reinterpret_cast<float4*>(out + i) = make_float4(t.x / fmaxf(v[0], DC_TINY), t.y / fmaxf(v[1], DC_TINY), t.z / fmaxf(v[2], DC_TINY), t.w / fmaxf(v[3], DC_TINY));
    } else {
      const float4 t = *reinterpret_cast<const float4*>(out + i);
      *reinterpret_cast<float4*>(out + i) = make_float4(t.x * v[0], t.y * v[1], t.z * v[2], t.w * v[3]);
    }
  }
}

template <typename T, int C, int F>
__global__ __launch_bounds__(DC_THREADS) void deconv_kernel(const T* __restrict__ src, T* __restrict__ dst, const float* __restrict__ u_in, float* __restrict__ u_out,
                                                            float* __restrict__ mask_out, DcArgs a) {
  __shared__ DcLds<F> lds;
  const int R = a.radius, W = a.width, H = a.height;
  const int A = max(2 * R * a.nf, 1);   // (N == 0: the mask alone needs its 3x3 neighbourhood); A <= DcGeom<F>::APRON by the host's checks
  const int PW = DC_T + 2 * A;
  const int tid = (int)threadIdx.x;
  const bool first = (a.bits & DC_FIRST) != 0;
  const int x0 = (int)blockIdx.x * DC_T, y0 = (int)blockIdx.y * DC_T;
  const int gx0 = x0 - A, gy0 = y0 - A;

  // ---- o and u of the tile and its apron, clamped to the frame
  // DC_STAGE positions of a thread are asked for before the first is looked at: with one load in flight per thread the pass waits
  // for memory once per position.  A position past the last repeats the last and is not stored.
  {
    const float inv = 1.0f / (float)PW;
    const int n = PW * PW;
    for (int e0 = tid; e0 < n; e0 += DC_STAGE * DC_THREADS) {
      float x[DC_STAGE][C], v[DC_STAGE];
#pragma unroll
      for (int k = 0; k < DC_STAGE; k++) {
        int sy, sx;
        tdk_split_rc(min(e0 + k * DC_THREADS, n - 1), PW, inv, sy, sx);
        const size_t p = (size_t)min(max(gy0 + sy, 0), H - 1) * W + min(max(gx0 + sx, 0), W - 1);
#pragma unroll
        for (int c = 0; c < C; c++) x[k][c] = ld(src, C * p + c);
        v[k] = first ? 0.0f : u_in[p];
      }
#pragma unroll
      for (int k = 0; k < DC_STAGE; k++) {
        const int e = e0 + k * DC_THREADS;
        float y;
        if constexpr (C == 3) y = tdk_pos((a.l0 * x[k][0] + a.l1 * x[k][1]) + a.l2 * x[k][2]);
        else y = tdk_pos(x[k][0]);
        const float o = fmaxf(y, DC_TINY);
        if (e < n) lds.o[e] = o, lds.u[e] = first ? o : v[k];
      }
    }
  }
  __syncthreads();

  // ---- nf iterations; u is valid on [lo, hi) in both axes.  inside: the staged region lies in the frame (the same for the whole workgroup)
  // ... and the radius is one the three chunks of dc_rows4<3> take
  const bool inside = R <= 4 && gx0 >= 0 && gy0 >= 0 && gx0 + PW <= W && gy0 + PW <= H;
#pragma unroll 1
  for (int j = 0; j < a.nf; j++) {
    const int lo = 2 * R * j, hi = PW - lo;
    if (!inside) dc_rows(lds.u, lds.h, lo, hi, lo + R, hi - R, PW, gx0, a, tid);
    else dc_rows4<3>(lds.u, lds.h, lo, hi, lo + R, hi - R, PW, a, tid);
    __syncthreads();
    if (!inside) dc_cols<true>(lds.h, lds.q, lds.o, lo + R, hi - R, lo + R, hi - R, PW, gy0, a, tid);
    else dc_cols4<true>(lds.h, lds.q, lds.o, lo + R, hi - R, lo + R, hi - R, PW, a, tid);
    __syncthreads();
    if (!inside) dc_rows(lds.q, lds.h, lo + R, hi - R, lo + 2 * R, hi - 2 * R, PW, gx0, a, tid);
    else dc_rows4<3>(lds.q, lds.h, lo + R, hi - R, lo + 2 * R, hi - 2 * R, PW, a, tid);
    __syncthreads();
    if (!inside) dc_cols<false>(lds.h, lds.u, lds.o, lo + 2 * R, hi - 2 * R, lo + 2 * R, hi - 2 * R, PW, gy0, a, tid);
    else dc_cols4<false>(lds.h, lds.u, lds.o, lo + 2 * R, hi - 2 * R, lo + 2 * R, hi - 2 * R, PW, a, tid);
    __syncthreads();
  }

  // ---- the tile: four adjacent pixels per thread
  const int tr = tid / DC_GROUPS, tc = (tid % DC_GROUPS) * DC_PIX;
  const int y = y0 + tr, x = x0 + tc;
  if (y >= H || x >= W) return;
  const int sb = (A + tr) * PW + A + tc;
  const size_t pix = (size_t)y * W + x;

  if (!(a.bits & DC_LAST)) {
    float v[DC_PIX];
#pragma unroll
    for (int i = 0; i < DC_PIX; i++) v[i] = lds.u[sb + i];
    if (a.bits & DC_VEC_U) {
      s4_io<float>::store(u_out + pix, 0, v);
    } else {
#pragma unroll
      for (int i = 0; i < DC_PIX; i++)
        if (x + i < W) u_out[pix + i] = v[i];
    }
    return;
  }

  float m[DC_PIX], g[DC_PIX];
  if (a.bits & DC_MASK) {
    // minimum and maximum of the three rows in each of the six columns x - 1 .. x + 4, then of three columns per pixel
    float cmin[DC_PIX + 2], cmax[DC_PIX + 2];
#pragma unroll
    for (int q = 0; q < DC_PIX + 2; q++) {
      const float* p = lds.o + sb + q - 1;
      cmin[q] = fminf(fminf(p[-PW], p[0]), p[PW]);
      cmax[q] = fmaxf(fmaxf(p[-PW], p[0]), p[PW]);
    }
#pragma unroll
    for (int i = 0; i < DC_PIX; i++) {
      const float lo = fminf(fminf(cmin[i], cmin[i + 1]), cmin[i + 2]), hi = fmaxf(fmaxf(cmax[i], cmax[i + 1]), cmax[i + 2]);
      const float d = sqrtf(hi) - sqrtf(lo);
      const float e = fminf(fmaxf((d - a.t) * a.it, 0.0f), 1.0f);
      m[i] = (e * e) * (3.0f - 2.0f * e);
    }
  } else {
#pragma unroll
    for (int i = 0; i < DC_PIX; i++) m[i] = 1.0f;
  }
#pragma unroll
  for (int i = 0; i < DC_PIX; i++) {
    const float o = lds.o[sb + i];
    const float yn = o + m[i] * (lds.u[sb + i] - o);
    g[i] = fminf(fmaxf(yn / o, a.inv_gain), a.gain);
  }

  constexpr int NX = DC_PIX * C;
  float xv[NX], out[NX];
  if (a.bits & DC_VEC_IN) {
#pragma unroll
    for (int q = 0; q < C; q++) s4_io<T>::load(src + pix * C + 4 * q, 0, xv + 4 * q);   // (aligned to four elements: vec_in)
  } else {
#pragma unroll
    for (int i = 0; i < NX; i++) xv[i] = x + i / C < W ? ld(src, pix * C + i) : 0.0f;
  }
#pragma unroll
  for (int i = 0; i < NX; i++) {
    out[i] = (a.bits & DC_COPY) ? xv[i] : xv[i] * g[i / C];
    // The product is a float32 value and the store rounds that to binary16: two roundings.  The empty asm keeps the product a value
    // of its own, so that no instruction that multiplies and converts in one step (one rounding) can take its place.
    if constexpr (sizeof(T) == 2) asm volatile("" : "+v"(out[i]));
  }
  if (a.bits & DC_VEC_OUT) {
#pragma unroll
    for (int q = 0; q < C; q++) s4_io<T>::store(dst + pix * C + 4 * q, 0, out + 4 * q);
  } else {
#pragma unroll
    for (int i = 0; i < NX; i++)
      if (x + i / C < W) st(dst, pix * C + i, out[i]);
  }
  if (mask_out != nullptr) {
    if (a.bits & DC_VEC_M) {
      s4_io<float>::store(mask_out + pix, 0, m);
    } else {
#pragma unroll
      for (int i = 0; i < DC_PIX; i++)
        if (x + i < W) mask_out[pix + i] = m[i];
    }
  }
}

// Measured at 12 MP on the MI355X (profiles/r25/deconv_bench.txt): at every radius F = 1 is the fastest instantiation -- the passes over
// the apron of 2 R F cost more than the plane traffic a fused launch saves -- so F = 1 is the default and the others are for callers
// that force them.
int dc_default_fused(int radius) { return radius >= 1 ? 1 : 0; }
int dc_max_radius(int fused) { return fused == 1 ? DcGeom<1>::RMAX : fused == 2 ? DcGeom<2>::RMAX : fused == 4 ? DcGeom<4>::RMAX : 0; }
int dc_launch_count(int iterations, int fused) { return iterations == 0 ? 1 : tdk_div_up(iterations, fused); }
int dc_plane_count(int launches) { return launches - 1 < 2 ? launches - 1 : 2; }
size_t dc_plane_floats(int width, int height) { return tdk_align_up((size_t)width * height * sizeof(float), DC_WS_ALIGN) / sizeof(float); }
size_t dc_workspace_bytes(int width, int height, int launches) {
  const int planes = dc_plane_count(launches);
  return planes == 0 ? 0 : (size_t)planes * dc_plane_floats(width, height) * sizeof(float) + DC_WS_ALIGN;
}

// 0: fine; otherwise which argument is wrong (messages in tdk_deconv).  *fused receives F.
int dc_check(int channels, int dtype, int radius, int flags, int* fused) {
  if (channels != 1 && channels != 3) return 1;
  if (!tdk_float_dtype_ok(dtype)) return 2;
  if (radius < 1 || radius > DC_MAX_R) return 3;
  if (flags < 0 || (flags & ~(TDK_DECONV_MASK | TDK_DECONV_FUSE_MASK)) != 0) return 4;
  const int forced = (flags & TDK_DECONV_FUSE_MASK) >> TDK_DECONV_FUSE_SHIFT;
  if (forced != 0 && radius > dc_max_radius(forced)) return 5;
  *fused = forced != 0 ? forced : dc_default_fused(radius);
  return 0;
}

// The launches of a call: launch l runs iterations l*F .. min((l+1)*F, N) - 1, reads plane (l - 1) % 2 and writes plane l % 2.
template <typename T, int C, int F>
int dc_run(const void* src, void* dst, float* mask_out, float* planes, size_t plane_floats, DcArgs a, int iterations, hipStream_t st) {
  const int launches = dc_launch_count(iterations, F);
  const dim3 grid((unsigned)tdk_div_up(a.width, DC_T), (unsigned)tdk_div_up(a.height, DC_T));
  for (int l = 0; l < launches; l++) {
    a.nf = iterations - l * F < F ? iterations - l * F : F;
    const bool first = l == 0, last = l == launches - 1;
    a.bits = (a.bits & ~(DC_FIRST | DC_LAST)) | (first ? DC_FIRST : 0) | (last ? DC_LAST : 0);
    const float* u_in = first ? nullptr : planes + (size_t)((l - 1) & 1) * plane_floats;
    float* u_out = last ? nullptr : planes + (size_t)(l & 1) * plane_floats;
    const char* name = launches == 1 ? "tdk_deconv(only)" : first ? "tdk_deconv(first)" : last ? "tdk_deconv(last)" : "tdk_deconv(iterate)";
    TDK_LAUNCH(name, (deconv_kernel<T, C, F>), grid, dim3(DC_THREADS), 0, st, reinterpret_cast<const T*>(src), reinterpret_cast<T*>(dst), u_in, u_out, mask_out, a);
  }
  return TDK_OK;
}

template <typename T, int C>
int dc_dispatch(int fused, const void* src, void* dst, float* mask_out, float* planes, size_t plane_floats, const DcArgs& a, int iterations, hipStream_t st) {
  if (fused == 1) return dc_run<T, C, 1>(src, dst, mask_out, planes, plane_floats, a, iterations, st);
  if (fused == 2) return dc_run<T, C, 2>(src, dst, mask_out, planes, plane_floats, a, iterations, st);
  return dc_run<T, C, 4>(src, dst, mask_out, planes, plane_floats, a, iterations, st);
}

}  // namespace

TDK_EXPORT int tdk_deconv_abi_version(void) { return TDK_DECONV_ABI_VERSION; }

TDK_EXPORT int tdk_deconv_weights(float sigma, float* weights, int* radius) {
  return tdk_gaussian_taps("tdk_deconv_weights", sigma, 0.3f, 2.0f, DC_MAX_R, weights, radius);
}

TDK_EXPORT int tdk_deconv_fused_iterations(int radius) { return radius >= 1 && radius <= DC_MAX_R ? dc_default_fused(radius) : 0; }

TDK_EXPORT size_t tdk_deconv_workspace_bytes(int width, int height, int radius, int iterations) {
  if (!tdk_frame_size_ok(width, height) || radius < 1 || radius > DC_MAX_R || iterations < 0 || iterations > TDK_DECONV_MAX_ITERATIONS) return 0;
  return dc_workspace_bytes(width, height, dc_launch_count(iterations, dc_default_fused(radius)));
}

TDK_EXPORT size_t tdk_deconv_lds_bytes(int channels, int dtype, int radius, int flags) {
  int fused = 0;
  if (dc_check(channels, dtype, radius, flags, &fused) != 0 || dc_max_radius(fused) == 0) return 0;
  return fused == 1 ? sizeof(DcLds<1>) : fused == 2 ? sizeof(DcLds<2>) : sizeof(DcLds<4>);
}

TDK_EXPORT int tdk_deconv(const void* src, void* dst, float* mask_out, void* workspace, int width, int height, int channels, int dtype, const float* weights,
                          int radius, int iterations, float threshold, float max_gain, const float* luma, int flags, tdk_stream_t stream) {
  TDK_REQUIRE(src && dst, "tdk_deconv: null pointer (src or dst)");
  TDK_REQUIRE(weights, "tdk_deconv: null pointer (weights)");
  TDK_REQUIRE(luma, "tdk_deconv: null pointer (luma)");
  TDK_REQUIRE(tdk_frame_size_ok(width, height), "tdk_deconv: frame size %dx%d outside 1..%d", width, height, TDK_FRAME_MAX_SIZE);
  int fused = 0;
  const int bad = dc_check(channels, dtype, radius, flags, &fused);
  TDK_REQUIRE(bad != 1, "tdk_deconv: channels must be 1 or 3, got %d", channels);
  TDK_REQUIRE(bad != 2, "tdk_deconv: unsupported dtype tag %d", dtype);
  TDK_REQUIRE(bad != 3, "tdk_deconv: radius must be 1..%d, got %d", DC_MAX_R, radius);
  TDK_REQUIRE(bad != 4, "tdk_deconv: flags must be TDK_DECONV_MASK and a fused count in bits 8..11, the other bits are reserved, got %d", flags);
  TDK_REQUIRE(bad != 5 && dc_max_radius(fused) != 0, "tdk_deconv: the fused count of flags must be 0, 1, 2 or 4 and take the radius (R <= 6, 4, 2), got %d at radius %d",
              (flags & TDK_DECONV_FUSE_MASK) >> TDK_DECONV_FUSE_SHIFT, radius);
  const int bad_tap = tdk_first_bad_weight(weights, radius + 1);
  TDK_REQUIRE(bad_tap < 0, "tdk_deconv: weights[%d] must be finite and >= 0", bad_tap);
  TDK_REQUIRE(iterations >= 0 && iterations <= TDK_DECONV_MAX_ITERATIONS, "tdk_deconv: iterations must be 0..%d, got %d", TDK_DECONV_MAX_ITERATIONS, iterations);
  const bool mask = (flags & TDK_DECONV_MASK) != 0;
  TDK_REQUIRE(!mask || (isfinite(threshold) && threshold > 0.0f), "tdk_deconv: threshold must be finite and > 0");
  TDK_REQUIRE(max_gain >= 1.0f && max_gain <= DC_MAX_GAIN, "tdk_deconv: max_gain must lie in [1, %g]", (double)DC_MAX_GAIN);
  const int bad_luma = tdk_first_bad_weight(luma, 3);
  TDK_REQUIRE(bad_luma < 0, "tdk_deconv: luma weights must be finite and >= 0 (luma[%d])", bad_luma);
  TDK_REQUIRE(tdk_aligned(mask_out, 4), "tdk_deconv: mask_out must be aligned to 4 bytes");
  const int launches = dc_launch_count(iterations, fused);
  const size_t ws_bytes = dc_workspace_bytes(width, height, launches);
  TDK_REQUIRE(ws_bytes == 0 || workspace, "tdk_deconv: null pointer (workspace: %d launches need %zu bytes)", launches, ws_bytes);
  const size_t esz = tdk_dtype_bytes(dtype), n = (size_t)width * height, frame_bytes = n * channels * esz, plane_bytes = n * sizeof(float);
  TDK_REQUIRE(tdk_disjoint(src, frame_bytes, dst, frame_bytes), "tdk_deconv: src and dst overlap (every output reads its neighbours)");
  TDK_REQUIRE(!mask_out || (tdk_disjoint(mask_out, plane_bytes, src, frame_bytes) && tdk_disjoint(mask_out, plane_bytes, dst, frame_bytes)),
              "tdk_deconv: mask_out overlaps src or dst");
  TDK_REQUIRE(ws_bytes == 0 || (tdk_disjoint(workspace, ws_bytes, src, frame_bytes) && tdk_disjoint(workspace, ws_bytes, dst, frame_bytes) &&
                                (!mask_out || tdk_disjoint(workspace, ws_bytes, mask_out, plane_bytes))),
              "tdk_deconv: the workspace overlaps src, dst or mask_out");

  DcArgs a{};
  for (int k = 0; k <= radius; k++) a.w[k] = weights[k];
  a.l0 = luma[0], a.l1 = luma[1], a.l2 = luma[2];
  a.t = mask ? threshold : 1.0f, a.it = 1.0f / a.t;
  a.gain = max_gain, a.inv_gain = 1.0f / max_gain;
  a.width = width, a.height = height, a.radius = radius;
  a.bits = (mask ? DC_MASK : 0) | (iterations == 0 ? DC_COPY : 0);
  float* planes = ws_bytes == 0 ? nullptr : reinterpret_cast<float*>(tdk_align_up(reinterpret_cast<uintptr_t>(workspace), DC_WS_ALIGN));
  // a thread's four pixels as whole vectors: rows must hold whole groups and start on the vector's alignment
  if (tdk_vec4_ok(width, src, 4 * esz)) a.bits |= DC_VEC_IN;
  if (tdk_vec4_ok(width, dst, 4 * esz)) a.bits |= DC_VEC_OUT;
  if (width % DC_PIX == 0) a.bits |= DC_VEC_U;   // (the planes start on 16 bytes)
  if (tdk_vec4_ok(width, mask_out, 16)) a.bits |= DC_VEC_M;
  hipStream_t st = tdk_stream(stream);
  const size_t plane_floats = dc_plane_floats(width, height);
  if (dtype == TDK_F32) {
    if (channels == 1) return dc_dispatch<float, 1>(fused, src, dst, mask_out, planes, plane_floats, a, iterations, st);
    return dc_dispatch<float, 3>(fused, src, dst, mask_out, planes, plane_floats, a, iterations, st);
  }
  if (channels == 1) return dc_dispatch<__half, 1>(fused, src, dst, mask_out, planes, plane_floats, a, iterations, st);
  return dc_dispatch<__half, 3>(fused, src, dst, mask_out, planes, plane_floats, a, iterations, st);
}
