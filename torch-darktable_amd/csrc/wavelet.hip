// wavelet.hip -- a-trous wavelet shrinkage with a luma/chroma mode (include/tdk_hip_wavelet.h: tdk_wavelet), at most
// max(1, S - 1) launches for S scales.
//
// The specification is the head comment of include/tdk_hip_wavelet.h.  NK = C working-space channels per pixel.
//
// The rule every pass follows.  An LDS slot stands for a frame position, and a slot whose position lies outside the frame holds the
// value of the CLAMPED position -- the edge pixel's own value, at every scale.  A pass computes slot (r, q) as the pixel at the
// clamped slot (rc, qc) and reads its taps at plain offsets from there: the slot at qc + k p holds the value at clamp(x + k p), which
// is the tap the specification names.  One min/max per value instead of one per tap, and every value is the same expression tree
// wherever its tile lies: the result does not depend on the tiling.
//
// Fine launch, wavelet_fine<T, C, YCC, NF>: the NF = 1 or 2 finest scales (steps 1 and 2; a third fused scale would take a 14-pixel
// apron: 60 x 60 staged pixels for 32 x 32 results).  A workgroup of four waves owns WV_TW x WV_TH = 32 x 32 pixels; with the
// cumulative apron A = 2 (NF = 1) or 6 (NF = 2), PW = 32 + 2 A:
//   1. stage    c_0 of the tile and its apron goes to LDS, one PW x PW plane per channel; the frame index is clamped and the
//               colour transform runs here.
//   2. per channel:  rows of scale 0 (plane -> hor), columns (hor -> c_1 plane), rows of scale 1 (c_1 -> hor), and the columns of the
//               last fused scale in registers, four adjacent pixels per thread.  hor and c_1 are shared by the channels.
//   3. S <= NF: y = acc + c_S, the inverse transform, the store.  Otherwise acc and c_NF go to the workspace as float32 planes.
// Coarse launch, wavelet_coarse<T, C, YCC>: one scale s >= 2 per launch, step p = 1 << s.  The taps of a pixel lie p apart, so a
// workgroup takes WC_W = 128 adjacent columns of WC_R = 16 rows that lie p apart (one residue class of rows): 128 + 4 p columns of
// 16 + 4 rows staged per channel, both passes through LDS, the channels one after the other.  A launch reads c_s and acc and writes
// c_{s+1} (into the other plane set: neighbours read the apron) and acc (in place); the last launch adds c_S, inverts the colour
// transform and stores dst instead.
// Workspace: float32 planes with rows padded to four floats, so that a thread's four values move as one 16-byte access at any
// frame width: C planes of acc, C of c, and C more of c when more than one coarse launch follows (S >= 4).
// Global accesses of the frame: a thread's four pixels are 4 C elements; where rows hold whole groups (width % 4 == 0) and dst
// starts on a multiple of four elements they are stored as C vectors of four elements, per element otherwise.  Staging is per
// element, consecutive lanes on consecutive pixels.  Nothing is accumulated across lanes or workgroups.
#include <math.h>

#include "../../include/tdk_hip_wavelet.h"
#include "tdk_frame.h"

namespace {

constexpr int WV_THREADS = 256;
constexpr int WV_TW = 32, WV_TH = 32, WV_PIX = 4, WV_GROUPS = WV_TW / WV_PIX;   // fine: 8 threads per tile row, 32 rows
constexpr int WV_FUSED = 2;
constexpr int WC_W = 128, WC_R = 16, WC_MAX_P = 1 << (TDK_WAVELET_MAX_SCALES - 1);   // coarse: columns, rows a step apart, largest step
constexpr int WC_ROWS = WC_R + 4, WC_MAX_SW = WC_W + 4 * WC_MAX_P;
constexpr int WV_MAX_S = TDK_WAVELET_MAX_SCALES;
constexpr int WV_MAX_SIZE = 65535;
static_assert(WV_THREADS == WV_GROUPS * WV_TH, "a thread per 4 pixels of the fine tile");
static_assert(WV_THREADS * WV_PIX * 2 == WC_W * WC_R, "a thread per 4 pixels of two rows of the coarse tile");

constexpr int wv_apron(int nf) { return nf == 1 ? 2 : 6; }
constexpr size_t wv_fine_lds(int channels, int nf) {
  const size_t pw = WV_TW + 2 * wv_apron(nf);
  return (size_t)(channels + nf) * pw * pw * sizeof(float);   // a plane per channel, hor, and the c_1 plane of NF = 2
}
constexpr size_t WC_LDS = (size_t)(WC_ROWS * WC_MAX_SW + WC_ROWS * WC_W) * sizeof(float);
static_assert(wv_fine_lds(3, 2) <= 64 * 1024 && WC_LDS <= 64 * 1024, "LDS of the largest launch");

struct WvFineArgs {
  float t[WV_FUSED * 3];     // thresholds of the fused scales: t[s * C + k]
  int width, height, pitch;  // pitch: floats per row of a workspace plane
  int final, vec_out;
};
struct WvCoarseArgs {
  float t[3];                // thresholds of this scale
  int width, height, pitch;
  int step, last, vec_out;
};

__device__ __forceinline__ float wv_taps(float m2, float m1, float c, float p1, float p2) {
  return (0.0625f * (m2 + p2) + 0.25f * (m1 + p1)) + 0.375f * c;
}
__device__ __forceinline__ float wv_shrink(float d, float t) {
  const float ad = fabsf(d);
  return ad > t ? copysignf(ad - t, d) : 0.0f;
}
// working space -> frame channels, in place
template <bool YCC> __device__ __forceinline__ void wv_inverse(float& v0, float& v1, float& v2) {
  if constexpr (YCC) {
    const float g = v0 - 0.25f * (v1 + v2);
    const float r = v2 + g, b = v1 + g;
    v0 = r, v1 = g, v2 = b;
  }
}
// the results of four adjacent pixels (working space, out[k * 4 + i]) to dst
template <typename T, int C, bool YCC> __device__ __forceinline__ void wv_store(T* dst, size_t o, float* out, int x, int W, int vec) {
  float e[4 * C];
#pragma unroll
  for (int i = 0; i < 4; i++) {
    if constexpr (C == 3) {
      float v0 = out[i], v1 = out[4 + i], v2 = out[8 + i];
      wv_inverse<YCC>(v0, v1, v2);
      e[3 * i] = v0, e[3 * i + 1] = v1, e[3 * i + 2] = v2;
    } else {
      e[i] = out[i];
    }
  }
  if (vec) {
#pragma unroll
    for (int q = 0; q < C; q++) s4_io<T>::store(dst + o + 4 * q, 0, e + 4 * q);
  } else {
#pragma unroll
    for (int i = 0; i < 4 * C; i++)
      if (x + i / C < W) st(dst, o + i, e[i]);
  }
}

template <typename T, int C, bool YCC, int NF>
__global__ __launch_bounds__(WV_THREADS) void wavelet_fine(const T* __restrict__ src, T* __restrict__ dst, float* __restrict__ acc_out,
                                                           float* __restrict__ c_out, WvFineArgs a) {
  static_assert(!YCC || C == 3, "the luma/chroma space needs three channels");
  constexpr int A = wv_apron(NF), PW = WV_TW + 2 * A, PLANE = PW * PW;
  __shared__ __attribute__((aligned(16))) float lds[(C + NF) * PLANE];
  float* hor = lds + C * PLANE;
  float* c1 = hor + PLANE;   // (NF = 2 only)

  const int tid = threadIdx.x, W = a.width, H = a.height;
  const int x0 = (int)blockIdx.x * WV_TW, y0 = (int)blockIdx.y * WV_TH;
  // slots of the frame's first and last column and row: a slot index is clamped to these
  const int qlo = A - x0, qhi = W - 1 - x0 + A, rlo = A - y0, rhi = H - 1 - y0 + A;

  // ---- 1. c_0 of the tile and its apron, clamped to the frame
  for (int it = tid; it < PLANE; it += WV_THREADS) {
    const int r = it / PW, q = it - r * PW;
    const int gy = min(max(y0 - A + r, 0), H - 1), gx = min(max(x0 - A + q, 0), W - 1);
    const size_t o = ((size_t)gy * W + gx) * C;
    if constexpr (YCC) {
      const float rr = ld(src, o), g = ld(src, o + 1), b = ld(src, o + 2);
      lds[it] = (0.25f * rr + 0.5f * g) + 0.25f * b;
      lds[PLANE + it] = b - g;
      lds[2 * PLANE + it] = rr - g;
    } else {
#pragma unroll
      for (int k = 0; k < C; k++) lds[k * PLANE + it] = ld(src, o + k);
    }
  }
  __syncthreads();

  const int tr = tid / WV_GROUPS, tc = (tid % WV_GROUPS) * WV_PIX;
  const int pix = (tr + A) * PW + tc + A;   // the slot of the thread's first pixel
  float out[4 * C], last[4 * C];             // acc and the coarsest c of the thread's four pixels, [k * 4 + i]

#pragma unroll
  for (int k = 0; k < C; k++) {
    const float* c0 = lds + k * PLANE;
    // rows of scale 0: every staged row, the columns scale 0 leaves (apron A - 2)
    for (int it = tid; it < PW * (PW - 4); it += WV_THREADS) {
      const int r = it / (PW - 4), q = it - r * (PW - 4) + 2;
      const float* s = c0 + r * PW + min(max(q, qlo), qhi);
      hor[r * PW + q] = wv_taps(s[-2], s[-1], s[0], s[1], s[2]);
    }
    __syncthreads();
    if constexpr (NF == 1) {
#pragma unroll
      for (int i = 0; i < 4; i++) {
        const float* s = hor + pix + i;
        const float n = wv_taps(s[-2 * PW], s[-PW], s[0], s[PW], s[2 * PW]);
        out[k * 4 + i] = wv_shrink(c0[pix + i] - n, a.t[k]);
        last[k * 4 + i] = n;
      }
    } else {
      // columns of scale 0: c_1 on the tile and an apron of 4
      for (int it = tid; it < (PW - 4) * (PW - 4); it += WV_THREADS) {
        const int r = it / (PW - 4) + 2, q = it - (r - 2) * (PW - 4) + 2;
        const float* s = hor + min(max(r, rlo), rhi) * PW + q;
        c1[r * PW + q] = wv_taps(s[-2 * PW], s[-PW], s[0], s[PW], s[2 * PW]);
      }
      __syncthreads();
      // rows of scale 1 (step 2): the rows of c_1, the columns of the tile
      for (int it = tid; it < (PW - 4) * WV_TW; it += WV_THREADS) {
        const int r = it / WV_TW + 2, q = it % WV_TW + A;
        const float* s = c1 + r * PW + min(max(q, qlo), qhi);
        hor[r * PW + q] = wv_taps(s[-4], s[-2], s[0], s[2], s[4]);
      }
      __syncthreads();
#pragma unroll
      for (int i = 0; i < 4; i++) {
        const float* s = hor + pix + i;
        const float n = wv_taps(s[-4 * PW], s[-2 * PW], s[0], s[2 * PW], s[4 * PW]);
        const float m = c1[pix + i];
        const float d0 = wv_shrink(c0[pix + i] - m, a.t[k]);
        out[k * 4 + i] = d0 + wv_shrink(m - n, a.t[C + k]);
        last[k * 4 + i] = n;
      }
    }
    if (k + 1 < C) __syncthreads();   // the next channel writes hor and c_1
  }

  // ---- 3. the frame, or the planes the coarse launches go on from
  const int y = y0 + tr, x = x0 + tc;
  if (y >= H || x >= W) return;
  if (a.final) {
#pragma unroll
    for (int i = 0; i < 4 * C; i++) out[i] = out[i] + last[i];
    wv_store<T, C, YCC>(dst, ((size_t)y * W + x) * C, out, x, W, a.vec_out);
  } else {
    const size_t plane = (size_t)a.pitch * H, o = (size_t)y * a.pitch + x;   // x % 4 == 0, and the pitch holds whole groups
#pragma unroll
    for (int k = 0; k < C; k++) {
      s4_io<float>::store(acc_out + k * plane + o, 0, out + 4 * k);
      s4_io<float>::store(c_out + k * plane + o, 0, last + 4 * k);
    }
  }
}

template <typename T, int C, bool YCC>
__global__ __launch_bounds__(WV_THREADS) void wavelet_coarse(const float* __restrict__ c_in, float* __restrict__ c_out, float* __restrict__ acc,
                                                             T* __restrict__ dst, WvCoarseArgs a) {
  static_assert(!YCC || C == 3, "the luma/chroma space needs three channels");
  __shared__ __attribute__((aligned(16))) float sig[WC_ROWS * WC_MAX_SW];
  __shared__ __attribute__((aligned(16))) float hor[WC_ROWS * WC_W];
  const int tid = threadIdx.x, W = a.width, H = a.height, p = a.step;
  const int SW = WC_W + 4 * p;                                             // staged columns
  const int x0 = (int)blockIdx.x * WC_W;
  const int res = (int)blockIdx.y % p, j0 = (int)blockIdx.y / p * WC_R;    // the rows res + p (j0 + j), j = 0 .. WC_R - 1
  if (res + p * j0 >= H) return;                                           // (the whole workgroup: no row of this class is left)
  const size_t plane = (size_t)a.pitch * H;

  const int wave = tid / 64, lane = tid % 64;
  const int tcx = (tid % 32) * WV_PIX, trow = tid / 32;                    // four pixels of the rows trow and trow + 8
  const int x = x0 + tcx;
  float out[2][4 * C];                                                     // the last launch: acc, then the result, [k * 4 + i]

#pragma unroll
  for (int k = 0; k < C; k++) {
    const float* ck = c_in + k * plane;
    // c_s: the rows two steps above to two steps below, the columns 2 p left to 2 p right, clamped to the frame
    for (int r = wave; r < WC_ROWS; r += WV_THREADS / 64) {
      const size_t row = (size_t)min(max(res + p * (j0 + r - 2), 0), H - 1) * a.pitch;
      for (int i = lane; i < SW; i += 64) sig[r * SW + i] = ck[row + min(max(x0 - 2 * p + i, 0), W - 1)];
    }
    __syncthreads();
    for (int it = tid; it < WC_ROWS * WC_W; it += WV_THREADS) {
      const float* s = sig + (it / WC_W) * SW + it % WC_W + 2 * p;
      hor[it] = wv_taps(s[-2 * p], s[-p], s[0], s[p], s[2 * p]);
    }
    __syncthreads();
#pragma unroll
    for (int half = 0; half < 2; half++) {
      const int j = trow + half * (WC_R / 2), y = res + p * (j0 + j);
      float v[5][4], n[4], own[4], ac[4];
#pragma unroll
      for (int d = 0; d < 5; d++) s4_io<float>::load(hor + (j + d) * WC_W + tcx, 0, v[d]);
      s4_io<float>::load(sig + (j + 2) * SW + 2 * p + tcx, 0, own);        // (SW and 2 p are multiples of 4)
      if (y < H && x < W) {
        const size_t o = (size_t)y * a.pitch + x;
        s4_io<float>::load(acc + k * plane + o, 0, ac);
#pragma unroll
        for (int i = 0; i < 4; i++) {
          n[i] = wv_taps(v[0][i], v[1][i], v[2][i], v[3][i], v[4][i]);
          ac[i] = ac[i] + wv_shrink(own[i] - n[i], a.t[k]);
        }
        if (a.last) {
#pragma unroll
          for (int i = 0; i < 4; i++) out[half][k * 4 + i] = ac[i] + n[i];
        } else {
          s4_io<float>::store(c_out + k * plane + o, 0, n);
          s4_io<float>::store(acc + k * plane + o, 0, ac);
        }
      }
    }
    if (k + 1 < C) __syncthreads();   // the next channel stages over sig and hor
  }

  if (a.last) {
#pragma unroll
    for (int half = 0; half < 2; half++) {
      const int y = res + p * (j0 + trow + half * (WC_R / 2));
      if (y < H && x < W) wv_store<T, C, YCC>(dst, ((size_t)y * W + x) * C, out[half], x, W, a.vec_out);
    }
  }
}

// the planes of a workspace: acc, c (written by the fine launch), and the second set of c
struct WvPlanes {
  float *acc, *c[2];
};

template <typename T, int C, bool YCC>
int launch(const void* src, void* dst, const WvPlanes& ws, int width, int height, int pitch, int scales, const float* thresholds, bool vec_out, hipStream_t st) {
  static const char* const names[WV_MAX_S] = {"", "", "tdk_wavelet(scale 2)", "tdk_wavelet(scale 3)", "tdk_wavelet(scale 4)"};
  WvFineArgs f{};
  const int nf = scales < WV_FUSED ? scales : WV_FUSED;
  for (int i = 0; i < nf * C; i++) f.t[i] = thresholds[i];
  f.width = width, f.height = height, f.pitch = pitch;
  f.final = scales <= WV_FUSED, f.vec_out = vec_out;
  const dim3 grid((unsigned)tdk_div_up(width, WV_TW), (unsigned)tdk_div_up(height, WV_TH));
  const T* s = reinterpret_cast<const T*>(src);
  T* d = reinterpret_cast<T*>(dst);
  if (nf == 1) TDK_LAUNCH("tdk_wavelet(fine)", (wavelet_fine<T, C, YCC, 1>), grid, dim3(WV_THREADS), 0, st, s, d, ws.acc, ws.c[0], f);
  else TDK_LAUNCH("tdk_wavelet(fine)", (wavelet_fine<T, C, YCC, 2>), grid, dim3(WV_THREADS), 0, st, s, d, ws.acc, ws.c[0], f);
  for (int sc = WV_FUSED; sc < scales; sc++) {
    WvCoarseArgs a{};
    for (int k = 0; k < C; k++) a.t[k] = thresholds[sc * C + k];
    a.width = width, a.height = height, a.pitch = pitch;
    a.step = 1 << sc, a.last = sc == scales - 1, a.vec_out = vec_out;
    const int classes = tdk_div_up(tdk_div_up(height, a.step), WC_R);   // tiles of rows per residue class
    const dim3 cgrid((unsigned)tdk_div_up(width, WC_W), (unsigned)(a.step * classes));
    const int in = (sc - WV_FUSED) & 1;
    TDK_LAUNCH(names[sc], (wavelet_coarse<T, C, YCC>), cgrid, dim3(WV_THREADS), 0, st, ws.c[in], ws.c[in ^ 1], ws.acc, d, a);
  }
  return TDK_OK;
}

template <typename T, int C> int dispatch(bool ycc, const void* src, void* dst, const WvPlanes& ws, int width, int height, int pitch, int scales,
                                          const float* thresholds, bool vec_out, hipStream_t st) {
  if constexpr (C == 3)
    if (ycc) return launch<T, 3, true>(src, dst, ws, width, height, pitch, scales, thresholds, vec_out, st);
  return launch<T, C, false>(src, dst, ws, width, height, pitch, scales, thresholds, vec_out, st);
}

// 0: fine; otherwise which argument is wrong (messages in tdk_wavelet)
int wv_check(int channels, int dtype, int scales, int flags) {
  if (channels != 1 && channels != 3) return 1;
  if (dtype != TDK_F32 && dtype != TDK_F16) return 2;
  if (scales < 1 || scales > WV_MAX_S) return 3;
  if (flags < 0 || (flags & ~TDK_WAVELET_YCC) != 0) return 4;
  if ((flags & TDK_WAVELET_YCC) && channels != 3) return 5;
  return 0;
}

bool wv_size_ok(int width, int height) { return width >= 1 && height >= 1 && width <= WV_MAX_SIZE && height <= WV_MAX_SIZE; }
int wv_pitch(int width) { return (int)tdk_align_up((size_t)width, 4); }
int wv_plane_sets(int scales) { return scales <= WV_FUSED ? 0 : scales == WV_FUSED + 1 ? 2 : 3; }   // acc, c, and the other c
constexpr size_t WV_WS_ALIGN = 16;   // the planes start on 16 bytes inside a workspace at any alignment

}  // namespace

TDK_EXPORT int tdk_wavelet_abi_version(void) { return TDK_WAVELET_ABI_VERSION; }

TDK_EXPORT int tdk_wavelet_band_norms(int scales, float* norms) {
  TDK_REQUIRE(norms, "tdk_wavelet_band_norms: null pointer");
  TDK_REQUIRE(scales >= 1 && scales <= WV_MAX_S, "tdk_wavelet_band_norms: scales must be 1..%d, got %d", WV_MAX_S, scales);
  // the one-dimensional response of c_s, centred in LEN taps: c_0 is the impulse, c_{s+1} = c_s filtered at step 1 << s
  constexpr int R = 2 * ((1 << WV_MAX_S) - 1), LEN = 2 * R + 1;
  static const double taps[5] = {0.0625, 0.25, 0.375, 0.25, 0.0625};
  double cur[LEN] = {0.0}, next[LEN];
  cur[R] = 1.0;
  for (int s = 0; s < WV_MAX_S; s++) {
    if (s >= scales) {
      norms[s] = 0.0f;
      continue;
    }
    const int p = 1 << s;
    for (int i = 0; i < LEN; i++) {
      double v = 0.0;
      for (int k = -2; k <= 2; k++) {
        const int j = i + k * p;
        if (j >= 0 && j < LEN) v += taps[k + 2] * cur[j];
      }
      next[i] = v;
    }
    double sum = 0.0;   // the two-dimensional response of d_s is cur x cur - next x next
    for (int i = 0; i < LEN; i++)
      for (int j = 0; j < LEN; j++) {
        const double d = cur[i] * cur[j] - next[i] * next[j];
        sum += d * d;
      }
    norms[s] = (float)sqrt(sum);
    for (int i = 0; i < LEN; i++) cur[i] = next[i];
  }
  return TDK_OK;
}

TDK_EXPORT size_t tdk_wavelet_workspace_bytes(int width, int height, int channels, int scales) {
  if (!wv_size_ok(width, height) || wv_check(channels, TDK_F32, scales, 0) != 0) return 0;
  const int sets = wv_plane_sets(scales);
  if (sets == 0) return 0;
  return (size_t)sets * channels * wv_pitch(width) * height * sizeof(float) + WV_WS_ALIGN;
}

TDK_EXPORT size_t tdk_wavelet_lds_bytes(int channels, int dtype, int scales, int flags) {
  if (wv_check(channels, dtype, scales, flags) != 0) return 0;
  const size_t fine = wv_fine_lds(channels, scales < WV_FUSED ? scales : WV_FUSED);
  return scales > WV_FUSED && WC_LDS > fine ? WC_LDS : fine;
}

TDK_EXPORT int tdk_wavelet(const void* src, void* dst, void* workspace, int width, int height, int channels, int dtype, int scales, const float* thresholds,
                           int flags, tdk_stream_t stream) {
  TDK_REQUIRE(src && dst, "tdk_wavelet: null pointer (src or dst)");
  TDK_REQUIRE(thresholds, "tdk_wavelet: null pointer (thresholds)");
  TDK_REQUIRE(wv_size_ok(width, height), "tdk_wavelet: frame size %dx%d outside 1..%d", width, height, WV_MAX_SIZE);
  const int bad = wv_check(channels, dtype, scales, flags);
  TDK_REQUIRE(bad != 1, "tdk_wavelet: channels must be 1 or 3, got %d", channels);
  TDK_REQUIRE(bad != 2, "tdk_wavelet: unsupported dtype tag %d (TDK_F32 or TDK_F16)", dtype);
  TDK_REQUIRE(bad != 3, "tdk_wavelet: scales must be 1..%d, got %d", WV_MAX_S, scales);
  TDK_REQUIRE(bad != 4, "tdk_wavelet: flags must be 0 or TDK_WAVELET_YCC, got %d", flags);
  TDK_REQUIRE(bad != 5, "tdk_wavelet: TDK_WAVELET_YCC needs three channels, got %d", channels);
  for (int i = 0; i < scales * channels; i++) TDK_REQUIRE(isfinite(thresholds[i]) && thresholds[i] >= 0.0f, "tdk_wavelet: thresholds[%d] must be finite and >= 0", i);
  const size_t esz = tdk_dtype_bytes(dtype), bytes = (size_t)width * height * channels * esz;
  TDK_REQUIRE(tdk_disjoint(src, bytes, dst, bytes), "tdk_wavelet: src and dst overlap (every output reads its neighbours)");
  const size_t ws_bytes = tdk_wavelet_workspace_bytes(width, height, channels, scales);
  TDK_REQUIRE(ws_bytes == 0 || workspace, "tdk_wavelet: null pointer (workspace: %d scales need %zu bytes)", scales, ws_bytes);
  TDK_REQUIRE(ws_bytes == 0 || (tdk_disjoint(workspace, ws_bytes, src, bytes) && tdk_disjoint(workspace, ws_bytes, dst, bytes)),
              "tdk_wavelet: the workspace overlaps src or dst");

  const int pitch = wv_pitch(width);
  WvPlanes ws{};
  if (ws_bytes != 0) {
    const size_t set = (size_t)channels * pitch * height;
    float* base = reinterpret_cast<float*>(tdk_align_up(reinterpret_cast<uintptr_t>(workspace), WV_WS_ALIGN));
    ws.acc = base, ws.c[0] = base + set;
    ws.c[1] = wv_plane_sets(scales) == 3 ? base + 2 * set : nullptr;   // (one coarse launch: it writes no c)
  }
  // a thread's four pixels as whole vectors of four elements: rows must hold whole groups and start on the vector's alignment
  const bool vec_out = width % WV_PIX == 0 && tdk_aligned(dst, 4 * esz);
  const bool ycc = (flags & TDK_WAVELET_YCC) != 0;
  hipStream_t st = tdk_stream(stream);
  TDK_DISPATCH_DTYPE(dtype, T, TDK_DISPATCH_CHANNELS_(channels, C, return (dispatch<T, C>(ycc, src, dst, ws, width, height, pitch, scales, thresholds, vec_out, st))));
}
