// defringe.hip -- purple-fringe removal on demosaiced frames (include/tdk_hip_defringe.h: tdk_defringe), two launches.
//
// The specification is the head comment of include/tdk_hip_defringe.h.
//
// Both kernels give a workgroup of four waves DF_T x DF_T = 32 x 32 pixels, and both stage the tile with an apron in static LDS so
// that every staged position holds the value of the CLAMPED pixel: a position outside the frame then holds exactly what the pixel
// on the edge holds, which is the specification's rule for indices outside the frame, and no later pass has a guard.
//
// Launch 1, "edge": a fixed number of workgroups (at most TDK_DEFRINGE_MAX_GROUPS) walk the tiles.  Per tile, with R the blur's
// radius and PW = 32 + 2 R:
//   cb, cr   Cb and Cr over PW x PW positions (the planes are sized for R = 12: 56 x 56)
//   hb, hr   their horizontal blur on the PW rows and the tile's 32 columns
//   E        the vertical blur of hb, hr on the tile, the differences and their squares; stored to the workspace plane (and edge_out)
// every pass a loop of the 256 threads over the region in row order (consecutive lanes, consecutive words of LDS).  A thread keeps
// the 64-bit sum of its pixels' q; the workgroup adds its threads' sums (shuffles, then four words of LDS) and writes ONE record.
// Every record the second launch reads is written by every call, so nothing is ever zeroed and there is no atomic.
//
// Launch 2, "correct": a workgroup per tile.  Every workgroup adds the records (integers: any order gives the same S) and forms th.
// A thread owns four adjacent pixels of a tile row.  A tile without a fringed pixel stores its input and is done.  Otherwise, with
// S_r the sample radius and PW = 32 + 2 S_r:
//   wt, pb, pr   1 / (E + th), wt*Cb and wt*Cr over PW x PW positions (sized for S_r = 8: 48 x 48), one division per position
//   flag         the owners' decisions, a byte per pixel of the tile
//   cb, cr       the new chroma of the fringed pixels
// The disc is walked a lane per pixel of a tile row (unrolled per sample radius, only where the flag is set), and the owner of a
// pixel reads the new chroma back.  The products are the specification's (wt_s*Cb_s, wt_s*Cr_s): it changes no bit whether they
// are formed while staging or inside the loop.
// No pixel's arithmetic depends on the tile or on the number of workgroups: deterministic.
#include <math.h>

#include "../../include/tdk_hip_defringe.h"
#include "tdk_frame.h"

namespace {

constexpr int DF_THREADS = 256;
constexpr int DF_T = TDK_DEFRINGE_TILE, DF_PIX = 4, DF_GROUPS = DF_T / DF_PIX;   // 8 threads per tile row, 32 rows
constexpr int DF_MAX_R = TDK_DEFRINGE_MAX_RADIUS, DF_MAX_S = TDK_DEFRINGE_MAX_SAMPLE_RADIUS;
constexpr int DF_MAX_WG = TDK_DEFRINGE_MAX_GROUPS;
constexpr size_t DF_WS_ALIGN = 16;
constexpr float DF_SCALE = (float)TDK_DEFRINGE_STAT_SCALE, DF_CAP = (float)TDK_DEFRINGE_STAT_CAP;
static_assert(DF_THREADS == DF_GROUPS * DF_T, "a thread per 4 pixels of the tile");

constexpr int DF_EP = DF_T + 2 * DF_MAX_R;   // pitch of the largest staged region of the edge launch
constexpr int DF_CP = DF_T + 2 * DF_MAX_S;   // ... of the correct launch
struct DfEdgeLds {
  float cb[DF_EP * DF_EP], cr[DF_EP * DF_EP], hb[DF_EP * DF_T], hr[DF_EP * DF_T];
  unsigned long long part[DF_THREADS / 64];
};
struct DfCorrectLds {
  float wt[DF_CP * DF_CP], pb[DF_CP * DF_CP], pr[DF_CP * DF_CP];
  float cb[DF_T * DF_T], cr[DF_T * DF_T];   // the new chroma of the tile's fringed pixels
  unsigned long long part[DF_THREADS / 64];
  int votes[DF_THREADS / 64];
  alignas(4) unsigned char flag[DF_T * DF_T];   // 1: the pixel is fringed
};
static_assert(sizeof(DfEdgeLds) <= 40 * 1024 && sizeof(DfCorrectLds) <= 40 * 1024, "four workgroups in the 160 KB of a CU");

struct DfArgs {
  float w[DF_MAX_R + 1];
  float strength, floor;
  int width, height, radius, sample_radius;
  int groups;              // workgroups of the edge launch = records
  int bits;                // DF_* below
};
enum : int {
  DF_STATIC = 1,                  // TDK_DEFRINGE_STATIC
  DF_VEC_IN = 2, DF_VEC_OUT = 4,  // whole vectors of four pixels for src, dst
  DF_VEC_E = 8,                   // ... of four floats for the workspace plane of E
};

template <bool SQRT> __device__ __forceinline__ float df_work(float x) {
  const float p = tdk_pos(x);
  return SQRT ? sqrtf(p) : p;
}


// the sum of a value over the workgroup, the same in every thread; `part` is one word per wave
__device__ __forceinline__ unsigned long long df_block_sum(unsigned long long v, unsigned long long* part) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
  __syncthreads();
  unsigned long long s = 0;
#pragma unroll
  for (int k = 0; k < DF_THREADS / 64; k++) s += part[k];
  return s;
}

// The two passes of the blur at the radius RR, so that the taps are unrolled without a condition per tap (twelve conditions kept as
// lane masks, next to the masks of three correctly rounded square roots, do not fit the scalar file).
// 2. the horizontal blur: PW rows, the tile's columns
template <int RR> __device__ __forceinline__ void df_rows(DfEdgeLds& lds, const float (&w)[DF_MAX_R + 1], int tid) {
  constexpr int PW = DF_T + 2 * RR;
  for (int e = tid; e < PW * DF_T; e += DF_THREADS) {
    const int r = e / DF_T, c = e % DF_T;
    const float *pb = lds.cb + r * PW + c + RR, *pr = lds.cr + r * PW + c + RR;
    float hb = w[0] * pb[0], hr = w[0] * pr[0];
#pragma unroll
    for (int k = 1; k <= RR; k++) {
      hb = hb + w[k] * (pb[-k] + pb[k]);
      hr = hr + w[k] * (pr[-k] + pr[k]);
    }
    lds.hb[e] = hb;
    lds.hr[e] = hr;
  }
}

// 3. the vertical blur on the tile, E and q; returns the sum of q over the thread's pixels inside the frame
template <int RR>
__device__ __forceinline__ unsigned long long df_cols(const DfEdgeLds& lds, const float (&w)[DF_MAX_R + 1], int tid, int x0, int y0, int W, int H,
                                                      float* __restrict__ eplane, float* __restrict__ edge_out) {
  constexpr int PW = DF_T + 2 * RR;
  unsigned long long acc = 0;
  for (int e = tid; e < DF_T * DF_T; e += DF_THREADS) {
    const int r = e / DF_T, c = e % DF_T;
    const float *pb = lds.hb + (r + RR) * DF_T + c, *pr = lds.hr + (r + RR) * DF_T + c;
    float vb = w[0] * pb[0], vr = w[0] * pr[0];
#pragma unroll
    for (int k = 1; k <= RR; k++) {
      vb = vb + w[k] * (pb[-k * DF_T] + pb[k * DF_T]);
      vr = vr + w[k] * (pr[-k * DF_T] + pr[k * DF_T]);
    }
    const int o = (r + RR) * PW + c + RR;
    const float db = lds.cb[o] - vb, dr = lds.cr[o] - vr;
    const float E = db * db + dr * dr;
    const int y = y0 + r, x = x0 + c;
    if (y < H && x < W) {
      const size_t i = (size_t)y * W + x;
      eplane[i] = E;
      if (edge_out) edge_out[i] = E;
      acc += (unsigned long long)floorf(fminf(E, DF_CAP) * DF_SCALE);
    }
  }
  return acc;
}

#define DF_ROWS(RR) df_rows<RR>(lds, w, tid)
#define DF_COLS(RR) acc += df_cols<RR>(lds, w, tid, x0, y0, W, H, eplane, edge_out)
#define DF_FOR_RADIUS(R, CALL)                                                                                                \
  switch (R) {                                                                                                                \
    case 1: CALL(1); break; case 2: CALL(2); break; case 3: CALL(3); break; case 4: CALL(4); break;                           \
    case 5: CALL(5); break; case 6: CALL(6); break; case 7: CALL(7); break; case 8: CALL(8); break;                           \
    case 9: CALL(9); break; case 10: CALL(10); break; case 11: CALL(11); break; default: CALL(12); break;                     \
  }

// ---- launch 1: E and one partial sum per workgroup
template <typename T, bool SQRT>
__global__ __launch_bounds__(DF_THREADS) void defringe_edge_kernel(const T* __restrict__ src, float* __restrict__ eplane, float* __restrict__ edge_out,
                                                                   unsigned long long* __restrict__ records, DfArgs a) {
  __shared__ DfEdgeLds lds;
  const int tid = (int)threadIdx.x;
  const int W = a.width, H = a.height, R = a.radius;
  const int PW = DF_T + 2 * R;
  const int tiles_x = (W + DF_T - 1) / DF_T, tiles = tiles_x * ((H + DF_T - 1) / DF_T);
  const float inv_pw = 1.0f / (float)PW;
  unsigned long long acc = 0;
  const float (&w)[DF_MAX_R + 1] = a.w;

  for (int tile = (int)blockIdx.x; tile < tiles; tile += (int)gridDim.x) {
    const int tyi = tile / tiles_x;
    const int x0 = (tile - tyi * tiles_x) * DF_T, y0 = tyi * DF_T;

    // 1. Cb, Cr of the clamped pixel
    for (int e = tid; e < PW * PW; e += DF_THREADS) {
      int r, c;
      tdk_split_rc(e, PW, inv_pw, r, c);
      const int gy = min(max(y0 - R + r, 0), H - 1), gx = min(max(x0 - R + c, 0), W - 1);
      const size_t i = ((size_t)gy * W + gx) * 3;
      const float tr = df_work<SQRT>(ld(src, i)), tg = df_work<SQRT>(ld(src, i + 1)), tb = df_work<SQRT>(ld(src, i + 2));
      lds.cb[e] = tb - tg;
      lds.cr[e] = tr - tg;
    }
    __syncthreads();

    // 2. the horizontal blur: PW rows, the tile's columns
    DF_FOR_RADIUS(R, DF_ROWS);
    __syncthreads();

    // 3. the vertical blur on the tile, E and q
    DF_FOR_RADIUS(R, DF_COLS);
    __syncthreads();   // the planes are staged again
  }

  const unsigned long long sum = df_block_sum(acc, lds.part);
  if (tid == 0) records[blockIdx.x] = sum;
}

// The sums of one fringed pixel over the disc of radius SS: dy ascending, then dx ascending.  Both loops unroll and the test folds, so
// every sample is three reads at a constant offset from the centre and three additions (a loop over a row's extent from a table
// spent more on its own counters and addresses than on the samples).
template <int SS> __device__ __forceinline__ void df_disc(const DfCorrectLds& lds, int centre, float& sa, float& sb, float& sn) {
  constexpr int PW = DF_T + 2 * SS;
  const float *pb = lds.pb + centre, *pr = lds.pr + centre, *wt = lds.wt + centre;
#pragma unroll
  for (int dy = -SS; dy <= SS; dy++) {
#pragma unroll
    for (int dx = -SS; dx <= SS; dx++)
      if (dx * dx + dy * dy <= SS * SS) {
        sa = sa + pb[dy * PW + dx];
        sb = sb + pr[dy * PW + dx];
        sn = sn + wt[dy * PW + dx];
      }
  }
}
#define DF_DISC(SS) df_disc<SS>(lds, centre, sa, sb, sn)
#define DF_FOR_SAMPLE_RADIUS(S, CALL)                                                                                         \
  switch (S) {                                                                                                                \
    case 1: CALL(1); break; case 2: CALL(2); break; case 3: CALL(3); break; case 4: CALL(4); break;                           \
    case 5: CALL(5); break; case 6: CALL(6); break; case 7: CALL(7); break; default: CALL(8); break;                          \
  }

// ---- launch 2: th, then the fringed pixels
template <typename T, bool SQRT>
__global__ __launch_bounds__(DF_THREADS) void defringe_correct_kernel(const T* __restrict__ src, T* __restrict__ dst, unsigned char* __restrict__ mask_out,
                                                                      tdk_defringe_stats* __restrict__ stats_out, const float* __restrict__ eplane,
                                                                      const unsigned long long* __restrict__ records, DfArgs a) {
  __shared__ DfCorrectLds lds;
  const int tid = (int)threadIdx.x;
  const int W = a.width, H = a.height, S = a.sample_radius;
  const bool first = blockIdx.x == 0 && blockIdx.y == 0;

  // th: the same in every thread of every workgroup.  A static threshold needs no record; the first workgroup still adds them when
  // the caller asked for S.
  float th;
  unsigned long long total = 0;
  const bool is_static = (a.bits & DF_STATIC) != 0;
  if (!is_static || (first && stats_out)) {   // (uniform over the workgroup: the barrier inside is reached by all or none)
    unsigned long long v = 0;
    for (int k = tid; k < a.groups; k += DF_THREADS) v += records[k];
    total = df_block_sum(v, lds.part);
  }
  if (is_static) {
    th = fmaxf(a.floor, a.strength);
  } else {
    const double n = (double)W * (double)H;
    const float avg = (float)((double)total / (n * 1048576.0));
    th = fmaxf(a.floor, a.strength * avg);
  }
  if (first && stats_out && tid == 0) {
    stats_out->sum = total;
    stats_out->threshold = th;
    stats_out->reserved = 0;
  }

  const int x0 = (int)blockIdx.x * DF_T, y0 = (int)blockIdx.y * DF_T;
  const int tr = tid / DF_GROUPS, tc = (tid % DF_GROUPS) * DF_PIX;
  const int y = y0 + tr, x = x0 + tc;
  const bool row_in = y < H && x < W;
  const size_t pix = (size_t)y * W + x;   // (read only where row_in)

  // the own pixels: E, the decision and the samples
  float own_e[DF_PIX] = {0.0f, 0.0f, 0.0f, 0.0f}, own[3 * DF_PIX];
  bool fringed[DF_PIX];
#pragma unroll
  for (int i = 0; i < 3 * DF_PIX; i++) own[i] = 0.0f;
  if (row_in) {
    if (a.bits & DF_VEC_E) {   // (width % 4 == 0: the whole group lies inside the frame)
      s4_io<float>::load(eplane + pix, 0, own_e);
    } else {
#pragma unroll
      for (int i = 0; i < DF_PIX; i++)
        if (x + i < W) own_e[i] = eplane[pix + i];
    }
    if (a.bits & DF_VEC_IN) {
      rgb4_io<T>::load(src + pix * 3, 0, own);
    } else {
#pragma unroll
      for (int i = 0; i < 3 * DF_PIX; i++)
        if (x + i / 3 < W) own[i] = ld(src, pix * 3 + i);
    }
  }
  bool any = false;
#pragma unroll
  for (int i = 0; i < DF_PIX; i++) {
    fringed[i] = row_in && x + i < W && own_e[i] > th;
    any = any || fringed[i];
  }
  const bool work = block_any_sync<DF_THREADS / 64>(any, lds.votes);

  if (work) {
    // wt, wt*Cb, wt*Cr of the clamped pixel
    const int PW = DF_T + 2 * S;
    const float inv_pw = 1.0f / (float)PW;
    for (int e = tid; e < PW * PW; e += DF_THREADS) {
      int r, c;
      tdk_split_rc(e, PW, inv_pw, r, c);
      const int gy = min(max(y0 - S + r, 0), H - 1), gx = min(max(x0 - S + c, 0), W - 1);
      const size_t p = (size_t)gy * W + gx;
      const float t_r = df_work<SQRT>(ld(src, p * 3)), t_g = df_work<SQRT>(ld(src, p * 3 + 1)), t_b = df_work<SQRT>(ld(src, p * 3 + 2));
      const float wt = 1.0f / (eplane[p] + th);
      lds.wt[e] = wt;
      lds.pb[e] = wt * (t_b - t_g);
      lds.pr[e] = wt * (t_r - t_g);
    }
    *reinterpret_cast<uchar4*>(lds.flag + tr * DF_T + tc) = make_uchar4(fringed[0], fringed[1], fringed[2], fringed[3]);
    __syncthreads();

    // The disc, a lane per pixel of a tile row: consecutive lanes read consecutive words.  (Walked by the owners, four pixels apart,
    // the 64 reads of a wave fall on 16 of the 64 banks, and at half the pixels fringed the launch took as long as with the loop
    // it replaced.)  In round j a thread takes pixel j * 256 + tid of the tile; the owner gets the new chroma back through LDS.
#pragma unroll 1
    for (int p = tid; p < DF_T * DF_T; p += DF_THREADS) {
      if (!lds.flag[p]) continue;
      float sa = 0.0f, sb = 0.0f, sn = 0.0f;
      const int centre = (p / DF_T + S) * PW + p % DF_T + S;
      DF_FOR_SAMPLE_RADIUS(S, DF_DISC);
      lds.cb[p] = sa / sn;
      lds.cr[p] = sb / sn;
    }
    __syncthreads();

#pragma unroll
    for (int i = 0; i < DF_PIX; i++) {
      if (!fringed[i]) continue;
      const float cb = lds.cb[tr * DF_T + tc + i], cr = lds.cr[tr * DF_T + tc + i];
      const float t_r = df_work<SQRT>(own[3 * i]), t_g = df_work<SQRT>(own[3 * i + 1]), t_b = df_work<SQRT>(own[3 * i + 2]);
      const float Y = (0.25f * t_r + 0.5f * t_g) + 0.25f * t_b;
      const float g = Y - 0.25f * (cb + cr);
      const float vr = fmaxf(g + cr, 0.0f), vg = fmaxf(g, 0.0f), vb = fmaxf(g + cb, 0.0f);
      own[3 * i] = SQRT ? vr * vr : vr;
      own[3 * i + 1] = SQRT ? vg * vg : vg;
      own[3 * i + 2] = SQRT ? vb * vb : vb;
    }
    // A new value is a float32 value and a binary16 store rounds that.  The empty asm keeps the value one of its own, so that no
    // instruction that computes and converts in one step can take its place.
    if constexpr (sizeof(T) == 2) {
#pragma unroll
      for (int i = 0; i < 3 * DF_PIX; i++) asm volatile("" : "+v"(own[i]));
    }
  }

  // a sample that was not rewritten is the input's: float32 as it is, binary16 converted to float32 and back (exact)
  if (!row_in) return;
  if (a.bits & DF_VEC_OUT) {
    rgb4_io<T>::store(dst + pix * 3, 0, own);
  } else {
#pragma unroll
    for (int i = 0; i < 3 * DF_PIX; i++)
      if (x + i / 3 < W) st(dst, pix * 3 + i, own[i]);
  }
  if (mask_out) {
#pragma unroll
    for (int i = 0; i < DF_PIX; i++)
      if (x + i < W) mask_out[pix + i] = fringed[i] ? 1 : 0;
  }
}

bool df_flags_ok(int flags) {
  if (flags & ~(TDK_DEFRINGE_LINEAR | TDK_DEFRINGE_STATIC | TDK_DEFRINGE_GROUPS_MASK)) return false;
  return ((flags & TDK_DEFRINGE_GROUPS_MASK) >> TDK_DEFRINGE_GROUPS_SHIFT) <= DF_MAX_WG;
}
size_t df_plane_bytes(int width, int height) { return tdk_align_up((size_t)width * height * sizeof(float), DF_WS_ALIGN); }
size_t df_workspace_bytes(int width, int height) { return df_plane_bytes(width, height) + DF_MAX_WG * sizeof(unsigned long long) + DF_WS_ALIGN; }

template <typename T, bool SQRT>
int df_run(const void* src, void* dst, unsigned char* mask_out, float* edge_out, tdk_defringe_stats* stats_out, float* eplane, unsigned long long* records,
           const DfArgs& a, hipStream_t st) {
  const dim3 tiles((unsigned)tdk_div_up(a.width, DF_T), (unsigned)tdk_div_up(a.height, DF_T));
  TDK_LAUNCH("tdk_defringe(edge)", (defringe_edge_kernel<T, SQRT>), dim3((unsigned)a.groups), dim3(DF_THREADS), 0, st, reinterpret_cast<const T*>(src), eplane,
             edge_out, records, a);
  TDK_LAUNCH("tdk_defringe(correct)", (defringe_correct_kernel<T, SQRT>), tiles, dim3(DF_THREADS), 0, st, reinterpret_cast<const T*>(src),
             reinterpret_cast<T*>(dst), mask_out, stats_out, eplane, records, a);
  return TDK_OK;
}

}  // namespace

TDK_EXPORT int tdk_defringe_abi_version(void) { return TDK_DEFRINGE_ABI_VERSION; }

TDK_EXPORT int tdk_defringe_weights(float sigma, float* weights, int* radius) {
  return tdk_gaussian_taps("tdk_defringe_weights", sigma, 0.5f, 4.0f, DF_MAX_R, weights, radius);
}

TDK_EXPORT size_t tdk_defringe_workspace_bytes(int width, int height) { return tdk_frame_size_ok(width, height) ? df_workspace_bytes(width, height) : 0; }

TDK_EXPORT size_t tdk_defringe_lds_bytes(int dtype, int radius, int sample_radius, int flags) {
  if (!tdk_float_dtype_ok(dtype) || radius < 1 || radius > DF_MAX_R || sample_radius < 1 || sample_radius > DF_MAX_S || !df_flags_ok(flags)) return 0;
  return sizeof(DfEdgeLds) > sizeof(DfCorrectLds) ? sizeof(DfEdgeLds) : sizeof(DfCorrectLds);
}

TDK_EXPORT int tdk_defringe(const void* src, void* dst, unsigned char* mask_out, float* edge_out, tdk_defringe_stats* stats_out, void* workspace, int width,
                            int height, int dtype, const float* weights, int radius, int sample_radius, float strength, float floor, int flags,
                            tdk_stream_t stream) {
  TDK_REQUIRE(src && dst, "tdk_defringe: null pointer (src or dst)");
  TDK_REQUIRE(weights, "tdk_defringe: null pointer (weights)");
  TDK_REQUIRE(workspace, "tdk_defringe: null pointer (workspace)");
  TDK_REQUIRE(tdk_frame_size_ok(width, height), "tdk_defringe: frame size %dx%d outside 1..%d", width, height, TDK_FRAME_MAX_SIZE);
  TDK_REQUIRE(tdk_float_dtype_ok(dtype), "tdk_defringe: unsupported dtype tag %d", dtype);
  TDK_REQUIRE(radius >= 1 && radius <= DF_MAX_R, "tdk_defringe: radius must be 1..%d, got %d", DF_MAX_R, radius);
  const int bad_tap = tdk_first_bad_weight(weights, radius + 1);
  TDK_REQUIRE(bad_tap < 0, "tdk_defringe: weights[%d] must be finite and >= 0", bad_tap);
  TDK_REQUIRE(sample_radius >= 1 && sample_radius <= DF_MAX_S, "tdk_defringe: sample_radius must be 1..%d, got %d", DF_MAX_S, sample_radius);
  TDK_REQUIRE(isfinite(strength) && strength >= 0.0f, "tdk_defringe: strength must be finite and >= 0");
  TDK_REQUIRE(isfinite(floor) && floor > 0.0f, "tdk_defringe: floor must be finite and > 0");
  TDK_REQUIRE(df_flags_ok(flags),
              "tdk_defringe: flags must be TDK_DEFRINGE_LINEAR, TDK_DEFRINGE_STATIC and a workgroup cap 0..%d in bits 8..18, the other bits are reserved, got %d",
              DF_MAX_WG, flags);
  TDK_REQUIRE(tdk_aligned(edge_out, 4), "tdk_defringe: edge_out must be aligned to 4 bytes");
  TDK_REQUIRE(tdk_aligned(stats_out, 8), "tdk_defringe: stats_out must be aligned to 8 bytes");
  const size_t esz = tdk_dtype_bytes(dtype), n = (size_t)width * height, frame_bytes = 3 * n * esz, ws_bytes = df_workspace_bytes(width, height);
  TDK_REQUIRE(tdk_disjoint(src, frame_bytes, dst, frame_bytes), "tdk_defringe: src and dst overlap (every output reads its neighbours)");
  // the optional outputs and the workspace: each against src, dst and every one before it
  const void* ptr[6] = {src, dst, mask_out, edge_out, stats_out, workspace};
  const size_t len[6] = {frame_bytes, frame_bytes, n, n * sizeof(float), sizeof(tdk_defringe_stats), ws_bytes};
  const char* what[6] = {"src", "dst", "mask_out", "edge_out", "stats_out", "the workspace"};
  for (int i = 2; i < 6; i++)
    for (int j = 0; j < i; j++)
      TDK_REQUIRE(!ptr[i] || !ptr[j] || tdk_disjoint(ptr[i], len[i], ptr[j], len[j]), "tdk_defringe: %s overlaps %s", what[i], what[j]);

  DfArgs a{};
  for (int k = 0; k <= radius; k++) a.w[k] = weights[k];
  a.strength = strength, a.floor = floor;
  a.width = width, a.height = height, a.radius = radius, a.sample_radius = sample_radius;
  const int cap = (flags & TDK_DEFRINGE_GROUPS_MASK) >> TDK_DEFRINGE_GROUPS_SHIFT;
  const long long tiles = (long long)tdk_div_up(width, DF_T) * tdk_div_up(height, DF_T);
  const int limit = cap ? cap : DF_MAX_WG;
  a.groups = tiles < limit ? (int)tiles : limit;
  a.bits = (flags & TDK_DEFRINGE_STATIC) ? DF_STATIC : 0;
  // a thread's four pixels as whole vectors: rows must hold whole groups and start on the vector's alignment
  if (tdk_vec4_ok(width, src, 4 * esz)) a.bits |= DF_VEC_IN;
  if (tdk_vec4_ok(width, dst, 4 * esz)) a.bits |= DF_VEC_OUT;
  if (width % DF_PIX == 0) a.bits |= DF_VEC_E;   // (the plane starts on 16 bytes)
  float* eplane = reinterpret_cast<float*>(tdk_align_up(reinterpret_cast<uintptr_t>(workspace), DF_WS_ALIGN));
  unsigned long long* records = reinterpret_cast<unsigned long long*>(reinterpret_cast<char*>(eplane) + df_plane_bytes(width, height));
  const bool linear = (flags & TDK_DEFRINGE_LINEAR) != 0;
  hipStream_t st = tdk_stream(stream);
  if (dtype == TDK_F32) {
    if (linear) return df_run<float, false>(src, dst, mask_out, edge_out, stats_out, eplane, records, a, st);
    return df_run<float, true>(src, dst, mask_out, edge_out, stats_out, eplane, records, a, st);
  }
  if (linear) return df_run<__half, false>(src, dst, mask_out, edge_out, stats_out, eplane, records, a, st);
  return df_run<__half, true>(src, dst, mask_out, edge_out, stats_out, eplane, records, a, st);
}
