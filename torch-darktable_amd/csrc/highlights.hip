// highlights.hip -- white balance that reconstructs clipped highlights (include/tdk_hip_highlights.h: tdk_highlights,
// tdk_highlights_chrominance), at most two launches, three with the finishing launch of tdk_highlights_chrominance.
//
// The specification is the head comment of include/tdk_hip_highlights.h.
//
// A tile is HL_TW x HL_TH = 128 x 16 sites; a workgroup of four waves stages it with an apron of two sites as v = L * g[c] and the
// clipped flag (hl_stage).  Rows and columns are staged in PAIRS, a 2 x 2 CFA cell per lane and step: the tile origin and the apron
// are even, so the CFA position of each of the four sites is a constant of the code and its gain a scalar -- no per-site colour
// lookup.  Sites outside the frame are staged as v = 0, flag = 0: adding +0 to a sum of non-negative values is exact, so a missing
// neighbour drops out of S_k by itself and only the counts n_k look at the frame's edge.
// After staging a thread owns a block of 2 x 4 sites (two cells).  In a Bayer frame the 3 x 3 neighbourhood of a site splits by
// position: for a red or blue site the two other colours are the cross (up, left, right, down: green) and the four corners; for a
// green site they are left + right and up + down.  mean_a + mean_b is commutative, so ref needs no colour order (hl_refs).
//
// Statistics launch, hl_stats<T>: HL_GROUPS = 256 workgroups walk the tiles grid-stride.  A tile whose staged area holds no clipped
// site is skipped right after staging (a workgroup-uniform branch: nearly every tile of a real frame).  Otherwise the flags are
// dilated along the rows into LDS (five bytes ORed by shifts of a 64-bit word) and along the columns in registers; a thread
// accumulates q and the count per CFA POSITION in integers.  At the end the workgroup reduces them (shuffles inside a wave, LDS
// across the waves), folds positions into colours and writes its 48-byte record -- every record on every call, nothing is zeroed.
// Apply launch, hl_apply<TI, TO>: a workgroup per tile.  Without a clipped site in the staged area it stores fmaxf(v, 0) and never
// reads the records; otherwise it sums the 256 records with integer adds (a record per thread), forms chroma in float64, or takes
// the caller's three floats, and rebuilds the clipped sites.
// Clip launch, hl_clip<TI, TO>: streaming, a site pair per lane, no LDS.
// No location is accumulated into by more than one thread, and the sums are integers: the bits do not depend on scheduling.  Global accesses are site pairs, consecutive lanes on
// consecutive pairs: 8-byte (float32) or 4-byte (binary16) accesses where the buffer starts on a pair, per element otherwise.
#include <math.h>

#include "../../include/tdk_hip_highlights.h"
#include "tdk_frame.h"

namespace {

constexpr int HL_THREADS = 256, HL_WAVES = HL_THREADS / 64;
constexpr int HL_TW = 128, HL_TH = 16, HL_APRON = 2;
constexpr int HL_PITCH = HL_TW + 2 * HL_APRON, HL_SROWS = HL_TH + 2 * HL_APRON;   // staged: 20 rows of 132 sites
constexpr int HL_CELLS_X = HL_PITCH / 2, HL_CELLS_Y = HL_SROWS / 2;               // ... as 10 rows of 66 cells
constexpr int HL_QUADS = HL_TW / 4;                                               // a thread's block is 2 rows x 4 columns
constexpr int HL_GROUPS = 256;                                                    // workgroups, and records, of the statistics launch
constexpr size_t HL_WS_ALIGN = 8;
static_assert(HL_THREADS == (HL_TH / 2) * HL_QUADS, "a thread per 2 x 4 sites of the tile");
static_assert(HL_GROUPS == HL_THREADS, "the apply launch reads a record per thread");
static_assert(HL_PITCH % 4 == 0 && HL_TW % 4 == 0, "flag rows are read as 32-bit words");

struct HlRecord {
  long long sum[3], cnt[3];
};
static_assert(sizeof(HlRecord) == 48, "record");

struct HlArgs {
  float threshold, low;
  int min_count;
  int w, h;
  uint32_t pattern;
  int tiles_x, tiles_y;
  int vec_in, vec_out;
};

// the staged tile; every kernel's shared memory is one static object, so that its size is the kernel's group segment
struct HlTile {
  alignas(16) float v[HL_SROWS * HL_PITCH];
  alignas(16) uint8_t flag[HL_SROWS * HL_PITCH];
  int any[2][HL_WAVES];
};
struct HlReduce {
  long long part[HL_WAVES][8];
  float chroma[4];
};
struct HlStatsLds {
  HlTile t;
  alignas(16) uint8_t near[HL_SROWS * HL_TW];   // flags ORed over the columns j-2 .. j+2
  HlReduce r;
};
struct HlApplyLds {
  HlTile t;
  HlReduce r;
};
static_assert(sizeof(HlStatsLds) <= 64 * 1024 && sizeof(HlApplyLds) <= sizeof(HlStatsLds), "LDS of the largest launch");

// per CFA position: colour, gain and the level the site clips at
struct HlSite {
  int col[4];
  float g[4], cl[4];
};
__device__ __forceinline__ HlSite hl_sites(const float* __restrict__ gains, const HlArgs& a) {
  const float gr = gains[0], gg = gains[1], gb = gains[2];
  HlSite s;
#pragma unroll
  for (int p = 0; p < 4; p++) {
    s.col[p] = (int)((a.pattern >> (2 * p)) & 3u);
    s.g[p] = s.col[p] == 0 ? gr : (s.col[p] == 2 ? gb : gg);
    s.cl[p] = a.threshold * s.g[p];
  }
  return s;
}

template <typename T> __device__ __forceinline__ void hl_load_pair(const T* src, size_t o, bool vec, float& l0, float& l1);
template <> __device__ __forceinline__ void hl_load_pair<float>(const float* src, size_t o, bool vec, float& l0, float& l1) {
  if (vec) {
    const float2 f = *reinterpret_cast<const float2*>(src + o);
    l0 = f.x, l1 = f.y;
  } else {
    l0 = src[o], l1 = src[o + 1];
  }
}
template <> __device__ __forceinline__ void hl_load_pair<__half>(const __half* src, size_t o, bool vec, float& l0, float& l1) {
  if (vec) {
    const float2 f = __half22float2(*reinterpret_cast<const __half2*>(src + o));
    l0 = f.x, l1 = f.y;
  } else {
    l0 = __half2float(src[o]), l1 = __half2float(src[o + 1]);
  }
}
template <typename T> __device__ __forceinline__ void hl_store_pair(T* dst, size_t o, bool vec, float v0, float v1);
template <> __device__ __forceinline__ void hl_store_pair<float>(float* dst, size_t o, bool vec, float v0, float v1) {
  if (vec) *reinterpret_cast<float2*>(dst + o) = make_float2(v0, v1);
  else dst[o] = v0, dst[o + 1] = v1;
}
template <> __device__ __forceinline__ void hl_store_pair<__half>(__half* dst, size_t o, bool vec, float v0, float v1) {
  if (vec) *reinterpret_cast<__half2*>(dst + o) = __floats2half2_rn(v0, v1);
  else dst[o] = __float2half_rn(v0), dst[o + 1] = __float2half_rn(v1);
}

// The tile at (x0, y0), both even, and its apron as v and flag; sites outside the frame as 0 / 0.  Returns whether any site the
// WORKGROUP staged is clipped; the barrier inside also publishes the tile.  `phase` alternates between successive calls.
template <typename T> __device__ __forceinline__ bool hl_stage(const T* __restrict__ src, const HlArgs& a, const HlSite& s, int x0, int y0, HlTile& t, int phase) {
  const int tid = threadIdx.x;
  bool mine = false;
  for (int e = tid; e < HL_CELLS_Y * HL_CELLS_X; e += HL_THREADS) {
    const int cy = e / HL_CELLS_X, cx = e - cy * HL_CELLS_X;
    const int gi = y0 - HL_APRON + 2 * cy, gj = x0 - HL_APRON + 2 * cx;   // even: the cell is inside or outside the frame as one
    float v[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    bool f[4] = {false, false, false, false};
    if (gi >= 0 && gi < a.h && gj >= 0 && gj < a.w) {
      float l[4];
      const size_t o = (size_t)gi * a.w + gj;
      hl_load_pair<T>(src, o, a.vec_in, l[0], l[1]);
      hl_load_pair<T>(src, o + a.w, a.vec_in, l[2], l[3]);
#pragma unroll
      for (int p = 0; p < 4; p++) {
        v[p] = l[p] * s.g[p];
        f[p] = l[p] >= a.threshold;
        mine = mine || f[p];
      }
    }
    const int at = 2 * cy * HL_PITCH + 2 * cx;
    *reinterpret_cast<float2*>(t.v + at) = make_float2(v[0], v[1]);
    *reinterpret_cast<float2*>(t.v + at + HL_PITCH) = make_float2(v[2], v[3]);
    *reinterpret_cast<uint16_t*>(t.flag + at) = (uint16_t)((f[0] ? 1u : 0u) | (f[1] ? 0x100u : 0u));
    *reinterpret_cast<uint16_t*>(t.flag + at + HL_PITCH) = (uint16_t)((f[2] ? 1u : 0u) | (f[3] ? 0x100u : 0u));
  }
  const bool wave_any = __ballot(mine) != 0;
  if (tid % 64 == 0) t.any[phase][tid / 64] = wave_any ? 1 : 0;
  __syncthreads();
  int any = 0;
#pragma unroll
  for (int k = 0; k < HL_WAVES; k++) any |= t.any[phase][k];
  return any != 0;
}

// The thread's 2 x 4 block at staged row r0, staged column c0 (frame row i0, column j0): raw[dr * 4 + dc] = v, ref[dr * 4 + dc].
__device__ __forceinline__ void hl_refs(const HlTile& t, const HlArgs& a, bool green0, int r0, int c0, int i0, int j0, float* raw, float* ref) {
  float m[4][6];
#pragma unroll
  for (int r = 0; r < 4; r++)
#pragma unroll
    for (int c = 0; c < 6; c++) {
      const float x = t.v[(r0 - 1 + r) * HL_PITCH + c0 - 1 + c];
      if (r >= 1 && r <= 2 && c >= 1 && c <= 4) raw[(r - 1) * 4 + c - 1] = x;
      m[r][c] = fmaxf(x, 0.0f);
    }
  float rin[4], cin[6];   // 1 inside the frame, 0 outside
#pragma unroll
  for (int r = 0; r < 4; r++) rin[r] = (i0 - 1 + r >= 0 && i0 - 1 + r < a.h) ? 1.0f : 0.0f;
#pragma unroll
  for (int c = 0; c < 6; c++) cin[c] = (j0 - 1 + c >= 0 && j0 - 1 + c < a.w) ? 1.0f : 0.0f;
#pragma unroll
  for (int dr = 0; dr < 2; dr++)
#pragma unroll
    for (int dc = 0; dc < 4; dc++) {
      const int r = dr + 1, c = dc + 1, p = 2 * dr + (dc & 1);
      const bool green = (p == 0 || p == 3) ? green0 : !green0;   // (uniform)
      const float rows = rin[r - 1] + rin[r + 1], cols = cin[c - 1] + cin[c + 1];
      float mean_a, mean_b;
      if (green) {   // left + right, up + down
        mean_a = ((0.0f + m[r][c - 1]) + m[r][c + 1]) / cols;
        mean_b = ((0.0f + m[r - 1][c]) + m[r + 1][c]) / rows;
      } else {       // the cross and the corners, row-major
        mean_a = ((((0.0f + m[r - 1][c]) + m[r][c - 1]) + m[r][c + 1]) + m[r + 1][c]) / (rows + cols);
        mean_b = ((((0.0f + m[r - 1][c - 1]) + m[r - 1][c + 1]) + m[r + 1][c - 1]) + m[r + 1][c + 1]) / (rows * cols);
      }
      ref[dr * 4 + dc] = 0.5f * (mean_a + mean_b);
    }
}

// val[0..N) summed over the workgroup with integer adds; the result is in r.part[0][0..N) after the call's last barrier
template <int N> __device__ __forceinline__ void hl_reduce(long long* val, HlReduce& r) {
  const int tid = threadIdx.x;
#pragma unroll
  for (int k = 0; k < N; k++)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) val[k] += __shfl_xor(val[k], o, 64);
  if (tid % 64 == 0) {
#pragma unroll
    for (int k = 0; k < N; k++) r.part[tid / 64][k] = val[k];
  }
  __syncthreads();
  if (tid < N) {
    long long s = 0;
#pragma unroll
    for (int w = 0; w < HL_WAVES; w++) s += r.part[w][tid];
    val[0] = s;
  }
  __syncthreads();
  if (tid < N) r.part[0][tid] = val[0];
  __syncthreads();
}

__device__ __forceinline__ float hl_chroma(long long sum, long long cnt, int min_count) {
  return cnt >= (long long)min_count ? (float)((double)sum / ((double)cnt * 1048576.0)) : 0.0f;
}

// the records summed: sum[3], cnt[3] in r.part[0][0..6)
__device__ __forceinline__ void hl_sum_records(const HlRecord* __restrict__ records, HlReduce& r) {
  const HlRecord rec = records[threadIdx.x];
  long long val[6] = {rec.sum[0], rec.sum[1], rec.sum[2], rec.cnt[0], rec.cnt[1], rec.cnt[2]};
  hl_reduce<6>(val, r);
}

template <typename T>
__global__ __launch_bounds__(HL_THREADS) void hl_stats(const T* __restrict__ src, const float* __restrict__ gains, HlRecord* __restrict__ records, HlArgs a) {
  __shared__ HlStatsLds lds;
  const int tid = threadIdx.x;
  const HlSite s = hl_sites(gains, a);
  const bool green0 = s.col[0] == 1;
  const int tiles_x = a.tiles_x, tiles = a.tiles_x * a.tiles_y;
  const int rp = tid / HL_QUADS, cq = tid % HL_QUADS;
  const int r0 = 2 * rp + HL_APRON, c0 = 4 * cq + HL_APRON;
  long long sum[4] = {0, 0, 0, 0};   // per CFA position
  int cnt[4] = {0, 0, 0, 0};
  int phase = 0;
  for (int tile = (int)blockIdx.x; tile < tiles; tile += HL_GROUPS, phase ^= 1) {
    const int ty = tile / tiles_x, tx = tile - ty * tiles_x;
    const int x0 = tx * HL_TW, y0 = ty * HL_TH;
    if (!hl_stage<T>(src, a, s, x0, y0, lds.t, phase)) continue;   // (the whole workgroup)
    // flags ORed over five columns: eight flag bytes as one 64-bit word, byte k of the result covers the bytes k .. k + 4
    for (int e = tid; e < HL_SROWS * HL_QUADS; e += HL_THREADS) {
      const int r = e / HL_QUADS, q = e - r * HL_QUADS;
      const uint32_t* f = reinterpret_cast<const uint32_t*>(lds.t.flag + r * HL_PITCH + 4 * q);
      const uint64_t x = (uint64_t)f[0] | ((uint64_t)f[1] << 32);
      const uint64_t y = x | (x >> 8) | (x >> 16) | (x >> 24) | (x >> 32);
      *reinterpret_cast<uint32_t*>(lds.near + r * HL_TW + 4 * q) = (uint32_t)y;
    }
    __syncthreads();
    const int i0 = y0 + 2 * rp, j0 = x0 + 4 * cq;
    if (i0 < a.h && j0 < a.w) {
      float raw[8], ref[8];
      hl_refs(lds.t, a, green0, r0, c0, i0, j0, raw, ref);
      uint32_t col5[6];
#pragma unroll
      for (int r = 0; r < 6; r++) col5[r] = *reinterpret_cast<const uint32_t*>(lds.near + (2 * rp + r) * HL_TW + 4 * cq);
      const uint32_t near[2] = {col5[0] | col5[1] | col5[2] | col5[3] | col5[4], col5[1] | col5[2] | col5[3] | col5[4] | col5[5]};
#pragma unroll
      for (int dr = 0; dr < 2; dr++)
#pragma unroll
        for (int dc = 0; dc < 4; dc++) {
          const int p = 2 * dr + (dc & 1), k = dr * 4 + dc;
          const bool clipped = lds.t.flag[(r0 + dr) * HL_PITCH + c0 + dc] != 0;
          const float d = raw[k] - ref[k];
          const bool in = !clipped && raw[k] > a.low * s.cl[p] && ((near[dr] >> (8 * dc)) & 0xffu) != 0 && fabsf(d) <= 64.0f && j0 + dc < a.w;
          if (in) {
            sum[p] += (long long)rintf(d * 1048576.0f);
            cnt[p] += 1;
          }
        }
    }
    __syncthreads();   // the next tile is staged over this one
  }
  long long val[8] = {sum[0], sum[1], sum[2], sum[3], cnt[0], cnt[1], cnt[2], cnt[3]};
  hl_reduce<8>(val, lds.r);
  if (tid < 3) {   // positions folded into colours
    long long sc = 0, nc = 0;
#pragma unroll
    for (int p = 0; p < 4; p++)
      if (s.col[p] == tid) sc += lds.r.part[0][p], nc += lds.r.part[0][4 + p];
    records[blockIdx.x].sum[tid] = sc;
    records[blockIdx.x].cnt[tid] = nc;
  }
}

__global__ __launch_bounds__(HL_THREADS) void hl_finish(const HlRecord* __restrict__ records, long long* __restrict__ stats, float* __restrict__ chroma, int min_count) {
  __shared__ HlReduce r;
  hl_sum_records(records, r);
  const int tid = threadIdx.x;
  if (tid < 3) {
    const long long sum = r.part[0][tid], cnt = r.part[0][3 + tid];
    if (stats != nullptr) stats[tid] = sum, stats[3 + tid] = cnt;
    if (chroma != nullptr) chroma[tid] = hl_chroma(sum, cnt, min_count);
  }
}

template <typename TI, typename TO>
__global__ __launch_bounds__(HL_THREADS) void hl_apply(const TI* __restrict__ src, TO* __restrict__ dst, const float* __restrict__ gains,
                                                       const HlRecord* __restrict__ records, const float* __restrict__ chroma_in, HlArgs a) {
  __shared__ HlApplyLds lds;
  const int tid = threadIdx.x;
  const HlSite s = hl_sites(gains, a);
  const int x0 = (int)blockIdx.x * HL_TW, y0 = (int)blockIdx.y * HL_TH;
  const bool any = hl_stage<TI>(src, a, s, x0, y0, lds.t, 0);
  const int rp = tid / HL_QUADS, cq = tid % HL_QUADS;
  const int r0 = 2 * rp + HL_APRON, c0 = 4 * cq + HL_APRON;
  const int i0 = y0 + 2 * rp, j0 = x0 + 4 * cq;
  const bool live = i0 < a.h && j0 < a.w;
  float out[8];
  if (!any) {
    if (!live) return;
#pragma unroll
    for (int dr = 0; dr < 2; dr++) {
      const float2 lo = *reinterpret_cast<const float2*>(lds.t.v + (r0 + dr) * HL_PITCH + c0);
      const float2 hi = *reinterpret_cast<const float2*>(lds.t.v + (r0 + dr) * HL_PITCH + c0 + 2);
      out[dr * 4] = fmaxf(lo.x, 0.0f), out[dr * 4 + 1] = fmaxf(lo.y, 0.0f), out[dr * 4 + 2] = fmaxf(hi.x, 0.0f), out[dr * 4 + 3] = fmaxf(hi.y, 0.0f);
    }
  } else {
    if (chroma_in != nullptr) {
      if (tid < 3) lds.r.chroma[tid] = chroma_in[tid];
    } else {
      hl_sum_records(records, lds.r);
      if (tid < 3) lds.r.chroma[tid] = hl_chroma(lds.r.part[0][tid], lds.r.part[0][3 + tid], a.min_count);
    }
    __syncthreads();
    if (!live) return;
    float ch[4];   // per CFA position
#pragma unroll
    for (int p = 0; p < 4; p++) ch[p] = lds.r.chroma[s.col[p]];
    float raw[8], ref[8];
    hl_refs(lds.t, a, s.col[0] == 1, r0, c0, i0, j0, raw, ref);
#pragma unroll
    for (int dr = 0; dr < 2; dr++)
#pragma unroll
      for (int dc = 0; dc < 4; dc++) {
        const int p = 2 * dr + (dc & 1), k = dr * 4 + dc;
        const bool clipped = lds.t.flag[(r0 + dr) * HL_PITCH + c0 + dc] != 0;
        out[k] = fmaxf(raw[k], clipped ? ref[k] + ch[p] : 0.0f);
      }
  }
#pragma unroll
  for (int dr = 0; dr < 2; dr++) {
    const size_t o = (size_t)(i0 + dr) * a.w + j0;
    hl_store_pair<TO>(dst, o, a.vec_out, out[dr * 4], out[dr * 4 + 1]);
    if (j0 + 2 < a.w) hl_store_pair<TO>(dst, o + 2, a.vec_out, out[dr * 4 + 2], out[dr * 4 + 3]);
  }
}

template <typename TI, typename TO>
__global__ __launch_bounds__(HL_THREADS) void hl_clip(const TI* __restrict__ src, TO* __restrict__ dst, const float* __restrict__ gains, HlArgs a) {
  const HlSite s = hl_sites(gains, a);
  const float m = fminf(fminf(a.threshold * gains[0], a.threshold * gains[1]), a.threshold * gains[2]);
  const int pairs = a.w / 2;
  for (int y = (int)blockIdx.y; y < a.h; y += (int)gridDim.y) {
    const float ge = (y & 1) ? s.g[2] : s.g[0], go = (y & 1) ? s.g[3] : s.g[1];
    for (int x = (int)blockIdx.x * HL_THREADS + (int)threadIdx.x; x < pairs; x += (int)gridDim.x * HL_THREADS) {
      const size_t o = (size_t)y * a.w + 2 * x;
      float l0, l1;
      hl_load_pair<TI>(src, o, a.vec_in, l0, l1);
      hl_store_pair<TO>(dst, o, a.vec_out, fminf(fmaxf(l0 * ge, 0.0f), m), fminf(fmaxf(l1 * go, 0.0f), m));
    }
  }
}

HlRecord* hl_records(void* workspace) { return reinterpret_cast<HlRecord*>(tdk_align_up(reinterpret_cast<uintptr_t>(workspace), HL_WS_ALIGN)); }

template <typename T> int launch_stats(const void* src, const float* gains, void* workspace, const HlArgs& a, hipStream_t st) {
  TDK_LAUNCH("tdk_highlights(statistics)", hl_stats<T>, dim3(HL_GROUPS), dim3(HL_THREADS), 0, st, reinterpret_cast<const T*>(src), gains, hl_records(workspace), a);
  return TDK_OK;
}

template <typename TI, typename TO>
int launch_apply(const void* src, void* dst, const float* gains, void* workspace, const float* chroma, int mode, const HlArgs& a, hipStream_t st) {
  const TI* s = reinterpret_cast<const TI*>(src);
  TO* d = reinterpret_cast<TO*>(dst);
  if (mode == TDK_HL_CLIP) {
    const int rows = a.h < 32768 ? a.h : 32768;
    TDK_LAUNCH("tdk_highlights(clip)", (hl_clip<TI, TO>), dim3((unsigned)tdk_div_up(a.w / 2, HL_THREADS), (unsigned)rows), dim3(HL_THREADS), 0, st, s, d, gains, a);
    return TDK_OK;
  }
  const dim3 grid((unsigned)a.tiles_x, (unsigned)a.tiles_y);
  const HlRecord* records = chroma ? nullptr : hl_records(workspace);
  TDK_LAUNCH("tdk_highlights(apply)", (hl_apply<TI, TO>), grid, dim3(HL_THREADS), 0, st, s, d, gains, records, chroma, a);
  return TDK_OK;
}


// the checks both entry points share; `who` is the entry point's name
int hl_check(const char* who, const void* src, int src_dtype, int width, int height, uint32_t pattern, const float* gains, float threshold, float low, int min_count) {
  TDK_REQUIRE(src, "%s: null pointer (src)", who);
  TDK_REQUIRE(gains, "%s: null pointer (gains)", who);
  TDK_REQUIRE(tdk_mosaic_size_ok(width, height), "%s: frame size %dx%d outside 2..%d", who, width, height, TDK_MOSAIC_MAX_SIZE);
  TDK_REQUIRE(width % 2 == 0 && height % 2 == 0, "%s: frame size %dx%d must be even in both axes (whole CFA cells)", who, width, height);
  TDK_REQUIRE(src_dtype == TDK_F32 || src_dtype == TDK_F16, "%s: unsupported dtype tag %d (src)", who, src_dtype);
  TDK_REQUIRE(tdk_pattern_ok(pattern), "%s: unknown Bayer pattern 0x%08x", who, pattern);
  TDK_REQUIRE(threshold > 0.0f && threshold <= 1.0f, "%s: threshold must lie in (0, 1]", who);
  TDK_REQUIRE(low >= 0.0f && low < 1.0f, "%s: low must lie in [0, 1)", who);
  TDK_REQUIRE(min_count >= 1, "%s: min_count must be >= 1, got %d", who, min_count);
  return TDK_OK;
}

HlArgs hl_args(const void* src, int src_dtype, const void* dst, int dst_dtype, int width, int height, uint32_t pattern, float threshold, float low, int min_count) {
  HlArgs a{};
  a.threshold = threshold, a.low = low, a.min_count = min_count;
  a.w = width, a.h = height, a.pattern = pattern;
  a.tiles_x = tdk_div_up(width, HL_TW), a.tiles_y = tdk_div_up(height, HL_TH);
  // a site pair as one access: the buffer must start on a pair (the width is even, so every row does then)
  a.vec_in = tdk_aligned(src, 2 * tdk_dtype_bytes(src_dtype));
  a.vec_out = dst != nullptr && tdk_aligned(dst, 2 * tdk_dtype_bytes(dst_dtype));
  return a;
}

}  // namespace

TDK_EXPORT int tdk_highlights_abi_version(void) { return TDK_HIGHLIGHTS_ABI_VERSION; }

TDK_EXPORT size_t tdk_highlights_workspace_bytes(void) { return (size_t)HL_GROUPS * sizeof(HlRecord) + HL_WS_ALIGN; }

TDK_EXPORT size_t tdk_highlights_lds_bytes(int mode) { return mode == TDK_HL_OPPOSED ? sizeof(HlStatsLds) : 0; }

TDK_EXPORT int tdk_highlights_chrominance(const void* src, int src_dtype, void* workspace, int width, int height, uint32_t pattern, const float* gains,
                                          float threshold, float low, int min_count, long long* stats, float* chroma, tdk_stream_t stream) {
  static const char* const who = "tdk_highlights_chrominance";
  const int rc = hl_check(who, src, src_dtype, width, height, pattern, gains, threshold, low, min_count);
  if (rc != TDK_OK) return rc;
  TDK_REQUIRE(workspace, "%s: null pointer (workspace)", who);
  TDK_REQUIRE(stats || chroma, "%s: null pointer (stats and chroma: one of them is needed)", who);
  TDK_REQUIRE(tdk_aligned(stats, 8), "%s: stats must be aligned to 8 bytes", who);
  const size_t src_bytes = (size_t)width * height * tdk_dtype_bytes(src_dtype), ws_bytes = tdk_highlights_workspace_bytes();
  const size_t stats_bytes = 6 * sizeof(long long), chroma_bytes = 3 * sizeof(float);
  TDK_REQUIRE(tdk_disjoint(workspace, ws_bytes, src, src_bytes) && tdk_disjoint(workspace, ws_bytes, gains, chroma_bytes), "%s: the workspace overlaps src or gains", who);
  TDK_REQUIRE(!stats || (tdk_disjoint(stats, stats_bytes, src, src_bytes) && tdk_disjoint(stats, stats_bytes, gains, chroma_bytes) &&
                         tdk_disjoint(stats, stats_bytes, workspace, ws_bytes)),
              "%s: stats overlaps src, gains or the workspace", who);
  TDK_REQUIRE(!chroma || (tdk_disjoint(chroma, chroma_bytes, src, src_bytes) && tdk_disjoint(chroma, chroma_bytes, gains, chroma_bytes) &&
                          tdk_disjoint(chroma, chroma_bytes, workspace, ws_bytes) && (!stats || tdk_disjoint(chroma, chroma_bytes, stats, stats_bytes))),
              "%s: chroma overlaps src, gains, stats or the workspace", who);
  const HlArgs a = hl_args(src, src_dtype, nullptr, TDK_F32, width, height, pattern, threshold, low, min_count);
  hipStream_t st = tdk_stream(stream);
  const int launched = src_dtype == TDK_F32 ? launch_stats<float>(src, gains, workspace, a, st) : launch_stats<__half>(src, gains, workspace, a, st);
  if (launched != TDK_OK) return launched;
  TDK_LAUNCH("tdk_highlights(finish)", hl_finish, dim3(1), dim3(HL_THREADS), 0, st, hl_records(workspace), stats, chroma, min_count);
  return TDK_OK;
}

TDK_EXPORT int tdk_highlights(const void* src, int src_dtype, void* dst, int dst_dtype, void* workspace, int width, int height, uint32_t pattern,
                              const float* gains, float threshold, float low, int min_count, int mode, const float* chroma, tdk_stream_t stream) {
  static const char* const who = "tdk_highlights";
  TDK_REQUIRE(dst, "%s: null pointer (dst)", who);
  const int rc = hl_check(who, src, src_dtype, width, height, pattern, gains, threshold, low, min_count);
  if (rc != TDK_OK) return rc;
  TDK_REQUIRE(dst_dtype == TDK_F32 || dst_dtype == TDK_F16, "%s: unsupported dtype tag %d (dst)", who, dst_dtype);
  TDK_REQUIRE(mode == TDK_HL_CLIP || mode == TDK_HL_OPPOSED, "%s: mode must be TDK_HL_CLIP or TDK_HL_OPPOSED, got %d", who, mode);
  TDK_REQUIRE(mode != TDK_HL_CLIP || (!workspace && !chroma), "%s: mode TDK_HL_CLIP takes no workspace and no chroma", who);
  const bool gather = mode == TDK_HL_OPPOSED && !chroma;
  TDK_REQUIRE(!gather || workspace, "%s: null pointer (workspace: the statistics need %zu bytes)", who, tdk_highlights_workspace_bytes());
  const size_t n = (size_t)width * height, src_bytes = n * tdk_dtype_bytes(src_dtype), dst_bytes = n * tdk_dtype_bytes(dst_dtype);
  const size_t ws_bytes = tdk_highlights_workspace_bytes(), three = 3 * sizeof(float);
  TDK_REQUIRE(tdk_disjoint(src, src_bytes, dst, dst_bytes), "%s: src and dst overlap (every output reads its neighbours)", who);
  TDK_REQUIRE(tdk_disjoint(gains, three, dst, dst_bytes), "%s: gains and dst overlap", who);
  TDK_REQUIRE(!chroma || tdk_disjoint(chroma, three, dst, dst_bytes), "%s: chroma and dst overlap", who);
  TDK_REQUIRE(!gather || (tdk_disjoint(workspace, ws_bytes, src, src_bytes) && tdk_disjoint(workspace, ws_bytes, dst, dst_bytes) &&
                          tdk_disjoint(workspace, ws_bytes, gains, three)),
              "%s: the workspace overlaps src, dst or gains", who);

  const HlArgs a = hl_args(src, src_dtype, dst, dst_dtype, width, height, pattern, threshold, low, min_count);
  hipStream_t st = tdk_stream(stream);
  if (gather) {
    const int launched = src_dtype == TDK_F32 ? launch_stats<float>(src, gains, workspace, a, st) : launch_stats<__half>(src, gains, workspace, a, st);
    if (launched != TDK_OK) return launched;
  }
  TDK_DISPATCH_DTYPE(src_dtype, TI, TDK_DISPATCH_DTYPE(dst_dtype, TO, return (launch_apply<TI, TO>(src, dst, gains, workspace, chroma, mode, a, st))));
}
