// noiseprofile.hip -- the Poisson-Gaussian noise model of a set of raw mosaics (include/tdk_hip_noise.h: tdk_noise_profile: one gather
// launch and two small finishing launches) and the variance-stabilising transform around a denoiser (tdk_noise_stabilize,
// tdk_noise_unstabilize: one streaming launch each).
//
// The specification is the head comment of include/tdk_hip_noise.h.
//
// Gather, np_gather<T>: NP_GRID = 512 workgroups of 512 lanes whatever the frame size and the number of frames (two per compute
// unit).  The work is cut into UNITS: a strip of 16 mosaic rows and 512 bytes of each row (128 float32 or 256 16-bit columns: 8 or
// 16 tiles of 16 x 16 sites, four 8 x 8 blocks each), numbered frame by frame and row of tiles by row of tiles, walked grid-stride.
// A lane reads 16 bytes of one row (a 16-byte vector when the address allows it, per element otherwise), so a row of the strip is
// 512 contiguous bytes of 32 lanes; the loads of the next unit are issued before the blocks of this one are worked on.  The lane
// converts its sites to q and stores them into LDS de-interleaved: stage[CFA position][tile][8 x 8] as uint16, so that a block is
// 64 consecutive values, and flags the block of a NaN.  Only complete tiles are read: nothing outside them is touched.
// A wave then takes eight blocks, eight lanes each: a lane reads row r of its block and the rows above and below as three 16-byte
// LDS reads (consecutive lanes, consecutive addresses), forms the row's part of S, qmin, qmax and the 64-bit E in registers, and three
// shuffle steps reduce them over the eight rows.  (A lane per sample needs six steps per block and is bound by their latency.)  The
// first lane of a block forms the bin and the level and counts with one 32-bit and one 64-bit LDS integer atomic; the three block
// counters are LDS atomics too.  The 64 block slots of the eight waves cover a unit in one pass.
// At the end every workgroup writes its record -- levels, sums, counters -- to its place in the workspace, also when it had no unit.
// Finish 1, np_reduce: sums the records into `counts` (integer adds; sixteen lanes share a counter's records).
// Finish 2, np_derive: one workgroup; a lane per (colour, bin) walks the 128 levels for the median and forms x, v, w in double, a
// lane per colour fits the line.
// No location is accumulated into by more than one workgroup and all sums are integers: the bits do not depend on scheduling.
//
// Transform, np_vst<TS, TD, KIND, FORWARD>: a lane takes four consecutive elements (one vector when source and destination are
// aligned to four elements, per element otherwise and in the tail); the three rows of constants are formed by every lane from the
// model and the gains in device memory.
#include <math.h>

#include "../../include/tdk_hip_noise.h"
#include "tdk_frame.h"

namespace {

constexpr int NP_THREADS = 512, NP_WAVES = NP_THREADS / 64;
constexpr int NP_GRID = TDK_NOISE_GRID;
constexpr int NP_ROWS = 16;                                   // mosaic rows of a unit: one row of tiles
constexpr int NP_GROUPS = NP_THREADS / NP_ROWS;               // lanes of a row, 16 bytes each
constexpr int NP_MAX_TILES = 16;                              // tiles of a unit at 16-bit storage
constexpr int NP_LEVELS = TDK_NOISE_LEVELS;
constexpr int NP_HIST_WORDS = 3 * TDK_NOISE_MAX_BINS * NP_LEVELS;
constexpr int NP_COUNTERS = 9;                                // all, nan, clipped: [which * 3 + colour]
constexpr int NP_RED_IDX = 32, NP_RED_LANES = NP_THREADS / NP_RED_IDX;   // np_reduce: counters of a workgroup, lanes per counter
constexpr int NP_DER_THREADS = 128;
constexpr size_t NP_WS_ALIGN = 8;
constexpr int NP_VST_THREADS = 256, NP_VST_GRID = 2048;   // a launch beyond NP_VST_GRID * NP_VST_THREADS * 4 elements makes every lane loop
static_assert(NP_GROUPS * 16 == TDK_NOISE_STRIP_BYTES, "the strip the header states");
static_assert(3 * TDK_NOISE_MAX_BINS <= NP_DER_THREADS, "a lane per (colour, bin)");
static_assert(NP_WAVES * 8 >= 4 * NP_MAX_TILES, "a block slot per block of a unit");

struct NpLds {
  uint32_t hist[NP_HIST_WORDS];                     // [colour][bin][level] at the call's bins
  unsigned long long sum[3 * TDK_NOISE_MAX_BINS];   // [colour][bin]
  unsigned long long cnt[NP_COUNTERS + 1];
  alignas(16) uint16_t stage[4 * NP_MAX_TILES * 64];   // [CFA position][tile][r * 8 + c]: a row of a block is 16 bytes
  uint32_t nan[4 * NP_MAX_TILES];                   // [tile * 4 + CFA position]: the block holds a NaN; cleared by the wave that reads it
};
static_assert(sizeof(NpLds) <= 64 * 1024, "LDS of the gather launch");

struct NpArgs {
  const void* frames[TDK_NOISE_MAX_FRAMES];
  int w, tiles_x, tiles_y;
  int units_per_row, units_per_frame, units;   // units of a row of tiles, of a frame, of the set
  int bins, clip_lo, clip_hi;
  float scale;
  uint32_t pattern;
};

struct NpDerive {
  int bins, min_count;
  float white;
};

// ---- storage: element j of the 16 bytes w, as float32
template <typename T> __device__ __forceinline__ float np_unpack(const uint32_t w[4], int j);
template <> __device__ __forceinline__ float np_unpack<float>(const uint32_t w[4], int j) { return __uint_as_float(w[j]); }
template <> __device__ __forceinline__ float np_unpack<__half>(const uint32_t w[4], int j) {
  return __half2float(__ushort_as_half((unsigned short)((w[j / 2] >> (16 * (j % 2))) & 0xffffu)));
}
template <> __device__ __forceinline__ float np_unpack<uint16_t>(const uint32_t w[4], int j) { return (float)((w[j / 2] >> (16 * (j % 2))) & 0xffffu); }

// the 16 bytes at p: one vector when p is on a 16-byte boundary, per element otherwise
template <typename T> __device__ __forceinline__ void np_load16(const T* p, uint32_t w[4]) {
  constexpr int PER = 16 / (int)sizeof(T);
  if ((reinterpret_cast<uintptr_t>(p) & 15u) == 0) {
    const uint4 u = *reinterpret_cast<const uint4*>(p);
    w[0] = u.x, w[1] = u.y, w[2] = u.z, w[3] = u.w;
  } else if constexpr (sizeof(T) == 4) {
    const uint32_t* q = reinterpret_cast<const uint32_t*>(p);
#pragma unroll
    for (int j = 0; j < 4; j++) w[j] = q[j];
  } else {
    const uint16_t* q = reinterpret_cast<const uint16_t*>(p);
#pragma unroll
    for (int j = 0; j < PER / 2; j++) w[j] = (uint32_t)q[2 * j] | ((uint32_t)q[2 * j + 1] << 16);
  }
}

// level(E) of the header
__device__ __forceinline__ int np_level(unsigned long long e) {
  if (e < 256ull) return 0;
  const int lg = 63 - __clzll((long long)e);
  const int l = 4 * (lg - 8) + (int)((e >> (lg - 2)) & 3ull) + 1;
  return l < NP_LEVELS - 1 ? l : NP_LEVELS - 1;
}
__device__ __forceinline__ unsigned long long np_level_edge(int l) { return (unsigned long long)(4 + ((l - 1) & 3)) << (((l - 1) >> 2) + 6); }

template <typename T>
__global__ __launch_bounds__(NP_THREADS) void np_gather(NpArgs a, unsigned char* __restrict__ records) {
  constexpr int PER = 16 / (int)sizeof(T);   // sites of a lane
  constexpr int TILES = 2 * PER;             // tiles of a unit: NP_GROUPS * PER / 16
  static_assert(TILES <= NP_MAX_TILES, "the staged strip");
  __shared__ NpLds lds;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int words = 3 * a.bins * NP_LEVELS;
  for (int i = tid; i < words; i += NP_THREADS) lds.hist[i] = 0u;
  if (tid < 3 * TDK_NOISE_MAX_BINS) lds.sum[tid] = 0ull;
  if (tid < NP_COUNTERS + 1) lds.cnt[tid] = 0ull;
  if (tid < 4 * NP_MAX_TILES) lds.nan[tid] = 0u;

  // the lane as a loader: row lrow of the strip, sites [lgrp * PER, lgrp * PER + PER) of it, all inside tile ltile
  const int lrow = tid / NP_GROUPS, lgrp = tid % NP_GROUPS;
  const int ltile = lgrp * PER / 16;
  const int lplane = 2 * (lrow & 1);                                           // + (column & 1): the CFA position
  const int lat = (lrow >> 1) * 8 + ((lgrp * PER) & 15) / 2;                   // r * 8 + c of the lane's first site; c is even
  // the lane as a worker: row r of one of the eight blocks of its wave; the first and the last row have no vertical difference
  const int r = lane & 7;
  const bool has_v = r >= 1 && r <= 6;

  uint32_t raw[4] = {0u, 0u, 0u, 0u};
  bool loaded = false;
  int tx0 = 0;
  auto fetch = [&](int unit) {
    const int f = unit / a.units_per_frame, rem = unit - f * a.units_per_frame;
    const int ty = rem / a.units_per_row;
    tx0 = (rem - ty * a.units_per_row) * TILES;
    loaded = tx0 + ltile < a.tiles_x;
    if (loaded) np_load16<T>(reinterpret_cast<const T*>(a.frames[f]) + (size_t)(ty * NP_ROWS + lrow) * a.w + (size_t)tx0 * 16 + lgrp * PER, raw);
  };

  int unit = (int)blockIdx.x;
  if (unit < a.units) fetch(unit);
  __syncthreads();
  while (unit < a.units) {
    const int first_tile = tx0;
    if (loaded) {
      uint32_t q[PER];
      bool bad[2] = {false, false};
#pragma unroll
      for (int m = 0; m < PER; m++) {
        const float x = np_unpack<T>(raw, m);
        bad[m & 1] = bad[m & 1] || x != x;
        q[m] = (uint32_t)(int)rintf(fminf(fmaxf(x * a.scale, 0.0f), 65535.0f));
      }
#pragma unroll
      for (int pc = 0; pc < 2; pc++) {
        uint32_t* to = reinterpret_cast<uint32_t*>(lds.stage + ((lplane + pc) * NP_MAX_TILES + ltile) * 64 + lat);
#pragma unroll
        for (int k = 0; k < PER / 4; k++) to[k] = q[pc + 4 * k] | (q[pc + 4 * k + 2] << 16);
        if (bad[pc]) lds.nan[ltile * 4 + lplane + pc] = 1u;
      }
    }
    __syncthreads();
    const int next = unit + NP_GRID;
    if (next < a.units) fetch(next);   // in flight while the blocks are worked on

    {
      // eight lanes per block, a lane per row of it: the row and its two neighbours are 16 bytes each
      const int b = wave * 8 + (lane >> 3), tile = b >> 2, p = b & 3;
      const bool live = b < 4 * TILES && first_tile + tile < a.tiles_x;   // (the others work on stale values and count nothing)
      const uint4* s = reinterpret_cast<const uint4*>(lds.stage + (p * NP_MAX_TILES + tile) * 64);
      const uint4 mid = s[r], above = s[r > 0 ? r - 1 : r], below = s[r < 7 ? r + 1 : r];
      const uint32_t wm[4] = {mid.x, mid.y, mid.z, mid.w}, wa[4] = {above.x, above.y, above.z, above.w}, wb[4] = {below.x, below.y, below.z, below.w};
      int q[8], up[8], down[8];
#pragma unroll
      for (int c = 0; c < 8; c++) {
        q[c] = (int)((wm[c / 2] >> (16 * (c % 2))) & 0xffffu);
        up[c] = (int)((wa[c / 2] >> (16 * (c % 2))) & 0xffffu);
        down[c] = (int)((wb[c / 2] >> (16 * (c % 2))) & 0xffffu);
      }
      unsigned long long e = 0ull;
      uint32_t sum = 0u;
      int qmin = q[0], qmax = q[0];
#pragma unroll
      for (int c = 0; c < 8; c++) {
        sum += (uint32_t)q[c];
        qmin = min(qmin, q[c]), qmax = max(qmax, q[c]);
        const int v = has_v ? 2 * q[c] - up[c] - down[c] : 0;
        const uint32_t av = (uint32_t)(v < 0 ? -v : v);
        e += (unsigned long long)av * av;
        if (c >= 1 && c <= 6) {
          const int h = 2 * q[c] - q[c - 1] - q[c + 1];
          const uint32_t ah = (uint32_t)(h < 0 ? -h : h);
          e += (unsigned long long)ah * ah;
        }
      }
#pragma unroll
      for (int o = 4; o > 0; o >>= 1) {   // over the eight rows of the block
        e += __shfl_xor(e, o, 64);
        sum += __shfl_xor(sum, o, 64);      // at most 64 * 65535
        qmin = min(qmin, __shfl_xor(qmin, o, 64)), qmax = max(qmax, __shfl_xor(qmax, o, 64));
      }
      if (live && r == 0) {
        const int k = (int)((a.pattern >> (2 * p)) & 3u);
        const bool bad = lds.nan[b] != 0u;
        if (bad) lds.nan[b] = 0u;
        atomicAdd(&lds.cnt[k], 1ull);
        if (bad) atomicAdd(&lds.cnt[3 + k], 1ull);
        else if (qmin < a.clip_lo || qmax > a.clip_hi) atomicAdd(&lds.cnt[6 + k], 1ull);
        else {
          const int i = (int)(((sum >> 6) * (uint32_t)a.bins) >> 16);
          atomicAdd(&lds.hist[(k * a.bins + i) * NP_LEVELS + np_level(e)], 1u);
          atomicAdd(&lds.sum[k * a.bins + i], (unsigned long long)sum);
        }
      }
    }
    __syncthreads();   // the strip and its flags are free again
    unit = next;
  }

  // ---- the record: levels, sums, counters
  const size_t rec_bytes = (size_t)words * 4 + (size_t)(3 * a.bins + NP_COUNTERS) * 8;
  unsigned char* rec = records + (size_t)blockIdx.x * rec_bytes;
  uint32_t* rec_hist = reinterpret_cast<uint32_t*>(rec);
  for (int i = tid; i < words; i += NP_THREADS) rec_hist[i] = lds.hist[i];
  unsigned long long* rec_sums = reinterpret_cast<unsigned long long*>(rec + (size_t)words * 4);
  if (tid < 3 * a.bins) rec_sums[tid] = lds.sum[tid];
  else if (tid < 3 * a.bins + NP_COUNTERS) rec_sums[tid] = lds.cnt[tid - 3 * a.bins];
}

// counts[o] from NP_GRID records: the order of a record is the order of `counts`
__global__ __launch_bounds__(NP_THREADS) void np_reduce(const unsigned char* __restrict__ records, int nrec, int bins, long long* __restrict__ counts) {
  __shared__ long long part[NP_RED_LANES][NP_RED_IDX];
  const int tid = threadIdx.x, idx = tid % NP_RED_IDX, lane = tid / NP_RED_IDX;
  const int words = 3 * bins * NP_LEVELS, outputs = words + 3 * bins + NP_COUNTERS;
  const int o = (int)blockIdx.x * NP_RED_IDX + idx;
  const size_t rec_bytes = (size_t)words * 4 + (size_t)(3 * bins + NP_COUNTERS) * 8;
  long long acc = 0;
  if (o < outputs) {
    for (int rc = lane; rc < nrec; rc += NP_RED_LANES) {
      const unsigned char* rec = records + (size_t)rc * rec_bytes;
      acc += o < words ? (long long)reinterpret_cast<const uint32_t*>(rec)[o] : reinterpret_cast<const long long*>(rec + (size_t)words * 4)[o - words];
    }
  }
  part[lane][idx] = acc;
  __syncthreads();
  if (tid < NP_RED_IDX && o < outputs) {
    long long total = 0;
#pragma unroll
    for (int l = 0; l < NP_RED_LANES; l++) total += part[l][tid];
    counts[o] = total;
  }
}

// model[3][4] and curve[2][3][bins] from counts
__global__ __launch_bounds__(NP_DER_THREADS) void np_derive(const long long* __restrict__ counts, float* __restrict__ model, float* __restrict__ curve, NpDerive d) {
  __shared__ double px[3 * TDK_NOISE_MAX_BINS], pv[3 * TDK_NOISE_MAX_BINS], pw[3 * TDK_NOISE_MAX_BINS];
  __shared__ int usable[3 * TDK_NOISE_MAX_BINS];
  const int tid = threadIdx.x, I = d.bins;
  if (tid < 3 * I) {
    const long long* hist = counts + (size_t)tid * NP_LEVELS;
    long long n = 0;
#pragma unroll 16
    for (int l = 0; l < NP_LEVELS; l++) n += hist[l];
    bool ok = n >= (long long)d.min_count;
    double x = 0.0, v = 0.0, w = 0.0;
    if (ok) {
      double rd = ceil(0.5 * (double)n);
      rd = rd < 1.0 ? 1.0 : (rd > (double)n ? (double)n : rd);
      const long long rank = (long long)rd;
      long long prev = 0, cum = 0;
      int at = -1;
#pragma unroll 16
      for (int l = 0; l < NP_LEVELS; l++) {   // (no early exit: the loads of a batch of levels are in flight together)
        const long long upto = cum + hist[l];
        if (at < 0 && upto >= rank) at = l, prev = cum;
        cum = upto;
      }
      ok = at != 0 && at != NP_LEVELS - 1;
      if (ok) {
        const double frac = (double)(rank - prev) / (double)hist[at];
        const double lo = (double)np_level_edge(at), hi = (double)np_level_edge(at + 1);
        const double e_med = lo + frac * (hi - lo);
        const double ws = (double)d.white / 65535.0;
        v = (e_med / (576.0 * TDK_NOISE_MEDIAN_FACTOR)) * (ws * ws);
        x = (((double)counts[(size_t)3 * I * NP_LEVELS + tid] / (64.0 * (double)n)) / 65535.0) * (double)d.white;
        w = (double)n / (v * v);
      }
    }
    px[tid] = x, pv[tid] = v, pw[tid] = w, usable[tid] = ok ? 1 : 0;
    curve[tid] = (float)x;
    curve[3 * I + tid] = (float)v;
  }
  __syncthreads();
  if (tid < 3) {
    double sw = 0.0, swx = 0.0, swxx = 0.0, swv = 0.0, swxv = 0.0;
    int bins_used = 0;
    for (int i = 0; i < I; i++) {
      const int at = tid * I + i;
      if (!usable[at]) continue;
      const double wx = pw[at] * px[at];
      sw += pw[at], swx += wx, swxx += wx * px[at], swv += pw[at] * pv[at], swxv += wx * pv[at];
      bins_used++;
    }
    const double det = sw * swxx - swx * swx;
    double fa = 0.0, fb = 0.0;
    const bool valid = bins_used >= 2 && det > 0.0;
    if (valid) {
      fa = (sw * swxv - swx * swv) / det;
      fb = (swxx * swv - swx * swxv) / det;
      if (fa < 0.0) fa = 0.0, fb = swv / sw;
      else if (fb < 0.0) fb = 0.0, fa = swxv / swxx;
    }
    model[4 * tid] = (float)fa, model[4 * tid + 1] = (float)fb, model[4 * tid + 2] = valid ? 1.0f : 0.0f, model[4 * tid + 3] = (float)bins_used;
  }
}

// ---- the transform
enum { NP_ONE = 0, NP_RGB = 1, NP_MOSAIC = 2 };
enum { NP_IDENTITY = 0, NP_GAUSS = 1, NP_POISSON = 2 };

struct NpRow {
  float a, c, k, sb, coa, sn2;   // a', c, k, sqrtf(b'), c / a', b' / (a' * a')
  int mode;
};

__device__ __forceinline__ NpRow np_row(const float* __restrict__ model, const float* __restrict__ gains, int row, float s) {
  const float g = gains ? gains[row] : 1.0f;
  const float a = g * model[4 * row], b = (g * g) * model[4 * row + 1];
  NpRow o;
  o.a = a;
  o.c = 0.375f * (a * a) + b;
  o.k = (2.0f * s) / a;
  o.sb = sqrtf(b);
  o.coa = o.c / a;
  o.sn2 = b / (a * a);
  o.mode = (model[4 * row + 2] == 0.0f || (a == 0.0f && b == 0.0f)) ? NP_IDENTITY : a == 0.0f ? NP_GAUSS : NP_POISSON;
  return o;
}

// row `row` of three, field by field: values, not addresses, so that the rows stay in registers
__device__ __forceinline__ NpRow np_pick(int row, const NpRow& r0, const NpRow& r1, const NpRow& r2) {
  NpRow o;
#define NP_PICK(f) o.f = row == 0 ? r0.f : row == 1 ? r1.f : r2.f
  NP_PICK(a), NP_PICK(c), NP_PICK(k), NP_PICK(sb), NP_PICK(coa), NP_PICK(sn2), NP_PICK(mode);
#undef NP_PICK
  return o;
}

template <bool FORWARD> __device__ __forceinline__ float np_value(float x, const NpRow& o, float s, int inverse) {
  if (o.mode == NP_IDENTITY) return x;
  if constexpr (FORWARD) {
    if (o.mode == NP_GAUSS) return (s * x) / o.sb;
    return o.k * sqrtf(fmaxf(o.a * x + o.c, 0.0f));
  } else {
    const float d = x / s;
    if (o.mode == NP_GAUSS) return d * o.sb;
    if (inverse == TDK_NOISE_ALGEBRAIC) return ((o.a * (d * d)) * 0.25f) - o.coa;
    const float D = fmaxf(d, 1.2247449f), D2 = D * D;
    const float I = (((((D2 * 0.25f) + (0.30618622f / D)) - (1.375f / D2)) + (0.76546554f / (D2 * D))) - 0.125f) - o.sn2;
    return o.a * fmaxf(I, 0.0f);
  }
}

template <typename TS, typename TD, int KIND, bool FORWARD>
__global__ __launch_bounds__(NP_VST_THREADS) void np_vst(const TS* __restrict__ src, TD* __restrict__ dst, int64_t count, uint32_t width, uint32_t pattern,
                                                         const float* __restrict__ model, const float* __restrict__ gains, float s, int inverse, int vectors) {
  constexpr int ROWS = KIND == NP_ONE ? 1 : 3;
  const NpRow r0 = np_row(model, gains, 0, s), r1 = np_row(model, gains, ROWS > 1 ? 1 : 0, s), r2 = np_row(model, gains, ROWS > 1 ? 2 : 0, s);
  const int64_t groups = (count + 3) / 4, step = (int64_t)gridDim.x * NP_VST_THREADS;
  int64_t g = (int64_t)blockIdx.x * NP_VST_THREADS + threadIdx.x;
  // element 4 * g of an RGB image has the channel (4 * g) % 3 == g % 3: kept up to date by additions (g starts below 2^31)
  uint32_t phase = (uint32_t)g % 3u;
  const uint32_t phase_step = (uint32_t)(step % 3);
  for (; g < groups; g += step, phase = (phase + phase_step) % 3u) {
    const int64_t e0 = 4 * g;
    int row[4] = {0, 0, 0, 0};
    if constexpr (KIND == NP_RGB) {
#pragma unroll
      for (int m = 0; m < 4; m++) row[m] = (int)((phase + (uint32_t)m) % 3u);
    } else if constexpr (KIND == NP_MOSAIC) {
      // a mosaic has fewer than 2^32 sites and an even width: sites e0, e0 + 1 share a row, and so do e0 + 2, e0 + 3
      const uint32_t e = (uint32_t)e0, i = e / width, j = e - i * width;
      const uint32_t i2 = j + 2u >= width ? i + 1u : i;
#pragma unroll
      for (int m = 0; m < 4; m++) row[m] = (int)((pattern >> (2u * (2u * ((m < 2 ? i : i2) & 1u) + (uint32_t)(m & 1)))) & 3u);
    }
    float x[4];
    const bool whole = e0 + 4 <= count;
    if (whole && vectors) s4_io<TS>::load(src, (size_t)g, x);
    else {
#pragma unroll
      for (int m = 0; m < 4; m++) x[m] = e0 + m < count ? ld<TS>(src, (size_t)(e0 + m)) : 0.0f;
    }
    float y[4];
#pragma unroll
    for (int m = 0; m < 4; m++) {
      y[m] = np_value<FORWARD>(x[m], KIND == NP_ONE ? r0 : np_pick(row[m], r0, r1, r2), s, inverse);
    }
    if (whole && vectors) s4_io<TD>::store(dst, (size_t)g, y);
    else {
#pragma unroll
      for (int m = 0; m < 4; m++)
        if (e0 + m < count) st<TD>(dst, (size_t)(e0 + m), y[m]);
    }
  }
}

bool np_bins_ok(int bins) { return bins >= 2 && bins <= TDK_NOISE_MAX_BINS; }
size_t np_dtype_bytes(int dtype) { return dtype == TDK_F32 ? 4 : 2; }
size_t np_rec_bytes(int bins) { return (size_t)3 * bins * NP_LEVELS * 4 + (size_t)(3 * bins + NP_COUNTERS) * 8; }

template <typename TS, typename TD, bool FORWARD>
int launch_vst(const char* what, const void* src, void* dst, int64_t count, int width, int channels, uint32_t pattern, const float* model, const float* gains, float s,
               int inverse, hipStream_t st) {
  const TS* from = reinterpret_cast<const TS*>(src);
  TD* to = reinterpret_cast<TD*>(dst);
  const int vectors = tdk_aligned(src, 4 * sizeof(TS)) && tdk_aligned(dst, 4 * sizeof(TD)) ? 1 : 0;
  const int64_t groups = (count + 3) / 4;
  const int64_t want = tdk_div_up64(groups, NP_VST_THREADS);
  const dim3 grid((unsigned)(want < NP_VST_GRID ? want : NP_VST_GRID)), block(NP_VST_THREADS);
  if (pattern) TDK_LAUNCH(what, (np_vst<TS, TD, NP_MOSAIC, FORWARD>), grid, block, 0, st, from, to, count, (uint32_t)width, pattern, model, gains, s, inverse, vectors);
  else if (channels == 3) TDK_LAUNCH(what, (np_vst<TS, TD, NP_RGB, FORWARD>), grid, block, 0, st, from, to, count, (uint32_t)width, pattern, model, gains, s, inverse, vectors);
  else TDK_LAUNCH(what, (np_vst<TS, TD, NP_ONE, FORWARD>), grid, block, 0, st, from, to, count, (uint32_t)width, pattern, model, gains, s, inverse, vectors);
  return TDK_OK;
}

template <bool FORWARD>
int np_transform(const char* who, const void* src, int src_dtype, void* dst, int dst_dtype, int64_t count, int width, int channels, uint32_t pattern,
                 const float* model, const float* gains, float sigma_out, int inverse, tdk_stream_t stream) {
  TDK_REQUIRE(src && dst && model, "%s: null pointer (src, dst or model)", who);
  TDK_REQUIRE((src_dtype == TDK_F32 || src_dtype == TDK_F16) && (dst_dtype == TDK_F32 || dst_dtype == TDK_F16), "%s: unsupported dtype tags %d -> %d", who,
              src_dtype, dst_dtype);
  TDK_REQUIRE(count >= 1, "%s: count must be >= 1, got %lld", who, (long long)count);
  TDK_REQUIRE(channels == 1 || channels == 3, "%s: channels must be 1 or 3, got %d", who, channels);
  if (pattern != 0u) {
    TDK_REQUIRE(tdk_pattern_ok(pattern), "%s: unknown Bayer pattern 0x%08x", who, pattern);
    TDK_REQUIRE(channels == 1, "%s: a mosaic has channels = 1, got %d", who, channels);
    TDK_REQUIRE(width >= 2 && width <= TDK_MOSAIC_MAX_SIZE && width % 2 == 0, "%s: mosaic width must be even, 2..%d, got %d", who, TDK_MOSAIC_MAX_SIZE, width);
    TDK_REQUIRE(count % width == 0 && count / width <= TDK_MOSAIC_MAX_SIZE && (count / width) % 2 == 0, "%s: a mosaic of width %d holds an even number of rows, at most %d; count is %lld",
                who, width, TDK_MOSAIC_MAX_SIZE, (long long)count);
  } else {
    TDK_REQUIRE(count % channels == 0, "%s: count %lld is no multiple of channels = %d", who, (long long)count, channels);
  }
  TDK_REQUIRE(isfinite(sigma_out) && sigma_out > 0.0f, "%s: sigma_out must be finite and > 0", who);
  TDK_REQUIRE(inverse == TDK_NOISE_ALGEBRAIC || inverse == TDK_NOISE_UNBIASED, "%s: unknown inverse %d", who, inverse);
  const size_t src_bytes = (size_t)count * np_dtype_bytes(src_dtype), dst_bytes = (size_t)count * np_dtype_bytes(dst_dtype);
  TDK_REQUIRE(tdk_disjoint(src, src_bytes, dst, dst_bytes), "%s: src and dst overlap", who);
  TDK_REQUIRE(tdk_disjoint(model, 48, dst, dst_bytes) && (!gains || tdk_disjoint(gains, 12, dst, dst_bytes)), "%s: the model or the gains overlap dst", who);
  hipStream_t st = tdk_stream(stream);
  if (src_dtype == TDK_F32)
    return dst_dtype == TDK_F32 ? launch_vst<float, float, FORWARD>(who, src, dst, count, width, channels, pattern, model, gains, sigma_out, inverse, st)
                                : launch_vst<float, __half, FORWARD>(who, src, dst, count, width, channels, pattern, model, gains, sigma_out, inverse, st);
  return dst_dtype == TDK_F32 ? launch_vst<__half, float, FORWARD>(who, src, dst, count, width, channels, pattern, model, gains, sigma_out, inverse, st)
                              : launch_vst<__half, __half, FORWARD>(who, src, dst, count, width, channels, pattern, model, gains, sigma_out, inverse, st);
}

}  // namespace

TDK_EXPORT int tdk_noise_abi_version(void) { return TDK_NOISE_ABI_VERSION; }

TDK_EXPORT size_t tdk_noise_workspace_bytes(int bins) { return np_bins_ok(bins) ? (size_t)NP_GRID * np_rec_bytes(bins) + NP_WS_ALIGN : 0; }

TDK_EXPORT size_t tdk_noise_lds_bytes(int bins) { return np_bins_ok(bins) ? sizeof(NpLds) : 0; }

TDK_EXPORT int tdk_noise_profile(const void* const* frames, int num_frames, int dtype, void* workspace, int width, int height, uint32_t pattern, int bins, float white,
                                 int clip_lo, int clip_hi, int min_count, long long* counts, float* model, float* curve, tdk_stream_t stream) {
  static const char* const who = "tdk_noise_profile";
  TDK_REQUIRE(frames && workspace && counts && model && curve, "%s: null pointer (frames, workspace, counts, model or curve)", who);
  TDK_REQUIRE(num_frames >= 1 && num_frames <= TDK_NOISE_MAX_FRAMES, "%s: num_frames must be 1..%d, got %d", who, TDK_NOISE_MAX_FRAMES, num_frames);
  for (int f = 0; f < num_frames; f++) TDK_REQUIRE(frames[f], "%s: null pointer (frames[%d])", who, f);
  TDK_REQUIRE(dtype == TDK_F32 || dtype == TDK_F16 || dtype == TDK_U16, "%s: unsupported dtype tag %d", who, dtype);
  TDK_REQUIRE(tdk_mosaic_size_ok(width, height), "%s: frame size %dx%d outside 2..%d", who, width, height, TDK_MOSAIC_MAX_SIZE);
  TDK_REQUIRE(width % 2 == 0 && height % 2 == 0, "%s: mosaic size %dx%d must be even in both axes (whole CFA cells)", who, width, height);
  TDK_REQUIRE(tdk_pattern_ok(pattern), "%s: unknown Bayer pattern 0x%08x", who, pattern);
  TDK_REQUIRE(np_bins_ok(bins), "%s: bins must be 2..%d, got %d", who, TDK_NOISE_MAX_BINS, bins);
  const float scale = 65535.0f / white;
  TDK_REQUIRE(isfinite(white) && white > 0.0f && isfinite(scale), "%s: white must be finite and > 0 with a finite 65535 / white", who);
  TDK_REQUIRE(clip_lo >= 0 && clip_lo <= clip_hi && clip_hi <= 65535, "%s: the clip limits need 0 <= clip_lo <= clip_hi <= 65535, got %d, %d", who, clip_lo, clip_hi);
  TDK_REQUIRE(min_count >= 1, "%s: min_count must be >= 1, got %d", who, min_count);
  TDK_REQUIRE(tdk_aligned(counts, 8), "%s: counts must be aligned to 8 bytes", who);
  const size_t frame_bytes = (size_t)width * height * np_dtype_bytes(dtype);
  const size_t ws_bytes = tdk_noise_workspace_bytes(bins);
  const size_t counts_bytes = (size_t)(3 * bins * NP_LEVELS + 3 * bins + NP_COUNTERS) * 8, model_bytes = 48, curve_bytes = (size_t)6 * bins * 4;
  for (int f = 0; f < num_frames; f++)
    TDK_REQUIRE(tdk_disjoint(frames[f], frame_bytes, workspace, ws_bytes) && tdk_disjoint(frames[f], frame_bytes, counts, counts_bytes) &&
                    tdk_disjoint(frames[f], frame_bytes, model, model_bytes) && tdk_disjoint(frames[f], frame_bytes, curve, curve_bytes),
                "%s: frames[%d] overlaps the workspace, counts, model or curve", who, f);
  TDK_REQUIRE(tdk_disjoint(workspace, ws_bytes, counts, counts_bytes) && tdk_disjoint(workspace, ws_bytes, model, model_bytes) &&
                  tdk_disjoint(workspace, ws_bytes, curve, curve_bytes) && tdk_disjoint(counts, counts_bytes, model, model_bytes) &&
                  tdk_disjoint(counts, counts_bytes, curve, curve_bytes) && tdk_disjoint(model, model_bytes, curve, curve_bytes),
              "%s: the workspace, counts, model and curve overlap", who);

  NpArgs a{};
  for (int f = 0; f < num_frames; f++) a.frames[f] = frames[f];
  a.w = width, a.tiles_x = width / 16, a.tiles_y = height / 16;
  const int tiles_per_unit = 2 * (16 / (int)np_dtype_bytes(dtype));
  a.units_per_row = tdk_div_up(a.tiles_x, tiles_per_unit);
  a.units_per_frame = a.units_per_row * a.tiles_y;   // at most 512 * 4095
  a.units = a.units_per_frame * num_frames;          // ... and 16 times that
  a.bins = bins, a.clip_lo = clip_lo, a.clip_hi = clip_hi, a.scale = scale, a.pattern = pattern;
  unsigned char* records = reinterpret_cast<unsigned char*>(tdk_align_up(reinterpret_cast<uintptr_t>(workspace), NP_WS_ALIGN));
  hipStream_t st = tdk_stream(stream);
  if (dtype == TDK_F32) TDK_LAUNCH("tdk_noise_profile(gather)", np_gather<float>, dim3(NP_GRID), dim3(NP_THREADS), 0, st, a, records);
  else if (dtype == TDK_F16) TDK_LAUNCH("tdk_noise_profile(gather)", np_gather<__half>, dim3(NP_GRID), dim3(NP_THREADS), 0, st, a, records);
  else TDK_LAUNCH("tdk_noise_profile(gather)", np_gather<uint16_t>, dim3(NP_GRID), dim3(NP_THREADS), 0, st, a, records);
  const int outputs = 3 * bins * NP_LEVELS + 3 * bins + NP_COUNTERS;
  TDK_LAUNCH("tdk_noise_profile(reduce)", np_reduce, dim3((unsigned)tdk_div_up(outputs, NP_RED_IDX)), dim3(NP_THREADS), 0, st, records, NP_GRID, bins, counts);
  NpDerive d{};
  d.bins = bins, d.min_count = min_count, d.white = white;
  TDK_LAUNCH("tdk_noise_profile(derive)", np_derive, dim3(1), dim3(NP_DER_THREADS), 0, st, counts, model, curve, d);
  return TDK_OK;
}

TDK_EXPORT int tdk_noise_stabilize(const void* src, int src_dtype, void* dst, int dst_dtype, int64_t count, int width, int channels, uint32_t pattern,
                                   const float* model, const float* gains, float sigma_out, tdk_stream_t stream) {
  return np_transform<true>("tdk_noise_stabilize", src, src_dtype, dst, dst_dtype, count, width, channels, pattern, model, gains, sigma_out, TDK_NOISE_UNBIASED, stream);
}

TDK_EXPORT int tdk_noise_unstabilize(const void* src, int src_dtype, void* dst, int dst_dtype, int64_t count, int width, int channels, uint32_t pattern,
                                     const float* model, const float* gains, float sigma_out, int inverse, tdk_stream_t stream) {
  return np_transform<false>("tdk_noise_unstabilize", src, src_dtype, dst, dst_dtype, count, width, channels, pattern, model, gains, sigma_out, inverse, stream);
}
