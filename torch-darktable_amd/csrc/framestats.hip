// framestats.hip -- per-channel histograms, percentiles, means and grey-world gains of a set of frames (include/tdk_hip_stats.h:
// tdk_framestats): one gather launch per frame and two small finishing launches.
//
// The specification is the head comment of include/tdk_hip_stats.h.
//
// Gather, fs_gather<T, KIND>: FS_GRID = 512 workgroups of 512 lanes whatever the frame size (two per compute unit).  The work is cut
// into UNITS of 16 pixels of one sampled row (image) or 16 columns of one sampled row pair, eight CFA cells (mosaic); the units of
// all sampled rows are numbered row by row and walked grid-stride.  Rows that the stride leaves out are never read.  A unit inside
// its row is read as 16-byte vectors when it starts on a 16-byte boundary and per element otherwise: every row gets a `head` (0..15
// pixels in front of the first whole unit, derived from the row's address) so that the units of a row are aligned whenever the
// element alignment of the row allows it; the head and the end of a row are the two partial units, read per element.  Nothing is
// read outside [row, row + width).
// A lane counts into LDS with integer atomics.  The histograms are replicated: `copies` (a power of two, at most 16, as many as fit
// FS_HIST_WORDS) copies of channels x bins words, a lane counts into copy (lane & (copies - 1)), and the copies start a multiple of
// 32 words plus one apart -- a flat frame (every lane on one bin) spreads over `copies` banks instead of serialising on one address.
// below / above / nan / valid / sum are per-lane registers, summed over the wave by shuffles and over the workgroup by 64-bit LDS
// atomics, one per wave and counter.  At the end every workgroup writes its record -- the bins summed over the copies, then the
// counters -- to its place in the frame's slot of the workspace, also when it had no unit to look at.
// Finish 1, fs_reduce: sums the records of the used slots into `counts` (integer adds; sixteen lanes share a counter's records).
// Finish 2, fs_derive: one workgroup; a block scan of each histogram (the channels, then their sum) gives the percentiles, lane 0
// forms the means and gains in double.
// No location is accumulated into by more than one workgroup and all sums are integers: the bits do not depend on scheduling.
#include <math.h>

#include "../../include/tdk_hip_stats.h"
#include "tdk_frame.h"

namespace {

constexpr int FS_THREADS = 512, FS_WAVES = FS_THREADS / 64;
constexpr int FS_GRID = TDK_STATS_GRID;
constexpr int FS_UNIT = 16;                                 // pixels (columns of a mosaic) of a lane per step
constexpr int FS_MAX_COPIES = 16;
constexpr int FS_HIST_WORDS = FS_MAX_COPIES * (3 * 256 + 1);  // 16 copies of 3 x 256 bins, 4 of 3 x 1024
constexpr int FS_COUNTERS = 5;                              // below, above, nan, valid, sum: the order in a record and in `counts`
constexpr int FS_RED_IDX = 32, FS_RED_LANES = FS_THREADS / FS_RED_IDX;   // fs_reduce: counters of a workgroup, lanes per counter
constexpr int FS_DER_THREADS = 256, FS_DER_BINS = TDK_STATS_MAX_BINS / FS_DER_THREADS;
constexpr size_t FS_WS_ALIGN = 8;
static_assert(FS_THREADS * FS_UNIT == TDK_STATS_CHUNK, "the chunk the header states");
static_assert(4 * (3 * TDK_STATS_MAX_BINS + 1) <= FS_HIST_WORDS, "four copies at the largest histogram");

enum { FS_IMAGE1 = 0, FS_IMAGE3 = 1, FS_MOSAIC = 2 };

struct FsLds {
  uint32_t hist[FS_HIST_WORDS];
  unsigned long long cnt[16];   // [which * 3 + k]
};
static_assert(sizeof(FsLds) <= 64 * 1024, "LDS of the gather launch");

struct FsArgs {
  int w, h, stride, bins;
  int rows, units_per_row;      // sampled rows (row pairs of a mosaic); units of one of them, the two partial ones included
  int64_t units;
  float lo, hi, scale, top, fbins;   // top = (float)(B - 1), fbins = (float)B
  uint32_t pattern;
  int copies, copy_stride;      // words
  int rec_words;                // channels * bins, padded to an even count
};

struct FsDerive {
  int channels, bins, nq, min_count;
  float lo, range;
  float q[TDK_STATS_MAX_QUANTILES];
};

// ---- storage
__device__ __forceinline__ float fs_cvt(float v) { return v; }
__device__ __forceinline__ float fs_cvt(__half v) { return __half2float(v); }
__device__ __forceinline__ float fs_cvt(uint8_t v) { return (float)v; }
__device__ __forceinline__ float fs_cvt(uint16_t v) { return (float)v; }

template <typename T> __device__ __forceinline__ float fs_unpack(const uint32_t w[4], int j);
template <> __device__ __forceinline__ float fs_unpack<float>(const uint32_t w[4], int j) { return __uint_as_float(w[j]); }
template <> __device__ __forceinline__ float fs_unpack<__half>(const uint32_t w[4], int j) {
  return __half2float(__ushort_as_half((unsigned short)((w[j / 2] >> (16 * (j % 2))) & 0xffffu)));
}
template <> __device__ __forceinline__ float fs_unpack<uint8_t>(const uint32_t w[4], int j) { return (float)((w[j / 4] >> (8 * (j % 4))) & 0xffu); }
template <> __device__ __forceinline__ float fs_unpack<uint16_t>(const uint32_t w[4], int j) { return (float)((w[j / 2] >> (16 * (j % 2))) & 0xffffu); }

// N consecutive elements at p: 16-byte vectors when p is on a 16-byte boundary, per element otherwise
template <typename T, int N> __device__ __forceinline__ void fs_load(const T* p, float* v) {
  constexpr int PER = 16 / (int)sizeof(T);
  static_assert(N % PER == 0, "whole vectors");
  if ((reinterpret_cast<uintptr_t>(p) & 15u) == 0) {
    const uint4* q = reinterpret_cast<const uint4*>(p);
#pragma unroll
    for (int k = 0; k < N / PER; k++) {
      const uint4 u = q[k];
      const uint32_t w[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
      for (int j = 0; j < PER; j++) v[k * PER + j] = fs_unpack<T>(w, j);
    }
  } else {
#pragma unroll
    for (int i = 0; i < N; i++) v[i] = fs_cvt(p[i]);
  }
}

// pixels in front of the first whole unit of the row at `row`, so that (row + head * C) is on a 16-byte boundary; C = 1 or 3
template <typename T, int C> __device__ __forceinline__ int fs_head(const T* row) {
  constexpr int M = 16 / (int)sizeof(T);                      // elements per vector: 4, 8 or 16
  constexpr int INV = C == 1 ? 1 : (M == 16 ? 11 : 3);        // the inverse of C modulo M
  const int u = (int)((reinterpret_cast<uintptr_t>(row) / sizeof(T)) % M);
  return ((M - u) % M * INV) % M;
}

// ---- a lane's counters: per MEMBER of a group (the channel of an image, the CFA position of a mosaic)
template <int M> struct FsAcc {
  uint32_t below[M], above[M], nan[M];
  long long sum[M];
  uint32_t valid;
};

// one group: its M members x[0..M), member m counting into the histogram at hist + off[m]
template <int M> __device__ __forceinline__ void fs_group(const float* x, uint32_t* hist, const int* off, const FsArgs& a, FsAcc<M>& acc) {
  bool ok = true;
  int q[M];
#pragma unroll
  for (int m = 0; m < M; m++) {
    const float v = x[m];
    q[m] = 0;
    if (v != v) {
      acc.nan[m] += 1u;
      ok = false;
    } else {
      const float t = (v - a.lo) * a.scale;
      const int b = (int)fminf(fmaxf(floorf(t), 0.0f), a.top);
      atomicAdd(hist + off[m] + b, 1u);
      acc.below[m] += v < a.lo ? 1u : 0u;
      acc.above[m] += v >= a.hi ? 1u : 0u;
      ok = ok && v >= a.lo && v < a.hi;
      q[m] = (int)rintf(fminf(fmaxf(t, 0.0f), a.fbins) * 1048576.0f);   // at most 2^30
    }
  }
  if (ok) {
    acc.valid += 1u;
#pragma unroll
    for (int m = 0; m < M; m++) acc.sum[m] += (long long)q[m];
  }
}

__device__ __forceinline__ unsigned long long fs_wave_sum(unsigned long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

template <typename T, int KIND>
__global__ __launch_bounds__(FS_THREADS) void fs_gather(const T* __restrict__ src, unsigned char* __restrict__ slot, FsArgs a) {
  constexpr bool MOSAIC = KIND == FS_MOSAIC;
  constexpr int C = KIND == FS_IMAGE1 ? 1 : 3;     // channels of the result
  constexpr int E = MOSAIC ? 1 : C;                // elements of a pixel in memory
  constexpr int M = MOSAIC ? 4 : C;                // members of a group
  __shared__ FsLds lds;
  const int tid = threadIdx.x;
  for (int i = tid; i < a.copies * a.copy_stride; i += FS_THREADS) lds.hist[i] = 0u;
  if (tid < 16) lds.cnt[tid] = 0ull;
  __syncthreads();

  uint32_t* hist = lds.hist + (tid & (a.copies - 1)) * a.copy_stride;
  int chan[M], off[M];
#pragma unroll
  for (int m = 0; m < M; m++) {
    chan[m] = MOSAIC ? (int)((a.pattern >> (2 * m)) & 3u) : m;
    off[m] = chan[m] * a.bins;
  }
  FsAcc<M> acc;
#pragma unroll
  for (int m = 0; m < M; m++) acc.below[m] = 0u, acc.above[m] = 0u, acc.nan[m] = 0u, acc.sum[m] = 0;
  acc.valid = 0u;

  const int s = a.stride;
  const int64_t step = (int64_t)FS_GRID * FS_THREADS;
  for (int64_t unit = (int64_t)blockIdx.x * FS_THREADS + tid; unit < a.units; unit += step) {
    const int r = (int)unit / a.units_per_row, k = (int)unit - r * a.units_per_row;   // (units < 2^31: 65535 rows of 4097 units at most)
    if constexpr (!MOSAIC) {
      const T* row = src + (size_t)r * s * a.w * E;
      const int p0 = fs_head<T, C>(row) + FS_UNIT * (k - 1), p1 = p0 + FS_UNIT;   // the unit's pixels: [p0, p1) inside [0, w)
      const int from = p0 < 0 ? 0 : p0, to = p1 > a.w ? a.w : p1;
      int next = (from + s - 1) / s * s;                                          // the first sampled pixel of the unit
      if (next >= to) continue;
      if (p0 >= 0 && p1 <= a.w) {
        float v[FS_UNIT * E];
        fs_load<T, FS_UNIT * E>(row + (size_t)p0 * E, v);
#pragma unroll
        for (int px = 0; px < FS_UNIT; px++)
          if (p0 + px == next) {
            fs_group<M>(v + px * E, hist, off, a, acc);
            next += s;
          }
      } else {
        for (int px = next; px < to; px += s) {
          float x[M];
#pragma unroll
          for (int m = 0; m < M; m++) x[m] = fs_cvt(row[(size_t)px * E + m]);
          fs_group<M>(x, hist, off, a, acc);
        }
      }
    } else {
      const T* row0 = src + (size_t)2 * r * s * a.w;   // the row pair of cell row r * s
      const T* row1 = row0 + a.w;
      int head = fs_head<T, 1>(row0);
      if (head & 1) head = 0;                          // units hold whole cells: a row on an odd element is read per element
      const int p0 = head + FS_UNIT * (k - 1), p1 = p0 + FS_UNIT;
      const int from = p0 < 0 ? 0 : p0, to = p1 > a.w ? a.w : p1;   // columns, all even
      int next = ((from >> 1) + s - 1) / s * s;                     // the first sampled cell column of the unit
      if (2 * next >= to) continue;
      if (p0 >= 0 && p1 <= a.w) {
        float v0[FS_UNIT], v1[FS_UNIT];
        fs_load<T, FS_UNIT>(row0 + p0, v0);
        fs_load<T, FS_UNIT>(row1 + p0, v1);
#pragma unroll
        for (int c = 0; c < FS_UNIT / 2; c++)
          if ((p0 >> 1) + c == next) {
            const float x[4] = {v0[2 * c], v0[2 * c + 1], v1[2 * c], v1[2 * c + 1]};
            fs_group<4>(x, hist, off, a, acc);
            next += s;
          }
      } else {
        for (int cj = next; 2 * cj < to; cj += s) {
          const float x[4] = {fs_cvt(row0[2 * cj]), fs_cvt(row0[2 * cj + 1]), fs_cvt(row1[2 * cj]), fs_cvt(row1[2 * cj + 1])};
          fs_group<4>(x, hist, off, a, acc);
        }
      }
    }
  }

  // ---- the counters: over the wave by shuffles, over the workgroup (and from members to channels) by one LDS atomic per wave
#pragma unroll
  for (int m = 0; m < M; m++) {
    const unsigned long long part[FS_COUNTERS] = {fs_wave_sum(acc.below[m]), fs_wave_sum(acc.above[m]), fs_wave_sum(acc.nan[m]), fs_wave_sum(acc.valid),
                                                  fs_wave_sum((unsigned long long)acc.sum[m])};
    if (tid % 64 == 0) {
#pragma unroll
      for (int which = 0; which < FS_COUNTERS; which++) atomicAdd(&lds.cnt[which * 3 + chan[m]], part[which]);
    }
  }
  __syncthreads();

  // ---- the record: bins summed over the copies, then the counters as [which][channel]
  unsigned char* rec = slot + (size_t)blockIdx.x * ((size_t)a.rec_words * 4 + (size_t)FS_COUNTERS * C * 8);
  uint32_t* rec_hist = reinterpret_cast<uint32_t*>(rec);
  for (int i = tid; i < C * a.bins; i += FS_THREADS) {
    uint32_t n = 0u;
    for (int c = 0; c < a.copies; c++) n += lds.hist[c * a.copy_stride + i];
    rec_hist[i] = n;
  }
  if (tid < FS_COUNTERS * C) reinterpret_cast<unsigned long long*>(rec + (size_t)a.rec_words * 4)[tid] = lds.cnt[(tid / C) * 3 + tid % C];
}

// counts[k * (B + 5) + b] and counts[k * (B + 5) + B + which] from `records` records
__global__ __launch_bounds__(FS_THREADS) void fs_reduce(const unsigned char* __restrict__ records, int nrec, int channels, int bins, int rec_words,
                                                        long long* __restrict__ counts) {
  __shared__ long long part[FS_RED_LANES][FS_RED_IDX];
  const int tid = threadIdx.x, idx = tid % FS_RED_IDX, lane = tid / FS_RED_IDX;
  const int cb = channels * bins, outputs = cb + FS_COUNTERS * channels;
  const int o = (int)blockIdx.x * FS_RED_IDX + idx;
  const size_t rec_bytes = (size_t)rec_words * 4 + (size_t)FS_COUNTERS * channels * 8;
  long long acc = 0;
  if (o < outputs) {
    for (int r = lane; r < nrec; r += FS_RED_LANES) {
      const unsigned char* rec = records + (size_t)r * rec_bytes;
      acc += o < cb ? (long long)reinterpret_cast<const uint32_t*>(rec)[o] : reinterpret_cast<const long long*>(rec + (size_t)rec_words * 4)[o - cb];
    }
  }
  part[lane][idx] = acc;
  __syncthreads();
  if (tid < FS_RED_IDX && o < outputs) {
    long long total = 0;
#pragma unroll
    for (int l = 0; l < FS_RED_LANES; l++) total += part[l][tid];
    const int k = o < cb ? o / bins : (o - cb) % channels;
    const int at = o < cb ? o - k * bins : bins + (o - cb) / channels;
    counts[(size_t)k * (bins + FS_COUNTERS) + at] = total;
  }
}

// values: mean[C], percentile[C + 1][Q], gain[3]
__global__ __launch_bounds__(FS_DER_THREADS) void fs_derive(const long long* __restrict__ counts, float* __restrict__ values, FsDerive d) {
  __shared__ unsigned long long scan[FS_DER_THREADS];
  const int tid = threadIdx.x, C = d.channels, B = d.bins, row_len = B + FS_COUNTERS;
  const double w = (double)d.range / (double)B;
  float* pct = values + C;
  for (int row = 0; row <= C; row++) {   // the channels, then the pooled histogram
    unsigned long long h[FS_DER_BINS], local = 0ull;
#pragma unroll
    for (int j = 0; j < FS_DER_BINS; j++) {
      const int b = FS_DER_BINS * tid + j;
      unsigned long long n = 0ull;
      if (b < B) {
        if (row < C) n = (unsigned long long)counts[(size_t)row * row_len + b];
        else
          for (int k = 0; k < C; k++) n += (unsigned long long)counts[(size_t)k * row_len + b];
      }
      h[j] = n, local += n;
    }
    scan[tid] = local;
    __syncthreads();
    for (int o = 1; o < FS_DER_THREADS; o <<= 1) {
      const unsigned long long up = tid >= o ? scan[tid - o] : 0ull;
      __syncthreads();
      scan[tid] += up;
      __syncthreads();
    }
    const unsigned long long total = scan[FS_DER_THREADS - 1], before = scan[tid] - local;
    for (int qi = 0; qi < d.nq; qi++) {
      if (total == 0ull) {
        if (tid == 0) pct[row * d.nq + qi] = d.lo;
        continue;
      }
      double rd = ceil((double)d.q[qi] * (double)total);
      rd = rd < 1.0 ? 1.0 : (rd > (double)total ? (double)total : rd);
      const unsigned long long r = (unsigned long long)rd;
      unsigned long long prev = before;
#pragma unroll
      for (int j = 0; j < FS_DER_BINS; j++) {
        const unsigned long long cum = prev + h[j];
        if (prev < r && cum >= r) {   // exactly one bin of one lane
          const double frac = (double)(r - prev) / (double)h[j];
          pct[row * d.nq + qi] = (float)((double)d.lo + ((double)(FS_DER_BINS * tid + j) + frac) * w);
        }
        prev = cum;
      }
    }
    __syncthreads();   // the next row scans over this one
  }
  if (tid == 0) {
    float mean[3] = {0.0f, 0.0f, 0.0f};
    bool grey = C == 3;
    for (int k = 0; k < C; k++) {
      const long long valid = counts[(size_t)k * row_len + B + 3], sum = counts[(size_t)k * row_len + B + 4];
      const bool enough = valid >= (long long)d.min_count;
      mean[k] = enough ? (float)((double)d.lo + ((double)sum / ((double)valid * 1048576.0)) * w) : 0.0f;
      values[k] = mean[k];
      grey = grey && enough && mean[k] > 0.0f;
    }
    float* gain = pct + (C + 1) * d.nq;
    for (int k = 0; k < 3; k++) gain[k] = grey ? fminf(fmaxf(mean[1] / mean[k], 1.0f / 64.0f), 64.0f) : 1.0f;
  }
}

bool fs_shape_ok(int bins, int channels) { return bins >= 2 && bins <= TDK_STATS_MAX_BINS && (channels == 1 || channels == 3); }
size_t fs_dtype_bytes(int dtype) { return dtype == TDK_F32 ? 4 : (dtype == TDK_F16 || dtype == TDK_U16) ? 2 : 1; }

int fs_rec_words(int bins, int channels) { return (channels * bins + 1) / 2 * 2; }
size_t fs_rec_bytes(int bins, int channels) { return (size_t)fs_rec_words(bins, channels) * 4 + (size_t)FS_COUNTERS * channels * 8; }
size_t fs_slot_bytes(int bins, int channels) { return (size_t)FS_GRID * fs_rec_bytes(bins, channels); }
// the copies start a multiple of 32 words plus one apart: the same bin of two copies never shares a bank
int fs_copy_stride(int bins, int channels) { return (channels * bins + 31) / 32 * 32 + 1; }
int fs_copies(int bins, int channels) {
  int copies = 1;
  while (copies < FS_MAX_COPIES && 2 * copies * fs_copy_stride(bins, channels) <= FS_HIST_WORDS) copies *= 2;
  return copies;
}

template <typename T> int launch_gather(const void* src, unsigned char* slot, int kind, const FsArgs& a, hipStream_t st) {
  const T* s = reinterpret_cast<const T*>(src);
  if (kind == FS_IMAGE1) TDK_LAUNCH("tdk_framestats(gather)", (fs_gather<T, FS_IMAGE1>), dim3(FS_GRID), dim3(FS_THREADS), 0, st, s, slot, a);
  else if (kind == FS_IMAGE3) TDK_LAUNCH("tdk_framestats(gather)", (fs_gather<T, FS_IMAGE3>), dim3(FS_GRID), dim3(FS_THREADS), 0, st, s, slot, a);
  else TDK_LAUNCH("tdk_framestats(gather)", (fs_gather<T, FS_MOSAIC>), dim3(FS_GRID), dim3(FS_THREADS), 0, st, s, slot, a);
  return TDK_OK;
}

}  // namespace

TDK_EXPORT int tdk_framestats_abi_version(void) { return TDK_STATS_ABI_VERSION; }

TDK_EXPORT size_t tdk_framestats_workspace_bytes(int bins, int channels, int max_frames) {
  if (!fs_shape_ok(bins, channels) || max_frames < 1 || max_frames > TDK_STATS_MAX_FRAMES) return 0;
  return (size_t)max_frames * fs_slot_bytes(bins, channels) + FS_WS_ALIGN;
}

TDK_EXPORT size_t tdk_framestats_lds_bytes(int bins, int channels) { return fs_shape_ok(bins, channels) ? sizeof(FsLds) : 0; }

TDK_EXPORT int tdk_framestats(const void* const* frames, int num_frames, int dtype, void* workspace, int width, int height, int channels, uint32_t pattern,
                              int stride, int bins, float lo, float hi, int min_count, const float* quantiles, int num_quantiles, long long* counts,
                              float* values, tdk_stream_t stream) {
  static const char* const who = "tdk_framestats";
  TDK_REQUIRE(frames && workspace && counts && values, "%s: null pointer (frames, workspace, counts or values)", who);
  TDK_REQUIRE(num_frames >= 1 && num_frames <= TDK_STATS_MAX_FRAMES, "%s: num_frames must be 1..%d, got %d", who, TDK_STATS_MAX_FRAMES, num_frames);
  for (int f = 0; f < num_frames; f++) TDK_REQUIRE(frames[f], "%s: null pointer (frames[%d])", who, f);
  TDK_REQUIRE(dtype == TDK_F32 || dtype == TDK_F16 || dtype == TDK_U8 || dtype == TDK_U16, "%s: unsupported dtype tag %d", who, dtype);
  TDK_REQUIRE(tdk_frame_size_ok(width, height), "%s: frame size %dx%d outside 1..%d", who, width, height, TDK_FRAME_MAX_SIZE);
  TDK_REQUIRE(channels == 1 || channels == 3, "%s: channels must be 1 or 3, got %d", who, channels);
  if (pattern != 0u) {
    TDK_REQUIRE(tdk_pattern_ok(pattern), "%s: unknown Bayer pattern 0x%08x", who, pattern);
    TDK_REQUIRE(channels == 3, "%s: a mosaic has channels = 3 (R, G, B), got %d", who, channels);
    TDK_REQUIRE(width % 2 == 0 && height % 2 == 0, "%s: mosaic size %dx%d must be even in both axes (whole CFA cells)", who, width, height);
  }
  TDK_REQUIRE(stride >= 1 && stride <= TDK_FRAME_MAX_SIZE, "%s: stride must be 1..%d, got %d", who, TDK_FRAME_MAX_SIZE, stride);
  TDK_REQUIRE(bins >= 2 && bins <= TDK_STATS_MAX_BINS, "%s: bins must be 2..%d, got %d", who, TDK_STATS_MAX_BINS, bins);
  const float range = hi - lo, scale = (float)bins / range;
  TDK_REQUIRE(isfinite(lo) && isfinite(hi) && lo < hi && isfinite(range) && isfinite(scale), "%s: the range needs finite lo < hi with a finite bins / (hi - lo)", who);
  TDK_REQUIRE(min_count >= 1, "%s: min_count must be >= 1, got %d", who, min_count);
  TDK_REQUIRE(num_quantiles >= 0 && num_quantiles <= TDK_STATS_MAX_QUANTILES, "%s: num_quantiles must be 0..%d, got %d", who, TDK_STATS_MAX_QUANTILES, num_quantiles);
  TDK_REQUIRE(num_quantiles == 0 || quantiles, "%s: null pointer (quantiles)", who);
  for (int i = 0; i < num_quantiles; i++) TDK_REQUIRE(quantiles[i] >= 0.0f && quantiles[i] <= 1.0f, "%s: quantiles[%d] must lie in [0, 1]", who, i);
  TDK_REQUIRE(tdk_aligned(counts, 8), "%s: counts must be aligned to 8 bytes", who);
  const size_t frame_bytes = (size_t)width * height * (pattern ? 1 : channels) * fs_dtype_bytes(dtype);
  const size_t ws_bytes = tdk_framestats_workspace_bytes(bins, channels, num_frames);
  const size_t counts_bytes = (size_t)channels * (bins + FS_COUNTERS) * 8, values_bytes = (size_t)(channels + (channels + 1) * num_quantiles + 3) * 4;
  for (int f = 0; f < num_frames; f++)
    TDK_REQUIRE(tdk_disjoint(frames[f], frame_bytes, workspace, ws_bytes) && tdk_disjoint(frames[f], frame_bytes, counts, counts_bytes) &&
                    tdk_disjoint(frames[f], frame_bytes, values, values_bytes),
                "%s: frames[%d] overlaps the workspace, counts or values", who, f);
  TDK_REQUIRE(tdk_disjoint(workspace, ws_bytes, counts, counts_bytes) && tdk_disjoint(workspace, ws_bytes, values, values_bytes) &&
                  tdk_disjoint(counts, counts_bytes, values, values_bytes),
              "%s: the workspace, counts and values overlap", who);

  FsArgs a{};
  a.w = width, a.h = height, a.stride = stride, a.bins = bins;
  a.rows = tdk_div_up(pattern ? height / 2 : height, stride);
  a.units_per_row = tdk_div_up(width, FS_UNIT) + 1;
  a.units = (int64_t)a.rows * a.units_per_row;
  a.lo = lo, a.hi = hi, a.scale = scale, a.top = (float)(bins - 1), a.fbins = (float)bins;
  a.pattern = pattern;
  a.copies = fs_copies(bins, channels), a.copy_stride = fs_copy_stride(bins, channels);
  a.rec_words = fs_rec_words(bins, channels);
  const int kind = pattern ? FS_MOSAIC : channels == 1 ? FS_IMAGE1 : FS_IMAGE3;
  unsigned char* records = reinterpret_cast<unsigned char*>(tdk_align_up(reinterpret_cast<uintptr_t>(workspace), FS_WS_ALIGN));
  hipStream_t st = tdk_stream(stream);
  for (int f = 0; f < num_frames; f++) {
    unsigned char* slot = records + (size_t)f * fs_slot_bytes(bins, channels);
    const int rc = dtype == TDK_F32   ? launch_gather<float>(frames[f], slot, kind, a, st)
                   : dtype == TDK_F16 ? launch_gather<__half>(frames[f], slot, kind, a, st)
                   : dtype == TDK_U8  ? launch_gather<uint8_t>(frames[f], slot, kind, a, st)
                                      : launch_gather<uint16_t>(frames[f], slot, kind, a, st);
    if (rc != TDK_OK) return rc;
  }
  const int outputs = channels * (bins + FS_COUNTERS);
  TDK_LAUNCH("tdk_framestats(reduce)", fs_reduce, dim3((unsigned)tdk_div_up(outputs, FS_RED_IDX)), dim3(FS_THREADS), 0, st, records, num_frames * FS_GRID, channels,
             bins, a.rec_words, counts);
  FsDerive d{};
  d.channels = channels, d.bins = bins, d.nq = num_quantiles, d.min_count = min_count;
  d.lo = lo, d.range = range;
  for (int i = 0; i < num_quantiles; i++) d.q[i] = quantiles[i];
  TDK_LAUNCH("tdk_framestats(derive)", fs_derive, dim3(1), dim3(FS_DER_THREADS), 0, st, counts, values, d);
  return TDK_OK;
}
