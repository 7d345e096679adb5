// motion.hip -- block-matching motion estimation on raw mosaics and the motion-compensated temporal denoiser
// (include/tdk_hip_motion.h: tdk_motion_pyramid and tdk_motion_match, one launch each; tdk_motion_temporal_denoise: one tile launch
// and a one-lane launch that advances the frame index).
//
// The specification is the head comment of include/tdk_hip_motion.h.
//
// Pyramid, mo_pyramid<TS>: a workgroup of 256 lanes owns the 32 x 16 level-0 values of one tile of the temporal filter (64 x 32 sites).
// A lane turns two CFA cells into grey values, the tile goes to LDS, and level k + 1 is reduced from level k there: the tile's origin
// is a multiple of 8 values, so the 2 x 2 blocks of every level (and the clamp at the plane's last row and column) stay inside it.
// Match, mo_match: one wave per tile.  Per level the block (16 x 32 bytes) and the search window ((16 + 2R) x (32 + 2R) bytes, fetched
// with clamped coordinates, so the LDS copy answers ref[clamp(p + d)] for every candidate) are staged as dwords; a lane owns a
// candidate and walks the block four samples per v_sad_u8, the window dword shifted into place from two neighbours; the winner is the
// wave's minimum of the candidates' keys.
// Compensated filter, mc_filter<TS, TA, TO, R>: tp_filter of temporal.hip (256 lanes, 32 x 64 tile, eight sites per lane, two staged
// planes and two planes of row sums in LDS, the rolled column loop) with the history read at a per-workgroup uniform displacement:
// the element offset dy * w + dx on the two state reads and an in-frame test of the history site.  Whether a lane's group goes as
// 16-byte vectors or per element is decided by the shifted address, as tp_filter decides by the plain one.
#include <math.h>

#include "../../include/tdk_hip_motion.h"
#include "tdk_frame.h"

namespace {

constexpr int MO_MAX_SIZE = 65535;
constexpr int MO_BW = 32, MO_BH = 16;                 // the block of a tile at every level; the tile's level-0 values
constexpr int MO_THREADS = 256;                       // of the pyramid launch
constexpr int MO_WAVE = 64;                           // of the match launch
constexpr int MO_WIN_DWORDS = (MO_BW + 2 * TDK_MOTION_MAX_SEARCH) / 4 + 1;   // dwords of a staged window row: one more than the
                                                                             // widest window, for the shifted read of the last group
constexpr int MO_WIN_ROWS = MO_BH + 2 * TDK_MOTION_MAX_SEARCH;
static_assert(2 * MO_BW == TDK_MOTION_TILE_W && 2 * MO_BH == TDK_MOTION_TILE_H, "a tile is its level-0 block");
static_assert(TDK_MOTION_TILE_W == TDK_TEMPORAL_TILE_W && TDK_MOTION_TILE_H == TDK_TEMPORAL_TILE_H, "the tiles of the temporal filter");
static_assert(2 * ((TDK_MOTION_MAX_SEARCH + 1) * (1 << (TDK_MOTION_MAX_LEVELS - 1)) - 1) == TDK_MOTION_MAX_DISPLACEMENT, "the largest displacement");

struct MoGeometry {
  int w[TDK_MOTION_MAX_LEVELS], h[TDK_MOTION_MAX_LEVELS];
  size_t at[TDK_MOTION_MAX_LEVELS];   // byte offset of a level in its slot
  size_t slot;                        // bytes of a slot
};

MoGeometry mo_geometry(int width, int height, int levels) {
  MoGeometry g{};
  int w = width / 2, h = height / 2;
  for (int k = 0; k < levels; k++) {
    g.w[k] = w, g.h[k] = h, g.at[k] = g.slot;
    g.slot += tdk_align_up((size_t)w * (size_t)h, 16);
    w = (w + 1) / 2, h = (h + 1) / 2;
  }
  return g;
}

bool mo_dtype_ok(int dtype) { return dtype == TDK_F32 || dtype == TDK_F16; }
bool mo_size_ok(int width, int height) {
  return width >= 2 && height >= 2 && width <= MO_MAX_SIZE && height <= MO_MAX_SIZE && width % 2 == 0 && height % 2 == 0;
}
bool mo_levels_ok(int levels) { return levels >= 1 && levels <= TDK_MOTION_MAX_LEVELS; }

// ================================================================ pyramid
struct MoPyramidArgs {
  const void* src;
  unsigned char* pyramid;
  const uint32_t* index;
  int which, levels, w, h;   // w, h: sites
  float scale;
  MoGeometry g;
};

// four sites of a frame row from column j0 (a multiple of four): `live` of them are inside the frame, the others read as 0
template <typename T> __device__ __forceinline__ void mo_fetch4(const T* __restrict__ base, size_t at, int live, float x[4]) {
  if (live == 4 && (reinterpret_cast<uintptr_t>(base + at) & (4 * sizeof(T) - 1)) == 0) s4_io<T>::load(base + at, 0, x);
  else {
#pragma unroll
    for (int m = 0; m < 4; m++) x[m] = m < live ? ld<T>(base, at + m) : 0.0f;
  }
}

__device__ __forceinline__ uint32_t mo_grey(float x00, float x01, float x10, float x11, float scale) {
  const float q = (x00 + x01) + (x10 + x11);
  const float u = fminf(fmaxf(q * scale, 0.0f), 1.0f);
  return (uint32_t)(__fsqrt_rn(u) * 255.0f + 0.5f);
}

template <typename TS> __global__ __launch_bounds__(MO_THREADS) void mo_pyramid(MoPyramidArgs a) {
  // the tile at every level, one behind the other: 16 x 32, 8 x 16, 4 x 8, 2 x 4 values
  __shared__ unsigned char lds[MO_BH * MO_BW * 2];
  const int tid = threadIdx.x;
  const uint32_t slot = a.index ? ((*a.index + (uint32_t)a.which) & 1u) : (uint32_t)a.which;
  unsigned char* __restrict__ dst = a.pyramid + (size_t)slot * a.g.slot;
  const TS* __restrict__ src = reinterpret_cast<const TS*>(a.src);

  // ---- level 0: two cells of tile row r
  {
    const int r = tid / (MO_BW / 2), cp = tid % (MO_BW / 2);
    const int I = (int)blockIdx.y * MO_BH + r, J = (int)blockIdx.x * MO_BW + 2 * cp;
    const int cells = I < a.g.h[0] ? min(max(a.g.w[0] - J, 0), 2) : 0;
    uint32_t g[2] = {0u, 0u};
    if (cells > 0) {
      float top[4], bottom[4];
      const size_t at = (size_t)(2 * I) * (size_t)a.w + (size_t)(2 * J);
      mo_fetch4<TS>(src, at, 2 * cells, top);
      mo_fetch4<TS>(src, at + (size_t)a.w, 2 * cells, bottom);
      g[0] = mo_grey(top[0], top[1], bottom[0], bottom[1], a.scale);
      if (cells > 1) g[1] = mo_grey(top[2], top[3], bottom[2], bottom[3], a.scale);
#pragma unroll
      for (int m = 0; m < 2; m++)
        if (m < cells) dst[a.g.at[0] + (size_t)I * (size_t)a.g.w[0] + (size_t)(J + m)] = (unsigned char)g[m];
    }
    lds[r * MO_BW + 2 * cp] = (unsigned char)g[0];
    lds[r * MO_BW + 2 * cp + 1] = (unsigned char)g[1];
  }

  // ---- level k + 1 from level k of the tile
  int from = 0;   // where level k starts in lds
  for (int k = 0; k + 1 < a.levels; k++) {
    __syncthreads();
    const int pw = MO_BW >> k, ph = MO_BH >> k;      // the tile at level k
    const int tw = pw >> 1, th = ph >> 1;            // ... and at level k + 1
    const int to = from + pw * ph;
    if (tid < tw * th) {
      const int r = tid / tw, c = tid % tw;
      const int R = (((int)blockIdx.y * MO_BH) >> (k + 1)) + r, Cc = (((int)blockIdx.x * MO_BW) >> (k + 1)) + c;
      uint32_t v = 0u;
      if (R < a.g.h[k + 1] && Cc < a.g.w[k + 1]) {
        // the clamp to the last row and column of level k, in the tile's coordinates: its origin at level k is twice that at level k + 1
        const int r1 = 2 * r + ((2 * R + 1 < a.g.h[k]) ? 1 : 0), c1 = 2 * c + ((2 * Cc + 1 < a.g.w[k]) ? 1 : 0);
        const uint32_t s = (uint32_t)lds[from + 2 * r * pw + 2 * c] + (uint32_t)lds[from + 2 * r * pw + c1] + (uint32_t)lds[from + r1 * pw + 2 * c] +
                           (uint32_t)lds[from + r1 * pw + c1];
        v = (s + 2u) >> 2;
        dst[a.g.at[k + 1] + (size_t)R * (size_t)a.g.w[k + 1] + (size_t)Cc] = (unsigned char)v;
      }
      lds[to + r * tw + c] = (unsigned char)v;
    }
    from = to;
  }
}

// ================================================================ match
struct MoMatchArgs {
  const unsigned char* cur;
  const unsigned char* ref;
  const uint32_t* index;
  int which_cur, which_ref, levels, search, tiles_x;
  uint32_t zero_bias;
  int16_t* field;
  uint32_t* costs;
  MoGeometry g;
};

// four bytes of row y of a plane from column x, both clamped to the plane, lowest column in the lowest byte
__device__ __forceinline__ uint32_t mo_gather4(const unsigned char* __restrict__ plane, int w, int h, int y, int x) {
  const unsigned char* __restrict__ row = plane + (size_t)min(max(y, 0), h - 1) * (size_t)w;
  uint32_t out = 0u;
#pragma unroll
  for (int b = 0; b < 4; b++) out |= (uint32_t)row[min(max(x + b, 0), w - 1)] << (8 * b);
  return out;
}

__device__ __forceinline__ uint32_t mo_wave_min(uint32_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = min(v, (uint32_t)__shfl_xor((int)v, o, 64));
  return v;
}
__device__ __forceinline__ uint32_t mo_wave_add(uint32_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += (uint32_t)__shfl_xor((int)v, o, 64);
  return v;
}

__global__ __launch_bounds__(MO_WAVE) void mo_match(MoMatchArgs a) {
  __shared__ uint32_t block[MO_BH * MO_BW / 4];
  __shared__ uint32_t window[MO_WIN_ROWS * MO_WIN_DWORDS];
  const int lane = threadIdx.x;
  const int tx = blockIdx.x, ty = blockIdx.y;
  const size_t tile = (size_t)ty * (size_t)a.tiles_x + (size_t)tx;

  uint32_t slot_cur = (uint32_t)a.which_cur, slot_ref = (uint32_t)a.which_ref;
  if (a.index) {
    const uint32_t idx = *a.index;
    if (idx == 0u) {   // no history: the first frame is defined
      if (lane == 0) {
        a.field[2 * tile] = 0, a.field[2 * tile + 1] = 0;
        if (a.costs) a.costs[2 * tile] = 0u, a.costs[2 * tile + 1] = 0u;
      }
      return;
    }
    slot_cur = (idx + slot_cur) & 1u, slot_ref = (idx + slot_ref) & 1u;
  }
  const unsigned char* __restrict__ cur = a.cur + (size_t)slot_cur * a.g.slot;
  const unsigned char* __restrict__ ref = a.ref + (size_t)slot_ref * a.g.slot;

  int dy = 0, dx = 0;      // the displacement chosen at the level above, then at this level
  uint32_t best = 0u;      // the winner's key at this level
  for (int k = a.levels - 1; k >= 0; k--) {
    const int w = a.g.w[k], h = a.g.h[k];
    const int R = k == a.levels - 1 ? a.search : 1;
    const int by = 2 * dy, bx = 2 * dx;              // (0 at the coarsest level)
    const int top = ((MO_BH * ty + MO_BH / 2) >> k) - MO_BH / 2, left = ((MO_BW * tx + MO_BW / 2) >> k) - MO_BW / 2;
    __syncthreads();                                 // the level above has been read
    for (int t = lane; t < MO_BH * MO_BW / 4; t += MO_WAVE) block[t] = mo_gather4(cur + a.g.at[k], w, h, top + t / (MO_BW / 4), left + 4 * (t % (MO_BW / 4)));
    for (int t = lane; t < (MO_BH + 2 * R) * MO_WIN_DWORDS; t += MO_WAVE)
      window[t] = mo_gather4(ref + a.g.at[k], w, h, top + by - R + t / MO_WIN_DWORDS, left + bx - R + 4 * (t % MO_WIN_DWORDS));
    __syncthreads();
    const int side = 2 * R + 1;
    uint32_t key = 0xFFFFFFFFu;
    for (int cand = lane; cand < side * side; cand += MO_WAVE) {
      const int sy = cand / side, sx = cand % side;  // the offset plus R: where the block lies in the window
      const int shift = 8 * (sx & 3);
      uint32_t cost = 0u;
#pragma unroll 2
      for (int r = 0; r < MO_BH; r++) {
        const uint32_t* __restrict__ wrow = window + (r + sy) * MO_WIN_DWORDS + (sx >> 2);
        uint32_t lo = wrow[0];
#pragma unroll
        for (int g = 0; g < MO_BW / 4; g++) {
          const uint32_t hi = wrow[g + 1];
          const uint32_t moved = (uint32_t)((((uint64_t)hi << 32) | (uint64_t)lo) >> shift);
          cost = __builtin_amdgcn_sad_u8(block[r * (MO_BW / 4) + g], moved, cost);
          lo = hi;
        }
      }
      const int oy = sy - R, ox = sx - R;
      key = min(key, (cost << 14) | ((uint32_t)(oy * oy + ox * ox) << 8) | ((uint32_t)(oy + 4) << 4) | (uint32_t)(ox + 4));
    }
    best = mo_wave_min(key);
    dy = by + (int)((best >> 4) & 15u) - 4;
    dx = bx + (int)(best & 15u) - 4;
  }

  // ---- the zero preference: the level-0 block of ref at no displacement
  const int top = MO_BH * ty, left = MO_BW * tx;     // (16 ty + 8) - 8, (32 tx + 16) - 16
  __syncthreads();
  for (int t = lane; t < MO_BH * MO_BW / 4; t += MO_WAVE) window[t] = mo_gather4(ref + a.g.at[0], a.g.w[0], a.g.h[0], top + t / (MO_BW / 4), left + 4 * (t % (MO_BW / 4)));
  __syncthreads();
  uint32_t zero = 0u;
  for (int t = lane; t < MO_BH * MO_BW / 4; t += MO_WAVE) zero = __builtin_amdgcn_sad_u8(block[t], window[t], zero);
  zero = mo_wave_add(zero);
  uint32_t cost = best >> 14;
  if (cost + a.zero_bias >= zero) dy = 0, dx = 0, cost = zero;
  if (lane == 0) {
    a.field[2 * tile] = (int16_t)(2 * dy), a.field[2 * tile + 1] = (int16_t)(2 * dx);
    if (a.costs) a.costs[2 * tile] = cost, a.costs[2 * tile + 1] = zero;
  }
}

// ================================================================ compensated filter (the tile body of temporal.hip)
constexpr int MC_TW = TDK_TEMPORAL_TILE_W, MC_TH = TDK_TEMPORAL_TILE_H;
constexpr int MC_THREADS = 256;
constexpr int MC_GROUP = 8;                          // sites of a lane in the interior
constexpr int MC_GROUPS = MC_TW / MC_GROUP;          // lanes of a tile row
constexpr int MC_SIDE = 4;                           // staged columns on either side of the tile: one unit of four sites
constexpr int MC_SW = MC_TW + 2 * MC_SIDE;           // floats of a staged row
constexpr int MC_UNITS = MC_SW / 4;                  // units of four sites of a staged row
static_assert(MC_TH * MC_GROUPS == MC_THREADS, "a lane per group of the tile");
static_assert(MC_SIDE >= 3, "the apron of the largest radius");

template <int R> struct McLds {   // the layout of temporal.hip: tdk_temporal_lds_bytes(R)
  alignas(16) float e[(MC_TH + 2 * R) * MC_SW];      // staged: tile and apron
  alignas(16) float v[(MC_TH + 2 * R) * MC_SW];
  alignas(16) float re[(MC_TH + 2 * R) * MC_TW];     // row sums of the tile's columns
  alignas(16) float rv[(MC_TH + 2 * R) * MC_TW];
};
static_assert(sizeof(McLds<3>) <= 64 * 1024, "LDS of the filter launch");
static_assert(36 * 3 + 64 <= MC_THREADS, "a lane per apron unit");
#define MC_WAVES(R) ((160 * 1024) / (int)sizeof(McLds<R>))
static_assert(MC_WAVES(2) == 4 && MC_WAVES(3) == 3, "workgroups per compute unit");

struct McArgs {
  const void* src;
  void* out;
  unsigned char* state;
  size_t acc_bytes, cnt_bytes;   // PA and PC of tdk_hip_temporal.h
  int w, h;
  uint32_t pattern;
  const float* model;
  const float* gains;
  float t_hi, inv, c2, n_max, v_min;
  const uint32_t* field;         // (dy, dx) of a tile as one word: dy in the low half
};

struct McRow {
  float a, b;   // a', b'
  bool valid;
};

__device__ __forceinline__ McRow mc_row(const float* __restrict__ model, const float* __restrict__ gains, int row) {
  const float g = gains ? gains[row] : 1.0f;
  McRow o;
  o.a = g * model[4 * row];
  o.b = (g * g) * model[4 * row + 1];
  o.valid = model[4 * row + 2] != 0.0f;
  return o;
}

// row k of three, field by field: values, not addresses, so that the rows stay in registers
__device__ __forceinline__ McRow mc_pick(int k, const McRow& r0, const McRow& r1, const McRow& r2) {
  McRow o;
  o.a = k == 0 ? r0.a : k == 1 ? r1.a : r2.a;
  o.b = k == 0 ? r0.b : k == 1 ? r1.b : r2.b;
  o.valid = k == 0 ? r0.valid : k == 1 ? r1.valid : r2.valid;
  return o;
}

// ---- storage: M consecutive elements at p, as float32.  One or two 16-byte vectors (8 bytes for four binary16) when p is on such a
// boundary, per element otherwise.
template <typename T, int M> __device__ __forceinline__ bool mc_vector_ok(const T* p) {
  constexpr uintptr_t ALIGN = M * sizeof(T) >= 16 ? 16 : M * sizeof(T);
  return (reinterpret_cast<uintptr_t>(p) & (ALIGN - 1)) == 0;
}

template <int M> __device__ __forceinline__ void mc_load(const float* p, float x[M]) {
#pragma unroll
  for (int k = 0; k < M / 4; k++) {
    const float4 u = reinterpret_cast<const float4*>(p)[k];
    x[4 * k] = u.x, x[4 * k + 1] = u.y, x[4 * k + 2] = u.z, x[4 * k + 3] = u.w;
  }
}
template <int M> __device__ __forceinline__ void mc_load(const __half* p, float x[M]) {
  uint32_t w[M / 2];
  if constexpr (M == 8) {
    const uint4 u = *reinterpret_cast<const uint4*>(p);
    w[0] = u.x, w[1] = u.y, w[2] = u.z, w[3] = u.w;
  } else {
    const uint2 u = *reinterpret_cast<const uint2*>(p);
    w[0] = u.x, w[1] = u.y;
  }
#pragma unroll
  for (int k = 0; k < M; k++) x[k] = __half2float(__ushort_as_half((unsigned short)((w[k / 2] >> (16 * (k % 2))) & 0xffffu)));
}
template <int M> __device__ __forceinline__ void mc_store(float* p, const float y[M]) {
#pragma unroll
  for (int k = 0; k < M / 4; k++) reinterpret_cast<float4*>(p)[k] = make_float4(y[4 * k], y[4 * k + 1], y[4 * k + 2], y[4 * k + 3]);
}
template <int M> __device__ __forceinline__ void mc_store(__half* p, const float y[M]) {
  uint32_t w[M / 2];
#pragma unroll
  for (int k = 0; k < M / 2; k++)
    w[k] = (uint32_t)__half_as_ushort(__float2half_rn(y[2 * k])) | ((uint32_t)__half_as_ushort(__float2half_rn(y[2 * k + 1])) << 16);
  if constexpr (M == 8) *reinterpret_cast<uint4*>(p) = make_uint4(w[0], w[1], w[2], w[3]);
  else *reinterpret_cast<uint2*>(p) = make_uint2(w[0], w[1]);
}

// the elements lo <= m < hi of the M at base[at + m], the others read as 0; `at` is a place in the plane whenever lo < hi covers it
template <typename T, int M> __device__ __forceinline__ void mc_fetch(const T* __restrict__ base, int64_t at, int lo, int hi, float x[M]) {
  if (lo == 0 && hi == M && mc_vector_ok<T, M>(base + at)) mc_load<M>(base + at, x);
  else {
#pragma unroll
    for (int m = 0; m < M; m++) x[m] = (m >= lo && m < hi) ? ld<T>(base, (size_t)(at + m)) : 0.0f;
  }
}
template <typename T, int M> __device__ __forceinline__ void mc_put(T* __restrict__ base, size_t at, int live, const float y[M]) {
  if (live == M && mc_vector_ok<T, M>(base + at)) mc_store<M>(base + at, y);
  else {
#pragma unroll
    for (int m = 0; m < M; m++)
      if (m < live) st<T>(base, at + m, y[m]);
  }
}

// e and v of one site (a site outside the frame is not asked)
__device__ __forceinline__ void mc_site(float x, float A, float N, const McRow& r, float v_min, float& e, float& v) {
  const float d = x - A;
  const float var = fmaxf(r.a * fmaxf(A, 0.0f) + r.b, v_min);
  v = r.valid ? var + var / fmaxf(N, 1.0f) : 0.0f;
  e = r.valid ? d * d : 0.0f;
}

template <typename TS, typename TA, typename TO, int R>
__global__ __launch_bounds__(MC_THREADS, MC_WAVES(R)) void mc_filter(McArgs a) {
  __shared__ McLds<R> lds;
  const int tid = threadIdx.x;
  const int x0 = (int)blockIdx.x * MC_TW, y0 = (int)blockIdx.y * MC_TH;

  // the frame index: the same word for every lane of every workgroup; this launch only reads it
  const uint32_t idx = *reinterpret_cast<const uint32_t*>(a.state);
  const bool first = idx == 0u;
  const size_t to_plane = idx & 1u, from_plane = to_plane ^ 1u;
  unsigned char* planes = a.state + TDK_TEMPORAL_HEAD_BYTES;
  const TA* __restrict__ acc_src = reinterpret_cast<const TA*>(planes + from_plane * a.acc_bytes);
  TA* __restrict__ acc_dst = reinterpret_cast<TA*>(planes + to_plane * a.acc_bytes);
  const __half* __restrict__ cnt_src = reinterpret_cast<const __half*>(planes + 2 * a.acc_bytes + from_plane * a.cnt_bytes);
  __half* __restrict__ cnt_dst = reinterpret_cast<__half*>(planes + 2 * a.acc_bytes + to_plane * a.cnt_bytes);
  const TS* __restrict__ src = reinterpret_cast<const TS*>(a.src);
  TO* __restrict__ out = reinterpret_cast<TO*>(a.out);

  // the displacement of this output tile, odd values masked: uniform over the workgroup, and over its apron
  const uint32_t word = a.field[(size_t)blockIdx.y * (size_t)gridDim.x + (size_t)blockIdx.x];
  const int dy = (int)(int16_t)(word & 0xffffu) & ~1, dx = (int)(int16_t)(word >> 16) & ~1;
  // the history sites of a group of M at (i, j0) with `live` sites in the frame: elements lo <= m < hi at hat + m
  auto history = [&](int i, int j0, int live, int& lo, int& hi, int64_t& hat) {
    const int hi_row = i + dy, hj = j0 + dx;
    lo = hi = 0;
    hat = 0;
    if (first || live <= 0 || hi_row < 0 || hi_row >= a.h) return;
    lo = max(0, -hj), hi = min(live, a.w - hj);
    if (hi <= lo) {
      lo = hi = 0;
      return;
    }
    hat = (int64_t)hi_row * (int64_t)a.w + (int64_t)hj;
  };

  const McRow r0 = mc_row(a.model, a.gains, 0), r1 = mc_row(a.model, a.gains, 1), r2 = mc_row(a.model, a.gains, 2);
  // the model rows of the even and the odd columns of frame row i (every unit starts at an even column)
  auto rows_of = [&](int i, McRow& even, McRow& odd) {
    const uint32_t pair = (a.pattern >> (4u * ((uint32_t)i & 1u))) & 15u;
    even = mc_pick((int)(pair & 3u), r0, r1, r2);
    odd = mc_pick((int)(pair >> 2), r0, r1, r2);
  };

  // ---- 1. interior: eight sites of tile row ty
  const int ty = tid / MC_GROUPS, gx = tid % MC_GROUPS;
  const int i = y0 + ty, j0 = x0 + MC_GROUP * gx;
  const int live = i < a.h ? min(max(a.w - j0, 0), MC_GROUP) : 0;
  const size_t at = (size_t)i * (size_t)a.w + (size_t)j0;   // (not formed into an address unless live > 0)
  float x[MC_GROUP], A[MC_GROUP], N[MC_GROUP];
  McRow even, odd;
  rows_of(i, even, odd);
  {
#pragma unroll
    for (int m = 0; m < MC_GROUP; m++) x[m] = A[m] = N[m] = 0.0f;
    if (live > 0) {
      mc_fetch<TS, MC_GROUP>(src, (int64_t)at, 0, live, x);
      int lo, hi;
      int64_t hat;
      history(i, j0, live, lo, hi, hat);
      if (hi > lo) {
        mc_fetch<TA, MC_GROUP>(acc_src, hat, lo, hi, A);
        mc_fetch<__half, MC_GROUP>(cnt_src, hat, lo, hi, N);
      }
    }
    float e[MC_GROUP], v[MC_GROUP];
#pragma unroll
    for (int m = 0; m < MC_GROUP; m++) {
      mc_site(x[m], A[m], N[m], (m & 1) ? odd : even, a.v_min, e[m], v[m]);
      if (m >= live) e[m] = v[m] = 0.0f;
    }
    const int to = (ty + R) * MC_SW + MC_SIDE + MC_GROUP * gx;
    mc_store<MC_GROUP>(lds.e + to, e);
    mc_store<MC_GROUP>(lds.v + to, v);
  }

  // ---- 2. apron: R rows above, R rows below (whole staged rows), one unit left and right of each tile row
  if (tid < 2 * R * MC_UNITS + 2 * MC_TH) {
    int srow, unit;
    if (tid < 2 * R * MC_UNITS) {
      const int band = tid / (R * MC_UNITS), u = tid - band * (R * MC_UNITS);
      srow = band * (R + MC_TH) + u / MC_UNITS;
      unit = u % MC_UNITS;
    } else {
      const int u = tid - 2 * R * MC_UNITS;
      srow = R + (u >> 1);
      unit = (u & 1) ? MC_UNITS - 1 : 0;
    }
    const int ai = y0 - R + srow, aj = x0 - MC_SIDE + 4 * unit;
    const int alive = (ai >= 0 && ai < a.h && aj >= 0) ? min(max(a.w - aj, 0), 4) : 0;
    float ax[4] = {0.0f, 0.0f, 0.0f, 0.0f}, aA[4] = {0.0f, 0.0f, 0.0f, 0.0f}, aN[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (alive > 0) {
      const int64_t aat = (int64_t)ai * (int64_t)a.w + (int64_t)aj;
      mc_fetch<TS, 4>(src, aat, 0, alive, ax);
      int lo, hi;
      int64_t hat;
      history(ai, aj, alive, lo, hi, hat);
      if (hi > lo) {
        mc_fetch<TA, 4>(acc_src, hat, lo, hi, aA);
        mc_fetch<__half, 4>(cnt_src, hat, lo, hi, aN);
      }
    }
    McRow aeven, aodd;
    rows_of(ai, aeven, aodd);
    float e[4], v[4];
#pragma unroll
    for (int m = 0; m < 4; m++) {
      mc_site(ax[m], aA[m], aN[m], (m & 1) ? aodd : aeven, a.v_min, e[m], v[m]);
      if (m >= alive) e[m] = v[m] = 0.0f;
    }
    mc_store<4>(lds.e + srow * MC_SW + 4 * unit, e);
    mc_store<4>(lds.v + srow * MC_SW + 4 * unit, v);
  }
  __syncthreads();

  // ---- 3. row sums: four columns of a staged row per step
#pragma unroll 1
  for (int t = tid; t < (MC_TH + 2 * R) * (MC_TW / 4); t += MC_THREADS) {
    const int srow = t / (MC_TW / 4), cu = t % (MC_TW / 4);
    float we[12], wv[12];
    mc_load<12>(lds.e + srow * MC_SW + 4 * cu, we);   // staged columns 4 cu .. 4 cu + 11: tile columns 4 cu - 4 .. 4 cu + 7
    mc_load<12>(lds.v + srow * MC_SW + 4 * cu, wv);
    float se[4], sv[4];
#pragma unroll
    for (int m = 0; m < 4; m++) {
      float e = 0.0f, v = 0.0f;
#pragma unroll
      for (int k = -R; k <= R; k++) e += we[4 + m + k], v += wv[4 + m + k];
      se[m] = e, sv[m] = v;
    }
    mc_store<4>(lds.re + srow * MC_TW + 4 * cu, se);
    mc_store<4>(lds.rv + srow * MC_TW + 4 * cu, sv);
  }
  __syncthreads();

  // ---- 4. column sums and the update
  if (live > 0) {
    float E[MC_GROUP], V[MC_GROUP];
#pragma unroll
    for (int m = 0; m < MC_GROUP; m++) E[m] = V[m] = 0.0f;
#pragma unroll 1
    for (int dr = 0; dr <= 2 * R; dr++) {   // (not unrolled: the loads of all rows at once cost the registers of a fourth wave)
      float pe[MC_GROUP], pv[MC_GROUP];
      mc_load<MC_GROUP>(lds.re + (ty + dr) * MC_TW + MC_GROUP * gx, pe);
      mc_load<MC_GROUP>(lds.rv + (ty + dr) * MC_TW + MC_GROUP * gx, pv);
#pragma unroll
      for (int m = 0; m < MC_GROUP; m++) E[m] += pe[m], V[m] += pv[m];
    }
    float e[MC_GROUP], v[MC_GROUP];   // of the lane's own sites, as staged in step 1
    mc_load<MC_GROUP>(lds.e + (ty + R) * MC_SW + MC_SIDE + MC_GROUP * gx, e);
    mc_load<MC_GROUP>(lds.v + (ty + R) * MC_SW + MC_SIDE + MC_GROUP * gx, v);
    float y[MC_GROUP], n1[MC_GROUP];
#pragma unroll
    for (int m = 0; m < MC_GROUP; m++) {
      const McRow& r = (m & 1) ? odd : even;
      const float d = x[m] - A[m];
      const float t = E[m] / V[m];
      float s = fminf(fmaxf((a.t_hi - t) * a.inv, 0.0f), 1.0f);
      if (e[m] > a.c2 * v[m]) s = 0.0f;
      n1[m] = r.valid ? fminf(s * N[m] + 1.0f, a.n_max) : 1.0f;
      y[m] = n1[m] == 1.0f ? x[m] : A[m] + d / n1[m];
    }
    mc_put<TA, MC_GROUP>(acc_dst, at, live, y);
    mc_put<__half, MC_GROUP>(cnt_dst, at, live, n1);
    mc_put<TO, MC_GROUP>(out, at, live, y);
  }
}

__global__ void mc_advance(uint32_t* head) {
  if (threadIdx.x == 0) {
    const uint32_t idx = *head;
    *head = idx == 0xFFFFFFFFu ? 2u : idx + 1u;
  }
}

bool mc_pattern_ok(uint32_t pattern) {
  return pattern == TDK_PATTERN_RGGB || pattern == TDK_PATTERN_BGGR || pattern == TDK_PATTERN_GRBG || pattern == TDK_PATTERN_GBRG;
}
size_t mc_plane_bytes(int width, int height, size_t element) { return tdk_align_up((size_t)width * (size_t)height * element, 16); }

template <typename TS, typename TA, typename TO, int R> int mc_launch(const McArgs& a, hipStream_t st) {
  const dim3 grid((unsigned)tdk_div_up(a.w, MC_TW), (unsigned)tdk_div_up(a.h, MC_TH)), block(MC_THREADS);
  TDK_LAUNCH("tdk_motion_temporal_denoise(filter)", (mc_filter<TS, TA, TO, R>), grid, block, 0, st, a);
  return TDK_OK;
}

template <typename TS, typename TA, typename TO> int mc_launch_radius(const McArgs& a, int radius, hipStream_t st) {
  return radius == 2 ? mc_launch<TS, TA, TO, 2>(a, st) : mc_launch<TS, TA, TO, 3>(a, st);
}

template <typename TS, typename TA> int mc_launch_out(const McArgs& a, int out_dtype, int radius, hipStream_t st) {
  return out_dtype == TDK_F32 ? mc_launch_radius<TS, TA, float>(a, radius, st) : mc_launch_radius<TS, TA, __half>(a, radius, st);
}

template <typename TS> int mc_launch_state(const McArgs& a, int state_dtype, int out_dtype, int radius, hipStream_t st) {
  return state_dtype == TDK_F32 ? mc_launch_out<TS, float>(a, out_dtype, radius, st) : mc_launch_out<TS, __half>(a, out_dtype, radius, st);
}

template <typename TS> int mo_launch_pyramid(const MoPyramidArgs& a, hipStream_t st) {
  const dim3 grid((unsigned)tdk_div_up(a.w, TDK_MOTION_TILE_W), (unsigned)tdk_div_up(a.h, TDK_MOTION_TILE_H)), block(MO_THREADS);
  TDK_LAUNCH("tdk_motion_pyramid", mo_pyramid<TS>, grid, block, 0, st, a);
  return TDK_OK;
}

}  // namespace

TDK_EXPORT int tdk_motion_abi_version(void) { return TDK_MOTION_ABI_VERSION; }

TDK_EXPORT size_t tdk_motion_pyramid_bytes(int width, int height, int levels) {
  if (!mo_size_ok(width, height) || !mo_levels_ok(levels)) return 0;
  return 2 * mo_geometry(width, height, levels).slot;
}

TDK_EXPORT int tdk_motion_pyramid(const void* src, int src_dtype, int width, int height, float scale, int levels, void* pyramid, const uint32_t* index, int which,
                                  tdk_stream_t stream) {
  static const char* const who = "tdk_motion_pyramid";
  TDK_REQUIRE(src && pyramid, "%s: null pointer (src or pyramid)", who);
  TDK_REQUIRE(mo_dtype_ok(src_dtype), "%s: unsupported dtype tag %d", who, src_dtype);
  TDK_REQUIRE(width >= 2 && height >= 2 && width <= MO_MAX_SIZE && height <= MO_MAX_SIZE, "%s: frame size %dx%d outside 2..%d", who, width, height, MO_MAX_SIZE);
  TDK_REQUIRE(width % 2 == 0 && height % 2 == 0, "%s: mosaic size %dx%d must be even in both axes (whole CFA cells)", who, width, height);
  TDK_REQUIRE(isfinite(scale) && scale > 0.0f, "%s: scale must be finite and > 0", who);
  TDK_REQUIRE(mo_levels_ok(levels), "%s: levels must be 1..%d, got %d", who, TDK_MOTION_MAX_LEVELS, levels);
  TDK_REQUIRE(which == 0 || which == 1, "%s: which must be 0 or 1, got %d", who, which);
  TDK_REQUIRE(tdk_aligned(pyramid, 16), "%s: pyramid must be aligned to 16 bytes", who);
  TDK_REQUIRE(!index || tdk_aligned(index, 4), "%s: index must be aligned to 4 bytes", who);
  const size_t src_bytes = (size_t)width * (size_t)height * tdk_dtype_bytes(src_dtype);
  TDK_REQUIRE(tdk_disjoint(src, src_bytes, pyramid, tdk_motion_pyramid_bytes(width, height, levels)), "%s: src and pyramid overlap", who);

  MoPyramidArgs a{};
  a.src = src, a.pyramid = reinterpret_cast<unsigned char*>(pyramid), a.index = index, a.which = which, a.levels = levels;
  a.w = width, a.h = height, a.scale = scale, a.g = mo_geometry(width, height, levels);
  hipStream_t st = tdk_stream(stream);
  return src_dtype == TDK_F32 ? mo_launch_pyramid<float>(a, st) : mo_launch_pyramid<__half>(a, st);
}

TDK_EXPORT int tdk_motion_match(const void* pyramid_cur, int which_cur, const void* pyramid_ref, int which_ref, int width, int height, int levels, int search,
                                uint32_t zero_bias, const uint32_t* index, int16_t* field, uint32_t* costs, tdk_stream_t stream) {
  static const char* const who = "tdk_motion_match";
  TDK_REQUIRE(pyramid_cur && pyramid_ref && field, "%s: null pointer (pyramid_cur, pyramid_ref or field)", who);
  TDK_REQUIRE(width >= 2 && height >= 2 && width <= MO_MAX_SIZE && height <= MO_MAX_SIZE, "%s: frame size %dx%d outside 2..%d", who, width, height, MO_MAX_SIZE);
  TDK_REQUIRE(width % 2 == 0 && height % 2 == 0, "%s: mosaic size %dx%d must be even in both axes (whole CFA cells)", who, width, height);
  TDK_REQUIRE(mo_levels_ok(levels), "%s: levels must be 1..%d, got %d", who, TDK_MOTION_MAX_LEVELS, levels);
  TDK_REQUIRE(search >= 1 && search <= TDK_MOTION_MAX_SEARCH, "%s: search must be 1..%d, got %d", who, TDK_MOTION_MAX_SEARCH, search);
  TDK_REQUIRE(zero_bias <= TDK_MOTION_MAX_ZERO_BIAS, "%s: zero_bias must be 0..%d, got %u", who, TDK_MOTION_MAX_ZERO_BIAS, zero_bias);
  TDK_REQUIRE((which_cur == 0 || which_cur == 1) && (which_ref == 0 || which_ref == 1), "%s: which_cur and which_ref must be 0 or 1, got %d and %d", who,
              which_cur, which_ref);
  TDK_REQUIRE(tdk_aligned(pyramid_cur, 16) && tdk_aligned(pyramid_ref, 16), "%s: the pyramids must be aligned to 16 bytes", who);
  TDK_REQUIRE(!index || tdk_aligned(index, 4), "%s: index must be aligned to 4 bytes", who);
  TDK_REQUIRE(tdk_aligned(field, 4), "%s: field must be aligned to 4 bytes", who);
  TDK_REQUIRE(!costs || tdk_aligned(costs, 8), "%s: costs must be aligned to 8 bytes", who);
  const size_t tiles = (size_t)tdk_div_up(width, TDK_MOTION_TILE_W) * (size_t)tdk_div_up(height, TDK_MOTION_TILE_H);
  const size_t pyramid_bytes = tdk_motion_pyramid_bytes(width, height, levels), field_bytes = tiles * 4, costs_bytes = tiles * 8;
  TDK_REQUIRE(tdk_disjoint(field, field_bytes, pyramid_cur, pyramid_bytes) && tdk_disjoint(field, field_bytes, pyramid_ref, pyramid_bytes) &&
                  (!costs || (tdk_disjoint(costs, costs_bytes, pyramid_cur, pyramid_bytes) && tdk_disjoint(costs, costs_bytes, pyramid_ref, pyramid_bytes) &&
                              tdk_disjoint(costs, costs_bytes, field, field_bytes))),
              "%s: field, costs and the pyramids overlap", who);

  MoMatchArgs a{};
  a.cur = reinterpret_cast<const unsigned char*>(pyramid_cur), a.ref = reinterpret_cast<const unsigned char*>(pyramid_ref), a.index = index;
  a.which_cur = which_cur, a.which_ref = which_ref, a.levels = levels, a.search = search, a.tiles_x = tdk_div_up(width, TDK_MOTION_TILE_W);
  a.zero_bias = zero_bias, a.field = field, a.costs = costs, a.g = mo_geometry(width, height, levels);
  const dim3 grid((unsigned)a.tiles_x, (unsigned)tdk_div_up(height, TDK_MOTION_TILE_H)), block(MO_WAVE);
  TDK_LAUNCH("tdk_motion_match", mo_match, grid, block, 0, tdk_stream(stream), a);
  return TDK_OK;
}

TDK_EXPORT int tdk_motion_temporal_denoise(const void* src, int src_dtype, void* out, int out_dtype, void* state, int state_dtype, int width, int height,
                                           uint32_t pattern, const float* model, const float* gains, int radius, float t_lo, float t_hi, float pixel_c2,
                                           float n_max, float v_min, const int16_t* field, tdk_stream_t stream) {
  static const char* const who = "tdk_motion_temporal_denoise";
  TDK_REQUIRE(src && out && state && model && field, "%s: null pointer (src, out, state, model or field)", who);
  TDK_REQUIRE(mo_dtype_ok(src_dtype) && mo_dtype_ok(out_dtype) && mo_dtype_ok(state_dtype), "%s: unsupported dtype tags %d -> %d, state %d", who, src_dtype,
              out_dtype, state_dtype);
  TDK_REQUIRE(width >= 2 && height >= 2 && width <= MO_MAX_SIZE && height <= MO_MAX_SIZE, "%s: frame size %dx%d outside 2..%d", who, width, height, MO_MAX_SIZE);
  TDK_REQUIRE(width % 2 == 0 && height % 2 == 0, "%s: mosaic size %dx%d must be even in both axes (whole CFA cells)", who, width, height);
  TDK_REQUIRE(mc_pattern_ok(pattern), "%s: unknown Bayer pattern 0x%08x", who, pattern);
  TDK_REQUIRE(radius == 2 || radius == 3, "%s: radius must be 2 or 3, got %d", who, radius);
  const float inv = 1.0f / (t_hi - t_lo);
  TDK_REQUIRE(isfinite(t_lo) && isfinite(t_hi) && t_lo > 0.0f && t_hi > t_lo && isfinite(inv),
              "%s: the thresholds need 0 < t_lo < t_hi, finite, with a finite 1 / (t_hi - t_lo)", who);
  TDK_REQUIRE(pixel_c2 > 0.0f, "%s: pixel_c2 must be > 0 (+inf turns the per-site test off)", who);
  TDK_REQUIRE(n_max >= 1.0f && n_max <= (float)TDK_TEMPORAL_MAX_FRAMES, "%s: n_max must be 1..%d", who, TDK_TEMPORAL_MAX_FRAMES);
  TDK_REQUIRE(isfinite(v_min) && v_min > 0.0f, "%s: v_min must be finite and > 0", who);
  TDK_REQUIRE(tdk_aligned(state, 16), "%s: state must be aligned to 16 bytes", who);
  TDK_REQUIRE(tdk_aligned(field, 4), "%s: field must be aligned to 4 bytes", who);
  const size_t sites = (size_t)width * (size_t)height;
  const size_t src_bytes = sites * tdk_dtype_bytes(src_dtype), out_bytes = sites * tdk_dtype_bytes(out_dtype);
  const size_t state_bytes = tdk_temporal_state_bytes(width, height, state_dtype);
  const size_t field_bytes = (size_t)tdk_div_up(width, MC_TW) * (size_t)tdk_div_up(height, MC_TH) * 4;
  TDK_REQUIRE(tdk_disjoint(src, src_bytes, out, out_bytes) && tdk_disjoint(src, src_bytes, state, state_bytes) && tdk_disjoint(out, out_bytes, state, state_bytes),
              "%s: src, out and state overlap", who);
  TDK_REQUIRE(tdk_disjoint(model, 48, out, out_bytes) && tdk_disjoint(model, 48, state, state_bytes) &&
                  (!gains || (tdk_disjoint(gains, 12, out, out_bytes) && tdk_disjoint(gains, 12, state, state_bytes))),
              "%s: the model or the gains overlap out or state", who);
  TDK_REQUIRE(tdk_disjoint(field, field_bytes, out, out_bytes) && tdk_disjoint(field, field_bytes, state, state_bytes), "%s: the field overlaps out or state", who);

  McArgs a{};
  a.src = src, a.out = out, a.state = reinterpret_cast<unsigned char*>(state);
  a.acc_bytes = mc_plane_bytes(width, height, tdk_dtype_bytes(state_dtype)), a.cnt_bytes = mc_plane_bytes(width, height, 2);
  a.w = width, a.h = height, a.pattern = pattern, a.model = model, a.gains = gains;
  a.t_hi = t_hi, a.inv = inv, a.c2 = pixel_c2, a.n_max = n_max, a.v_min = v_min;
  a.field = reinterpret_cast<const uint32_t*>(field);
  hipStream_t st = tdk_stream(stream);
  const int rc = src_dtype == TDK_F32 ? mc_launch_state<float>(a, state_dtype, out_dtype, radius, st) : mc_launch_state<__half>(a, state_dtype, out_dtype, radius, st);
  if (rc != TDK_OK) return rc;
  TDK_LAUNCH("tdk_motion_temporal_denoise(advance)", mc_advance, dim3(1), dim3(1), 0, st, reinterpret_cast<uint32_t*>(state));
  return TDK_OK;
}
