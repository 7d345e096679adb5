// motion.hip -- block-matching motion estimation on raw mosaics and the motion-compensated temporal denoiser
// (include/tdk_hip_motion.h: tdk_motion_pyramid and tdk_motion_match, one launch each; tdk_motion_temporal_denoise: one tile launch
// and a one-lane launch that advances the frame index).
//
// The specification is the head comment of include/tdk_hip_motion.h.
//
// Pyramid, mo_pyramid<TS>: a workgroup of 256 lanes owns the 32 x 16 level-0 values of one tile of the temporal filter (64 x 32 sites).
// A lane turns two CFA cells into grey values, the tile goes to LDS, and level k + 1 is reduced from level k there: the tile's origin
// is a multiple of 8 values, so the 2 x 2 blocks of every level (and the clamp at the plane's last row and column) stay inside it.  The
// body stands in tdk_motion_pyramid.h, which hdralign.hip instantiates a second time with the scale of a bracket's frame.
// Match, mo_match: one wave per tile.  Per level the block (16 x 32 bytes) and the search window ((16 + 2R) x (32 + 2R) bytes, fetched
// with clamped coordinates, so the LDS copy answers ref[clamp(p + d)] for every candidate) are staged as dwords; a lane owns a
// candidate and walks the block four samples per v_sad_u8, the window dword shifted into place from two neighbours; the winner is the
// wave's minimum of the candidates' keys.
// Compensated filter, mc_filter<TS, TA, TO, R>: the tile body of tp_filter (tt_filter_tile of tdk_temporal_tile.h, one text for both
// kernels; its steps are listed at the head of temporal.hip) with the history read at a per-workgroup uniform displacement
// (McHistoryDisplaced): the element offset dy * w + dx on the two state reads and an in-frame test of the history site.  Whether a
// lane's group goes as 16-byte vectors or per element is decided by the shifted address, as tp_filter decides by the plain one.  The
// entry point shares the checks of tdk_temporal_denoise (tt_check); the pyramid reads its sites with mt_fetch of tdk_mosaic_tile.h.
#include "../../include/tdk_hip_motion.h"
#include "tdk_motion_pyramid.h"
#include "tdk_temporal_tile.h"

namespace {

constexpr int MO_WAVE = 64;                           // of the match launch
constexpr int MO_WIN_DWORDS = (MO_BW + 2 * TDK_MOTION_MAX_SEARCH) / 4 + 1;   // dwords of a staged window row: one more than the
                                                                             // widest window, for the shifted read of the last group
constexpr int MO_WIN_ROWS = MO_BH + 2 * TDK_MOTION_MAX_SEARCH;
static_assert(TDK_MOTION_TILE_W == TDK_TEMPORAL_TILE_W && TDK_MOTION_TILE_H == TDK_TEMPORAL_TILE_H, "the tiles of the temporal filter");
static_assert(2 * ((TDK_MOTION_MAX_SEARCH + 1) * (1 << (TDK_MOTION_MAX_LEVELS - 1)) - 1) == TDK_MOTION_MAX_DISPLACEMENT, "the largest displacement");

// ================================================================ pyramid (the tile body of tdk_motion_pyramid.h)
template <typename TS> __global__ __launch_bounds__(MO_THREADS) void mo_pyramid(MoPyramidArgs a) {
  __shared__ unsigned char lds[MO_PYRAMID_LDS];
  mo_pyramid_tile<TS>(lds, a, MoScaleGiven{});
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

// ================================================================ compensated filter (the tile body of tdk_temporal_tile.h)
struct McArgs : TtArgs {
  const uint32_t* field;   // (dy, dx) of a tile as one word: dy in the low half
};

// The history of a group lies (dy, dx) from its sites, the displacement of the output tile: what of it is inside the frame.
struct McHistoryDisplaced {
  int dy, dx, w, h;
  __device__ __forceinline__ void operator()(bool first, int i, int j0, int64_t, int live, int& lo, int& hi, int64_t& hat) const {
    const int hi_row = i + dy, hj = j0 + dx;
    lo = hi = 0;
    hat = 0;
    if (first || live <= 0 || hi_row < 0 || hi_row >= h) return;
    lo = max(0, -hj), hi = min(live, w - hj);
    if (hi <= lo) {
      lo = hi = 0;
      return;
    }
    hat = (int64_t)hi_row * (int64_t)w + (int64_t)hj;
  }
};

template <typename TS, typename TA, typename TO, int R>
__global__ __launch_bounds__(MT_THREADS, TT_WAVES<R>) void mc_filter(McArgs a) {
  __shared__ typename TtTile<R>::Lds lds;
  // the displacement of this output tile, odd values masked: uniform over the workgroup, and over its apron
  const uint32_t word = a.field[(size_t)blockIdx.y * (size_t)gridDim.x + (size_t)blockIdx.x];
  const int dy = (int)(int16_t)(word & 0xffffu) & ~1, dx = (int)(int16_t)(word >> 16) & ~1;
  tt_filter_tile<TS, TA, TO, R>(lds, a, McHistoryDisplaced{dy, dx, a.w, a.h});
}

__global__ void mc_advance(uint32_t* head) { tt_advance(head); }

template <typename TS, typename TA, typename TO, int R> int mc_launch(const McArgs& a, hipStream_t st) {
  const dim3 grid((unsigned)tdk_div_up(a.w, TtTile<R>::TW), (unsigned)tdk_div_up(a.h, TtTile<R>::TH)), block(MT_THREADS);
  TDK_LAUNCH("tdk_motion_temporal_denoise(filter)", (mc_filter<TS, TA, TO, R>), grid, block, 0, st, a);
  return TDK_OK;
}

template <typename TS, typename TA, typename TO> int mc_launch_radius(const McArgs& a, int radius, hipStream_t st) {
  return radius == 2 ? mc_launch<TS, TA, TO, 2>(a, st) : mc_launch<TS, TA, TO, 3>(a, st);
}

template <typename TS> int mo_launch_pyramid(const MoPyramidArgs& a, hipStream_t st) {
  const dim3 grid((unsigned)tdk_div_up(a.w, TDK_MOTION_TILE_W), (unsigned)tdk_div_up(a.h, TDK_MOTION_TILE_H)), block(MO_THREADS);
  TDK_LAUNCH("tdk_motion_pyramid", mo_pyramid<TS>, grid, block, 0, st, a);
  return TDK_OK;
}

}  // namespace

TDK_EXPORT int tdk_motion_abi_version(void) { return TDK_MOTION_ABI_VERSION; }

TDK_EXPORT size_t tdk_motion_pyramid_bytes(int width, int height, int levels) { return mo_pyramid_bytes(width, height, levels); }

TDK_EXPORT int tdk_motion_pyramid(const void* src, int src_dtype, int width, int height, float scale, int levels, void* pyramid, const uint32_t* index, int which,
                                  tdk_stream_t stream) {
  MoPyramidArgs a{};
  if (const int rc = mo_check_pyramid("tdk_motion_pyramid", src, src_dtype, width, height, scale, levels, pyramid, index, which, a)) return rc;
  hipStream_t st = tdk_stream(stream);
  return src_dtype == TDK_F32 ? mo_launch_pyramid<float>(a, st) : mo_launch_pyramid<__half>(a, st);
}

TDK_EXPORT int tdk_motion_match(const void* pyramid_cur, int which_cur, const void* pyramid_ref, int which_ref, int width, int height, int levels, int search,
                                uint32_t zero_bias, const uint32_t* index, int16_t* field, uint32_t* costs, tdk_stream_t stream) {
  static const char* const who = "tdk_motion_match";
  TDK_REQUIRE(pyramid_cur && pyramid_ref && field, "%s: null pointer (pyramid_cur, pyramid_ref or field)", who);
  TDK_REQUIRE(tdk_mosaic_size_ok(width, height), "%s: frame size %dx%d outside 2..%d", who, width, height, TDK_MOSAIC_MAX_SIZE);
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
  McArgs a{};
  if (const int rc = tt_check(who, src, src_dtype, out, out_dtype, state, state_dtype, width, height, pattern, model, gains, radius, t_lo, t_hi, pixel_c2, n_max,
                              v_min, a))
    return rc;
  TDK_REQUIRE(tdk_aligned(field, 4), "%s: field must be aligned to 4 bytes", who);
  const size_t out_bytes = (size_t)width * (size_t)height * tdk_dtype_bytes(out_dtype), state_bytes = tdk_temporal_state_bytes(width, height, state_dtype);
  const size_t field_bytes = (size_t)tdk_div_up(width, TDK_MOTION_TILE_W) * (size_t)tdk_div_up(height, TDK_MOTION_TILE_H) * 4;
  TDK_REQUIRE(tdk_disjoint(field, field_bytes, out, out_bytes) && tdk_disjoint(field, field_bytes, state, state_bytes), "%s: the field overlaps out or state", who);
  a.field = reinterpret_cast<const uint32_t*>(field);
  hipStream_t st = tdk_stream(stream);
  int rc = TDK_OK;
  TDK_DISPATCH_DTYPE(src_dtype, TS, TDK_DISPATCH_DTYPE(state_dtype, TA, TDK_DISPATCH_DTYPE(out_dtype, TO, rc = mc_launch_radius<TS, TA, TO>(a, radius, st))));
  if (rc != TDK_OK) return rc;
  TDK_LAUNCH("tdk_motion_temporal_denoise(advance)", mc_advance, dim3(1), dim3(1), 0, st, reinterpret_cast<uint32_t*>(state));
  return TDK_OK;
}
