// tdk_motion_pyramid.h -- the tile body of the grey pyramid (include/tdk_hip_motion.h), shared by mo_pyramid of motion.hip and
// ha_pyramid of hdralign.hip (include/tdk_hip_hdralign.h), with the geometry of a pyramid buffer, its arguments and the checks of the
// two entry points.  The two kernels differ in where the scale of the grey formula comes from: a kernel argument, or the exposures of
// a bracket read on the device.  That is a type, so the plain pyramid pays nothing for the other.  It launches nothing.
#pragma once

#include "../../include/tdk_hip_motion.h"
#include "tdk_mosaic_tile.h"

constexpr int MO_BW = 32, MO_BH = 16;                 // the block of a tile at every level; the tile's level-0 values
constexpr int MO_THREADS = 256;                       // of the pyramid launch
constexpr int MO_PYRAMID_LDS = MO_BH * MO_BW * 2;     // bytes: the tile at every level, one behind the other: 16 x 32, 8 x 16, 4 x 8, 2 x 4 values
static_assert(2 * MO_BW == TDK_MOTION_TILE_W && 2 * MO_BH == TDK_MOTION_TILE_H, "a tile is its level-0 block");

struct MoGeometry {
  int w[TDK_MOTION_MAX_LEVELS], h[TDK_MOTION_MAX_LEVELS];
  size_t at[TDK_MOTION_MAX_LEVELS];   // byte offset of a level in its slot
  size_t slot;                        // bytes of a slot
};

static inline MoGeometry mo_geometry(int width, int height, int levels) {
  MoGeometry g{};
  int w = width / 2, h = height / 2;
  for (int k = 0; k < levels; k++) {
    g.w[k] = w, g.h[k] = h, g.at[k] = g.slot;
    g.slot += tdk_align_up((size_t)w * (size_t)h, 16);
    w = (w + 1) / 2, h = (h + 1) / 2;
  }
  return g;
}

static inline bool mo_levels_ok(int levels) { return levels >= 1 && levels <= TDK_MOTION_MAX_LEVELS; }

struct MoPyramidArgs {
  const void* src;
  unsigned char* pyramid;
  const uint32_t* index;
  int which, levels, w, h;   // w, h: sites
  float scale;
  MoGeometry g;
};

// ---- the scale of the grey formula.  The plain pyramid takes the host's.
// Its square root is the hardware's (v_sqrt_f32, within one ulp): on about one cell in ten thousand, where sqrt(u) * 255 + 0.5 comes to lie
// on a whole number, the grey value is one below that of the correctly rounded root the header asks for.  Its bits are pinned; the
// bracket pyramid takes the correctly rounded root.
struct MoScaleGiven {
  __device__ __forceinline__ float operator()(const MoPyramidArgs& a) const { return a.scale; }
  static __device__ __forceinline__ float root(float u) { return __fsqrt_rn(u); }
};
// A frame of a bracket is brought into the units of the longest frame: scale * (e_hi / exposures[frame]), e_hi by the rule of
// tdk_hip_hdr.h (a later frame replaces an earlier one only when >).  The same value in every lane of every workgroup.
struct MoScaleOfBracket {
  const float* exposures;
  int nf, frame;
  __device__ __forceinline__ float operator()(const MoPyramidArgs& a) const {
    float e_hi = exposures[0];
#pragma unroll 1
    for (int f = 1; f < nf; f++) {
      const float e = exposures[f];
      if (e > e_hi) e_hi = e;
    }
    return a.scale * (e_hi / exposures[frame]);
  }
  static __device__ __forceinline__ float root(float u) { return sqrtf(u); }   // correctly rounded
};

template <typename Scale> __device__ __forceinline__ uint32_t mo_grey(float x00, float x01, float x10, float x11, float scale) {
  const float q = (x00 + x01) + (x10 + x11);
  const float u = fminf(fmaxf(q * scale, 0.0f), 1.0f);
  return (uint32_t)(Scale::root(u) * 255.0f + 0.5f);
}

// lds: MO_PYRAMID_LDS bytes of the workgroup
template <typename TS, typename Scale> __device__ __forceinline__ void mo_pyramid_tile(unsigned char (&lds)[MO_PYRAMID_LDS], const MoPyramidArgs& a, const Scale& scale_of) {
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
      const float scale = scale_of(a);   // (asked where it is used: the plain pyramid's is a kernel argument)
      float top[4], bottom[4];
      const size_t at = (size_t)(2 * I) * (size_t)a.w + (size_t)(2 * J);
      mt_fetch<TS, 4>(src, (int64_t)at, 0, 2 * cells, top);
      mt_fetch<TS, 4>(src, (int64_t)(at + (size_t)a.w), 0, 2 * cells, bottom);
      g[0] = mo_grey<Scale>(top[0], top[1], bottom[0], bottom[1], scale);
      if (cells > 1) g[1] = mo_grey<Scale>(top[2], top[3], bottom[2], bottom[3], scale);
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

// ---- host side: the checks of tdk_motion_pyramid, which tdk_hdralign_pyramid shares, and the arguments
static inline size_t mo_pyramid_bytes(int width, int height, int levels) {
  if (!mt_size_ok(width, height) || !mo_levels_ok(levels)) return 0;
  return 2 * mo_geometry(width, height, levels).slot;
}

static inline int mo_check_pyramid(const char* who, const void* src, int src_dtype, int width, int height, float scale, int levels, void* pyramid,
                                   const uint32_t* index, int which, MoPyramidArgs& a) {
  TDK_REQUIRE(src && pyramid, "%s: null pointer (src or pyramid)", who);
  TDK_REQUIRE(mt_dtype_ok(src_dtype), "%s: unsupported dtype tag %d", who, src_dtype);
  TDK_REQUIRE(tdk_mosaic_size_ok(width, height), "%s: frame size %dx%d outside 2..%d", who, width, height, TDK_MOSAIC_MAX_SIZE);
  TDK_REQUIRE(width % 2 == 0 && height % 2 == 0, "%s: mosaic size %dx%d must be even in both axes (whole CFA cells)", who, width, height);
  TDK_REQUIRE(isfinite(scale) && scale > 0.0f, "%s: scale must be finite and > 0", who);
  TDK_REQUIRE(mo_levels_ok(levels), "%s: levels must be 1..%d, got %d", who, TDK_MOTION_MAX_LEVELS, levels);
  TDK_REQUIRE(which == 0 || which == 1, "%s: which must be 0 or 1, got %d", who, which);
  TDK_REQUIRE(tdk_aligned(pyramid, 16), "%s: pyramid must be aligned to 16 bytes", who);
  TDK_REQUIRE(!index || tdk_aligned(index, 4), "%s: index must be aligned to 4 bytes", who);
  const size_t src_bytes = (size_t)width * (size_t)height * tdk_dtype_bytes(src_dtype);
  TDK_REQUIRE(tdk_disjoint(src, src_bytes, pyramid, mo_pyramid_bytes(width, height, levels)), "%s: src and pyramid overlap", who);
  a.src = src, a.pyramid = reinterpret_cast<unsigned char*>(pyramid), a.index = index, a.which = which, a.levels = levels;
  a.w = width, a.h = height, a.scale = scale, a.g = mo_geometry(width, height, levels);
  return TDK_OK;
}
