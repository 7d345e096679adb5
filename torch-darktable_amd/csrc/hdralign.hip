// hdralign.hip -- exposure brackets of a moving rig (include/tdk_hip_hdralign.h: tdk_hdralign_pyramid and tdk_hdralign_merge, one
// launch each).  The specification is the head comment of that header.
//
// Both kernels are bodies that exist once in the tree, instantiated here with another policy:
//   ha_pyramid<TS>: mo_pyramid_tile of tdk_motion_pyramid.h (the body of mo_pyramid of motion.hip) with the scale of the grey formula
//     computed from the bracket's exposures on the device (MoScaleOfBracket).
//   ha_merge<TS, TO, R>: hd_merge_tile of tdk_hdr_tile.h (the body of hd_merge of hdrmerge.hip; its steps are listed at the head of
//     that file) with every frame read at a per-workgroup uniform displacement (HdDisplaced).  Step 0 also reads the displacement of
//     every frame at the motion tile the output tile lies in, into LDS of its own behind the merge's; the clip bits, the anchor sample
//     and the per-frame fetch read at the displaced address, and whether the displaced sample is inside the frame is one more term of
//     the clip bit.
#include "../../include/tdk_hip_hdralign.h"
#include "tdk_hdr_tile.h"
#include "tdk_motion_pyramid.h"

namespace {

static_assert(HdDisplaced::TILE_W == TDK_MOTION_TILE_W && HdDisplaced::TILE_H == TDK_MOTION_TILE_H, "the tile of a displacement");

template <int R> struct HaLds {
  HdLds<R> merge;
  int dy[HD_F], dx[HD_F];   // the displacement of every frame at this output tile
};
static_assert(sizeof(HaLds<3>) <= 64 * 1024 && sizeof(HaLds<2>) == sizeof(HdLds<2>) + 64 && sizeof(HaLds<3>) == sizeof(HdLds<3>) + 64, "LDS of the merge launch");

struct HaArgs {
  HdArgs merge;
  const uint32_t* fields;
  int tiles_x, tiles_y;
};

template <typename TS, typename TO, int R>
__global__ __launch_bounds__(MT_THREADS, HD_WAVES) void ha_merge(HaArgs a) {
  __shared__ HaLds<R> lds;
  hd_merge_tile<TS, TO, R>(lds.merge, a.merge, HdDisplaced{lds.dy, lds.dx, a.fields, a.tiles_x, a.tiles_y});
}

struct HaPyramidArgs {
  MoPyramidArgs pyramid;
  const float* exposures;
  int nf, frame;
};

template <typename TS> __global__ __launch_bounds__(MO_THREADS) void ha_pyramid(HaPyramidArgs a) {
  __shared__ unsigned char lds[MO_PYRAMID_LDS];
  mo_pyramid_tile<TS>(lds, a.pyramid, MoScaleOfBracket{a.exposures, a.nf, a.frame});
}

template <typename TS, typename TO, int R> int ha_launch(const HaArgs& a, hipStream_t st) {
  const dim3 grid((unsigned)tdk_div_up(a.merge.w, HdTile<R>::TW), (unsigned)tdk_div_up(a.merge.h, HdTile<R>::TH)), block(MT_THREADS);
  TDK_LAUNCH("tdk_hdralign_merge", (ha_merge<TS, TO, R>), grid, block, 0, st, a);
  return TDK_OK;
}

template <typename TS, typename TO> int ha_launch_radius(const HaArgs& a, int radius, hipStream_t st) {
  return radius == 2 ? ha_launch<TS, TO, 2>(a, st) : ha_launch<TS, TO, 3>(a, st);
}

template <typename TS> int ha_launch_pyramid(const HaPyramidArgs& a, hipStream_t st) {
  const dim3 grid((unsigned)tdk_div_up(a.pyramid.w, TDK_MOTION_TILE_W), (unsigned)tdk_div_up(a.pyramid.h, TDK_MOTION_TILE_H)), block(MO_THREADS);
  TDK_LAUNCH("tdk_hdralign_pyramid", ha_pyramid<TS>, grid, block, 0, st, a);
  return TDK_OK;
}

}  // namespace

TDK_EXPORT int tdk_hdralign_abi_version(void) { return TDK_HDRALIGN_ABI_VERSION; }

TDK_EXPORT size_t tdk_hdralign_lds_bytes(int radius) { return radius == 2 ? sizeof(HaLds<2>) : radius == 3 ? sizeof(HaLds<3>) : 0; }

TDK_EXPORT int tdk_hdralign_pyramid(const void* src, int src_dtype, int width, int height, float scale, int levels, void* pyramid, int which,
                                    const float* exposures, int num_frames, int frame, tdk_stream_t stream) {
  static const char* const who = "tdk_hdralign_pyramid";
  HaPyramidArgs a{};
  if (const int rc = mo_check_pyramid(who, src, src_dtype, width, height, scale, levels, pyramid, nullptr, which, a.pyramid)) return rc;
  TDK_REQUIRE(exposures, "%s: null pointer (exposures)", who);
  TDK_REQUIRE(num_frames >= 2 && num_frames <= HD_F, "%s: num_frames must be 2..%d, got %d", who, HD_F, num_frames);
  TDK_REQUIRE(frame >= 0 && frame < num_frames, "%s: frame must be a frame index below %d, got %d", who, num_frames, frame);
  TDK_REQUIRE(tdk_aligned(exposures, 4), "%s: exposures must be aligned to 4 bytes", who);
  TDK_REQUIRE(tdk_disjoint(exposures, (size_t)num_frames * sizeof(float), pyramid, mo_pyramid_bytes(width, height, levels)), "%s: exposures and pyramid overlap", who);
  a.exposures = exposures, a.nf = num_frames, a.frame = frame;
  hipStream_t st = tdk_stream(stream);
  return src_dtype == TDK_F32 ? ha_launch_pyramid<float>(a, st) : ha_launch_pyramid<__half>(a, st);
}

TDK_EXPORT int tdk_hdralign_merge(const void* const* frames, int num_frames, int src_dtype, void* out, int out_dtype, unsigned char* mask, int width, int height,
                                  uint32_t pattern, const float* exposures, int ref, const float* model, int radius, float clip, float t_lo, float t_hi,
                                  float pixel_c2, float v_min, const int16_t* fields, tdk_stream_t stream) {
  static const char* const who = "tdk_hdralign_merge";
  HaArgs a{};
  if (const int rc = hd_check(who, frames, num_frames, src_dtype, out, out_dtype, mask, width, height, pattern, exposures, ref, 0, model, radius, clip, t_lo, t_hi,
                              pixel_c2, v_min, a.merge))
    return rc;
  TDK_REQUIRE(fields, "%s: null pointer (fields)", who);
  TDK_REQUIRE(tdk_aligned(fields, 4), "%s: fields must be aligned to 4 bytes", who);
  a.tiles_x = tdk_div_up(width, TDK_MOTION_TILE_W), a.tiles_y = tdk_div_up(height, TDK_MOTION_TILE_H);
  const size_t sites = (size_t)width * (size_t)height, out_bytes = sites * tdk_dtype_bytes(out_dtype);
  const size_t field_bytes = (size_t)num_frames * (size_t)a.tiles_x * (size_t)a.tiles_y * 4;
  TDK_REQUIRE(tdk_disjoint(fields, field_bytes, out, out_bytes) && (!mask || tdk_disjoint(fields, field_bytes, mask, sites)), "%s: the fields overlap out or mask", who);
  a.fields = reinterpret_cast<const uint32_t*>(fields);
  hipStream_t st = tdk_stream(stream);
  TDK_DISPATCH_DTYPE(src_dtype, TS, TDK_DISPATCH_DTYPE(out_dtype, TO, return ha_launch_radius<TS, TO>(a, radius, st)));
  return TDK_OK;
}
