// hdrmerge.hip -- the noise-weighted merge of an exposure bracket of raw mosaics (include/tdk_hip_hdr.h: tdk_hdr_merge, one tile launch).
//
// The specification is the head comment of include/tdk_hip_hdr.h.  The storage helpers, the rows of the noise model, the tile geometry
// with its apron mapping and staged LDS planes, the column sums and the threshold step are those of the temporal filters:
// tdk_mosaic_tile.h, with a tile of 32 x 32 sites and four sites per lane.  The row sums are that header's too, but written out in the
// frame loop (the reason stands there).  Steps 0 to 2 and 4 and the arithmetic of a site in a frame are the merge's own; the body, its
// arguments and the checks of the entry point stand in tdk_hdr_tile.h, which hdralign.hip instantiates a second time with every frame read
// at a displacement.
//
// hd_merge<TS, TO, R>: a workgroup of 256 lanes owns an output tile of 32 rows of 32 sites (HdTile<R>).  A lane takes four
// consecutive sites of one tile row (the interior) and, the first 20 R + 64 lanes, one unit of four sites of the apron: the R rows above
// and below and one unit left and right of the tile.  What a lane knows about its sites stays in its registers through the frame loop.
//   0. every lane finds the shortest and the longest exposure; F lanes write the ratios k_f and one lane the frame addresses into LDS,
//      where a lane can index them with the anchor of a site.
//   1. clip bits: bit f of a byte per site, on the tile and an apron of R + 1 sites, units of four sites round-robin over the lanes
//      (the first read of the frames; the loads of a frame go to addresses clamped into the frame and are all in flight together).
//      Sites outside the frame have no bit set.
//   2. anchors: per interior and apron site the OR of the 3 x 3 clip bytes, the anchor frame g, R = x_g / k_g (one more sample, from the
//      frame the site chose) and u_g.
//   3. per frame f: the lane stages eps and v of its sites (the third read of the frames; a site outside the frame, saturated in f,
//      blown or anchored on f is staged as +0.0f), row sums, column sums, then the weight of f at the four interior sites goes into
//      num and den.
//   4. out = num / den or R, and the mask byte.
#include "tdk_hdr_tile.h"

namespace {

template <typename TS, typename TO, int R>
__global__ __launch_bounds__(MT_THREADS, HD_WAVES) void hd_merge(HdArgs a) {
  __shared__ HdLds<R> lds;
  hd_merge_tile<TS, TO, R>(lds, a, HdInPlace{});
}

template <typename TS, typename TO, int R> int hd_launch(const HdArgs& a, hipStream_t st) {
  const dim3 grid((unsigned)tdk_div_up(a.w, HdTile<R>::TW), (unsigned)tdk_div_up(a.h, HdTile<R>::TH)), block(MT_THREADS);
  TDK_LAUNCH("tdk_hdr_merge", (hd_merge<TS, TO, R>), grid, block, 0, st, a);
  return TDK_OK;
}

template <typename TS, typename TO> int hd_launch_radius(const HdArgs& a, int radius, hipStream_t st) {
  return radius == 2 ? hd_launch<TS, TO, 2>(a, st) : hd_launch<TS, TO, 3>(a, st);
}

}  // namespace

TDK_EXPORT int tdk_hdr_abi_version(void) { return TDK_HDR_ABI_VERSION; }

TDK_EXPORT size_t tdk_hdr_lds_bytes(int radius) { return radius == 2 ? sizeof(HdLds<2>) : radius == 3 ? sizeof(HdLds<3>) : 0; }

TDK_EXPORT int tdk_hdr_merge(const void* const* frames, int num_frames, int src_dtype, void* out, int out_dtype, unsigned char* mask, int width, int height,
                             uint32_t pattern, const float* exposures, int ref, const float* model, int radius, float clip, float t_lo, float t_hi,
                             float pixel_c2, float v_min, tdk_stream_t stream) {
  HdArgs a{};
  if (const int rc = hd_check("tdk_hdr_merge", frames, num_frames, src_dtype, out, out_dtype, mask, width, height, pattern, exposures, ref, -1, model, radius, clip,
                              t_lo, t_hi, pixel_c2, v_min, a))
    return rc;
  hipStream_t st = tdk_stream(stream);
  TDK_DISPATCH_DTYPE(src_dtype, TS, TDK_DISPATCH_DTYPE(out_dtype, TO, return hd_launch_radius<TS, TO>(a, radius, st)));
  return TDK_OK;
}
