// temporal.hip -- the motion-adaptive recursive temporal denoiser on raw mosaics (include/tdk_hip_temporal.h: tdk_temporal_denoise: one
// tile launch and a one-lane launch that advances the frame index; tdk_temporal_reset: a one-lane launch).
//
// The specification is the head comment of include/tdk_hip_temporal.h.
//
// The tile body described below is tt_filter_tile of tdk_temporal_tile.h, which motion.hip runs as well, with the history read at a
// displacement; the arguments and their checks (tt_check) are there too.  Storage helpers, model rows, tile geometry and window sums are
// those of tdk_mosaic_tile.h, which hdrmerge.hip uses as well.  This file keeps the kernels, their launches and the entry points.
//
// Filter, tp_filter<TS, TA, TO, R>: a workgroup of 256 lanes owns an output tile of 32 rows of 64 sites (TtTile<R>).  Every
// workgroup reads the frame index from the head of the state with one uniform load and derives the source and destination planes
// from its parity: nothing on the host knows which plane is which, so a captured call replays any number of times.
//   1. interior: a lane takes eight consecutive sites of one tile row (32 rows x 8 lanes = 256): the sample, the running average
//      and the count, each as 16-byte vectors when its address allows it and per element otherwise and at the frame's right edge.
//      It forms e and v, stores them as float4 into two LDS planes and keeps x, A and N in registers for step 4.
//   2. apron: the R rows above and below and one unit of four sites left and right of the tile, (36 R + 64) units of four
//      sites, one per lane.  Sites outside the frame are staged as +0.0f: no e or v is -0, so adding them leaves every bit of the
//      sums of the specification (which skip them) as it is.
//   3. row sums: a lane reads three float4 of a staged row and writes the four (2R + 1)-term sums of the middle one, every sum
//      from 0.0f in ascending column order, into two more LDS planes.
//   4. column sums: a lane adds the 2R + 1 row sums of each of its eight sites in ascending row order, applies the update and
//      stores the new average, the new count and the output.
// Advance, tp_advance: one lane writes the next index in plain C++.  Reset, tp_reset: one lane writes 0.
#include "tdk_temporal_tile.h"

namespace {

template <typename TS, typename TA, typename TO, int R>
__global__ __launch_bounds__(MT_THREADS, TT_WAVES<R>) void tp_filter(TtArgs a) {
  __shared__ typename TtTile<R>::Lds lds;
  tt_filter_tile<TS, TA, TO, R>(lds, a, TtHistoryInPlace{});
}

__global__ void tp_advance(uint32_t* head) { tt_advance(head); }

__global__ void tp_reset(uint32_t* head) {
  if (threadIdx.x == 0) *head = 0u;
}

template <typename TS, typename TA, typename TO, int R> int tp_launch(const TtArgs& a, hipStream_t st) {
  const dim3 grid((unsigned)tdk_div_up(a.w, TtTile<R>::TW), (unsigned)tdk_div_up(a.h, TtTile<R>::TH)), block(MT_THREADS);
  TDK_LAUNCH("tdk_temporal_denoise(filter)", (tp_filter<TS, TA, TO, R>), grid, block, 0, st, a);
  return TDK_OK;
}

template <typename TS, typename TA, typename TO> int tp_launch_radius(const TtArgs& a, int radius, hipStream_t st) {
  return radius == 2 ? tp_launch<TS, TA, TO, 2>(a, st) : tp_launch<TS, TA, TO, 3>(a, st);
}

}  // namespace

TDK_EXPORT int tdk_temporal_abi_version(void) { return TDK_TEMPORAL_ABI_VERSION; }

TDK_EXPORT size_t tdk_temporal_state_bytes(int width, int height, int state_dtype) {
  if (!mt_size_ok(width, height) || !mt_dtype_ok(state_dtype)) return 0;
  return TDK_TEMPORAL_HEAD_BYTES + 2 * mt_plane_bytes(width, height, tdk_dtype_bytes(state_dtype)) + 2 * mt_plane_bytes(width, height, 2);
}

TDK_EXPORT size_t tdk_temporal_lds_bytes(int radius) { return radius == 2 ? sizeof(TtTile<2>::Lds) : radius == 3 ? sizeof(TtTile<3>::Lds) : 0; }

TDK_EXPORT int tdk_temporal_reset(void* state, tdk_stream_t stream) {
  static const char* const who = "tdk_temporal_reset";
  TDK_REQUIRE(state, "%s: null pointer (state)", who);
  TDK_REQUIRE(tdk_aligned(state, 16), "%s: state must be aligned to 16 bytes", who);
  TDK_LAUNCH("tdk_temporal_reset", tp_reset, dim3(1), dim3(1), 0, tdk_stream(stream), reinterpret_cast<uint32_t*>(state));
  return TDK_OK;
}

TDK_EXPORT int tdk_temporal_denoise(const void* src, int src_dtype, void* out, int out_dtype, void* state, int state_dtype, int width, int height,
                                    uint32_t pattern, const float* model, const float* gains, int radius, float t_lo, float t_hi, float pixel_c2, float n_max,
                                    float v_min, tdk_stream_t stream) {
  static const char* const who = "tdk_temporal_denoise";
  TDK_REQUIRE(src && out && state && model, "%s: null pointer (src, out, state or model)", who);
  TtArgs a{};
  if (const int rc = tt_check(who, src, src_dtype, out, out_dtype, state, state_dtype, width, height, pattern, model, gains, radius, t_lo, t_hi, pixel_c2, n_max,
                              v_min, a))
    return rc;
  hipStream_t st = tdk_stream(stream);
  int rc = TDK_OK;
  TDK_DISPATCH_DTYPE(src_dtype, TS, TDK_DISPATCH_DTYPE(state_dtype, TA, TDK_DISPATCH_DTYPE(out_dtype, TO, rc = tp_launch_radius<TS, TA, TO>(a, radius, st))));
  if (rc != TDK_OK) return rc;
  TDK_LAUNCH("tdk_temporal_denoise(advance)", tp_advance, dim3(1), dim3(1), 0, st, reinterpret_cast<uint32_t*>(state));
  return TDK_OK;
}
