// tdk_frame.h -- host-side argument helpers of the frame operators: resample, warp, sharpen, nlmeans, rawprepare on frames of TDK_F32 |
// TDK_F16 | TDK_U8 elements with 1 or 3 interleaved channels, and the stages bound to one frame size (toneequal, dehaze, filmic, deconv,
// lmmse, defringe) on TDK_F32 | TDK_F16.  The helpers answer a question; the message of a failed check stays with the entry point
// that reports it.  The one exception is tdk_gaussian_taps, the whole body of the three tdk_*_weights entry points.  The stages on raw
// (H, W) mosaics (rawprepare, highlights, cacorrect, noiseprofile, framestats and the tile kernels of tdk_mosaic_tile.h) ask for a
// pattern and a mosaic size here.
#pragma once

#include "../../include/tdk_hip_resample.h"   // TDK_U8
#include "tdk_common.h"

#include <math.h>

constexpr int TDK_FRAME_MAX_SIZE = 65535;   // the largest width and height of a frame

static inline bool tdk_frame_size_ok(int width, int height) { return width >= 1 && height >= 1 && width <= TDK_FRAME_MAX_SIZE && height <= TDK_FRAME_MAX_SIZE; }
constexpr int TDK_MOSAIC_MAX_SIZE = TDK_FRAME_MAX_SIZE;   // of a raw mosaic, whose smallest side is one CFA cell

static inline bool tdk_mosaic_size_ok(int width, int height) { return width >= 2 && height >= 2 && width <= TDK_MOSAIC_MAX_SIZE && height <= TDK_MOSAIC_MAX_SIZE; }
static inline bool tdk_pattern_ok(uint32_t pattern) {
  return pattern == TDK_PATTERN_RGGB || pattern == TDK_PATTERN_BGGR || pattern == TDK_PATTERN_GRBG || pattern == TDK_PATTERN_GBRG;
}
static inline bool tdk_float_dtype_ok(int dtype) { return dtype == TDK_F32 || dtype == TDK_F16; }
static inline size_t tdk_dtype_bytes(int dtype) { return dtype == TDK_F32 ? 4 : dtype == TDK_F16 ? 2 : 1; }

// index of the first of n weights (blur taps, luminance weights) that is not finite or is below 0; -1: none
static inline int tdk_first_bad_weight(const float* w, int n) {
  for (int k = 0; k < n; k++)
    if (!(isfinite(w[k]) && w[k] >= 0.0f)) return k;
  return -1;
}

// true: a thread's four adjacent pixels can go as whole vectors of `bytes` bytes: rows hold whole groups of four and start on the
// vector's alignment
static inline bool tdk_vec4_ok(int width, const void* ptr, size_t bytes) { return width % 4 == 0 && tdk_aligned(ptr, bytes); }

// The taps of a Gaussian of `sigma` in [lo, hi], cut at R = ceil(3 sigma) and normalised to w0 + 2 (w1 + .. + wR) = 1 in float64:
// weights[0 .. max_radius] (zeros behind R) and *radius = R.  An entry point's hi keeps R <= max_radius <= TDK_TAPS_MAX_RADIUS.
constexpr int TDK_TAPS_MAX_RADIUS = 12;
static inline int tdk_gaussian_taps(const char* who, float sigma, float lo, float hi, int max_radius, float* weights, int* radius) {
  TDK_REQUIRE(weights && radius, "%s: null pointer", who);
  TDK_REQUIRE(sigma >= lo && sigma <= hi, "%s: sigma must lie in [%g, %g]", who, (double)lo, (double)hi);
  const double s = (double)sigma;
  const int R = (int)ceil(3.0 * s);
  TDK_REQUIRE(R <= max_radius && max_radius <= TDK_TAPS_MAX_RADIUS, "%s: radius %d beyond the %d taps of the call", who, R, max_radius);
  double w[TDK_TAPS_MAX_RADIUS + 1] = {1.0}, tail = 0.0;
  for (int k = 1; k <= R; k++) {
    w[k] = exp(-(double)(k * k) / (2.0 * s * s));
    tail += w[k];
  }
  const double norm = w[0] + 2.0 * tail;
  for (int k = 0; k <= max_radius; k++) weights[k] = k <= R ? (float)(w[k] / norm) : 0.0f;
  *radius = R;
  return TDK_OK;
}

// true: the byte ranges [p, p + pn) and [q, q + qn) share nothing
static inline bool tdk_disjoint(const void* p, size_t pn, const void* q, size_t qn) {
  const char *a = reinterpret_cast<const char*>(p), *b = reinterpret_cast<const char*>(q);
  return a + pn <= b || b + qn <= a;
}

// Run a statement with the storage type T and the channel count C of a (dtype, channels) pair that the caller has checked:
// anything but TDK_F32 and TDK_F16 is TDK_U8, anything but 1 channel is 3.
#define TDK_DISPATCH_CHANNELS_(channels, C, ...)                                                         \
  do {                                                                                                   \
    if ((channels) == 1) { constexpr int C = 1; __VA_ARGS__; }                                           \
    else { constexpr int C = 3; __VA_ARGS__; }                                                           \
  } while (0)
#define TDK_DISPATCH_FRAME(dtype, channels, T, C, ...)                                                   \
  do {                                                                                                   \
    if ((dtype) == TDK_F32) { using T = float; TDK_DISPATCH_CHANNELS_(channels, C, __VA_ARGS__); }       \
    else if ((dtype) == TDK_F16) { using T = __half; TDK_DISPATCH_CHANNELS_(channels, C, __VA_ARGS__); } \
    else { using T = uint8_t; TDK_DISPATCH_CHANNELS_(channels, C, __VA_ARGS__); }                        \
  } while (0)
