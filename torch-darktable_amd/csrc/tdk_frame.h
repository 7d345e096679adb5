// tdk_frame.h -- host-side argument helpers of the stand-alone frame operators (resample, warp, sharpen, nlmeans, rawprepare):
// frames of TDK_F32 | TDK_F16 | TDK_U8 elements, 1 or 3 interleaved channels.  The helpers answer a question; the message of a
// failed check stays with the entry point that reports it.
#pragma once

#include "../../include/tdk_hip_resample.h"   // TDK_U8
#include "tdk_common.h"

static inline size_t tdk_dtype_bytes(int dtype) { return dtype == TDK_F32 ? 4 : dtype == TDK_F16 ? 2 : 1; }

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
