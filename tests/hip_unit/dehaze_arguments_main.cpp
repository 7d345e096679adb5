// Stand-alone host program: every argument error of tdk_dehaze and tdk_dehaze_ambient with pointers that are never dereferenced
// (weights is a host array and is read), for a run under a host sanitizer (no device is touched: each call returns before any HIP
// call).  Build, from the repository root:
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//     tests/hip_unit/dehaze_arguments_main.cpp torch-darktable_amd/csrc/dehaze.hip torch-darktable_amd/csrc/runtime.hip -o dehaze_arguments
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../../include/tdk_hip_dehaze.h"

static int failures = 0;

static void expect(int rc, const char* word, const char* what) {
  const char* msg = tdk_last_error();
  if (rc != TDK_ERR_INVALID_ARGUMENT || !msg || !strstr(msg, word)) {
    printf("FAIL %s: rc %d, message '%s' (expected '%s')\n", what, rc, msg ? msg : "(null)", word);
    failures++;
  }
}

int main() {
  char* const fake = reinterpret_cast<char*>(uintptr_t(1) << 30);
  const int w = 640, h = 480, cells = 80 * 60;
  void *src = fake, *dst = fake + (1 << 24), *ws = fake + (3 << 24);
  float* t = reinterpret_cast<float*>(fake + (2 << 24));
  float* amb = reinterpret_cast<float*>(fake + (4 << 24));
  const float rec709[3] = {0.2126f, 0.7152f, 0.0722f};
  const float bad_nan[3] = {0.2f, NAN, 0.1f}, bad_inf[3] = {INFINITY, 0.7f, 0.1f}, bad_neg[3] = {0.2f, 0.7f, -0.1f};
  const size_t frame = size_t(w) * h * 3 * 4, plane = size_t(w) * h * 4;
  auto as_f = [](char* p) { return reinterpret_cast<float*>(p); };

  // tdk_dehaze(src, dst, t, ws, amb, w, h, dtype, cell, rd, rg, count, eps, strength, floor, weights, flags, stream)
  expect(tdk_dehaze(nullptr, dst, t, ws, amb, w, h, TDK_F32, 8, 1, 4, 48, 1e-3f, 0.9f, 0.1f, rec709, 0, nullptr), "null pointer (src)", "src");
  expect(tdk_dehaze(src, nullptr, nullptr, ws, amb, w, h, TDK_F32, 8, 1, 4, 48, 1e-3f, 0.9f, 0.1f, rec709, 0, nullptr), "null pointer (dst and transmission_out", "dst and t");
  expect(tdk_dehaze(src, dst, t, nullptr, amb, w, h, TDK_F32, 8, 1, 4, 48, 1e-3f, 0.9f, 0.1f, rec709, 0, nullptr), "null pointer (workspace)", "workspace");
  expect(tdk_dehaze(src, dst, t, ws, nullptr, w, h, TDK_F32, 8, 1, 4, 48, 1e-3f, 0.9f, 0.1f, rec709, 0, nullptr), "null pointer (ambient)", "ambient");
  expect(tdk_dehaze(src, dst, t, ws, amb, w, h, TDK_F32, 8, 1, 4, 48, 1e-3f, 0.9f, 0.1f, nullptr, 0, nullptr), "null pointer (weights)", "weights");
  expect(tdk_dehaze(src, dst, t, ws, amb, 0, h, TDK_F32, 8, 1, 4, 48, 1e-3f, 0.9f, 0.1f, rec709, 0, nullptr), "frame size", "width 0");
  expect(tdk_dehaze(src, dst, t, ws, amb, w, 65536, TDK_F32, 8, 1, 4, 48, 1e-3f, 0.9f, 0.1f, rec709, 0, nullptr), "frame size", "height 65536");
  expect(tdk_dehaze(src, dst, t, ws, amb, -3, h, TDK_F32, 8, 1, 4, 48, 1e-3f, 0.9f, 0.1f, rec709, 0, nullptr), "frame size", "width -3");
  expect(tdk_dehaze(src, dst, t, ws, amb, 65535, 65535, TDK_F32, 2, 1, 4, 48, 1e-3f, 0.9f, 0.1f, rec709, 0, nullptr), "cells is larger than", "grid too large");
  expect(tdk_dehaze(src, dst, t, ws, amb, w, h, 2, 8, 1, 4, 48, 1e-3f, 0.9f, 0.1f, rec709, 0, nullptr), "dtype", "uint8");
  expect(tdk_dehaze(src, dst, t, ws, amb, w, h, -1, 8, 1, 4, 48, 1e-3f, 0.9f, 0.1f, rec709, 0, nullptr), "dtype", "dtype -1");
  for (int cell : {0, 1, 3, 6, 32, -8}) expect(tdk_dehaze(src, dst, t, ws, amb, w, h, TDK_F32, cell, 1, 4, 1, 1e-3f, 0.9f, 0.1f, rec709, 0, nullptr), "cell must be", "cell");
  for (int rd : {-1, 5, 100}) expect(tdk_dehaze(src, dst, t, ws, amb, w, h, TDK_F32, 8, rd, 4, 48, 1e-3f, 0.9f, 0.1f, rec709, 0, nullptr), "dark_radius must be", "dark_radius");
  for (int rg : {-1, 9, 100}) expect(tdk_dehaze(src, dst, t, ws, amb, w, h, TDK_F32, 8, 1, rg, 48, 1e-3f, 0.9f, 0.1f, rec709, 0, nullptr), " radius must be", "radius");
  for (int count : {-1, cells + 1}) expect(tdk_dehaze(src, dst, t, ws, amb, w, h, TDK_F32, 8, 1, 4, count, 1e-3f, 0.9f, 0.1f, rec709, 0, nullptr), "count must be 0..4800", "count");
  for (float eps : {0.0f, -1e-4f, NAN, INFINITY}) expect(tdk_dehaze(src, dst, t, ws, amb, w, h, TDK_F32, 8, 1, 4, 48, eps, 0.9f, 0.1f, rec709, 0, nullptr), "eps must be", "eps");
  for (float s : {-0.1f, 1.5f, NAN, INFINITY}) expect(tdk_dehaze(src, dst, t, ws, amb, w, h, TDK_F32, 8, 1, 4, 48, 1e-3f, s, 0.1f, rec709, 0, nullptr), "strength must be", "strength");
  for (float f : {0.0f, 0.015f, 1.01f, NAN, -1.0f}) expect(tdk_dehaze(src, dst, t, ws, amb, w, h, TDK_F32, 8, 1, 4, 48, 1e-3f, 0.9f, f, rec709, 0, nullptr), "floor must be", "floor");
  expect(tdk_dehaze(src, dst, t, ws, amb, w, h, TDK_F32, 8, 1, 4, 48, 1e-3f, 0.9f, 0.1f, bad_nan, 0, nullptr), "weights[1]", "weights nan");
  expect(tdk_dehaze(src, dst, t, ws, amb, w, h, TDK_F32, 8, 1, 4, 48, 1e-3f, 0.9f, 0.1f, bad_inf, 0, nullptr), "weights[0]", "weights inf");
  expect(tdk_dehaze(src, dst, t, ws, amb, w, h, TDK_F32, 8, 1, 4, 48, 1e-3f, 0.9f, 0.1f, bad_neg, 0, nullptr), "weights[2]", "weights negative");
  expect(tdk_dehaze(src, dst, t, ws, amb, w, h, TDK_F32, 8, 1, 4, 48, 1e-3f, 0.9f, 0.1f, rec709, 1, nullptr), "flags", "flags");
  expect(tdk_dehaze(src, dst, t, ws, as_f(fake + (4 << 24) + 2), w, h, TDK_F32, 8, 1, 4, 48, 1e-3f, 0.9f, 0.1f, rec709, 0, nullptr), "ambient must be aligned", "ambient alignment");
  expect(tdk_dehaze(src, dst, as_f(fake + (2 << 24) + 1), ws, amb, w, h, TDK_F32, 8, 1, 4, 48, 1e-3f, 0.9f, 0.1f, rec709, 0, nullptr), "transmission_out must be aligned", "t alignment");
  expect(tdk_dehaze(src, fake + 64, t, ws, amb, w, h, TDK_F32, 8, 1, 4, 48, 1e-3f, 0.9f, 0.1f, rec709, 0, nullptr), "src and dst overlap", "dst in src");
  expect(tdk_dehaze(src, fake + frame - 4, t, ws, amb, w, h, TDK_F32, 8, 1, 4, 48, 1e-3f, 0.9f, 0.1f, rec709, 0, nullptr), "src and dst overlap", "dst on the last element of src");
  expect(tdk_dehaze(src, fake + frame / 2 - 2, t, ws, amb, w, h, TDK_F16, 8, 1, 4, 48, 1e-3f, 0.9f, 0.1f, rec709, 0, nullptr), "src and dst overlap", "binary16 dst on the last element of src");
  expect(tdk_dehaze(src, dst, as_f(fake + 128), ws, amb, w, h, TDK_F32, 8, 1, 4, 48, 1e-3f, 0.9f, 0.1f, rec709, 0, nullptr), "transmission_out overlaps", "t in src");
  expect(tdk_dehaze(src, dst, as_f(fake + (1 << 24) - plane + 4), ws, amb, w, h, TDK_F32, 8, 1, 4, 48, 1e-3f, 0.9f, 0.1f, rec709, 0, nullptr), "transmission_out overlaps", "t into dst");
  expect(tdk_dehaze(src, dst, t, ws, as_f(fake + 16), w, h, TDK_F32, 8, 1, 4, 48, 1e-3f, 0.9f, 0.1f, rec709, 0, nullptr), "ambient overlaps", "ambient in src");
  expect(tdk_dehaze(src, dst, t, ws, as_f(fake + (1 << 24) + 16), w, h, TDK_F32, 8, 1, 4, 0, 1e-3f, 0.9f, 0.1f, rec709, 0, nullptr), "ambient overlaps", "ambient in dst");
  expect(tdk_dehaze(src, nullptr, t, ws, as_f(fake + (2 << 24) - 8), w, h, TDK_F32, 8, 1, 4, 48, 1e-3f, 0.9f, 0.1f, rec709, 0, nullptr), "ambient overlaps", "ambient into t");
  expect(tdk_dehaze(src, dst, t, fake + 16, amb, w, h, TDK_F32, 8, 1, 4, 48, 1e-3f, 0.9f, 0.1f, rec709, 0, nullptr), "the workspace overlaps", "workspace in src");
  expect(tdk_dehaze(src, dst, t, fake + (1 << 24) - 64, amb, w, h, TDK_F32, 8, 1, 4, 48, 1e-3f, 0.9f, 0.1f, rec709, 0, nullptr), "the workspace overlaps", "workspace into dst");
  expect(tdk_dehaze(src, dst, t, fake + (4 << 24) - 100, amb, w, h, TDK_F32, 8, 1, 4, 48, 1e-3f, 0.9f, 0.1f, rec709, 0, nullptr), "the workspace overlaps", "workspace into ambient");
  expect(tdk_dehaze(src, nullptr, t, fake + (2 << 24) + 4, amb, w, h, TDK_F32, 8, 1, 4, 48, 1e-3f, 0.9f, 0.1f, rec709, 0, nullptr), "the workspace overlaps", "workspace in t");

  // tdk_dehaze_ambient(src, amb, ws, w, h, dtype, cell, rd, count, flags, stream)
  expect(tdk_dehaze_ambient(nullptr, amb, ws, w, h, TDK_F32, 8, 1, 48, 0, nullptr), "null pointer (src)", "ambient: src");
  expect(tdk_dehaze_ambient(src, nullptr, ws, w, h, TDK_F32, 8, 1, 48, 0, nullptr), "null pointer (ambient)", "ambient: ambient");
  expect(tdk_dehaze_ambient(src, amb, nullptr, w, h, TDK_F32, 8, 1, 48, 0, nullptr), "null pointer (workspace)", "ambient: workspace");
  expect(tdk_dehaze_ambient(src, amb, ws, w, 0, TDK_F32, 8, 1, 48, 0, nullptr), "frame size", "ambient: height 0");
  expect(tdk_dehaze_ambient(src, amb, ws, 65535, 65535, TDK_F16, 2, 1, 48, 0, nullptr), "cells is larger than", "ambient: grid too large");
  expect(tdk_dehaze_ambient(src, amb, ws, w, h, 2, 8, 1, 48, 0, nullptr), "dtype", "ambient: uint8");
  expect(tdk_dehaze_ambient(src, amb, ws, w, h, TDK_F32, 5, 1, 48, 0, nullptr), "cell must be", "ambient: cell");
  expect(tdk_dehaze_ambient(src, amb, ws, w, h, TDK_F32, 8, 5, 48, 0, nullptr), "dark_radius must be", "ambient: dark_radius");
  for (int count : {0, -1, cells + 1}) expect(tdk_dehaze_ambient(src, amb, ws, w, h, TDK_F32, 8, 1, count, 0, nullptr), "count must be 1..4800", "ambient: count");
  expect(tdk_dehaze_ambient(src, amb, ws, w, h, TDK_F32, 8, 1, 48, 2, nullptr), "flags", "ambient: flags");
  expect(tdk_dehaze_ambient(src, as_f(fake + (4 << 24) + 1), ws, w, h, TDK_F32, 8, 1, 48, 0, nullptr), "ambient must be aligned", "ambient: alignment");
  expect(tdk_dehaze_ambient(src, as_f(fake + frame - 4), ws, w, h, TDK_F32, 8, 1, 48, 0, nullptr), "ambient overlaps src", "ambient: ambient in src");
  expect(tdk_dehaze_ambient(src, amb, fake + 16, w, h, TDK_F32, 8, 1, 48, 0, nullptr), "the workspace overlaps", "ambient: workspace in src");
  expect(tdk_dehaze_ambient(src, amb, fake + (4 << 24) - 100, w, h, TDK_F32, 8, 1, 48, 0, nullptr), "the workspace overlaps", "ambient: workspace into ambient");

  const size_t lds2 = tdk_dehaze_lds_bytes(TDK_F32, 2, 4, 8), lds16 = tdk_dehaze_lds_bytes(TDK_F16, 16, 0, 0);
  if (tdk_dehaze_workspace_bytes(640, 480, 8) != size_t(TDK_DEHAZE_PLANES * 80 * 60 * 4 + 16) || tdk_dehaze_workspace_bytes(1, 1, 16) != size_t(TDK_DEHAZE_PLANES * 4 + 16) ||
      tdk_dehaze_workspace_bytes(65535, 65535, 16) != size_t(TDK_DEHAZE_PLANES) * 4096 * 4096 * 4 + 16 || tdk_dehaze_workspace_bytes(65535, 65535, 8) != 0 ||
      tdk_dehaze_workspace_bytes(640, 480, 3) != 0 || tdk_dehaze_workspace_bytes(0, 480, 8) != 0 || lds2 == 0 || lds2 > 65536 || lds16 == 0 || lds16 > lds2 ||
      tdk_dehaze_lds_bytes(2, 8, 1, 4) != 0 || tdk_dehaze_lds_bytes(TDK_F32, 5, 1, 4) != 0 || tdk_dehaze_lds_bytes(TDK_F32, 8, 5, 4) != 0 ||
      tdk_dehaze_lds_bytes(TDK_F32, 8, 1, 9) != 0 || tdk_dehaze_abi_version() != TDK_DEHAZE_ABI_VERSION) {
    printf("FAIL queries\n");
    failures++;
  }
  printf("%d failures\n", failures);
  return failures != 0;
}
