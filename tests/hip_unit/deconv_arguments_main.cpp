// Stand-alone host program: every argument error of tdk_deconv and tdk_deconv_weights with device pointers that are never
// dereferenced (weights and luma are host arrays and are read), and the host queries, for a run under a host sanitizer (no device is
// touched: each call returns before any HIP call).  Build, from the repository root:
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//     tests/hip_unit/deconv_arguments_main.cpp torch-darktable_amd/csrc/deconv.hip torch-darktable_amd/csrc/runtime.hip -o deconv_arguments
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../../include/tdk_hip_deconv.h"

static int failures = 0;

static void expect(int rc, const char* word, const char* what) {
  const char* msg = tdk_last_error();
  if (rc != TDK_ERR_INVALID_ARGUMENT || !msg || !strstr(msg, word) || strncmp(msg, "tdk_deconv", 10) != 0) {
    printf("FAIL %s: rc %d, message '%s' (expected '%s')\n", what, rc, msg ? msg : "(null)", word);
    failures++;
  }
}

int main() {
  char* const fake = reinterpret_cast<char*>(uintptr_t(1) << 30);
  const int w = 640, h = 480;
  void *src = fake, *dst = fake + (1 << 24), *ws = fake + (3 << 24);
  float* m = reinterpret_cast<float*>(fake + (2 << 24));
  float taps[TDK_DECONV_MAX_RADIUS + 1];
  int radius = 0;
  if (tdk_deconv_weights(0.7f, taps, &radius) != TDK_OK || radius != 3 || taps[4] != 0.0f || taps[6] != 0.0f || !(taps[0] > taps[1] && taps[1] > taps[2] && taps[3] > 0.0f)) {
    printf("FAIL tdk_deconv_weights(0.7)\n");
    failures++;
  }
  const float rec709[3] = {0.2126f, 0.7152f, 0.0722f};
  const float luma_nan[3] = {0.2f, NAN, 0.1f}, luma_inf[3] = {INFINITY, 0.7f, 0.1f}, luma_neg[3] = {0.2f, 0.7f, -0.1f};
  const float taps_nan[4] = {0.5f, NAN, 0.1f, 0.0f}, taps_inf[4] = {INFINITY, 0.2f, 0.1f, 0.0f}, taps_neg[4] = {0.5f, 0.2f, 0.1f, -0.01f};
  const size_t frame = size_t(w) * h * 3 * 4, plane = size_t(w) * h * 4;
  auto as_f = [](char* p) { return reinterpret_cast<float*>(p); };
  const int M = TDK_DECONV_MASK;

  // tdk_deconv(src, dst, mask_out, ws, w, h, channels, dtype, weights, radius, iterations, threshold, max_gain, luma, flags, stream)
  expect(tdk_deconv(nullptr, dst, m, ws, w, h, 3, TDK_F32, taps, 3, 8, 0.02f, 4.0f, rec709, M, nullptr), "null pointer (src or dst)", "src");
  expect(tdk_deconv(src, nullptr, m, ws, w, h, 3, TDK_F32, taps, 3, 8, 0.02f, 4.0f, rec709, M, nullptr), "null pointer (src or dst)", "dst");
  expect(tdk_deconv(src, dst, m, ws, w, h, 3, TDK_F32, nullptr, 3, 8, 0.02f, 4.0f, rec709, M, nullptr), "null pointer (weights)", "weights");
  expect(tdk_deconv(src, dst, m, ws, w, h, 3, TDK_F32, taps, 3, 8, 0.02f, 4.0f, nullptr, M, nullptr), "null pointer (luma)", "luma");
  expect(tdk_deconv(src, dst, m, nullptr, w, h, 3, TDK_F32, taps, 3, 8, 0.02f, 4.0f, rec709, M, nullptr), "null pointer (workspace", "workspace");
  expect(tdk_deconv(src, dst, m, ws, 0, h, 3, TDK_F32, taps, 3, 8, 0.02f, 4.0f, rec709, M, nullptr), "frame size", "width 0");
  expect(tdk_deconv(src, dst, m, ws, w, 65536, 3, TDK_F32, taps, 3, 8, 0.02f, 4.0f, rec709, M, nullptr), "frame size", "height 65536");
  expect(tdk_deconv(src, dst, m, ws, -3, h, 3, TDK_F32, taps, 3, 8, 0.02f, 4.0f, rec709, M, nullptr), "frame size", "width -3");
  for (int c : {0, 2, 4, -1}) expect(tdk_deconv(src, dst, m, ws, w, h, c, TDK_F32, taps, 3, 8, 0.02f, 4.0f, rec709, M, nullptr), "channels must be 1 or 3", "channels");
  for (int d : {2, 3, -1}) expect(tdk_deconv(src, dst, m, ws, w, h, 3, d, taps, 3, 8, 0.02f, 4.0f, rec709, M, nullptr), "dtype", "dtype");
  for (int r : {0, -1, 7, 100}) expect(tdk_deconv(src, dst, m, ws, w, h, 3, TDK_F32, taps, r, 8, 0.02f, 4.0f, rec709, M, nullptr), "radius must be 1..6", "radius");
  expect(tdk_deconv(src, dst, m, ws, w, h, 3, TDK_F32, taps_nan, 3, 8, 0.02f, 4.0f, rec709, M, nullptr), "weights[1]", "weights nan");
  expect(tdk_deconv(src, dst, m, ws, w, h, 3, TDK_F32, taps_inf, 3, 8, 0.02f, 4.0f, rec709, M, nullptr), "weights[0]", "weights inf");
  expect(tdk_deconv(src, dst, m, ws, w, h, 3, TDK_F32, taps_neg, 3, 8, 0.02f, 4.0f, rec709, M, nullptr), "weights[3]", "weights negative");
  for (int n : {-1, 51, 1 << 20}) expect(tdk_deconv(src, dst, m, ws, w, h, 3, TDK_F32, taps, 3, n, 0.02f, 4.0f, rec709, M, nullptr), "iterations must be 0..50", "iterations");
  for (float t : {0.0f, -0.02f, NAN, INFINITY}) expect(tdk_deconv(src, dst, m, ws, w, h, 3, TDK_F32, taps, 3, 8, t, 4.0f, rec709, M, nullptr), "threshold must be", "threshold");
  for (float g : {0.99f, 16.5f, 0.0f, NAN, INFINITY}) expect(tdk_deconv(src, dst, m, ws, w, h, 3, TDK_F32, taps, 3, 8, 0.02f, g, rec709, M, nullptr), "max_gain must lie in", "max_gain");
  expect(tdk_deconv(src, dst, m, ws, w, h, 3, TDK_F32, taps, 3, 8, 0.02f, 4.0f, luma_nan, M, nullptr), "luma[1]", "luma nan");
  expect(tdk_deconv(src, dst, m, ws, w, h, 3, TDK_F32, taps, 3, 8, 0.02f, 4.0f, luma_inf, M, nullptr), "luma[0]", "luma inf");
  expect(tdk_deconv(src, dst, m, ws, w, h, 3, TDK_F32, taps, 3, 8, 0.02f, 4.0f, luma_neg, M, nullptr), "luma[2]", "luma negative");
  for (int f : {2, 4, 128, M | 4096, -1}) expect(tdk_deconv(src, dst, m, ws, w, h, 3, TDK_F32, taps, 3, 8, 0.02f, 4.0f, rec709, f, nullptr), "reserved", "reserved flags");
  for (int f : {3, 4, 5, 8, 15}) expect(tdk_deconv(src, dst, m, ws, w, h, 3, TDK_F32, taps, 3, 8, 0.02f, 4.0f, rec709, M | (f << TDK_DECONV_FUSE_SHIFT), nullptr), "fused count", "fused count");
  expect(tdk_deconv(src, dst, as_f(fake + (2 << 24) + 2), ws, w, h, 3, TDK_F32, taps, 3, 8, 0.02f, 4.0f, rec709, M, nullptr), "mask_out must be aligned", "mask_out alignment");
  expect(tdk_deconv(src, fake + 64, m, ws, w, h, 3, TDK_F32, taps, 3, 8, 0.02f, 4.0f, rec709, M, nullptr), "src and dst overlap", "dst in src");
  expect(tdk_deconv(src, fake + frame - 4, m, ws, w, h, 3, TDK_F32, taps, 3, 8, 0.02f, 4.0f, rec709, M, nullptr), "src and dst overlap", "dst on the last element of src");
  expect(tdk_deconv(src, fake + frame / 2 - 2, m, ws, w, h, 3, TDK_F16, taps, 3, 8, 0.02f, 4.0f, rec709, M, nullptr), "src and dst overlap", "binary16 dst on the last element of src");
  expect(tdk_deconv(src, dst, as_f(fake + 128), ws, w, h, 3, TDK_F32, taps, 3, 8, 0.02f, 4.0f, rec709, M, nullptr), "mask_out overlaps", "mask_out in src");
  expect(tdk_deconv(src, dst, as_f(fake + (1 << 24) - plane + 4), ws, w, h, 3, TDK_F32, taps, 3, 8, 0.02f, 4.0f, rec709, M, nullptr), "mask_out overlaps", "mask_out into dst");
  expect(tdk_deconv(src, dst, m, fake + 16, w, h, 3, TDK_F32, taps, 3, 8, 0.02f, 4.0f, rec709, M, nullptr), "the workspace overlaps", "workspace in src");
  expect(tdk_deconv(src, dst, m, fake + (1 << 24) - 64, w, h, 3, TDK_F32, taps, 3, 8, 0.02f, 4.0f, rec709, M, nullptr), "the workspace overlaps", "workspace into dst");
  expect(tdk_deconv(src, dst, m, fake + (2 << 24) + 4, w, h, 3, TDK_F32, taps, 3, 8, 0.02f, 4.0f, rec709, M, nullptr), "the workspace overlaps", "workspace in mask_out");

  // tdk_deconv_weights(sigma, weights, radius)
  for (float s : {0.29f, 2.01f, 0.0f, -1.0f, NAN, INFINITY}) expect(tdk_deconv_weights(s, taps, &radius), "sigma must lie in [0.3, 2]", "sigma");
  expect(tdk_deconv_weights(0.7f, nullptr, &radius), "null pointer", "weights: weights");
  expect(tdk_deconv_weights(0.7f, taps, nullptr), "null pointer", "weights: radius");
  for (float s : {0.3f, 2.0f}) {
    float sum = 0.0f;
    if (tdk_deconv_weights(s, taps, &radius) != TDK_OK || radius != (s < 1.0f ? 1 : 6)) failures++, printf("FAIL weights at sigma %g\n", (double)s);
    for (int k = 1; k <= radius; k++) sum += 2.0f * taps[k];
    if (fabsf(sum + taps[0] - 1.0f) > 1e-6f) failures++, printf("FAIL the taps of sigma %g sum to %g\n", (double)s, (double)(sum + taps[0]));
  }

  const size_t aligned_plane = (plane + 15) / 16 * 16;
  bool ok = tdk_deconv_abi_version() == TDK_DECONV_ABI_VERSION;
  for (int r = 1; r <= TDK_DECONV_MAX_RADIUS; r++) {
    const int f = tdk_deconv_fused_iterations(r);
    ok = ok && (f == 1 || f == 2 || f == 4) && f <= TDK_DECONV_MAX_FUSED;
    ok = ok && tdk_deconv_workspace_bytes(w, h, r, 0) == 0 && tdk_deconv_workspace_bytes(w, h, r, f) == 0;
    ok = ok && tdk_deconv_workspace_bytes(w, h, r, f + 1) == aligned_plane + 16 && tdk_deconv_workspace_bytes(w, h, r, 2 * f + 1) == 2 * aligned_plane + 16;
    ok = ok && tdk_deconv_workspace_bytes(w, h, r, TDK_DECONV_MAX_ITERATIONS) == 2 * aligned_plane + 16;
    const size_t lds = tdk_deconv_lds_bytes(3, TDK_F32, r, M);
    ok = ok && lds > 0 && lds <= 65536 && lds == tdk_deconv_lds_bytes(1, TDK_F16, r, f << TDK_DECONV_FUSE_SHIFT);
  }
  ok = ok && tdk_deconv_fused_iterations(0) == 0 && tdk_deconv_fused_iterations(7) == 0;
  ok = ok && tdk_deconv_workspace_bytes(0, h, 3, 8) == 0 && tdk_deconv_workspace_bytes(w, 65536, 3, 8) == 0 && tdk_deconv_workspace_bytes(w, h, 7, 8) == 0 &&
       tdk_deconv_workspace_bytes(w, h, 3, 51) == 0 && tdk_deconv_workspace_bytes(w, h, 3, -1) == 0;
  ok = ok && tdk_deconv_lds_bytes(2, TDK_F32, 3, 0) == 0 && tdk_deconv_lds_bytes(3, 2, 3, 0) == 0 && tdk_deconv_lds_bytes(3, TDK_F32, 7, 0) == 0 &&
       tdk_deconv_lds_bytes(3, TDK_F32, 3, 2) == 0 && tdk_deconv_lds_bytes(3, TDK_F32, 3, 4 << TDK_DECONV_FUSE_SHIFT) == 0;
  if (!ok) {
    printf("FAIL queries\n");
    failures++;
  }
  printf("%d failures\n", failures);
  return failures != 0;
}
