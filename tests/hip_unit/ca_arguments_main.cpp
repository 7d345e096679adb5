// Stand-alone host program: every argument error of tdk_ca_correct and tdk_ca_estimate with pointers that are never dereferenced, for a run
// under a host sanitizer (no device is touched: each call returns before any HIP call).  Build, from the repository root:
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -ffp-contract=off -Xarch_host -fsanitize=address \
//     tests/hip_unit/ca_arguments_main.cpp torch-darktable_amd/csrc/cacorrect.hip torch-darktable_amd/csrc/runtime.hip -o ca_arguments
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../../include/tdk_hip_ca.h"

static int failures = 0;

static void expect(int rc, const char* word, const char* what) {
  const char* msg = tdk_last_error();
  if (rc != TDK_ERR_INVALID_ARGUMENT || !msg || !strstr(msg, word)) {
    printf("FAIL %s: rc %d, message '%s' (expected '%s')\n", what, rc, msg ? msg : "(null)", word);
    failures++;
  }
}

int main() {
  const uint32_t RGGB = TDK_PATTERN_RGGB;
  char* const fake = reinterpret_cast<char*>(uintptr_t(1) << 30);
  const int w = 640, h = 480;
  void *src = fake, *out = fake + (1 << 24), *ws = fake + (3 << 24);
  float* model = reinterpret_cast<float*>(fake + (2 << 24));
  const float nan = NAN, inf = INFINITY;

  expect(tdk_ca_correct(nullptr, TDK_F32, out, TDK_F32, w, h, RGGB, model, 1, 1, 1, 0, nullptr), "null pointer", "correct src");
  expect(tdk_ca_correct(src, TDK_F32, nullptr, TDK_F32, w, h, RGGB, model, 1, 1, 1, 0, nullptr), "null pointer", "correct out");
  expect(tdk_ca_correct(src, TDK_F32, out, TDK_F32, w, h, RGGB, nullptr, 1, 1, 1, 0, nullptr), "null pointer", "correct model");
  expect(tdk_ca_correct(src, 2, out, TDK_F32, w, h, RGGB, model, 1, 1, 1, 0, nullptr), "dtype", "correct src_dtype");
  expect(tdk_ca_correct(src, TDK_F32, out, -1, w, h, RGGB, model, 1, 1, 1, 0, nullptr), "dtype", "correct out_dtype");
  expect(tdk_ca_correct(src, TDK_F32, out, TDK_F32, 0, h, RGGB, model, 1, 1, 1, 0, nullptr), "frame size", "correct width");
  expect(tdk_ca_correct(src, TDK_F32, out, TDK_F32, w, 65536, RGGB, model, 1, 1, 1, 0, nullptr), "frame size", "correct height");
  expect(tdk_ca_correct(src, TDK_F32, out, TDK_F32, 641, h, RGGB, model, 1, 1, 1, 0, nullptr), "even", "correct odd width");
  expect(tdk_ca_correct(src, TDK_F32, out, TDK_F32, w, h, 0x1234, model, 1, 1, 1, 0, nullptr), "Bayer pattern", "correct pattern");
  expect(tdk_ca_correct(src, TDK_F32, out, TDK_F32, w, h, RGGB, model, 1, 1, 1, 2, nullptr), "interp", "correct interp");
  expect(tdk_ca_correct(src, TDK_F32, out, TDK_F32, w, h, RGGB, model, nan, 1, 1, 0, nullptr), "centre", "correct x0");
  expect(tdk_ca_correct(src, TDK_F32, out, TDK_F32, w, h, RGGB, model, 1, inf, 1, 0, nullptr), "centre", "correct y0");
  expect(tdk_ca_correct(src, TDK_F32, out, TDK_F32, w, h, RGGB, model, 1, 1, 0, 0, nullptr), "rn", "correct rn");
  expect(tdk_ca_correct(src, TDK_F32, fake + 64, TDK_F32, w, h, RGGB, model, 1, 1, 1, 0, nullptr), "out overlaps src", "correct overlap");
  expect(tdk_ca_correct(src, TDK_F32, out, TDK_F32, w, h, RGGB, reinterpret_cast<float*>(reinterpret_cast<char*>(out) + 16), 1, 1, 1, 0, nullptr), "out overlaps the model",
         "correct model overlap");

  const void* frames[TDK_CA_MAX_FRAMES + 1];
  for (int f = 0; f <= TDK_CA_MAX_FRAMES; f++) frames[f] = fake + (size_t(4 + f) << 24);
  const void* holed[3] = {frames[0], nullptr, frames[2]};
  float* fitted = reinterpret_cast<float*>(fake + (size_t(40) << 24));
  const float* noise = fitted + 64;
  expect(tdk_ca_estimate(nullptr, 3, TDK_F32, w, h, RGGB, noise, 0, 0.95f, 64, 2, 1, 1, 1, ws, fitted, nullptr), "null pointer", "estimate frames");
  expect(tdk_ca_estimate(frames, 3, TDK_F32, w, h, RGGB, noise, 0, 0.95f, 64, 2, 1, 1, 1, nullptr, fitted, nullptr), "null pointer", "estimate workspace");
  expect(tdk_ca_estimate(frames, 3, TDK_F32, w, h, RGGB, noise, 0, 0.95f, 64, 2, 1, 1, 1, ws, nullptr, nullptr), "null pointer", "estimate model");
  expect(tdk_ca_estimate(holed, 3, TDK_F32, w, h, RGGB, noise, 0, 0.95f, 64, 2, 1, 1, 1, ws, fitted, nullptr), "null pointer (frame 1)", "estimate frame 1");
  expect(tdk_ca_estimate(frames, 0, TDK_F32, w, h, RGGB, noise, 0, 0.95f, 64, 2, 1, 1, 1, ws, fitted, nullptr), "num_frames", "estimate no frame");
  expect(tdk_ca_estimate(frames, 17, TDK_F32, w, h, RGGB, noise, 0, 0.95f, 64, 2, 1, 1, 1, ws, fitted, nullptr), "num_frames", "estimate 17 frames");
  expect(tdk_ca_estimate(frames, 3, 3, w, h, RGGB, noise, 0, 0.95f, 64, 2, 1, 1, 1, ws, fitted, nullptr), "dtype", "estimate dtype");
  expect(tdk_ca_estimate(frames, 3, TDK_F32, w, 479, RGGB, noise, 0, 0.95f, 64, 2, 1, 1, 1, ws, fitted, nullptr), "even", "estimate odd height");
  expect(tdk_ca_estimate(frames, 3, TDK_F32, w, h, 0, noise, 0, 0.95f, 64, 2, 1, 1, 1, ws, fitted, nullptr), "Bayer pattern", "estimate pattern");
  expect(tdk_ca_estimate(frames, 3, TDK_F32, w, h, RGGB, noise, 2, 0.95f, 64, 2, 1, 1, 1, ws, fitted, nullptr), "fit", "estimate fit");
  expect(tdk_ca_estimate(frames, 3, TDK_F32, w, h, RGGB, noise, 0, nan, 64, 2, 1, 1, 1, ws, fitted, nullptr), "clip", "estimate clip");
  expect(tdk_ca_estimate(frames, 3, TDK_F32, w, h, RGGB, noise, 0, 0.95f, 15, 2, 1, 1, 1, ws, fitted, nullptr), "block", "estimate block");
  expect(tdk_ca_estimate(frames, 3, TDK_F32, w, h, RGGB, noise, 0, 0.95f, 64, 9, 1, 1, 1, ws, fitted, nullptr), "max_shift", "estimate max_shift");
  expect(tdk_ca_estimate(frames, 3, TDK_F32, w, h, RGGB, noise, 0, 0.95f, 64, 2, nan, 1, 1, ws, fitted, nullptr), "centre", "estimate x0");
  expect(tdk_ca_estimate(frames, 3, TDK_F32, w, h, RGGB, noise, 0, 0.95f, 64, 2, 1, 1, -1, ws, fitted, nullptr), "rn", "estimate rn");
  expect(tdk_ca_estimate(frames, 16, TDK_F32, w, h, RGGB, noise, 0, 0.95f, 64, 2, 1, 1, 1, const_cast<void*>(frames[15]), fitted, nullptr), "overlaps frame 15",
         "estimate workspace in the last frame");
  expect(tdk_ca_estimate(frames, 3, TDK_F32, w, h, RGGB, noise, 0, 0.95f, 64, 2, 1, 1, 1, ws, reinterpret_cast<float*>(ws), nullptr), "workspace and model overlap",
         "estimate model in workspace");
  expect(tdk_ca_estimate(frames, 3, TDK_F32, w, h, RGGB, fitted + 4, 0, 0.95f, 64, 2, 1, 1, 1, ws, fitted, nullptr), "the noise model overlaps", "estimate noise model");
  if (tdk_ca_lds_bytes(0, TDK_F32) != 17472 || tdk_ca_lds_bytes(1, TDK_F16) != 19712 || tdk_ca_lds_bytes(2, TDK_F32) != 0 ||
      tdk_ca_workspace_bytes(640, 480, 64) != size_t(10 * 7 * 2 * 17 * 8) || tdk_ca_workspace_bytes(640, 480, 15) != 0 || tdk_ca_abi_version() != TDK_CA_ABI_VERSION) {
    printf("FAIL queries\n");
    failures++;
  }
  printf("%d failures\n", failures);
  return failures != 0;
}
