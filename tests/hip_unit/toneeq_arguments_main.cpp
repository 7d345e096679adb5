// Stand-alone host program: every argument error of tdk_toneeq with pointers that are never dereferenced (weights is a host array
// and is read), for a run under a host sanitizer (no device is touched: each call returns before any HIP call).  Build, from the
// repository root:
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//     tests/hip_unit/toneeq_arguments_main.cpp torch-darktable_amd/csrc/toneequal.hip torch-darktable_amd/csrc/runtime.hip -o toneeq_arguments
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../../include/tdk_hip_toneeq.h"

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
  const int w = 640, h = 480;
  void *src = fake, *dst = fake + (1 << 24), *ws = fake + (3 << 24);
  float* mask = reinterpret_cast<float*>(fake + (2 << 24));
  const float* table = reinterpret_cast<const float*>(fake + (4 << 24));
  const float rec709[3] = {0.2126f, 0.7152f, 0.0722f};
  const float bad_nan[3] = {0.2f, NAN, 0.1f}, bad_inf[3] = {INFINITY, 0.7f, 0.1f}, bad_neg[3] = {0.2f, 0.7f, -0.1f};
  const size_t frame = size_t(w) * h * 3 * 4, plane = size_t(w) * h * 4;

  expect(tdk_toneeq(nullptr, dst, mask, ws, table, w, h, TDK_F32, 8, 4, 1e-4f, rec709, 0, nullptr), "null pointer (src)", "src");
  expect(tdk_toneeq(src, nullptr, nullptr, ws, table, w, h, TDK_F32, 8, 4, 1e-4f, rec709, 0, nullptr), "null pointer (dst and mask_out", "dst and mask_out");
  expect(tdk_toneeq(src, dst, mask, nullptr, table, w, h, TDK_F32, 8, 4, 1e-4f, rec709, 0, nullptr), "null pointer (workspace)", "workspace");
  expect(tdk_toneeq(src, dst, mask, ws, nullptr, w, h, TDK_F32, 8, 4, 1e-4f, rec709, 0, nullptr), "null pointer (table)", "table");
  expect(tdk_toneeq(src, dst, mask, ws, table, w, h, TDK_F32, 8, 4, 1e-4f, nullptr, 0, nullptr), "null pointer (weights)", "weights");
  expect(tdk_toneeq(src, dst, mask, ws, table, 0, h, TDK_F32, 8, 4, 1e-4f, rec709, 0, nullptr), "frame size", "width 0");
  expect(tdk_toneeq(src, dst, mask, ws, table, w, 65536, TDK_F32, 8, 4, 1e-4f, rec709, 0, nullptr), "frame size", "height 65536");
  expect(tdk_toneeq(src, dst, mask, ws, table, -3, h, TDK_F32, 8, 4, 1e-4f, rec709, 0, nullptr), "frame size", "width -3");
  expect(tdk_toneeq(src, dst, mask, ws, table, w, h, 2, 8, 4, 1e-4f, rec709, 0, nullptr), "dtype", "uint8");
  expect(tdk_toneeq(src, dst, mask, ws, table, w, h, -1, 8, 4, 1e-4f, rec709, 0, nullptr), "dtype", "dtype -1");
  for (int cell : {0, 1, 3, 6, 32, -8}) expect(tdk_toneeq(src, dst, mask, ws, table, w, h, TDK_F32, cell, 4, 1e-4f, rec709, 0, nullptr), "cell must be", "cell");
  for (int radius : {-1, 9, 100}) expect(tdk_toneeq(src, dst, mask, ws, table, w, h, TDK_F32, 8, radius, 1e-4f, rec709, 0, nullptr), "radius must be", "radius");
  for (float eps : {0.0f, -1e-4f, NAN, INFINITY}) expect(tdk_toneeq(src, dst, mask, ws, table, w, h, TDK_F32, 8, 4, eps, rec709, 0, nullptr), "eps must be", "eps");
  expect(tdk_toneeq(src, dst, mask, ws, table, w, h, TDK_F32, 8, 4, 1e-4f, bad_nan, 0, nullptr), "weights[1]", "weights nan");
  expect(tdk_toneeq(src, dst, mask, ws, table, w, h, TDK_F32, 8, 4, 1e-4f, bad_inf, 0, nullptr), "weights[0]", "weights inf");
  expect(tdk_toneeq(src, dst, mask, ws, table, w, h, TDK_F32, 8, 4, 1e-4f, bad_neg, 0, nullptr), "weights[2]", "weights negative");
  expect(tdk_toneeq(src, dst, mask, ws, table, w, h, TDK_F32, 8, 4, 1e-4f, rec709, 1, nullptr), "flags", "flags");
  expect(tdk_toneeq(src, dst, mask, ws, reinterpret_cast<const float*>(fake + (4 << 24) + 2), w, h, TDK_F32, 8, 4, 1e-4f, rec709, 0, nullptr), "table must be aligned", "table alignment");
  expect(tdk_toneeq(src, dst, reinterpret_cast<float*>(fake + (2 << 24) + 1), ws, table, w, h, TDK_F32, 8, 4, 1e-4f, rec709, 0, nullptr), "mask_out must be aligned", "mask alignment");
  expect(tdk_toneeq(src, fake + 64, mask, ws, table, w, h, TDK_F32, 8, 4, 1e-4f, rec709, 0, nullptr), "src and dst overlap", "dst in src");
  expect(tdk_toneeq(src, fake + frame - 4, mask, ws, table, w, h, TDK_F32, 8, 4, 1e-4f, rec709, 0, nullptr), "src and dst overlap", "dst on the last element of src");
  expect(tdk_toneeq(src, fake + frame / 2 - 2, mask, ws, table, w, h, TDK_F16, 8, 4, 1e-4f, rec709, 0, nullptr), "src and dst overlap", "binary16 dst on the last element of src");
  expect(tdk_toneeq(src, dst, reinterpret_cast<float*>(fake + 128), ws, table, w, h, TDK_F32, 8, 4, 1e-4f, rec709, 0, nullptr), "mask_out overlaps", "mask in src");
  expect(tdk_toneeq(src, dst, reinterpret_cast<float*>(fake + (1 << 24) - plane + 4), ws, table, w, h, TDK_F32, 8, 4, 1e-4f, rec709, 0, nullptr), "mask_out overlaps", "mask into dst");
  expect(tdk_toneeq(src, dst, mask, ws, reinterpret_cast<const float*>(fake + (1 << 24) + 16), w, h, TDK_F32, 8, 4, 1e-4f, rec709, 0, nullptr), "the table overlaps", "table in dst");
  expect(tdk_toneeq(src, nullptr, mask, ws, reinterpret_cast<const float*>(fake + (2 << 24) - 8), w, h, TDK_F32, 8, 4, 1e-4f, rec709, 0, nullptr), "the table overlaps", "table into mask");
  expect(tdk_toneeq(src, dst, mask, fake + 16, table, w, h, TDK_F32, 8, 4, 1e-4f, rec709, 0, nullptr), "the workspace overlaps", "workspace in src");
  expect(tdk_toneeq(src, dst, mask, fake + (1 << 24) - 64, table, w, h, TDK_F32, 8, 4, 1e-4f, rec709, 0, nullptr), "the workspace overlaps", "workspace into dst");
  expect(tdk_toneeq(src, dst, mask, fake + (4 << 24) - 100, table, w, h, TDK_F32, 8, 4, 1e-4f, rec709, 0, nullptr), "the workspace overlaps", "workspace into the table");
  expect(tdk_toneeq(src, nullptr, mask, fake + (2 << 24) + 4, table, w, h, TDK_F32, 8, 4, 1e-4f, rec709, 0, nullptr), "the workspace overlaps", "workspace in mask");

  const size_t lds2 = tdk_toneeq_lds_bytes(TDK_F32, 2, 8), lds16 = tdk_toneeq_lds_bytes(TDK_F16, 16, 0);
  if (tdk_toneeq_workspace_bytes(640, 480, 8) != size_t(3 * 80 * 60 * 4 + 16) || tdk_toneeq_workspace_bytes(1, 1, 16) != size_t(3 * 4 + 16) ||
      tdk_toneeq_workspace_bytes(65535, 65535, 2) != size_t(3) * 32768 * 32768 * 4 + 16 || tdk_toneeq_workspace_bytes(640, 480, 3) != 0 ||
      tdk_toneeq_workspace_bytes(0, 480, 8) != 0 || lds2 == 0 || lds2 > 65536 || lds16 == 0 || lds16 > lds2 || tdk_toneeq_lds_bytes(2, 8, 4) != 0 ||
      tdk_toneeq_lds_bytes(TDK_F32, 5, 4) != 0 || tdk_toneeq_lds_bytes(TDK_F32, 8, 9) != 0 || tdk_toneeq_abi_version() != TDK_TONEEQ_ABI_VERSION) {
    printf("FAIL queries\n");
    failures++;
  }
  printf("%d failures\n", failures);
  return failures != 0;
}
