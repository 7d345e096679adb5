// Stand-alone host program: every argument error of tdk_lmmse with device pointers that are never dereferenced, and the host
// queries, for a run under a host sanitizer (no device is touched: each call returns before any HIP call).  Build, from the
// repository root:
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//     tests/hip_unit/lmmse_arguments_main.cpp torch-darktable_amd/csrc/lmmse.hip torch-darktable_amd/csrc/runtime.hip -o lmmse_arguments
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../../include/tdk_hip_lmmse.h"

static int failures = 0;

static void expect(int rc, const char* word, const char* what) {
  const char* msg = tdk_last_error();
  if (rc != TDK_ERR_INVALID_ARGUMENT || !msg || !strstr(msg, word) || strncmp(msg, "tdk_lmmse:", 10) != 0) {
    printf("FAIL %s: rc %d, message '%s' (expected '%s')\n", what, rc, msg ? msg : "(null)", word);
    failures++;
  }
}

int main() {
  char* const fake = reinterpret_cast<char*>(uintptr_t(1) << 30);
  const int w = 640, h = 480;
  void *src = fake, *dst = fake + (1 << 24);
  const uint32_t P = TDK_PATTERN_RGGB;
  const size_t plane = size_t(w) * h * 4, frame = 3 * plane;

  // tdk_lmmse(src, dst, width, height, pattern, src_dtype, dst_dtype, flags, stream)
  expect(tdk_lmmse(nullptr, dst, w, h, P, TDK_F32, TDK_F32, 0, nullptr), "null pointer (src or dst)", "src");
  expect(tdk_lmmse(src, nullptr, w, h, P, TDK_F32, TDK_F32, 0, nullptr), "null pointer (src or dst)", "dst");
  for (int v : {1, 0, -3, 65536}) {
    expect(tdk_lmmse(src, dst, v, h, P, TDK_F32, TDK_F32, 0, nullptr), "frame size", "width");
    expect(tdk_lmmse(src, dst, w, v, P, TDK_F32, TDK_F32, 0, nullptr), "frame size", "height");
  }
  for (uint32_t p : {0u, 1u, 0x94949495u, 0x94941616u, 0xffffffffu, 0x55555555u})
    expect(tdk_lmmse(src, dst, w, h, p, TDK_F32, TDK_F32, 0, nullptr), "none of the four Bayer patterns", "pattern");
  for (int d : {2, 3, -1}) {
    expect(tdk_lmmse(src, dst, w, h, P, d, TDK_F32, 0, nullptr), "(src)", "src dtype");
    expect(tdk_lmmse(src, dst, w, h, P, TDK_F16, d, 0, nullptr), "(dst)", "dst dtype");
  }
  for (int f : {2, 3, 4, 256, -1, 1 << 30}) expect(tdk_lmmse(src, dst, w, h, P, TDK_F32, TDK_F32, f, nullptr), "reserved", "reserved flags");
  // overlap, in bytes of the two dtypes: src is one plane, dst three
  expect(tdk_lmmse(src, src, w, h, P, TDK_F32, TDK_F32, 0, nullptr), "src and dst overlap", "dst == src");
  expect(tdk_lmmse(src, fake + plane - 4, w, h, P, TDK_F32, TDK_F32, TDK_LMMSE_LINEAR, nullptr), "src and dst overlap", "dst on the last element of src");
  expect(tdk_lmmse(src, fake + plane / 2 - 2, w, h, P, TDK_F16, TDK_F32, 0, nullptr), "src and dst overlap", "dst on the last element of a binary16 src");
  expect(tdk_lmmse(src, fake - frame + 4, w, h, P, TDK_F32, TDK_F32, 0, nullptr), "src and dst overlap", "the last element of dst on src");
  expect(tdk_lmmse(src, fake - frame / 2 + 2, w, h, P, TDK_F32, TDK_F16, 0, nullptr), "src and dst overlap", "the last element of a binary16 dst on src");

  bool ok = tdk_lmmse_abi_version() == TDK_LMMSE_ABI_VERSION;
  const size_t lds = tdk_lmmse_lds_bytes(TDK_F32, TDK_F32, 0);
  ok = ok && lds > 0 && lds <= 65536;
  for (int s : {TDK_F32, TDK_F16})
    for (int d : {TDK_F32, TDK_F16})
      for (int f : {0, TDK_LMMSE_LINEAR}) ok = ok && tdk_lmmse_lds_bytes(s, d, f) == lds;
  ok = ok && tdk_lmmse_lds_bytes(2, TDK_F32, 0) == 0 && tdk_lmmse_lds_bytes(TDK_F32, -1, 0) == 0 && tdk_lmmse_lds_bytes(TDK_F32, TDK_F32, 2) == 0 &&
       tdk_lmmse_lds_bytes(TDK_F32, TDK_F32, -1) == 0;
  if (!ok) {
    printf("FAIL queries\n");
    failures++;
  }
  printf("%d failures\n", failures);
  return failures != 0;
}
