// Stand-alone host program: every argument error of tdk_demosaic_scaled and tdk_decode12_demosaic_scaled with device pointers that
// are never dereferenced, and the host queries, for a run under a host sanitizer (no device is touched: each call returns before any
// HIP call).  Build, from the repository root:
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//     tests/hip_unit/scaled_arguments_main.cpp torch-darktable_amd/csrc/scaled_demosaic.hip torch-darktable_amd/csrc/runtime.hip -o scaled_arguments
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../../include/tdk_hip_scaled.h"

static int failures = 0;

static void expect(int rc, const char* word, const char* what, const char* who = "tdk_demosaic_scaled:") {
  const char* msg = tdk_last_error();
  if (rc != TDK_ERR_INVALID_ARGUMENT || !msg || !strstr(msg, word) || strncmp(msg, who, strlen(who)) != 0) {
    printf("FAIL %s: rc %d, message '%s' (expected '%s')\n", what, rc, msg ? msg : "(null)", word);
    failures++;
  }
}

int main() {
  char* const fake = reinterpret_cast<char*>(uintptr_t(1) << 30);
  const int w = 640, h = 480, ow = 160, oh = 120;
  void *src = fake, *dst = fake + (1 << 24);
  const float* gains = reinterpret_cast<const float*>(fake + (1 << 25));
  const uint8_t* packed = reinterpret_cast<const uint8_t*>(fake);
  const uint32_t P = TDK_PATTERN_RGGB;
  const char* const packed_name = "tdk_decode12_demosaic_scaled:";
  const size_t plane = size_t(w) * h * 4, frame = size_t(ow) * oh * 3 * 4;

  // tdk_demosaic_scaled(src, dst, gains, width, height, out_width, out_height, pattern, src_dtype, dst_dtype, stream)
  expect(tdk_demosaic_scaled(nullptr, dst, gains, w, h, ow, oh, P, TDK_F32, TDK_F32, nullptr), "null pointer (src or dst)", "src");
  expect(tdk_demosaic_scaled(src, nullptr, nullptr, w, h, ow, oh, P, TDK_F32, TDK_F32, nullptr), "null pointer (src or dst)", "dst");
  expect(tdk_decode12_demosaic_scaled(nullptr, dst, gains, w, h, ow, oh, P, 0, TDK_F32, nullptr), "null pointer (src or dst)", "packed", packed_name);
  for (int v : {1, 0, -3, 65536}) {
    expect(tdk_demosaic_scaled(src, dst, gains, v, h, ow, oh, P, TDK_F32, TDK_F32, nullptr), "mosaic size", "width");
    expect(tdk_demosaic_scaled(src, dst, nullptr, w, v, ow, oh, P, TDK_F32, TDK_F32, nullptr), "mosaic size", "height");
    expect(tdk_decode12_demosaic_scaled(packed, dst, gains, w, v, ow, oh, P, 1, TDK_F32, nullptr), "mosaic size", "packed height", packed_name);
  }
  for (int v : {0, -1}) {
    expect(tdk_demosaic_scaled(src, dst, gains, w, h, v, oh, P, TDK_F32, TDK_F32, nullptr), "below 1x1", "out_width");
    expect(tdk_demosaic_scaled(src, dst, gains, w, h, ow, v, P, TDK_F32, TDK_F32, nullptr), "below 1x1", "out_height");
  }
  expect(tdk_demosaic_scaled(src, dst, gains, w, h, 321, oh, P, TDK_F32, TDK_F32, nullptr), "below 2:1", "ratio below 2 along x");
  expect(tdk_demosaic_scaled(src, dst, gains, w, h, ow, 241, P, TDK_F32, TDK_F32, nullptr), "below 2:1", "ratio below 2 along y");
  expect(tdk_demosaic_scaled(src, dst, gains, w, h, w, h, P, TDK_F32, TDK_F32, nullptr), "below 2:1", "the same size");
  expect(tdk_demosaic_scaled(src, dst, gains, w, h, 39, oh, P, TDK_F32, TDK_F32, nullptr), "beyond 16:1", "ratio beyond 16 along x");
  expect(tdk_demosaic_scaled(src, dst, gains, w, h, ow, 29, P, TDK_F32, TDK_F32, nullptr), "beyond 16:1", "ratio beyond 16 along y");
  expect(tdk_decode12_demosaic_scaled(packed, dst, gains, w, h, ow, 29, P, 0, TDK_F32, nullptr), "beyond 16:1", "packed ratio", packed_name);
  expect(tdk_decode12_demosaic_scaled(packed, dst, gains, 641, h, ow, oh, P, 0, TDK_F32, nullptr), "width must be even", "packed odd width", packed_name);
  for (uint32_t p : {0u, 1u, 0x94949495u, 0x94941616u, 0xffffffffu, 0x55555555u}) {
    expect(tdk_demosaic_scaled(src, dst, gains, w, h, ow, oh, p, TDK_F32, TDK_F32, nullptr), "invalid Bayer pattern", "pattern");
    expect(tdk_decode12_demosaic_scaled(packed, dst, nullptr, w, h, ow, oh, p, 0, TDK_F16, nullptr), "invalid Bayer pattern", "packed pattern", packed_name);
  }
  for (int d : {2, 3, -1}) {
    expect(tdk_demosaic_scaled(src, dst, gains, w, h, ow, oh, P, d, TDK_F32, nullptr), "unsupported src dtype", "src dtype");
    expect(tdk_demosaic_scaled(src, dst, gains, w, h, ow, oh, P, TDK_F16, d, nullptr), "unsupported dst dtype", "dst dtype");
    expect(tdk_decode12_demosaic_scaled(packed, dst, gains, w, h, ow, oh, P, 1, d, nullptr), "unsupported dst dtype", "packed dst dtype", packed_name);
  }
  // overlap, in bytes: src is one plane of its dtype (or the packed bytes), dst the reduced frame
  expect(tdk_demosaic_scaled(src, src, gains, w, h, ow, oh, P, TDK_F32, TDK_F32, nullptr), "src and dst overlap", "dst == src");
  expect(tdk_demosaic_scaled(src, fake + plane - 4, gains, w, h, ow, oh, P, TDK_F32, TDK_F32, nullptr), "src and dst overlap", "dst on the last element of src");
  expect(tdk_demosaic_scaled(src, fake + plane / 2 - 2, gains, w, h, ow, oh, P, TDK_F16, TDK_F32, nullptr), "src and dst overlap", "dst on the last element of a binary16 src");
  expect(tdk_demosaic_scaled(src, fake - frame + 4, gains, w, h, ow, oh, P, TDK_F32, TDK_F32, nullptr), "src and dst overlap", "the last element of dst on src");
  expect(tdk_demosaic_scaled(src, fake - frame / 2 + 2, gains, w, h, ow, oh, P, TDK_F32, TDK_F16, nullptr), "src and dst overlap", "the last element of a binary16 dst on src");
  expect(tdk_decode12_demosaic_scaled(packed, fake + size_t(w) * h * 3 / 2 - 1, gains, w, h, ow, oh, P, 0, TDK_F32, nullptr), "src and dst overlap", "dst on the last packed byte",
         packed_name);
  expect(tdk_demosaic_scaled(src, dst, reinterpret_cast<const float*>(fake + (1 << 24) + frame - 4), w, h, ow, oh, P, TDK_F32, TDK_F32, nullptr), "gains and dst overlap",
         "gains on the last element of dst");

  bool ok = tdk_scaled_abi_version() == TDK_SCALED_ABI_VERSION;
  const size_t lds = tdk_demosaic_scaled_lds_bytes(w, h, ow, oh);
  ok = ok && lds > 0 && lds <= 80 * 1024;
  ok = ok && tdk_demosaic_scaled_lds_bytes(2, 2, 1, 1) == lds && tdk_demosaic_scaled_lds_bytes(65535, 65535, 4096, 4096) == lds;
  ok = ok && tdk_demosaic_scaled_lds_bytes(1, 2, 1, 1) == 0 && tdk_demosaic_scaled_lds_bytes(w, h, 321, oh) == 0 && tdk_demosaic_scaled_lds_bytes(w, h, ow, 29) == 0 &&
       tdk_demosaic_scaled_lds_bytes(w, h, 0, oh) == 0 && tdk_demosaic_scaled_lds_bytes(65536, h, 4096, oh) == 0;
  int tw = -1, th = -1;
  ok = ok && tdk_demosaic_scaled_tile(w, h, ow, oh, &tw, &th) == TDK_OK && tw == 64 && th == 14;
  ok = ok && tdk_demosaic_scaled_tile(w, h, 40, 30, &tw, &th) == TDK_OK && tw == 32 && th >= 1 && th <= 32;
  ok = ok && tdk_demosaic_scaled_tile(65535, 65535, 4096, 4096, &tw, &th) == TDK_OK && tw == 32 && th >= 1;
  if (!ok) {
    printf("FAIL queries\n");
    failures++;
  }
  expect(tdk_demosaic_scaled_tile(w, h, ow, oh, nullptr, &th), "null pointer", "tile: null", "tdk_demosaic_scaled_tile:");
  expect(tdk_demosaic_scaled_tile(w, h, 321, oh, &tw, &th), "not a legal call", "tile: ratio", "tdk_demosaic_scaled_tile:");
  printf("%d failures\n", failures);
  return failures != 0;
}
