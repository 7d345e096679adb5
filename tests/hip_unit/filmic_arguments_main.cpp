// Stand-alone host program: every argument error of tdk_filmic with pointers that are never dereferenced (weights is a host array
// and is read), for a run under a host sanitizer (no device is touched: each call returns before any HIP call).  Build, from the
// repository root:
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//     tests/hip_unit/filmic_arguments_main.cpp torch-darktable_amd/csrc/filmic.hip torch-darktable_amd/csrc/runtime.hip -o filmic_arguments
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../../include/tdk_hip_filmic.h"

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
  const int64_t npix = 640 * 480;
  void *src = fake, *dst = fake + (1 << 24);
  auto as_f = [](char* p) { return reinterpret_cast<const float*>(p); };
  const float *curve = as_f(fake + (2 << 24)), *enc = as_f(fake + (3 << 24)), *expo = as_f(fake + (4 << 24));
  const float rec709[3] = {0.2126f, 0.7152f, 0.0722f};
  const float bad_nan[3] = {0.2f, NAN, 0.1f}, bad_inf[3] = {INFINITY, 0.7f, 0.1f}, bad_neg[3] = {0.2f, 0.7f, -0.1f};
  const size_t n = size_t(npix) * 3, src_bytes = n * 4;

  // tdk_filmic(src, dst, curve, encode, exposure, npix, src_dtype, dst_dtype, norm, weights, flags, stream)
  expect(tdk_filmic(nullptr, dst, curve, enc, expo, npix, TDK_F32, TDK_U8, TDK_FILMIC_MAX, rec709, 0, nullptr), "null pointer (src)", "src");
  expect(tdk_filmic(src, nullptr, curve, enc, expo, npix, TDK_F32, TDK_U8, TDK_FILMIC_MAX, rec709, 0, nullptr), "null pointer (dst)", "dst");
  expect(tdk_filmic(src, dst, nullptr, enc, expo, npix, TDK_F32, TDK_U8, TDK_FILMIC_MAX, rec709, 0, nullptr), "null pointer (curve)", "curve");
  expect(tdk_filmic(src, dst, curve, enc, nullptr, npix, TDK_F32, TDK_U8, TDK_FILMIC_MAX, rec709, 0, nullptr), "null pointer (exposure)", "exposure");
  expect(tdk_filmic(src, dst, curve, enc, expo, npix, TDK_F32, TDK_U8, TDK_FILMIC_MAX, nullptr, 0, nullptr), "null pointer (weights)", "weights");
  for (int64_t bad : {int64_t(-1), -(int64_t(1) << 40), int64_t(1) << 62})
    expect(tdk_filmic(src, dst, curve, enc, expo, bad, TDK_F32, TDK_U8, TDK_FILMIC_MAX, rec709, 0, nullptr), "npix", "npix");
  for (int d : {TDK_U8, 3, -1}) expect(tdk_filmic(src, dst, curve, enc, expo, npix, d, TDK_U8, TDK_FILMIC_MAX, rec709, 0, nullptr), "source dtype", "source dtype");
  for (int d : {3, -1, 7}) expect(tdk_filmic(src, dst, curve, enc, expo, npix, TDK_F32, d, TDK_FILMIC_MAX, rec709, 0, nullptr), "destination dtype", "destination dtype");
  for (int norm : {-1, 4, 100}) expect(tdk_filmic(src, dst, curve, enc, expo, npix, TDK_F32, TDK_U8, norm, rec709, 0, nullptr), "norm must be", "norm");
  expect(tdk_filmic(src, dst, curve, enc, expo, npix, TDK_F32, TDK_U8, TDK_FILMIC_LUMA, bad_nan, 0, nullptr), "weights[1]", "weights nan");
  expect(tdk_filmic(src, dst, curve, enc, expo, npix, TDK_F32, TDK_U8, TDK_FILMIC_LUMA, bad_inf, 0, nullptr), "weights[0]", "weights inf");
  expect(tdk_filmic(src, dst, curve, enc, expo, npix, TDK_F32, TDK_U8, TDK_FILMIC_MAX, bad_neg, 0, nullptr), "weights[2]", "weights negative");
  for (int flags : {1, 2, -1}) expect(tdk_filmic(src, dst, curve, enc, expo, npix, TDK_F32, TDK_U8, TDK_FILMIC_MAX, rec709, flags, nullptr), "flags is reserved", "flags");
  for (int off : {1, 2, 3}) {
    expect(tdk_filmic(src, dst, as_f(fake + (2 << 24) + off), enc, expo, npix, TDK_F32, TDK_U8, TDK_FILMIC_MAX, rec709, 0, nullptr), "curve must be aligned", "curve alignment");
    expect(tdk_filmic(src, dst, curve, as_f(fake + (3 << 24) + off), expo, npix, TDK_F32, TDK_U8, TDK_FILMIC_MAX, rec709, 0, nullptr), "encode must be aligned", "encode alignment");
    expect(tdk_filmic(src, dst, curve, enc, as_f(fake + (4 << 24) + off), npix, TDK_F32, TDK_U8, TDK_FILMIC_MAX, rec709, 0, nullptr), "exposure must be aligned", "exposure alignment");
  }
  expect(tdk_filmic(fake + 2, dst, curve, enc, expo, npix, TDK_F32, TDK_U8, TDK_FILMIC_MAX, rec709, 0, nullptr), "src must be aligned", "float32 src alignment");
  expect(tdk_filmic(fake + 1, dst, curve, enc, expo, npix, TDK_F16, TDK_U8, TDK_FILMIC_MAX, rec709, 0, nullptr), "src must be aligned", "binary16 src alignment");
  expect(tdk_filmic(src, fake + (1 << 24) + 2, curve, enc, expo, npix, TDK_F32, TDK_F32, TDK_FILMIC_MAX, rec709, 0, nullptr), "dst must be aligned", "float32 dst alignment");
  expect(tdk_filmic(src, fake + (1 << 24) + 1, curve, enc, expo, npix, TDK_F32, TDK_F16, TDK_FILMIC_MAX, rec709, 0, nullptr), "dst must be aligned", "binary16 dst alignment");
  expect(tdk_filmic(src, src, curve, enc, expo, npix, TDK_F32, TDK_U8, TDK_FILMIC_MAX, rec709, 0, nullptr), "src and dst overlap", "dst == src");
  expect(tdk_filmic(src, fake + 64, curve, enc, expo, npix, TDK_F32, TDK_U8, TDK_FILMIC_MAX, rec709, 0, nullptr), "src and dst overlap", "dst in src");
  expect(tdk_filmic(src, fake - n + 1, curve, enc, expo, npix, TDK_F32, TDK_U8, TDK_FILMIC_MAX, rec709, 0, nullptr), "src and dst overlap", "dst onto the first byte of src");
  expect(tdk_filmic(src, fake + src_bytes - 1, curve, enc, expo, npix, TDK_F32, TDK_U8, TDK_FILMIC_MAX, rec709, 0, nullptr), "src and dst overlap", "dst on the last byte of src");
  expect(tdk_filmic(src, fake + src_bytes / 2 - 2, curve, enc, expo, npix, TDK_F16, TDK_F16, TDK_FILMIC_MAX, rec709, 0, nullptr), "src and dst overlap", "binary16 dst on the last element of src");
  expect(tdk_filmic(src, dst, as_f(fake + (1 << 24)), enc, expo, npix, TDK_F32, TDK_U8, TDK_FILMIC_MAX, rec709, 0, nullptr), "curve and dst overlap", "curve at dst");
  expect(tdk_filmic(src, dst, as_f(fake + (1 << 24) - 2 * TDK_FILMIC_TABLE * 4 + 4), enc, expo, npix, TDK_F32, TDK_U8, TDK_FILMIC_MAX, rec709, 0, nullptr), "curve and dst overlap", "curve into dst");
  expect(tdk_filmic(src, dst, curve, as_f(fake + (1 << 24) + 8), expo, npix, TDK_F32, TDK_U8, TDK_FILMIC_MAX, rec709, 0, nullptr), "encode and dst overlap", "encode in dst");
  expect(tdk_filmic(src, dst, curve, as_f(fake + (1 << 24) - TDK_FILMIC_ENC_TABLE * 4 + 4), expo, npix, TDK_F32, TDK_U8, TDK_FILMIC_MAX, rec709, 0, nullptr), "encode and dst overlap", "encode into dst");
  expect(tdk_filmic(src, dst, curve, enc, as_f(fake + (1 << 24) + n - 4), npix, TDK_F32, TDK_U8, TDK_FILMIC_MAX, rec709, 0, nullptr), "exposure and dst overlap", "exposure in dst");

  // no pixels: every check passes, nothing is launched
  if (tdk_filmic(src, dst, curve, enc, expo, 0, TDK_F32, TDK_U8, TDK_FILMIC_MAX, rec709, 0, nullptr) != TDK_OK ||
      tdk_filmic(src, dst, curve, nullptr, expo, 0, TDK_F16, TDK_F32, TDK_FILMIC_NONE, rec709, 0, nullptr) != TDK_OK) {
    printf("FAIL npix 0\n");
    failures++;
  }
  if (tdk_filmic_lds_bytes() != size_t(16 * (TDK_FILMIC_TABLE - 1) + 8 * (TDK_FILMIC_ENC_TABLE - 1)) || tdk_filmic_lds_bytes() > 65536 ||
      tdk_filmic_abi_version() != TDK_FILMIC_ABI_VERSION) {
    printf("FAIL queries\n");
    failures++;
  }
  printf("%d failures\n", failures);
  return failures != 0;
}
