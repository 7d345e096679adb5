// Stand-alone host program: every argument error of tdk_hdralign_pyramid and tdk_hdralign_merge with device pointers that are never
// dereferenced (frames is a host array and is read), and the host queries, for a run under a host sanitizer (no device is touched:
// each call returns before any HIP call).  Build, from the repository root:
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//     tests/hip_unit/hdralign_arguments_main.cpp torch-darktable_amd/csrc/hdralign.hip torch-darktable_amd/csrc/hdrmerge.hip \
//     torch-darktable_amd/csrc/runtime.hip -o hdralign_arguments
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../../include/tdk_hip_hdralign.h"

static int failures = 0;

static void expect(int rc, const char* who, const char* word, const char* what) {
  const char* msg = tdk_last_error();
  if (rc != TDK_ERR_INVALID_ARGUMENT || !msg || !strstr(msg, word) || strncmp(msg, who, strlen(who)) != 0) {
    printf("FAIL %s: rc %d, message '%s' (expected '%s: ... %s')\n", what, rc, msg ? msg : "(null)", who, word);
    failures++;
  }
}

int main() {
  char* const fake = reinterpret_cast<char*>(uintptr_t(1) << 30);
  const int w = 640, h = 480, nf = 3;
  const size_t step = size_t(1) << 24;   // more than a float32 frame
  const uint32_t rggb = 0x94949494u;
  const void* frames[8];
  for (int f = 0; f < 8; f++) frames[f] = fake + f * step;
  void* out = fake + 8 * step;
  unsigned char* mask = reinterpret_cast<unsigned char*>(fake + 9 * step);
  const float* exposures = reinterpret_cast<const float*>(fake + 10 * step);
  const float* model = reinterpret_cast<const float*>(fake + 10 * step + 64);
  const int16_t* fields = reinterpret_cast<const int16_t*>(fake + 11 * step);
  auto as_f = [](char* p) { return reinterpret_cast<const float*>(p); };
  auto as_i = [](char* p) { return reinterpret_cast<const int16_t*>(p); };
  auto as_m = [](char* p) { return reinterpret_cast<unsigned char*>(p); };
  const char* const M = "tdk_hdralign_merge";

  // tdk_hdralign_merge(frames, num_frames, src_dtype, out, out_dtype, mask, width, height, pattern, exposures, ref, model, radius, clip, t_lo, t_hi, pixel_c2,
  //                    v_min, fields, stream)
  auto merge = [&](const void* const* fr, int n, int sd, void* o, int od, unsigned char* m, int ww, int hh, uint32_t p, const float* e, int ref, const float* mo,
                   int r, float clip, float lo, float hi, float c2, float vmin, const int16_t* fi) {
    return tdk_hdralign_merge(fr, n, sd, o, od, m, ww, hh, p, e, ref, mo, r, clip, lo, hi, c2, vmin, fi, nullptr);
  };
  expect(merge(nullptr, nf, TDK_F32, out, TDK_F16, mask, w, h, rggb, exposures, 0, model, 2, 0.95f, 1.5f, 3.0f, 16.0f, 1e-12f, fields), M, "null pointer", "frames");
  expect(merge(frames, nf, TDK_F32, nullptr, TDK_F16, mask, w, h, rggb, exposures, 0, model, 2, 0.95f, 1.5f, 3.0f, 16.0f, 1e-12f, fields), M, "null pointer", "out");
  expect(merge(frames, nf, TDK_F32, out, TDK_F16, mask, w, h, rggb, nullptr, 0, model, 2, 0.95f, 1.5f, 3.0f, 16.0f, 1e-12f, fields), M, "null pointer", "exposures");
  expect(merge(frames, nf, TDK_F32, out, TDK_F16, mask, w, h, rggb, exposures, 0, nullptr, 2, 0.95f, 1.5f, 3.0f, 16.0f, 1e-12f, fields), M, "null pointer", "model");
  expect(merge(frames, nf, TDK_F32, out, TDK_F16, mask, w, h, rggb, exposures, 0, model, 2, 0.95f, 1.5f, 3.0f, 16.0f, 1e-12f, nullptr), M, "null pointer (fields)", "fields");
  for (int f = 0; f < nf; f++) {
    const void* holed[8];
    for (int k = 0; k < 8; k++) holed[k] = k == f ? nullptr : frames[k];
    expect(merge(holed, nf, TDK_F32, out, TDK_F16, mask, w, h, rggb, exposures, 0, model, 2, 0.95f, 1.5f, 3.0f, 16.0f, 1e-12f, fields), M, "null pointer (frame", "a null frame");
  }
  for (int n : {1, 0, 9, -1})
    expect(merge(frames, n, TDK_F32, out, TDK_F16, mask, w, h, rggb, exposures, 0, model, 2, 0.95f, 1.5f, 3.0f, 16.0f, 1e-12f, fields), M, "num_frames", "num_frames");
  for (int d : {2, 3, -1}) {
    expect(merge(frames, nf, d, out, TDK_F16, mask, w, h, rggb, exposures, 0, model, 2, 0.95f, 1.5f, 3.0f, 16.0f, 1e-12f, fields), M, "dtype", "src_dtype");
    expect(merge(frames, nf, TDK_F32, out, d, mask, w, h, rggb, exposures, 0, model, 2, 0.95f, 1.5f, 3.0f, 16.0f, 1e-12f, fields), M, "dtype", "out_dtype");
  }
  for (int v : {0, -2, 65536}) {
    expect(merge(frames, nf, TDK_F32, out, TDK_F16, mask, v, h, rggb, exposures, 0, model, 2, 0.95f, 1.5f, 3.0f, 16.0f, 1e-12f, fields), M, "frame size", "width");
    expect(merge(frames, nf, TDK_F32, out, TDK_F16, mask, w, v, rggb, exposures, 0, model, 2, 0.95f, 1.5f, 3.0f, 16.0f, 1e-12f, fields), M, "frame size", "height");
  }
  for (int v : {641, 65535}) {
    expect(merge(frames, nf, TDK_F32, out, TDK_F16, mask, v, h, rggb, exposures, 0, model, 2, 0.95f, 1.5f, 3.0f, 16.0f, 1e-12f, fields), M, "even", "odd width");
    expect(merge(frames, nf, TDK_F32, out, TDK_F16, mask, w, v, rggb, exposures, 0, model, 2, 0.95f, 1.5f, 3.0f, 16.0f, 1e-12f, fields), M, "even", "odd height");
  }
  for (uint32_t p : {0x12345678u, 0u})
    expect(merge(frames, nf, TDK_F32, out, TDK_F16, mask, w, h, p, exposures, 0, model, 2, 0.95f, 1.5f, 3.0f, 16.0f, 1e-12f, fields), M, "Bayer pattern", "pattern");
  for (int r : {1, 0, 4, -2})
    expect(merge(frames, nf, TDK_F32, out, TDK_F16, mask, w, h, rggb, exposures, 0, model, r, 0.95f, 1.5f, 3.0f, 16.0f, 1e-12f, fields), M, "radius", "radius");
  for (int ref : {-1, -2, 3, 8})   // -1 is refused here
    expect(merge(frames, nf, TDK_F32, out, TDK_F16, mask, w, h, rggb, exposures, ref, model, 2, 0.95f, 1.5f, 3.0f, 16.0f, 1e-12f, fields), M, "ref must be a frame index", "ref");
  for (float c : {0.0f, -1.0f, NAN, INFINITY})
    expect(merge(frames, nf, TDK_F32, out, TDK_F16, mask, w, h, rggb, exposures, 0, model, 2, c, 1.5f, 3.0f, 16.0f, 1e-12f, fields), M, "clip", "clip");
  const float pairs[][2] = {{0.0f, 3.0f}, {-1.0f, 3.0f}, {3.0f, 3.0f}, {3.0f, 1.5f}, {NAN, 3.0f}, {1.5f, NAN}, {1.5f, INFINITY}, {1e-40f, 2e-40f}};
  for (const auto& t : pairs)
    expect(merge(frames, nf, TDK_F32, out, TDK_F16, mask, w, h, rggb, exposures, 0, model, 2, 0.95f, t[0], t[1], 16.0f, 1e-12f, fields), M, "thresholds", "thresholds");
  for (float c2 : {0.0f, -1.0f, NAN, -INFINITY})
    expect(merge(frames, nf, TDK_F32, out, TDK_F16, mask, w, h, rggb, exposures, 0, model, 2, 0.95f, 1.5f, 3.0f, c2, 1e-12f, fields), M, "pixel_c2", "pixel_c2");
  for (float v : {0.0f, -1e-12f, NAN, INFINITY})
    expect(merge(frames, nf, TDK_F32, out, TDK_F16, mask, w, h, rggb, exposures, 0, model, 2, 0.95f, 1.5f, 3.0f, 16.0f, v, fields), M, "v_min", "v_min");
  for (int f = 0; f < nf; f++) {
    expect(merge(frames, nf, TDK_F32, fake + f * step + 64, TDK_F16, mask, w, h, rggb, exposures, 0, model, 2, 0.95f, 1.5f, 3.0f, 16.0f, 1e-12f, fields), M, "overlaps frame", "out in a frame");
    expect(merge(frames, nf, TDK_F32, out, TDK_F16, as_m(fake + f * step + size_t(w) * h * 4 - 1), w, h, rggb, exposures, 0, model, 2, 0.95f, 1.5f, 3.0f, 16.0f, 1e-12f, fields), M,
           "overlaps frame", "mask on the last byte of a frame");
  }
  expect(merge(frames, nf, TDK_F32, out, TDK_F16, mask, w, h, rggb, as_f(fake + 8 * step + 16), 0, model, 2, 0.95f, 1.5f, 3.0f, 16.0f, 1e-12f, fields), M,
         "the exposures or the model overlap", "exposures in out");
  expect(merge(frames, nf, TDK_F32, out, TDK_F16, mask, w, h, rggb, exposures, 0, as_f(fake + 9 * step + size_t(w) * h - 4), 2, 0.95f, 1.5f, 3.0f, 16.0f, 1e-12f, fields), M,
         "the exposures or the model overlap", "model on the last bytes of mask");
  expect(merge(frames, nf, TDK_F32, out, TDK_F16, as_m(fake + 8 * step + size_t(w) * h * 2 - 1), w, h, rggb, exposures, 0, model, 2, 0.95f, 1.5f, 3.0f, 16.0f, 1e-12f, fields), M,
         "out and mask overlap", "mask on the last byte of out");
  for (int o : {1, 2, 3})
    expect(merge(frames, nf, TDK_F32, out, TDK_F16, mask, w, h, rggb, exposures, 0, model, 2, 0.95f, 1.5f, 3.0f, 16.0f, 1e-12f,
                 reinterpret_cast<const int16_t*>(fake + 11 * step + o)), M, "fields must be aligned", "fields alignment");
  const size_t field_bytes = size_t(nf) * 10 * 15 * 4;   // F x Tx x Ty displacements of two int16
  expect(merge(frames, nf, TDK_F32, out, TDK_F16, mask, w, h, rggb, exposures, 0, model, 2, 0.95f, 1.5f, 3.0f, 16.0f, 1e-12f, as_i(fake + 8 * step + 64)), M, "the fields overlap", "fields in out");
  expect(merge(frames, nf, TDK_F32, out, TDK_F16, mask, w, h, rggb, exposures, 0, model, 2, 0.95f, 1.5f, 3.0f, 16.0f, 1e-12f, as_i(fake + 8 * step - field_bytes + 4)), M,
         "the fields overlap", "fields into out");
  expect(merge(frames, nf, TDK_F32, out, TDK_F16, mask, w, h, rggb, exposures, 0, model, 2, 0.95f, 1.5f, 3.0f, 16.0f, 1e-12f, as_i(fake + 9 * step + size_t(w) * h - 4)), M,
         "the fields overlap", "fields on the last bytes of mask");
  expect(merge(frames, nf, TDK_F32, out, TDK_F16, mask, w, h, rggb, exposures, 0, model, 2, 0.95f, 1.5f, 3.0f, 16.0f, 1e-12f, as_i(fake + 9 * step - field_bytes + 4)), M,
         "the fields overlap", "fields into mask");

  // tdk_hdralign_pyramid(src, src_dtype, width, height, scale, levels, pyramid, which, exposures, num_frames, frame, stream)
  const char* const P = "tdk_hdralign_pyramid";
  void *src = fake, *pyramid = fake + step;
  const float* pe = as_f(fake + 2 * step);
  expect(tdk_hdralign_pyramid(nullptr, TDK_F32, w, h, 0.25f, 3, pyramid, 0, pe, nf, 1, nullptr), P, "null pointer", "src");
  expect(tdk_hdralign_pyramid(src, TDK_F32, w, h, 0.25f, 3, nullptr, 0, pe, nf, 1, nullptr), P, "null pointer", "pyramid");
  expect(tdk_hdralign_pyramid(src, TDK_F32, w, h, 0.25f, 3, pyramid, 0, nullptr, nf, 1, nullptr), P, "null pointer (exposures)", "exposures");
  for (int d : {2, 3, -1}) expect(tdk_hdralign_pyramid(src, d, w, h, 0.25f, 3, pyramid, 0, pe, nf, 1, nullptr), P, "dtype", "dtype");
  for (int v : {0, -2, 65536}) {
    expect(tdk_hdralign_pyramid(src, TDK_F32, v, h, 0.25f, 3, pyramid, 0, pe, nf, 1, nullptr), P, "frame size", "width");
    expect(tdk_hdralign_pyramid(src, TDK_F32, w, v, 0.25f, 3, pyramid, 0, pe, nf, 1, nullptr), P, "frame size", "height");
  }
  expect(tdk_hdralign_pyramid(src, TDK_F32, 641, h, 0.25f, 3, pyramid, 0, pe, nf, 1, nullptr), P, "even", "odd width");
  expect(tdk_hdralign_pyramid(src, TDK_F32, w, 481, 0.25f, 3, pyramid, 0, pe, nf, 1, nullptr), P, "even", "odd height");
  for (float s : {0.0f, -0.25f, NAN, INFINITY}) expect(tdk_hdralign_pyramid(src, TDK_F32, w, h, s, 3, pyramid, 0, pe, nf, 1, nullptr), P, "scale", "scale");
  for (int l : {0, 5, -1}) expect(tdk_hdralign_pyramid(src, TDK_F32, w, h, 0.25f, l, pyramid, 0, pe, nf, 1, nullptr), P, "levels", "levels");
  for (int wh : {2, -1}) expect(tdk_hdralign_pyramid(src, TDK_F32, w, h, 0.25f, 3, pyramid, wh, pe, nf, 1, nullptr), P, "which", "which");
  expect(tdk_hdralign_pyramid(src, TDK_F32, w, h, 0.25f, 3, fake + step + 8, 0, pe, nf, 1, nullptr), P, "aligned to 16", "pyramid alignment");
  for (int n : {1, 0, 9}) expect(tdk_hdralign_pyramid(src, TDK_F32, w, h, 0.25f, 3, pyramid, 0, pe, n, 1, nullptr), P, "num_frames", "num_frames");
  for (int f : {-1, 3, 8}) expect(tdk_hdralign_pyramid(src, TDK_F32, w, h, 0.25f, 3, pyramid, 0, pe, nf, f, nullptr), P, "frame must be", "frame");
  expect(tdk_hdralign_pyramid(src, TDK_F32, w, h, 0.25f, 3, pyramid, 0, as_f(fake + 2 * step + 2), nf, 1, nullptr), P, "exposures must be aligned", "exposures alignment");
  expect(tdk_hdralign_pyramid(src, TDK_F32, w, h, 0.25f, 3, fake + 1024, 0, pe, nf, 1, nullptr), P, "src and pyramid overlap", "pyramid in src");
  expect(tdk_hdralign_pyramid(src, TDK_F32, w, h, 0.25f, 3, pyramid, 0, as_f(fake + step + 64), nf, 1, nullptr), P, "exposures and pyramid overlap", "exposures in pyramid");

  bool ok = tdk_hdralign_abi_version() == TDK_HDRALIGN_ABI_VERSION;
  for (int r : {2, 3}) ok = ok && tdk_hdralign_lds_bytes(r) == tdk_hdr_lds_bytes(r) + 64 && tdk_hdralign_lds_bytes(r) <= 65536;
  for (int r : {0, 1, 4, -2}) ok = ok && tdk_hdralign_lds_bytes(r) == 0;
  if (!ok) {
    printf("FAIL queries\n");
    failures++;
  }
  printf("%d failures\n", failures);
  return failures != 0;
}
