// Stand-alone host program: every argument error of tdk_defringe with device pointers that are never dereferenced, and the host
// queries, for a run under a host sanitizer (no device is touched: each call returns before any HIP call).  Build, from the
// repository root:
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//     tests/hip_unit/defringe_arguments_main.cpp torch-darktable_amd/csrc/defringe.hip torch-darktable_amd/csrc/runtime.hip -o defringe_arguments
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../../include/tdk_hip_defringe.h"

static int failures = 0;

static void expect(int rc, const char* word, const char* what) {
  const char* msg = tdk_last_error();
  if (rc != TDK_ERR_INVALID_ARGUMENT || !msg || !strstr(msg, word) || strncmp(msg, "tdk_defringe:", 13) != 0) {
    printf("FAIL %s: rc %d, message '%s' (expected '%s')\n", what, rc, msg ? msg : "(null)", word);
    failures++;
  }
}

struct Call {
  const void* src;
  void* dst;
  unsigned char* mask;
  float* edge;
  tdk_defringe_stats* stats;
  void* ws;
  int w, h, dtype;
  const float* weights;
  int radius, sample_radius;
  float strength, floor;
  int flags;
  int run() const { return tdk_defringe(src, dst, mask, edge, stats, ws, w, h, dtype, weights, radius, sample_radius, strength, floor, flags, nullptr); }
};

int main() {
  char* const fake = reinterpret_cast<char*>(uintptr_t(1) << 30);
  const int w = 640, h = 480;
  const size_t plane = size_t(w) * h * 4, frame = 3 * plane, gap = size_t(1) << 24;
  float taps[TDK_DEFRINGE_MAX_RADIUS + 1];
  int radius = 0;
  bool ok = tdk_defringe_weights(2.0f, taps, &radius) == TDK_OK && radius == 6;
  const Call good = {fake, fake + gap, reinterpret_cast<unsigned char*>(fake + 2 * gap), reinterpret_cast<float*>(fake + 3 * gap),
                     reinterpret_cast<tdk_defringe_stats*>(fake + 4 * gap), fake + 5 * gap, w, h, TDK_F32, taps, 6, 6, 2.5f, 1e-4f, 0};
  Call c = good;

  c = good, c.src = nullptr, expect(c.run(), "null pointer (src or dst)", "src");
  c = good, c.dst = nullptr, expect(c.run(), "null pointer (src or dst)", "dst");
  c = good, c.weights = nullptr, expect(c.run(), "null pointer (weights)", "weights");
  c = good, c.ws = nullptr, expect(c.run(), "null pointer (workspace)", "workspace");
  for (int v : {0, -3, 65536}) {
    c = good, c.w = v, expect(c.run(), "frame size", "width");
    c = good, c.h = v, expect(c.run(), "frame size", "height");
  }
  for (int d : {2, 3, -1}) c = good, c.dtype = d, expect(c.run(), "unsupported dtype", "dtype");
  for (int r : {0, -1, 13, 64}) c = good, c.radius = r, expect(c.run(), "radius must be 1..12", "radius");
  for (float bad : {NAN, INFINITY, -0.5f, -1e-9f}) {
    float broken[TDK_DEFRINGE_MAX_RADIUS + 1];
    memcpy(broken, taps, sizeof(taps));
    broken[3] = bad;
    c = good, c.weights = broken, expect(c.run(), "weights[3]", "a tap");
  }
  for (int s : {0, -1, 9, 64}) c = good, c.sample_radius = s, expect(c.run(), "sample_radius must be 1..8", "sample radius");
  for (float s : {-1.0f, -1e-9f, NAN, INFINITY}) c = good, c.strength = s, expect(c.run(), "strength must be finite and >= 0", "strength");
  for (float f : {0.0f, -1e-4f, NAN, INFINITY}) c = good, c.floor = f, expect(c.run(), "floor must be finite and > 0", "floor");
  for (int f : {4, 8, 128, 1 << 19, -1, 1 << 30, 1025 << TDK_DEFRINGE_GROUPS_SHIFT, 2047 << TDK_DEFRINGE_GROUPS_SHIFT})
    c = good, c.flags = f, expect(c.run(), "reserved", "flags");
  c = good, c.edge = reinterpret_cast<float*>(fake + 3 * gap + 2), expect(c.run(), "edge_out must be aligned to 4 bytes", "edge_out alignment");
  c = good, c.stats = reinterpret_cast<tdk_defringe_stats*>(fake + 4 * gap + 4), expect(c.run(), "stats_out must be aligned to 8 bytes", "stats_out alignment");
  // overlap, in bytes of the dtype
  for (char* d : {fake, fake + 64, fake - frame + 4, fake + frame - 4}) c = good, c.dst = d, expect(c.run(), "src and dst overlap", "dst on src");
  c = good, c.dtype = TDK_F16, c.dst = fake + frame / 2 - 2, expect(c.run(), "src and dst overlap", "dst on the last element of a binary16 src");
  c = good, c.mask = reinterpret_cast<unsigned char*>(fake + frame - 1), expect(c.run(), "mask_out overlaps src", "mask_out on src");
  c = good, c.mask = reinterpret_cast<unsigned char*>(fake + gap - plane / 4 + 1), expect(c.run(), "mask_out overlaps dst", "mask_out on dst");
  c = good, c.edge = reinterpret_cast<float*>(fake + frame - 4), expect(c.run(), "edge_out overlaps src", "edge_out on src");
  c = good, c.edge = reinterpret_cast<float*>(fake + 2 * gap + plane / 4 - 4), expect(c.run(), "edge_out overlaps mask_out", "edge_out on mask_out");
  c = good, c.stats = reinterpret_cast<tdk_defringe_stats*>(fake + gap + frame - 8), expect(c.run(), "stats_out overlaps dst", "stats_out on dst");
  c = good, c.stats = reinterpret_cast<tdk_defringe_stats*>(fake + 3 * gap + plane - 8), expect(c.run(), "stats_out overlaps edge_out", "stats_out on edge_out");
  const size_t ws_bytes = tdk_defringe_workspace_bytes(w, h);
  c = good, c.ws = fake + frame - 1, expect(c.run(), "the workspace overlaps src", "workspace on src");
  c = good, c.ws = fake + 4 * gap - ws_bytes + 8, expect(c.run(), "the workspace overlaps stats_out", "workspace on stats_out");
  c = good, c.ws = fake + 3 * gap - 16, expect(c.run(), "the workspace overlaps edge_out", "workspace on edge_out");

  ok = ok && tdk_defringe_abi_version() == TDK_DEFRINGE_ABI_VERSION;
  ok = ok && ws_bytes == (plane + 15) / 16 * 16 + TDK_DEFRINGE_MAX_GROUPS * 8 + 16 && tdk_defringe_workspace_bytes(1, 1) == 16 + 8192 + 16;
  ok = ok && tdk_defringe_workspace_bytes(0, 5) == 0 && tdk_defringe_workspace_bytes(5, 65536) == 0 && tdk_defringe_workspace_bytes(65535, 65535) > (size_t(1) << 33);
  const size_t lds = tdk_defringe_lds_bytes(TDK_F32, 6, 6, 0);
  ok = ok && lds > 0 && lds <= 65536;
  for (int d : {TDK_F32, TDK_F16})
    for (int r : {1, 12})
      for (int s : {1, 8})
        for (int f : {0, TDK_DEFRINGE_LINEAR, TDK_DEFRINGE_STATIC, 3 | (2 << TDK_DEFRINGE_GROUPS_SHIFT)}) ok = ok && tdk_defringe_lds_bytes(d, r, s, f) == lds;
  ok = ok && tdk_defringe_lds_bytes(2, 6, 6, 0) == 0 && tdk_defringe_lds_bytes(TDK_F32, 0, 6, 0) == 0 && tdk_defringe_lds_bytes(TDK_F32, 13, 6, 0) == 0 &&
       tdk_defringe_lds_bytes(TDK_F32, 6, 0, 0) == 0 && tdk_defringe_lds_bytes(TDK_F32, 6, 9, 0) == 0 && tdk_defringe_lds_bytes(TDK_F32, 6, 6, 4) == 0 &&
       tdk_defringe_lds_bytes(TDK_F32, 6, 6, -1) == 0;
  float out[TDK_DEFRINGE_MAX_RADIUS + 1];
  for (float sigma : {0.5f, 1.0f, 2.0f, 3.3f, 4.0f}) {
    ok = ok && tdk_defringe_weights(sigma, out, &radius) == TDK_OK && radius == (int)ceil(3.0 * (double)sigma);
    double sum = out[0];
    for (int k = 1; k <= TDK_DEFRINGE_MAX_RADIUS; k++) sum += 2.0 * out[k], ok = ok && (k <= radius ? out[k] > 0.0f && out[k] < out[k - 1] : out[k] == 0.0f);
    ok = ok && fabs(sum - 1.0) < 1e-6;
  }
  ok = ok && tdk_defringe_weights(0.49f, out, &radius) == TDK_ERR_INVALID_ARGUMENT && tdk_defringe_weights(4.01f, out, &radius) == TDK_ERR_INVALID_ARGUMENT &&
       tdk_defringe_weights(NAN, out, &radius) == TDK_ERR_INVALID_ARGUMENT && tdk_defringe_weights(2.0f, nullptr, &radius) == TDK_ERR_INVALID_ARGUMENT &&
       tdk_defringe_weights(2.0f, out, nullptr) == TDK_ERR_INVALID_ARGUMENT;
  if (!ok) {
    printf("FAIL queries\n");
    failures++;
  }
  printf("%d failures\n", failures);
  return failures != 0;
}
