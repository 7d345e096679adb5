// Stand-alone host program: the three tdk_*_weights entry points, one body in csrc/tdk_frame.h (tdk_gaussian_taps), over their sigma
// ranges and both ends just outside them; where the ranges overlap (sigma 0.5 .. 2) the three give the same bits.  For a run under a
// host sanitizer (no device is touched: the entry points make no HIP call).  Build, from the repository root:
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//     tests/hip_unit/frame_layer_main.cpp torch-darktable_amd/csrc/sharpen.hip torch-darktable_amd/csrc/deconv.hip \
//     torch-darktable_amd/csrc/defringe.hip torch-darktable_amd/csrc/runtime.hip -o frame_layer
#include <math.h>
#include <stdio.h>
#include <string.h>

#include "../../include/tdk_hip_deconv.h"
#include "../../include/tdk_hip_defringe.h"
#include "../../include/tdk_hip_sharpen.h"

static int failures = 0;

static void fail(const char* name, float sigma, const char* what) {
  printf("FAIL %s(%.9g): %s ('%s')\n", name, (double)sigma, what, tdk_last_error() ? tdk_last_error() : "(null)");
  failures++;
}

struct Entry {
  const char* name;
  int (*fn)(float, float*, int*);
  float lo, hi;
  int max_radius;
  const char* range;   // as the message spells it
};

// The taps of `e` at sigma into out[0 .. 13): a canary behind max_radius stays, the taps fall, sum to 1 and end in zeros.
static bool taps(const Entry& e, float sigma, float* out, int* radius) {
  const float canary = -77.0f;
  for (int k = 0; k <= 13; k++) out[k] = canary;
  if (e.fn(sigma, out, radius) != TDK_OK) return fail(e.name, sigma, "refused inside its range"), false;
  if (*radius != (int)ceil(3.0 * (double)sigma) || *radius > e.max_radius) return fail(e.name, sigma, "radius is not ceil(3 sigma)"), false;
  double sum = out[0];
  for (int k = 1; k <= e.max_radius; k++) {
    sum += 2.0 * out[k];
    if (k <= *radius ? !(out[k] > 0.0f && out[k] < out[k - 1]) : out[k] != 0.0f) return fail(e.name, sigma, "taps do not fall to zeros behind the radius"), false;
  }
  if (fabs(sum - 1.0) >= 1e-6) return fail(e.name, sigma, "taps do not sum to 1"), false;
  for (int k = e.max_radius + 1; k <= 13; k++)
    if (out[k] != canary) return fail(e.name, sigma, "wrote behind max_radius + 1 values"), false;
  return true;
}

static void refused(const Entry& e, float sigma, float* w, int* r, const char* word) {
  char want[96];
  snprintf(want, sizeof want, "%s: %s", e.name, word);
  const int rc = e.fn(sigma, w, r);
  if (rc != TDK_ERR_INVALID_ARGUMENT || !tdk_last_error() || strcmp(tdk_last_error(), want) != 0) fail(e.name, sigma, want);
}

int main() {
  const Entry entries[3] = {{"tdk_sharpen_weights", tdk_sharpen_weights, 0.25f, 4.0f, TDK_SHARPEN_MAX_RADIUS, "sigma must lie in [0.25, 4]"},
                            {"tdk_deconv_weights", tdk_deconv_weights, 0.3f, 2.0f, TDK_DECONV_MAX_RADIUS, "sigma must lie in [0.3, 2]"},
                            {"tdk_defringe_weights", tdk_defringe_weights, 0.5f, 4.0f, TDK_DEFRINGE_MAX_RADIUS, "sigma must lie in [0.5, 4]"}};
  float out[3][14];
  int radius[3];
  for (const Entry& e : entries) {
    for (int i = 0; i <= 64; i++) taps(e, i == 64 ? e.hi : e.lo + (e.hi - e.lo) * (float)i / 64.0f, out[0], &radius[0]);
    for (float sigma : {nextafterf(e.lo, 0.0f), nextafterf(e.hi, 8.0f), e.lo - 0.01f, e.hi + 0.01f, 0.0f, -1.0f, (float)NAN, (float)INFINITY})
      refused(e, sigma, out[0], &radius[0], e.range);
    refused(e, 1.0f, nullptr, &radius[0], "null pointer");
    refused(e, 1.0f, out[0], nullptr, "null pointer");
  }
  // one body: the same bits from all three wherever all three take the sigma
  for (int i = 0; i <= 96; i++) {
    const float sigma = i == 96 ? 2.0f : 0.5f + 1.5f * (float)i / 96.0f;
    bool ok = true;
    for (int n = 0; n < 3; n++) ok = taps(entries[n], sigma, out[n], &radius[n]) && ok;
    if (ok && (radius[0] != radius[1] || radius[0] != radius[2] || memcmp(out[0], out[1], (TDK_DECONV_MAX_RADIUS + 1) * sizeof(float)) != 0 ||
               memcmp(out[0], out[2], (TDK_DEFRINGE_MAX_RADIUS + 1) * sizeof(float)) != 0))
      fail("the three entry points", sigma, "differ in their bits");
  }
  printf("%d failures\n", failures);
  return failures != 0;
}
