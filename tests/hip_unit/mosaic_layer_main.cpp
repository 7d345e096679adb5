// Stand-alone host program: what the entry points on raw mosaics say to a size and to a pattern -- tdk_raw_prepare, tdk_highlights,
// tdk_ca_correct, tdk_noise_profile, tdk_framestats in its mosaic mode, tdk_temporal_denoise and tdk_hdr_merge share tdk_pattern_ok and
// tdk_mosaic_size_ok (csrc/tdk_frame.h) and keep their own words.  Pointers are never dereferenced (no device is touched: each call returns
// before any HIP call; a size and a pattern that pass are followed by an argument that does not), for a run under a host sanitizer.
// Build, from the repository root:
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -ffp-contract=off -Xarch_host -fsanitize=address,undefined tests/hip_unit/mosaic_layer_main.cpp \
//     torch-darktable_amd/csrc/{rawprepare,highlights,cacorrect,noiseprofile,framestats,temporal,hdrmerge,runtime}.hip -o mosaic_layer
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../../include/tdk_hip_ca.h"
#include "../../include/tdk_hip_hdr.h"
#include "../../include/tdk_hip_highlights.h"
#include "../../include/tdk_hip_noise.h"
#include "../../include/tdk_hip_raw.h"
#include "../../include/tdk_hip_stats.h"
#include "../../include/tdk_hip_temporal.h"

static int failures = 0, calls = 0;

static char* const fake = reinterpret_cast<char*>(uintptr_t(1) << 32);
static void* at(int slot) { return fake + (size_t(slot) << 24); }
static float* floats(int slot) { return reinterpret_cast<float*>(at(slot)); }
static const void* const frames[2] = {at(1), at(2)};
static const float levels[4] = {0.0f, 0.0f, 0.0f, 0.0f}, scales[4] = {1.0f, 1.0f, 1.0f, 1.0f};   // (read on the host)

// every call gets a size, a pattern and, behind them, one argument its entry point refuses: `later` is the word of that refusal
struct Entry {
  const char* name;
  const char* even;    // the first words of "... size WxH must be even in both axes (whole CFA cells)"
  const char* later;
  int lowest;          // the smallest side
  bool pattern_first;  // the pattern is looked at before the whole cells
  int (*call)(int, int, uint32_t);
};

static const Entry entries[] = {
    {"tdk_raw_prepare", "frame", "tdk_raw_prepare: min_count must be 1..4, got 0", 2, false,
     [](int w, int h, uint32_t p) {
       return tdk_raw_prepare(at(1), TDK_RAW_F32, at(3), TDK_F32, nullptr, w, h, p, levels, scales, 0, 0.02f, 0.5f, 0, nullptr, 0, 0, nullptr, 1, nullptr);
     }},
    {"tdk_highlights", "frame", "tdk_highlights: min_count must be >= 1, got 0", 2, false,
     [](int w, int h, uint32_t p) {
       return tdk_highlights(at(1), TDK_F32, at(3), TDK_F32, at(4), w, h, p, floats(5), 0.98f, 0.2f, 0, TDK_HL_OPPOSED, nullptr, nullptr);
     }},
    {"tdk_ca_correct", "mosaic", "tdk_ca_correct: interp must be 0 (bilinear) or 1 (bicubic), got 2", 2, false,
     [](int w, int h, uint32_t p) { return tdk_ca_correct(at(1), TDK_F32, at(3), TDK_F32, w, h, p, floats(5), 1.0f, 1.0f, 1.0f, 2, nullptr); }},
    {"tdk_noise_profile", "mosaic", "tdk_noise_profile: bins must be 2..32, got 1", 2, false,
     [](int w, int h, uint32_t p) {
       return tdk_noise_profile(frames, 2, TDK_F32, at(4), w, h, p, 1, 1.0f, 1, 64224, 32, reinterpret_cast<long long*>(at(6)), floats(5), floats(7), nullptr);
     }},
    {"tdk_framestats", "mosaic", "tdk_framestats: stride must be 1..65535, got 0", 1, true,
     [](int w, int h, uint32_t p) {
       return tdk_framestats(frames, 2, TDK_F32, at(4), w, h, 3, p, 0, 256, 0.0f, 1.0f, 64, nullptr, 0, reinterpret_cast<long long*>(at(6)), floats(7), nullptr);
     }},
    {"tdk_temporal_denoise", "mosaic", "tdk_temporal_denoise: radius must be 2 or 3, got 1", 2, false,
     [](int w, int h, uint32_t p) {
       return tdk_temporal_denoise(at(1), TDK_F32, at(3), TDK_F32, at(8), TDK_F32, w, h, p, floats(5), nullptr, 1, 1.5f, 3.0f, 16.0f, 8.0f, 1e-12f, nullptr);
     }},
    {"tdk_hdr_merge", "mosaic", "tdk_hdr_merge: radius must be 2 or 3, got 1", 2, false,
     [](int w, int h, uint32_t p) {
       return tdk_hdr_merge(frames, 2, TDK_F32, at(3), TDK_F32, nullptr, w, h, p, floats(7), -1, floats(5), 1, 0.95f, 1.5f, 3.0f, 16.0f, 1e-12f, nullptr);
     }},
};

static void expect(const Entry& e, int w, int h, uint32_t pattern, const char* want) {
  const int rc = e.call(w, h, pattern);
  const char* msg = tdk_last_error();
  calls++;
  if (rc != TDK_ERR_INVALID_ARGUMENT || !msg || strcmp(msg, want)) {
    printf("FAIL %s %dx%d 0x%08x: rc %d, message '%s' (expected '%s')\n", e.name, w, h, pattern, rc, msg ? msg : "(null)", want);
    failures++;
  }
}

int main() {
  const int sizes[] = {0, 1, 2, 3, 65534, 65535, 65536, 65537};
  const uint32_t patterns[] = {TDK_PATTERN_RGGB, TDK_PATTERN_BGGR, TDK_PATTERN_GRBG, TDK_PATTERN_GBRG}, words[] = {0x1234u, ~TDK_PATTERN_RGGB};
  char range[160], even[160], unknown[160];
  for (const Entry& e : entries)
    for (const int size : sizes)
      for (int axis = 0; axis < 2; axis++) {
        const int w = axis ? 8 : size, h = axis ? size : 8;
        const bool in_range = size >= e.lowest && size <= 65535, whole = size % 2 == 0;
        snprintf(range, sizeof range, "%s: frame size %dx%d outside %d..65535", e.name, w, h, e.lowest);
        snprintf(even, sizeof even, "%s: %s size %dx%d must be even in both axes (whole CFA cells)", e.name, e.even, w, h);
        for (const uint32_t pattern : patterns) expect(e, w, h, pattern, !in_range ? range : !whole ? even : e.later);
        for (const uint32_t word : words) {
          snprintf(unknown, sizeof unknown, "%s: unknown Bayer pattern 0x%08x", e.name, word);
          expect(e, w, h, word, !in_range ? range : !whole && !e.pattern_first ? even : unknown);
        }
      }
  printf("%d calls, %d failures\n", calls, failures);
  return failures != 0;
}
