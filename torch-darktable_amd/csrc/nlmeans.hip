// nlmeans.hip -- non-local means (include/tdk_hip_denoise.h: tdk_nlmeans), one launch, no workspace.
//
// A workgroup of four waves owns a tile of (64 - 2P) x 32 output pixels.  The tile and its S + P halo are staged once in LDS as
// C planes with the edge replication resolved at load time, so everything after the barrier indexes LDS without a clamp.
// A lane owns one image column and eight output rows: its own 8 + 2P patch-row samples stay in registers for the whole search,
// and per offset d it reads the 8 + 2P samples of column x + dx from LDS, forms the weighted squared difference of each row,
// sums 2P + 1 of them down its column (direct sums: a running sum would cancel, and D / h^2 amplifies what is left), and sums
// 2P + 1 columns across neighbouring lanes with whole-wave DPP shifts (wave_shr:1 / wave_shl:1, no LDS traffic).  The P lanes at
// either end of a wave have no complete neighbourhood: they only feed their neighbours, hence 64 - 2P output columns per wave.
// Sum(w) and Sum(w (x(p) - x(p+d))) stay in registers across all offsets; the result is x(p) - Sum(w diff) / Sum(w), which is
// the specified quotient with the centre pixel factored out: a constant image comes back exactly, and the sums stay small.
// Nothing is accumulated across lanes or workgroups, so the bits do not depend on scheduling.
//
// Memory traffic is one read of the tile (plus halo) and one write per pixel against (2S + 1)^2 offsets of arithmetic, well under
// 1 % of the kernel's time, so there is a single element-wise staging and store path: it holds at any element alignment and any
// width, and the aligned and the offset call run the same instructions.
#include <float.h>
#include <math.h>

#include "../../include/tdk_hip_denoise.h"
#include "tdk_frame.h"

namespace {

constexpr int NLM_ROWS = 8;                    // output rows per lane
constexpr int NLM_WAVES = 4;                   // waves per workgroup, stacked vertically
constexpr int NLM_TH = NLM_ROWS * NLM_WAVES;   // tile height
constexpr int NLM_MAX_S = 10, NLM_MAX_P = 4;
// LDS row stride, the same for every S: the patch rows of a column then sit at compile-time offsets from one address per plane
constexpr int NLM_LW = 64 + 2 * NLM_MAX_S;

struct NlmArgs {
  int width, height, S;
  float negk;   // -log2(e) / ((2P + 1)^2 h^2): w = exp2(sum * negk)
  float cw[3];
};

static inline size_t lds_bytes(int S, int P, int C) { return (size_t)C * (NLM_TH + 2 * (S + P)) * NLM_LW * sizeof(float); }

// whole-wave shifts by one lane; the lane shifted in at the end reads 0 (bound_ctrl)
__device__ __forceinline__ float from_left(float v) {   // lane i <- lane i - 1
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x138 /* wave_shr:1 */, 0xf, 0xf, true));
}
__device__ __forceinline__ float from_right(float v) {  // lane i <- lane i + 1
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x130 /* wave_shl:1 */, 0xf, 0xf, true));
}
// v(x - P) + ... + v(x + P) over lanes, 2P shifted adds
template <int P> __device__ __forceinline__ float lane_box_sum(float v) {
  float a = v, b = v;
#pragma unroll
  for (int k = 0; k < P; k++) a = from_left(a) + v;        // v(x) + ... + v(x - P)
#pragma unroll
  for (int k = 1; k < P; k++) b = from_right(b) + v;       // v(x) + ... + v(x + P - 1)
  return from_right(b) + a;
}

template <typename T, int C, int P> __global__ __launch_bounds__(64 * NLM_WAVES) void nlmeans_kernel(const T* __restrict__ in, T* __restrict__ out, NlmArgs a) {
  extern __shared__ float lds[];   // C planes of LH rows, 64 + 2S of the NLM_LW columns of a row in use
  constexpr int ER = NLM_ROWS + 2 * P;   // patch rows a lane's eight outputs touch
  constexpr int TW = 64 - 2 * P;
  const int W = a.width, H = a.height, S = a.S;
  constexpr int LW = NLM_LW;
  const int LH = NLM_TH + 2 * (S + P), used = 64 + 2 * S;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int ox = (int)blockIdx.x * TW - P - S;   // image position of the LDS plane's (0, 0)
  const int oy = (int)blockIdx.y * NLM_TH - P - S;

  for (int i = wave; i < LH; i += NLM_WAVES) {
    const int cy = min(max(oy + i, 0), H - 1);
    const T* row = in + (size_t)cy * W * C;
    for (int k = lane; k < used * C; k += 64) {
      const int j = k / C, c = k - j * C;
      const int cx = min(max(ox + j, 0), W - 1);
      lds[(c * LH + i) * LW + j] = ld(row, (size_t)cx * C + c);
    }
  }
  __syncthreads();

  const int r0 = wave * NLM_ROWS;
  const int gx = (int)blockIdx.x * TW - P + lane;      // this lane's image column (the end lanes: neighbours' halo)
  const int gy0 = (int)blockIdx.y * NLM_TH + r0;       // image row of this lane's first output
  const float* base = lds + (r0 + S) * LW + lane + S;  // patch row 0 (image row gy0 - P) of this lane's column
  const int plane = LH * LW;

  float own[ER][C];
#pragma unroll
  for (int k = 0; k < ER; k++)
#pragma unroll
    for (int c = 0; c < C; c++) own[k][c] = base[c * plane + k * LW];

  // The loop-invariant factors live in VGPRs: a VALU instruction with an SGPR source issues at half rate on gfx950 (DESIGN.md
  // §3.0), and they are read 3 (8 + 2P) + 8 times per offset.  The empty asm keeps hipcc from moving them back.
  float cw[C], negk = a.negk;
#pragma unroll
  for (int c = 0; c < C; c++) {
    cw[c] = a.cw[c];
    asm volatile("" : "+v"(cw[c]));
  }
  asm volatile("" : "+v"(negk));

  float wsum[NLM_ROWS], acc[NLM_ROWS][C];
#pragma unroll
  for (int r = 0; r < NLM_ROWS; r++) {
    wsum[r] = 0.0f;
#pragma unroll
    for (int c = 0; c < C; c++) acc[r][c] = 0.0f;
  }

  for (int dy = -S; dy <= S; dy++) {
    for (int dx = -S; dx <= S; dx++) {
      const float* q = base + dy * LW + dx;
      const bool col_ok = (unsigned)(gx + dx) < (unsigned)W;
      float e[ER], diff[NLM_ROWS][C];
#pragma unroll
      for (int k = 0; k < ER; k++) {
        float s = 0.0f;
#pragma unroll
        for (int c = 0; c < C; c++) {
          const float d = own[k][c] - q[c * plane + k * LW];
          s = c == 0 ? (d * cw[0]) * d : fmaf(d * cw[c], d, s);
          if (k >= P && k < P + NLM_ROWS) diff[k - P][c] = d;
        }
        e[k] = s;
      }
#pragma unroll
      for (int r = 0; r < NLM_ROWS; r++) {
        float v = e[r];
#pragma unroll
        for (int t = 1; t <= 2 * P; t++) v += e[r + t];
        float w = __builtin_amdgcn_exp2f(lane_box_sum<P>(v) * negk);
        w = (col_ok && (unsigned)(gy0 + r + dy) < (unsigned)H) ? w : 0.0f;   // a candidate outside the image is skipped
        wsum[r] += w;
#pragma unroll
        for (int c = 0; c < C; c++) acc[r][c] = fmaf(w, diff[r][c], acc[r][c]);
      }
    }
  }

  if (lane >= P && lane < 64 - P && gx < W) {
#pragma unroll
    for (int r = 0; r < NLM_ROWS; r++) {
      const int gy = gy0 + r;
      if (gy < H) {
#pragma unroll
        for (int c = 0; c < C; c++) st(out, ((size_t)gy * W + gx) * C + c, own[r + P][c] - acc[r][c] / wsum[r]);
      }
    }
  }
}

template <typename T, int C, int P> int launch_p(const void* image, void* out, const NlmArgs& a, hipStream_t st) {
  const dim3 grid((unsigned)tdk_div_up(a.width, 64 - 2 * P), (unsigned)tdk_div_up(a.height, NLM_TH));
  const size_t lds = lds_bytes(a.S, P, C);
  TDK_LAUNCH("tdk_nlmeans", (nlmeans_kernel<T, C, P>), grid, dim3(64 * NLM_WAVES), lds, st, reinterpret_cast<const T*>(image), reinterpret_cast<T*>(out), a);
  return TDK_OK;
}

template <typename T, int C> int launch(const void* image, void* out, int P, const NlmArgs& a, hipStream_t st) {
  switch (P) {
    case 1: return launch_p<T, C, 1>(image, out, a, st);
    case 2: return launch_p<T, C, 2>(image, out, a, st);
    case 3: return launch_p<T, C, 3>(image, out, a, st);
    default: return launch_p<T, C, 4>(image, out, a, st);
  }
}

}  // namespace

TDK_EXPORT int tdk_denoise_abi_version(void) { return TDK_DENOISE_ABI_VERSION; }

TDK_EXPORT size_t tdk_nlmeans_lds_bytes(int search_radius, int patch_radius, int channels) {
  if (search_radius < 1 || search_radius > NLM_MAX_S || patch_radius < 1 || patch_radius > NLM_MAX_P || (channels != 1 && channels != 3)) return 0;
  return lds_bytes(search_radius, patch_radius, channels);
}

TDK_EXPORT int tdk_nlmeans(const void* image, void* out, int width, int height, int channels, int dtype, int search_radius, int patch_radius, float h,
                           const float* host_channel_weights, tdk_stream_t stream) {
  TDK_REQUIRE(image && out, "tdk_nlmeans: null pointer");
  TDK_REQUIRE(width > 0 && height > 0 && width <= (1 << 20) && height <= (1 << 20), "tdk_nlmeans: image %dx%d outside 1..2^20", width, height);
  TDK_REQUIRE(channels == 1 || channels == 3, "tdk_nlmeans: channels must be 1 or 3, got %d", channels);
  TDK_REQUIRE(dtype == TDK_F32 || dtype == TDK_F16, "tdk_nlmeans: unsupported dtype tag %d", dtype);
  TDK_REQUIRE(search_radius >= 1 && search_radius <= NLM_MAX_S, "tdk_nlmeans: search_radius %d outside 1..%d", search_radius, NLM_MAX_S);
  TDK_REQUIRE(patch_radius >= 1 && patch_radius <= NLM_MAX_P, "tdk_nlmeans: patch_radius %d outside 1..%d", patch_radius, NLM_MAX_P);
  TDK_REQUIRE(isfinite(h) && h > 0.0f, "tdk_nlmeans: h must be positive and finite");
  const size_t bytes = (size_t)width * height * channels * tdk_dtype_bytes(dtype);
  TDK_REQUIRE(tdk_disjoint(image, bytes, out, bytes), "tdk_nlmeans: image and out overlap (every output reads its neighbours)");
  NlmArgs a;
  a.width = width;
  a.height = height;
  a.S = search_radius;
  float total = 0.0f;
  for (int c = 0; c < 3; c++) {
    a.cw[c] = c < channels ? (host_channel_weights ? host_channel_weights[c] : 1.0f) : 0.0f;
    TDK_REQUIRE(isfinite(a.cw[c]) && a.cw[c] >= 0.0f, "tdk_nlmeans: channel weight %d must be finite and not negative", c);
    total += a.cw[c];
  }
  TDK_REQUIRE(total > 0.0f, "tdk_nlmeans: the channel weights are all zero");
  const int side = 2 * patch_radius + 1;
  // a tiny h overflows the factor: the largest finite one gives the same weights (1 where the patches are equal, else 0)
  a.negk = (float)fmax(-1.4426950408889634 / ((double)(side * side) * (double)h * (double)h), -(double)FLT_MAX);
  hipStream_t st = tdk_stream(stream);
  if (dtype == TDK_F32) return channels == 1 ? launch<float, 1>(image, out, patch_radius, a, st) : launch<float, 3>(image, out, patch_radius, a, st);
  return channels == 1 ? launch<__half, 1>(image, out, patch_radius, a, st) : launch<__half, 3>(image, out, patch_radius, a, st);
}
