// filmic.hip -- scene-referred tone mapping (include/tdk_hip_filmic.h: tdk_filmic): a curve over log2 of a pixel norm, applied to
// the channel ratios, a pull into the gamut and a display encoding, one launch, no workspace.
//
// The specification is the head comment of include/tdk_hip_filmic.h.  The kernel streams: a lane takes FM_PIX = 16 consecutive pixels
// per step, 48 elements, which are 16-byte accesses for all storage types (12 for float32, 6 for binary16, 3 for uint8).
//
// Alignment (as csrc/colorlut.hip does it, restated here).  A group of 16 pixels is a whole number of 16-byte vectors, so a buffer
// needs only its FIRST group on a 16-byte boundary: the host picks `head`, the number of pixels in front of the first group (0..15),
// so that the side with the narrower elements has its groups aligned (the destination on a tie).  The other side is vectorised when
// the same head aligns it too and moves per element otherwise (FilmicArgs::vec_in, vec_out).  The head pixels and the tail
// (npix - head) % 16 go one pixel per lane in workgroup 0.
//
// Workgroups are persistent: FM_THREADS = 512 lanes, a grid of at most three workgroups per compute unit (80 VGPRs: six waves per
// SIMD; the kernel is bound by its arithmetic, and a third workgroup measured 3 to 6 % over two), each striding over the groups.
// The tables are staged in static LDS once per workgroup, every node next to its successor:
//   fm_td[j] = {T[j], T[j+1], D[j], D[j+1]}     j = 0 .. 1023     one 16-byte read gives a lane both lerps of step 3
//   fm_g[j]  = {G[j], G[j+1]}                   j = 0 .. 511      one 8-byte read gives the lerp of step 6
// The lanes of a wave gather at unrelated indices, so the reads are wide ones: a 16-byte read moves four times the bytes per LDS
// cycle of four 4-byte reads.  The arithmetic does not know where a value came from: the bits are those of the plain tables.
// Nothing is accumulated across lanes or workgroups: the bits do not depend on scheduling.
#include <math.h>

#include "../../include/tdk_hip_filmic.h"
#include "tdk_frame.h"

namespace {

constexpr int FM_THREADS = 512;
constexpr int FM_PIX = 16, FM_EL = FM_PIX * 3;   // pixels and elements of a lane per step
constexpr int FM_WG_PER_CU = 3;
constexpr int FM_NODES = TDK_FILMIC_TABLE - 1, FM_ENC_NODES = TDK_FILMIC_ENC_TABLE - 1;
constexpr size_t FM_LDS_BYTES = sizeof(float4) * FM_NODES + sizeof(float2) * FM_ENC_NODES;
static_assert(TDK_FILMIC_TABLE == (TDK_FILMIC_EV_MAX - TDK_FILMIC_EV_MIN) * TDK_FILMIC_STEPS + 1, "entries of the curve tables");
static_assert(TDK_FILMIC_ENC_TABLE == -TDK_FILMIC_ENC_EV_MIN * TDK_FILMIC_STEPS + 1, "entries of the encoding table");
static_assert(TDK_FILMIC_STEPS == 32, "the index takes the five leading bits of the mantissa");
static_assert(FM_LDS_BYTES * FM_WG_PER_CU <= 160 * 1024 && FM_LDS_BYTES <= 64 * 1024, "three workgroups per CU, static LDS");

struct FilmicArgs {
  float w[3];
  int has_encode;
  int vec_in, vec_out;   // 16-byte accesses on the source groups, the destination groups
  int head;              // pixels in front of the first group
  int64_t npix, groups;
};

// ---- storage: the load and store of the specification
__device__ __forceinline__ float fm_ld(const float* p, int64_t i) { return p[i]; }
__device__ __forceinline__ float fm_ld(const __half* p, int64_t i) { return __half2float(p[i]); }
__device__ __forceinline__ uint32_t fm_u8(float v) { return (uint32_t)rintf(fminf(fmaxf(v, 0.0f), 1.0f) * 255.0f); }
__device__ __forceinline__ void fm_st(float* p, int64_t i, float v) { p[i] = v; }
__device__ __forceinline__ void fm_st(__half* p, int64_t i, float v) { p[i] = __float2half_rn(v); }
__device__ __forceinline__ void fm_st(uint8_t* p, int64_t i, float v) { p[i] = (uint8_t)fm_u8(v); }

// 48 consecutive elements as 16-byte vectors; p is 16-byte aligned
__device__ __forceinline__ void fm_load48(const float* p, float v[FM_EL]) {
  const float4* q = reinterpret_cast<const float4*>(p);
#pragma unroll
  for (int k = 0; k < FM_EL / 4; k++) {
    const float4 a = q[k];
    v[4 * k] = a.x, v[4 * k + 1] = a.y, v[4 * k + 2] = a.z, v[4 * k + 3] = a.w;
  }
}
__device__ __forceinline__ void fm_load48(const __half* p, float v[FM_EL]) {
  const uint4* q = reinterpret_cast<const uint4*>(p);
#pragma unroll
  for (int k = 0; k < FM_EL / 8; k++) {
    const uint4 u = q[k];
    const uint32_t w[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const float2 f = __half22float2(*reinterpret_cast<const __half2*>(&w[j]));
      v[8 * k + 2 * j] = f.x, v[8 * k + 2 * j + 1] = f.y;
    }
  }
}
__device__ __forceinline__ void fm_store48(float* p, const float v[FM_EL]) {
  float4* q = reinterpret_cast<float4*>(p);
#pragma unroll
  for (int k = 0; k < FM_EL / 4; k++) q[k] = make_float4(v[4 * k], v[4 * k + 1], v[4 * k + 2], v[4 * k + 3]);
}
__device__ __forceinline__ void fm_store48(__half* p, const float v[FM_EL]) {
  uint4* q = reinterpret_cast<uint4*>(p);
#pragma unroll
  for (int k = 0; k < FM_EL / 8; k++) {
    uint32_t w[4];
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const __half2 h = __floats2half2_rn(v[8 * k + 2 * j], v[8 * k + 2 * j + 1]);
      w[j] = *reinterpret_cast<const uint32_t*>(&h);
    }
    q[k] = make_uint4(w[0], w[1], w[2], w[3]);
  }
}
__device__ __forceinline__ void fm_store48(uint8_t* p, const float v[FM_EL]) {
  uint4* q = reinterpret_cast<uint4*>(p);
#pragma unroll
  for (int k = 0; k < FM_EL / 16; k++) {
    uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int j = 0; j < 16; j++) w[j / 4] |= fm_u8(v[16 * k + j]) << (8 * (j % 4));
    q[k] = make_uint4(w[0], w[1], w[2], w[3]);
  }
}

// ---- the steps on one pixel
__device__ __forceinline__ float fm_xmin() { return __uint_as_float(0x35800000u); }    // 2^-20
__device__ __forceinline__ float fm_xmax() { return __uint_as_float(0x457FFFFFu); }    // the largest float32 below 2^12
__device__ __forceinline__ float fm_below_one() { return __uint_as_float(0x3F7FFFFFu); }   // 1 - 2^-24

// step 3: the node index and the fraction of a value clamped into the table whose first octave is 2^ev_min
__device__ __forceinline__ int fm_index(float clamped, int ev_min, float& f) {
  const uint32_t bits = __float_as_uint(clamped);
  const int ex = (int)(bits >> 23) - 127;
  const uint32_t M = bits & 0x7FFFFFu;
  f = (float)(M & 0x3FFFFu) / 262144.0f;
  return (ex - ev_min) * TDK_FILMIC_STEPS + (int)(M >> 18);
}

// step 6
__device__ __forceinline__ float fm_encode(float o, const float2* g, float g0) {
  const float oc = fminf(tdk_pos(o), fm_below_one());
  const float lo = __uint_as_float(0x37800000u);   // 2^-16
  float f;
  const int i = fm_index(fmaxf(oc, lo), TDK_FILMIC_ENC_EV_MIN, f);
  const float2 n = g[i];
  const float curve = n.x + f * (n.y - n.x);
  const float linear = (oc * 65536.0f) * g0;
  return oc < lo ? linear : curve;
}

template <int NORM> __device__ __forceinline__ void fm_pixel(float& x0, float& x1, float& x2, float e, const float4* td, const float2* g, float g0, const FilmicArgs& a) {
  const float p0 = fminf(tdk_pos(x0 * e), fm_xmax()), p1 = fminf(tdk_pos(x1 * e), fm_xmax()), p2 = fminf(tdk_pos(x2 * e), fm_xmax());
  float o0, o1, o2;
  if constexpr (NORM == TDK_FILMIC_NONE) {
    const float p[3] = {p0, p1, p2};
    float o[3];
#pragma unroll
    for (int c = 0; c < 3; c++) {
      float f;
      const int i = fm_index(fminf(fmaxf(p[c], fm_xmin()), fm_xmax()), TDK_FILMIC_EV_MIN, f);
      const float4 n = td[i];
      o[c] = n.x + f * (n.y - n.x);
    }
    o0 = o[0], o1 = o[1], o2 = o[2];
  } else {
    float N;
    if constexpr (NORM == TDK_FILMIC_MAX) {
      N = fmaxf(fmaxf(p0, p1), p2);
    } else if constexpr (NORM == TDK_FILMIC_LUMA) {
      N = (a.w[0] * p0 + a.w[1] * p1) + a.w[2] * p2;
    } else {
      const float q0 = p0 * p0, q1 = p1 * p1, q2 = p2 * p2;
      const float k0 = q0 * p0, k1 = q1 * p1, k2 = q2 * p2;
      const float den = (q0 + q1) + q2, num = (k0 + k1) + k2;
      N = den > 0.0f ? num / den : 0.0f;
    }
    const float Nc = fminf(fmaxf(N, fm_xmin()), fm_xmax());
    float f;
    const int i = fm_index(Nc, TDK_FILMIC_EV_MIN, f);
    const float4 n = td[i];
    const float y = n.x + f * (n.y - n.x);
    const float d = n.z + f * (n.w - n.z);
    o0 = y * (1.0f + d * (p0 / Nc - 1.0f));
    o1 = y * (1.0f + d * (p1 / Nc - 1.0f));
    o2 = y * (1.0f + d * (p2 / Nc - 1.0f));
    const float m = fmaxf(fmaxf(o0, o1), o2);
    if (m > 1.0f) {
      if (y >= 1.0f) {
        o0 = o1 = o2 = 1.0f;
      } else {
        const float gain = (1.0f - y) / (m - y);
        o0 = y + (o0 - y) * gain;
        o1 = y + (o1 - y) * gain;
        o2 = y + (o2 - y) * gain;
      }
    }
  }
  if (a.has_encode) o0 = fm_encode(o0, g, g0), o1 = fm_encode(o1, g, g0), o2 = fm_encode(o2, g, g0);
  x0 = o0, x1 = o1, x2 = o2;
}

template <typename TS, typename TD, int NORM>
__global__ __launch_bounds__(FM_THREADS, 2 * FM_WG_PER_CU) void filmic_kernel(const TS* __restrict__ src, TD* __restrict__ dst, const float* __restrict__ curve,
                                                               const float* __restrict__ encode, const float* __restrict__ exposure, FilmicArgs a) {
  __shared__ __attribute__((aligned(16))) float4 fm_td[FM_NODES];
  __shared__ __attribute__((aligned(16))) float2 fm_g[FM_ENC_NODES];
  const int tid = threadIdx.x;

  // ---- the tables, once per workgroup
  for (int j = tid; j < FM_NODES; j += FM_THREADS)
    fm_td[j] = make_float4(curve[j], curve[j + 1], curve[TDK_FILMIC_TABLE + j], curve[TDK_FILMIC_TABLE + j + 1]);
  if (a.has_encode)
    for (int j = tid; j < FM_ENC_NODES; j += FM_THREADS) fm_g[j] = make_float2(encode[j], encode[j + 1]);
  const float e = exposure[0];
  const float g0 = a.has_encode ? encode[0] : 0.0f;   // G[0], the slope of the encoding's linear part: the same for every pixel
  __syncthreads();

  // ---- the groups of 16 pixels
  const int64_t step = (int64_t)gridDim.x * FM_THREADS;
  for (int64_t gi = (int64_t)blockIdx.x * FM_THREADS + tid; gi < a.groups; gi += step) {
    const int64_t el = (a.head + gi * FM_PIX) * 3;
    float v[FM_EL];
    if (a.vec_in) {
      fm_load48(src + el, v);
    } else {
#pragma unroll
      for (int i = 0; i < FM_EL; i++) v[i] = fm_ld(src, el + i);
    }
#pragma unroll
    for (int p = 0; p < FM_PIX; p++) fm_pixel<NORM>(v[3 * p], v[3 * p + 1], v[3 * p + 2], e, fm_td, fm_g, g0, a);
    if (a.vec_out) {
      fm_store48(dst + el, v);
    } else {
#pragma unroll
      for (int i = 0; i < FM_EL; i++) fm_st(dst, el + i, v[i]);
    }
  }

  // ---- head and tail, a pixel per lane
  if (blockIdx.x == 0) {
    const int64_t body = a.head + a.groups * FM_PIX;
    const int tail = (int)(a.npix - body);
    if (tid < a.head + tail) {
      const int64_t el = (tid < a.head ? (int64_t)tid : body + (tid - a.head)) * 3;
      float x0 = fm_ld(src, el), x1 = fm_ld(src, el + 1), x2 = fm_ld(src, el + 2);
      fm_pixel<NORM>(x0, x1, x2, e, fm_td, fm_g, g0, a);
      fm_st(dst, el, x0), fm_st(dst, el + 1, x1), fm_st(dst, el + 2, x2);
    }
  }
}

// the head (in pixels, 0..15) that puts the groups of buffer p on 16-byte boundaries: 3 * esz * head = -p (mod 16)
int fm_head(const void* p, size_t esz) {
  const uintptr_t units = reinterpret_cast<uintptr_t>(p) / esz;   // the address in elements (buffers are element-aligned)
  const int m = (int)(16 / esz);                                   // elements per vector: 4, 8, 16
  return (int)(((m - units % m) % m) * (m == 16 ? 11 : 3) % m);    // the inverse of 3 mod 4, 8, 16 is 3, 3, 11
}

template <typename TS, typename TD, int NORM>
int launch(const void* src, void* dst, const float* curve, const float* encode, const float* exposure, const FilmicArgs& a, hipStream_t st) {
  const int64_t want = tdk_div_up64(a.groups, FM_THREADS), cap = (int64_t)FM_WG_PER_CU * tdk_device_cus();
  const dim3 grid((unsigned)(want < 1 ? 1 : want < cap ? want : cap));
  TDK_LAUNCH("tdk_filmic", (filmic_kernel<TS, TD, NORM>), grid, dim3(FM_THREADS), 0, st, reinterpret_cast<const TS*>(src), reinterpret_cast<TD*>(dst), curve, encode,
             exposure, a);
  return TDK_OK;
}

template <typename TS, typename TD>
int dispatch_norm(int norm, const void* src, void* dst, const float* curve, const float* encode, const float* exposure, const FilmicArgs& a, hipStream_t st) {
  if (norm == TDK_FILMIC_MAX) return launch<TS, TD, TDK_FILMIC_MAX>(src, dst, curve, encode, exposure, a, st);
  if (norm == TDK_FILMIC_LUMA) return launch<TS, TD, TDK_FILMIC_LUMA>(src, dst, curve, encode, exposure, a, st);
  if (norm == TDK_FILMIC_POWER) return launch<TS, TD, TDK_FILMIC_POWER>(src, dst, curve, encode, exposure, a, st);
  return launch<TS, TD, TDK_FILMIC_NONE>(src, dst, curve, encode, exposure, a, st);
}

template <typename TS>
int dispatch_dst(int dst_dtype, int norm, const void* src, void* dst, const float* curve, const float* encode, const float* exposure, const FilmicArgs& a,
                 hipStream_t st) {
  if (dst_dtype == TDK_F32) return dispatch_norm<TS, float>(norm, src, dst, curve, encode, exposure, a, st);
  if (dst_dtype == TDK_F16) return dispatch_norm<TS, __half>(norm, src, dst, curve, encode, exposure, a, st);
  return dispatch_norm<TS, uint8_t>(norm, src, dst, curve, encode, exposure, a, st);
}

}  // namespace

TDK_EXPORT int tdk_filmic_abi_version(void) { return TDK_FILMIC_ABI_VERSION; }

TDK_EXPORT size_t tdk_filmic_lds_bytes(void) { return FM_LDS_BYTES; }

TDK_EXPORT int tdk_filmic(const void* src, void* dst, const float* curve, const float* encode, const float* exposure, int64_t npix, int src_dtype, int dst_dtype,
                          int norm, const float* weights, int flags, tdk_stream_t stream) {
  TDK_REQUIRE(src, "tdk_filmic: null pointer (src)");
  TDK_REQUIRE(dst, "tdk_filmic: null pointer (dst)");
  TDK_REQUIRE(curve, "tdk_filmic: null pointer (curve)");
  TDK_REQUIRE(exposure, "tdk_filmic: null pointer (exposure)");
  TDK_REQUIRE(weights, "tdk_filmic: null pointer (weights)");
  TDK_REQUIRE(npix >= 0, "tdk_filmic: npix must be >= 0, got %lld", (long long)npix);
  TDK_REQUIRE(tdk_float_dtype_ok(src_dtype), "tdk_filmic: unsupported source dtype tag %d (float32 or binary16)", src_dtype);
  TDK_REQUIRE(dst_dtype == TDK_F32 || dst_dtype == TDK_F16 || dst_dtype == TDK_U8, "tdk_filmic: unsupported destination dtype tag %d", dst_dtype);
  TDK_REQUIRE(norm == TDK_FILMIC_MAX || norm == TDK_FILMIC_LUMA || norm == TDK_FILMIC_POWER || norm == TDK_FILMIC_NONE,
              "tdk_filmic: norm must be TDK_FILMIC_MAX, _LUMA, _POWER or _NONE, got %d", norm);
  const int bad_weight = tdk_first_bad_weight(weights, 3);
  TDK_REQUIRE(bad_weight < 0, "tdk_filmic: weights[%d] must be finite and >= 0", bad_weight);
  TDK_REQUIRE(flags == 0, "tdk_filmic: flags is reserved and must be 0, got %d", flags);
  const size_t ssz = tdk_dtype_bytes(src_dtype), dsz = tdk_dtype_bytes(dst_dtype);
  TDK_REQUIRE(tdk_aligned(src, ssz), "tdk_filmic: src must be aligned to its elements (%zu bytes)", ssz);
  TDK_REQUIRE(tdk_aligned(dst, dsz), "tdk_filmic: dst must be aligned to its elements (%zu bytes)", dsz);
  TDK_REQUIRE(tdk_aligned(curve, 4), "tdk_filmic: curve must be aligned to 4 bytes");
  TDK_REQUIRE(!encode || tdk_aligned(encode, 4), "tdk_filmic: encode must be aligned to 4 bytes");
  TDK_REQUIRE(tdk_aligned(exposure, 4), "tdk_filmic: exposure must be aligned to 4 bytes");
  TDK_REQUIRE((uint64_t)npix <= (uint64_t)INT64_MAX / 16, "tdk_filmic: npix is too large, got %lld", (long long)npix);
  const size_t src_bytes = (size_t)npix * 3 * ssz, dst_bytes = (size_t)npix * 3 * dsz;
  if (npix > 0) {
    TDK_REQUIRE(tdk_disjoint(src, src_bytes, dst, dst_bytes), "tdk_filmic: src and dst overlap (in-place use is not supported)");
    TDK_REQUIRE(tdk_disjoint(curve, sizeof(float) * 2 * TDK_FILMIC_TABLE, dst, dst_bytes), "tdk_filmic: curve and dst overlap");
    TDK_REQUIRE(!encode || tdk_disjoint(encode, sizeof(float) * TDK_FILMIC_ENC_TABLE, dst, dst_bytes), "tdk_filmic: encode and dst overlap");
    TDK_REQUIRE(tdk_disjoint(exposure, sizeof(float), dst, dst_bytes), "tdk_filmic: exposure and dst overlap");
  }
  if (npix == 0) return TDK_OK;

  FilmicArgs a{};
  for (int c = 0; c < 3; c++) a.w[c] = weights[c];
  a.has_encode = encode != nullptr;
  a.npix = npix;
  // the head that aligns the side with the narrower elements (the stricter demand; the destination on a tie); the other side is
  // vectorised when the same head aligns it
  const int hs = fm_head(src, ssz), hd = fm_head(dst, dsz);
  const int ms = (int)(16 / ssz), md = (int)(16 / dsz);
  const int head = ms > md ? hs : hd;
  a.vec_in = head % ms == hs % ms, a.vec_out = head % md == hd % md;
  a.head = (int)(npix < head ? npix : head);
  a.groups = (npix - a.head) / FM_PIX;
  hipStream_t st = tdk_stream(stream);
  if (src_dtype == TDK_F32) return dispatch_dst<float>(dst_dtype, norm, src, dst, curve, encode, exposure, a, st);
  return dispatch_dst<__half>(dst_dtype, norm, src, dst, curve, encode, exposure, a, st);
}
