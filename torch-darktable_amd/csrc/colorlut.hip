// colorlut.hip -- 3x3 matrix, shaper curves and a 3D LUT on every pixel (include/tdk_hip_lut.h: tdk_color_lut), one launch, no
// workspace.
//
// The specification is the head comment of include/tdk_hip_lut.h.  The kernel streams: a lane takes CL_PIX = 16 consecutive pixels
// per step, 48 elements, which are 16-byte accesses for all three storage types (12 for float32, 6 for binary16, 3 for uint8).
//
// Alignment.  A group of 16 pixels is a whole number of 16-byte vectors, so a buffer needs only its FIRST group on a 16-byte
// boundary: the host picks `head`, the number of pixels in front of the first group (0..15), so that the destination's groups are
// aligned -- or the source's, where the source has the narrower elements and so the stricter demand.  The other side is
// vectorised when the same head aligns it too (the usual case: both buffers come from an aligned allocation) and moves per
// element otherwise (LutArgs::vec_in, vec_out).  The head pixels and the tail (npix - head) % 16 go one pixel per lane in workgroup 0.
//
// Workgroups are persistent: CL_THREADS = 512 lanes, a grid of at most two workgroups per compute unit (128 VGPRs: four waves per
// SIMD), each striding over the groups.  The tables are loaded into LDS once per workgroup:
//   [0, 3 N^3)            the nodes of the 3D LUT, 12 bytes each, in memory order -- only in the staged kernels (NODES_LDS)
//   [3 N^3, + tables*S)   the shaper tables
// A lane's four (tetrahedral) or eight (trilinear) nodes are read as three 32-bit words each; in the other kernels the same offsets
// index the LUT in global memory (431 KB at N = 33, 3.3 MB at N = 65: resident in the 4 MiB L2 of an XCD).  Both give the same bits:
// the arithmetic does not know where a node came from.
//
// Tetrahedral interpolation selects its nodes by index arithmetic, not by branch: the three (fraction, stride) pairs are sorted by
// three compare-and-swap steps (strict comparisons on neighbours: a stable sort, ties stay in the order r, g, b) and the walk adds
// the strides in that order.
// Nothing is accumulated across lanes or workgroups: the bits do not depend on scheduling.
#include <math.h>

#include "../../include/tdk_hip_lut.h"
#include "tdk_frame.h"

namespace {

constexpr int CL_THREADS = 512;
constexpr int CL_PIX = 16, CL_EL = CL_PIX * 3;   // pixels and elements of a lane per step
constexpr int CL_WG_PER_CU = 2;
constexpr size_t CL_LDS_PLAIN = 64 * 1024;       // the dynamic-LDS size a kernel gets without raising its limit
static_assert(TDK_LUT_LDS_BUDGET * CL_WG_PER_CU <= 160 * 1024, "two workgroups per CU");
static_assert(12 * 17 * 17 * 17 + 4 * 3 * TDK_LUT_MAX_SHAPER <= TDK_LUT_LDS_BUDGET, "N = 17 is staged beside any shaper");

struct LutArgs {
  float m[9];
  float sh_lo, sh_scale, sh_top;             // sh_top = (float)(S - 1)
  float lut_lo[3], lut_scale[3], lut_top;    // lut_top = (float)(N - 1)
  int has_matrix, S, table_stride;           // S = 0: no shaper; table_stride = S with three tables, 0 with one
  int N, trilinear;                          // N = 0: no LUT
  int vec_in, vec_out, lut_vec;              // 16-byte accesses on the source groups, the destination groups, the LUT fill
  int head;                                  // pixels in front of the first group
  int64_t npix, groups;
};

// ---- storage: the load and store of the specification (they differ from ld / st of tdk_common.h in the uint8 scale)
__device__ __forceinline__ float cl_c255() { return __uint_as_float(0x3B808081u); }
__device__ __forceinline__ float cl_ld(const float* p, int64_t i) { return p[i]; }
__device__ __forceinline__ float cl_ld(const __half* p, int64_t i) { return __half2float(p[i]); }
__device__ __forceinline__ float cl_ld(const uint8_t* p, int64_t i) { return (float)p[i] * cl_c255(); }
__device__ __forceinline__ uint32_t cl_u8(float v) { return (uint32_t)rintf(fminf(fmaxf(v, 0.0f), 1.0f) * 255.0f); }
__device__ __forceinline__ void cl_st(float* p, int64_t i, float v) { p[i] = v; }
__device__ __forceinline__ void cl_st(__half* p, int64_t i, float v) { p[i] = __float2half_rn(v); }
__device__ __forceinline__ void cl_st(uint8_t* p, int64_t i, float v) { p[i] = (uint8_t)cl_u8(v); }

// 48 consecutive elements as 16-byte vectors; p is 16-byte aligned
__device__ __forceinline__ void cl_load48(const float* p, float v[CL_EL]) {
  const float4* q = reinterpret_cast<const float4*>(p);
#pragma unroll
  for (int k = 0; k < CL_EL / 4; k++) {
    const float4 a = q[k];
    v[4 * k] = a.x, v[4 * k + 1] = a.y, v[4 * k + 2] = a.z, v[4 * k + 3] = a.w;
  }
}
__device__ __forceinline__ void cl_load48(const __half* p, float v[CL_EL]) {
  const uint4* q = reinterpret_cast<const uint4*>(p);
#pragma unroll
  for (int k = 0; k < CL_EL / 8; k++) {
    const uint4 u = q[k];
    const uint32_t w[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const float2 f = __half22float2(*reinterpret_cast<const __half2*>(&w[j]));
      v[8 * k + 2 * j] = f.x, v[8 * k + 2 * j + 1] = f.y;
    }
  }
}
__device__ __forceinline__ void cl_load48(const uint8_t* p, float v[CL_EL]) {
  const uint4* q = reinterpret_cast<const uint4*>(p);
#pragma unroll
  for (int k = 0; k < CL_EL / 16; k++) {
    const uint4 u = q[k];
    const uint32_t w[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
    for (int j = 0; j < 16; j++) v[16 * k + j] = (float)((w[j / 4] >> (8 * (j % 4))) & 0xffu) * cl_c255();
  }
}
__device__ __forceinline__ void cl_store48(float* p, const float v[CL_EL]) {
  float4* q = reinterpret_cast<float4*>(p);
#pragma unroll
  for (int k = 0; k < CL_EL / 4; k++) q[k] = make_float4(v[4 * k], v[4 * k + 1], v[4 * k + 2], v[4 * k + 3]);
}
__device__ __forceinline__ void cl_store48(__half* p, const float v[CL_EL]) {
  uint4* q = reinterpret_cast<uint4*>(p);
#pragma unroll
  for (int k = 0; k < CL_EL / 8; k++) {
    uint32_t w[4];
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const __half2 h = __floats2half2_rn(v[8 * k + 2 * j], v[8 * k + 2 * j + 1]);
      w[j] = *reinterpret_cast<const uint32_t*>(&h);
    }
    q[k] = make_uint4(w[0], w[1], w[2], w[3]);
  }
}
__device__ __forceinline__ void cl_store48(uint8_t* p, const float v[CL_EL]) {
  uint4* q = reinterpret_cast<uint4*>(p);
#pragma unroll
  for (int k = 0; k < CL_EL / 16; k++) {
    uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int j = 0; j < 16; j++) w[j / 4] |= cl_u8(v[16 * k + j]) << (8 * (j % 4));
    q[k] = make_uint4(w[0], w[1], w[2], w[3]);
  }
}

// ---- the three stages on one pixel.  `sh` is the shaper in LDS; `nodes` the LUT, in LDS or in global memory.
__device__ __forceinline__ float cl_shape(float x, const float* T, const LutArgs& a) {
  const float t = fminf(fmaxf((x - a.sh_lo) * a.sh_scale, 0.0f), a.sh_top);
  const int k = min((int)t, a.S - 2);
  const float f = t - (float)k;
  const float t0 = T[k], t1 = T[k + 1];
  return t0 + f * (t1 - t0);
}

__device__ __forceinline__ float cl_lerp(float p, float q, float f) { return p + f * (q - p); }

// compare-and-swap of two (fraction, stride) pairs: afterwards fa >= fb; equal fractions stay as they are
__device__ __forceinline__ void cl_order(float& fa, int& da, float& fb, int& db) {
  const bool s = fb > fa;
  const float f0 = s ? fb : fa, f1 = s ? fa : fb;
  const int d0 = s ? db : da, d1 = s ? da : db;
  fa = f0, fb = f1, da = d0, db = d1;
}

template <typename P> __device__ __forceinline__ void cl_lut(float& r, float& g, float& b, P nodes, const LutArgs& a) {
  const int N = a.N;
  const float tr = fminf(fmaxf((r - a.lut_lo[0]) * a.lut_scale[0], 0.0f), a.lut_top);
  const float tg = fminf(fmaxf((g - a.lut_lo[1]) * a.lut_scale[1], 0.0f), a.lut_top);
  const float tb = fminf(fmaxf((b - a.lut_lo[2]) * a.lut_scale[2], 0.0f), a.lut_top);
  const int kr = min((int)tr, N - 2), kg = min((int)tg, N - 2), kb = min((int)tb, N - 2);
  const float fr = tr - (float)kr, fg = tg - (float)kg, fb = tb - (float)kb;
  const int sr = 3, sg = 3 * N, sb = 3 * N * N;       // element strides of the three axes
  const int o = ((kb * N + kg) * N + kr) * 3;
  float out[3];
  if (a.trilinear) {
    const int o10 = o + sg, o01 = o + sb, o11 = o + sg + sb;
#pragma unroll
    for (int c = 0; c < 3; c++) {
      const float c00 = cl_lerp(nodes[o + c], nodes[o + sr + c], fr);
      const float c10 = cl_lerp(nodes[o10 + c], nodes[o10 + sr + c], fr);
      const float c01 = cl_lerp(nodes[o01 + c], nodes[o01 + sr + c], fr);
      const float c11 = cl_lerp(nodes[o11 + c], nodes[o11 + sr + c], fr);
      out[c] = cl_lerp(cl_lerp(c00, c10, fg), cl_lerp(c01, c11, fg), fb);
    }
  } else {
    float f0 = fr, f1 = fg, f2 = fb;
    int d0 = sr, d1 = sg, d2 = sb;
    cl_order(f0, d0, f1, d1);
    cl_order(f1, d1, f2, d2);
    cl_order(f0, d0, f1, d1);
    const int o1 = o + d0, o2 = o1 + d1, o3 = o2 + d2;
#pragma unroll
    for (int c = 0; c < 3; c++) {
      const float l0 = nodes[o + c], l1 = nodes[o1 + c], l2 = nodes[o2 + c], l3 = nodes[o3 + c];
      out[c] = ((l0 + f0 * (l1 - l0)) + f1 * (l2 - l1)) + f2 * (l3 - l2);
    }
  }
  r = out[0], g = out[1], b = out[2];
}

template <typename P> __device__ __forceinline__ void cl_pixel(float& r, float& g, float& b, const float* sh, P nodes, const LutArgs& a) {
  if (a.has_matrix) {
    const float x = r, y = g, z = b;
    r = (a.m[0] * x + a.m[1] * y) + a.m[2] * z;
    g = (a.m[3] * x + a.m[4] * y) + a.m[5] * z;
    b = (a.m[6] * x + a.m[7] * y) + a.m[8] * z;
  }
  if (a.S) {
    r = cl_shape(r, sh, a);
    g = cl_shape(g, sh + a.table_stride, a);
    b = cl_shape(b, sh + 2 * a.table_stride, a);
  }
  if (a.N) cl_lut(r, g, b, nodes, a);
}

template <typename TS, typename TD, bool NODES_LDS>
__global__ __launch_bounds__(CL_THREADS, 4) void colorlut_kernel(const TS* __restrict__ src, TD* __restrict__ dst, const float* __restrict__ shaper,
                                                                 const float* __restrict__ lut, LutArgs a) {
  extern __shared__ __attribute__((aligned(16))) float cl_lds[];
  const int tid = threadIdx.x;
  const int lut_floats = NODES_LDS ? 3 * a.N * a.N * a.N : 0, sh_floats = a.S ? (a.table_stride ? 3 * a.S : a.S) : 0;
  float* sh = cl_lds + lut_floats;

  // ---- the tables, once per workgroup
  if constexpr (NODES_LDS) {
    const int n4 = a.lut_vec ? lut_floats / 4 : 0;
    for (int i = tid; i < n4; i += CL_THREADS) reinterpret_cast<float4*>(cl_lds)[i] = reinterpret_cast<const float4*>(lut)[i];
    for (int i = 4 * n4 + tid; i < lut_floats; i += CL_THREADS) cl_lds[i] = lut[i];
  }
  for (int i = tid; i < sh_floats; i += CL_THREADS) sh[i] = shaper[i];
  if (NODES_LDS || sh_floats) __syncthreads();

  // ---- the groups of 16 pixels
  const int64_t step = (int64_t)gridDim.x * CL_THREADS;
  for (int64_t gi = (int64_t)blockIdx.x * CL_THREADS + tid; gi < a.groups; gi += step) {
    const int64_t e = (a.head + gi * CL_PIX) * 3;
    float v[CL_EL];
    if (a.vec_in) {
      cl_load48(src + e, v);
    } else {
#pragma unroll
      for (int i = 0; i < CL_EL; i++) v[i] = cl_ld(src, e + i);
    }
#pragma unroll
    for (int p = 0; p < CL_PIX; p++) {
      if constexpr (NODES_LDS) cl_pixel(v[3 * p], v[3 * p + 1], v[3 * p + 2], sh, (const float*)cl_lds, a);
      else cl_pixel(v[3 * p], v[3 * p + 1], v[3 * p + 2], sh, lut, a);
    }
    if (a.vec_out) {
      cl_store48(dst + e, v);
    } else {
#pragma unroll
      for (int i = 0; i < CL_EL; i++) cl_st(dst, e + i, v[i]);
    }
  }

  // ---- head and tail, a pixel per lane
  if (blockIdx.x == 0) {
    const int64_t body = a.head + a.groups * CL_PIX;
    const int tail = (int)(a.npix - body);
    if (tid < a.head + tail) {
      const int64_t e = (tid < a.head ? (int64_t)tid : body + (tid - a.head)) * 3;
      float r = cl_ld(src, e), g = cl_ld(src, e + 1), b = cl_ld(src, e + 2);
      if constexpr (NODES_LDS) cl_pixel(r, g, b, sh, (const float*)cl_lds, a);
      else cl_pixel(r, g, b, sh, lut, a);
      cl_st(dst, e, r), cl_st(dst, e + 1, g), cl_st(dst, e + 2, b);
    }
  }
}

// the head (in pixels, 0..15) that puts the groups of buffer p on 16-byte boundaries: 3 * esz * head = -p (mod 16)
int cl_head(const void* p, size_t esz) {
  const uintptr_t units = reinterpret_cast<uintptr_t>(p) / esz;   // the address in elements (buffers are element-aligned)
  const int m = (int)(16 / esz);                                   // elements per vector: 4, 8, 16
  return (int)(((m - units % m) % m) * (m == 4 ? 3 : m == 8 ? 3 : 11) % m);   // the inverse of 3 mod 4, 8, 16 is 3, 3, 11
}

size_t cl_shaper_bytes(int shaper_size, int shaper_tables) { return sizeof(float) * (size_t)shaper_size * shaper_tables; }
size_t cl_node_bytes(int lut_size) { return 3 * sizeof(float) * (size_t)lut_size * lut_size * lut_size; }
bool cl_staged(int shaper_size, int shaper_tables, int lut_size, int flags) {
  return lut_size && !(flags & TDK_LUT_GLOBAL) && cl_node_bytes(lut_size) + cl_shaper_bytes(shaper_size, shaper_tables) <= TDK_LUT_LDS_BUDGET;
}

// 0: fine; otherwise which argument is wrong (messages in tdk_color_lut).  A size of 0 is a stage left out.
int cl_check(int shaper_size, int shaper_tables, int lut_size, int flags) {
  if (shaper_size != 0 && (shaper_size < 2 || shaper_size > TDK_LUT_MAX_SHAPER)) return 1;
  if (shaper_tables != 1 && shaper_tables != 3) return 2;
  if (lut_size != 0 && (lut_size < 2 || lut_size > TDK_LUT_MAX_SIZE)) return 3;
  if (flags != 0 && flags != TDK_LUT_GLOBAL) return 4;
  return 0;
}

template <typename TS, typename TD, bool NODES_LDS>
int launch(const void* src, void* dst, const float* shaper, const float* lut, const LutArgs& a, size_t lds, hipStream_t st) {
  if (lds > CL_LDS_PLAIN) {
    const int rc = tdk_raise_lds_limit(reinterpret_cast<const void*>(&colorlut_kernel<TS, TD, NODES_LDS>), TDK_LUT_LDS_BUDGET, "tdk_color_lut(hipFuncSetAttribute)");
    if (rc != TDK_OK) return rc;
  }
  const int64_t want = tdk_div_up64(a.groups, CL_THREADS), cap = (int64_t)CL_WG_PER_CU * tdk_device_cus();
  const dim3 grid((unsigned)(want < 1 ? 1 : want < cap ? want : cap));
  TDK_LAUNCH("tdk_color_lut", (colorlut_kernel<TS, TD, NODES_LDS>), grid, dim3(CL_THREADS), lds, st, reinterpret_cast<const TS*>(src), reinterpret_cast<TD*>(dst),
             shaper, lut, a);
  return TDK_OK;
}

template <typename TS> int dispatch_dst(int dst_dtype, bool staged, const void* src, void* dst, const float* shaper, const float* lut, const LutArgs& a, size_t lds,
                                        hipStream_t st) {
  if (staged) {
    if (dst_dtype == TDK_F32) return launch<TS, float, true>(src, dst, shaper, lut, a, lds, st);
    if (dst_dtype == TDK_F16) return launch<TS, __half, true>(src, dst, shaper, lut, a, lds, st);
    return launch<TS, uint8_t, true>(src, dst, shaper, lut, a, lds, st);
  }
  if (dst_dtype == TDK_F32) return launch<TS, float, false>(src, dst, shaper, lut, a, lds, st);
  if (dst_dtype == TDK_F16) return launch<TS, __half, false>(src, dst, shaper, lut, a, lds, st);
  return launch<TS, uint8_t, false>(src, dst, shaper, lut, a, lds, st);
}

bool cl_dtype_ok(int dtype) { return dtype == TDK_F32 || dtype == TDK_F16 || dtype == TDK_U8; }

}  // namespace

TDK_EXPORT int tdk_lut_abi_version(void) { return TDK_LUT_ABI_VERSION; }

TDK_EXPORT size_t tdk_lut_lds_bytes(int shaper_size, int shaper_tables, int lut_size, int flags) {
  if (cl_check(shaper_size, shaper_tables, lut_size, flags) != 0) return 0;
  return cl_shaper_bytes(shaper_size, shaper_tables) + (cl_staged(shaper_size, shaper_tables, lut_size, flags) ? cl_node_bytes(lut_size) : 0);
}

TDK_EXPORT int tdk_color_lut(const void* src, int src_dtype, void* dst, int dst_dtype, int64_t npix, const float* matrix, const float* shaper, int shaper_size,
                             int shaper_tables, float shaper_lo, float shaper_scale, const float* lut, int lut_size, const float* lut_lo, const float* lut_scale,
                             int interp, int flags, tdk_stream_t stream) {
  TDK_REQUIRE(src && dst, "tdk_color_lut: null pointer (src or dst)");
  TDK_REQUIRE(npix >= 0, "tdk_color_lut: npix must be >= 0, got %lld", (long long)npix);
  TDK_REQUIRE(cl_dtype_ok(src_dtype), "tdk_color_lut: unsupported source dtype tag %d", src_dtype);
  TDK_REQUIRE(cl_dtype_ok(dst_dtype), "tdk_color_lut: unsupported destination dtype tag %d", dst_dtype);
  if (!shaper) shaper_size = 0, shaper_tables = 1;   // a stage left out: its parameters are not read
  if (!lut) lut_size = 0;
  TDK_REQUIRE(!shaper || shaper_size != 0, "tdk_color_lut: shaper_size must be 2..%d, got 0", TDK_LUT_MAX_SHAPER);
  TDK_REQUIRE(!lut || lut_size != 0, "tdk_color_lut: lut_size must be 2..%d, got 0", TDK_LUT_MAX_SIZE);
  const int bad = cl_check(shaper_size, shaper_tables, lut_size, flags);
  TDK_REQUIRE(bad != 1, "tdk_color_lut: shaper_size must be 2..%d, got %d", TDK_LUT_MAX_SHAPER, shaper_size);
  TDK_REQUIRE(bad != 2, "tdk_color_lut: shaper_tables must be 1 or 3, got %d", shaper_tables);
  TDK_REQUIRE(bad != 3, "tdk_color_lut: lut_size must be 2..%d, got %d", TDK_LUT_MAX_SIZE, lut_size);
  TDK_REQUIRE(bad != 4, "tdk_color_lut: flags must be 0 or TDK_LUT_GLOBAL, got %d", flags);
  TDK_REQUIRE(interp == TDK_LUT_TETRAHEDRAL || interp == TDK_LUT_TRILINEAR, "tdk_color_lut: interp must be TDK_LUT_TETRAHEDRAL or TDK_LUT_TRILINEAR, got %d", interp);
  if (matrix)
    for (int k = 0; k < 9; k++) TDK_REQUIRE(isfinite(matrix[k]), "tdk_color_lut: matrix[%d] must be finite", k);
  if (shaper) TDK_REQUIRE(isfinite(shaper_lo) && isfinite(shaper_scale), "tdk_color_lut: shaper_lo and shaper_scale must be finite");
  if (lut) {
    TDK_REQUIRE(lut_lo && lut_scale, "tdk_color_lut: null pointer (lut_lo or lut_scale)");
    for (int c = 0; c < 3; c++) TDK_REQUIRE(isfinite(lut_lo[c]) && isfinite(lut_scale[c]), "tdk_color_lut: lut_lo[%d] and lut_scale[%d] must be finite", c, c);
  }
  const size_t ssz = tdk_dtype_bytes(src_dtype), dsz = tdk_dtype_bytes(dst_dtype);
  const size_t src_bytes = (size_t)npix * 3 * ssz, dst_bytes = (size_t)npix * 3 * dsz;
  if (npix > 0) {
    TDK_REQUIRE(tdk_disjoint(src, src_bytes, dst, dst_bytes), "tdk_color_lut: src and dst overlap (in-place use is not supported)");
    TDK_REQUIRE(!shaper || tdk_disjoint(shaper, cl_shaper_bytes(shaper_size, shaper_tables), dst, dst_bytes), "tdk_color_lut: the shaper and dst overlap");
    TDK_REQUIRE(!lut || tdk_disjoint(lut, cl_node_bytes(lut_size), dst, dst_bytes), "tdk_color_lut: the lut and dst overlap");
  }
  if (npix == 0) return TDK_OK;

  LutArgs a{};
  a.has_matrix = matrix != nullptr;
  for (int k = 0; k < 9; k++) a.m[k] = matrix ? matrix[k] : 0.0f;
  a.S = shaper_size, a.table_stride = shaper_tables == 3 ? shaper_size : 0;
  a.sh_lo = shaper ? shaper_lo : 0.0f, a.sh_scale = shaper ? shaper_scale : 0.0f, a.sh_top = (float)(shaper_size - 1);
  a.N = lut_size, a.trilinear = interp == TDK_LUT_TRILINEAR, a.lut_top = (float)(lut_size - 1);
  for (int c = 0; c < 3; c++) a.lut_lo[c] = lut ? lut_lo[c] : 0.0f, a.lut_scale[c] = lut ? lut_scale[c] : 0.0f;
  a.npix = npix;
  // the head that aligns the side with the narrower elements (the stricter demand; the destination on a tie); the other side is
  // vectorised when the same head aligns it
  const int hs = cl_head(src, ssz), hd = cl_head(dst, dsz);
  const int ms = (int)(16 / ssz), md = (int)(16 / dsz);
  const int head = ms > md ? hs : hd;
  a.vec_in = head % ms == hs % ms, a.vec_out = head % md == hd % md;
  a.head = (int)(npix < head ? npix : head);
  a.groups = (npix - a.head) / CL_PIX;
  a.lut_vec = lut && tdk_aligned(lut, 16);
  const bool staged = cl_staged(shaper_size, shaper_tables, lut_size, flags);
  const size_t lds = cl_shaper_bytes(shaper_size, shaper_tables) + (staged ? cl_node_bytes(lut_size) : 0);
  hipStream_t st = tdk_stream(stream);
  if (src_dtype == TDK_F32) return dispatch_dst<float>(dst_dtype, staged, src, dst, shaper, lut, a, lds, st);
  if (src_dtype == TDK_F16) return dispatch_dst<__half>(dst_dtype, staged, src, dst, shaper, lut, a, lds, st);
  return dispatch_dst<uint8_t>(dst_dtype, staged, src, dst, shaper, lut, a, lds, st);
}
