// rawprepare.hip -- sensor correction at the head of the chain (include/tdk_hip_raw.h: tdk_raw_prepare), one launch, no workspace.
//
// The specification is the head comment of include/tdk_hip_raw.h: decode (12-bit packed, uint16, float32 or binary16), black and
// white level (rp_linear), defective pixels against the four same-colour neighbours two sites away (rp_defect), a bilinear gain
// grid per CFA position, white balance and clip.
//
// A workgroup of four waves owns RP_TW x RP_TH pixels; a thread owns RP_PIX = 8 adjacent pixels of one row (12 packed bytes in,
// 32 or 16 bytes out), a wave four rows of 128.  Two forms of one kernel:
//   DEFECT = false  streaming: a thread reads its own eight pixels (three dwords / one or two 16-byte loads where the frame is
//                   aligned, per element otherwise) and nothing is staged.  Without shading there is no LDS and no barrier.
//   DEFECT = true   the tile with a two-pixel apron goes to LDS as linearised float32, one pixel PAIR per lane and step (two
//                   pixels are three packed bytes, and the apron is two pixels, so pairs never straddle it); positions outside
//                   the frame are staged as NaN.  Every comparison of the defect rules is false for a NaN, so a missing
//                   neighbour drops out of the rules by itself and the per-pixel code has no border test at all; the in-frame
//                   test lives in staging only, and a tile whose apron lies inside the frame takes a staging loop without it
//                   (the choice depends on blockIdx alone: a scalar branch).
// Lens shading: the records of the tile's columns and rows (node index and fraction: one integer division and one float division
// per tile column and per tile row, none per pixel) and the few grid nodes the tile touches are built in LDS by the workgroup.
// Nothing is accumulated across lanes or workgroups: the bits do not depend on scheduling.
#include <math.h>

#include "../../include/tdk_hip_raw.h"
#include "tdk_frame.h"

namespace {

constexpr int RP_THREADS = 256;
constexpr int RP_TW = 128, RP_TH = 16, RP_PIX = 8, RP_GROUPS = RP_TW / RP_PIX;   // 16 threads per tile row, 16 rows
constexpr int RP_APRON = 2;
constexpr int RP_PITCH = RP_TW + 2 * RP_APRON, RP_SROWS = RP_TH + 2 * RP_APRON;  // staged tile: 20 rows of 132 floats
constexpr int RP_PAIRS = RP_PITCH / 2;
// grid nodes under a tile: nodes are at least four pixels apart, so 128 columns meet at most 33 first nodes and their successors
constexpr int RP_NX = 36, RP_NY = 8;
constexpr int RP_MAX_GRID = 257;
static_assert(RP_THREADS == RP_GROUPS * RP_TH, "a thread per 8 pixels of the tile");
static_assert(RP_TW / 4 + 2 <= RP_NX && RP_TH / 4 + 2 <= RP_NY, "node box");

// LDS carve (floats); every offset is a multiple of four floats
constexpr int RP_OFF_COLQ = 0, RP_OFF_COLA = RP_TW, RP_OFF_ROWQ = 2 * RP_TW, RP_OFF_ROWA = 2 * RP_TW + RP_TH;
constexpr int RP_OFF_NODES = 2 * RP_TW + 2 * RP_TH, RP_SHADE_FLOATS = RP_OFF_NODES + RP_NX * RP_NY * 4;
constexpr int RP_PIX_FLOATS = RP_PITCH * RP_SROWS;

struct RpPacked {};   // tag: 12-bit packed bytes (either nibble order)

struct RpArgs {
  float black[4], scale[4];
  float threshold, ratio;
  int min_count, hot, dead;
  int w, h, gw, gh;
  uint32_t pattern;
  int ids, clip, vec_in, vec_out, vec_mask;
};

__device__ __forceinline__ void rp_unpack(uint32_t b0, uint32_t b1, uint32_t b2, bool ids, float& r0, float& r1) {
  uint32_t p0, p1;
  if (ids) {
    p0 = (b0 << 4) | (b2 & 0xfu);
    p1 = (b1 << 4) | (b2 >> 4);
  } else {
    p0 = ((b1 & 0xfu) << 8) | b0;
    p1 = (b2 << 4) | (b1 >> 4);
  }
  r0 = (float)p0;
  r1 = (float)p1;
}

// the pixel pair at (row i, even column j), as raw float32
template <typename IN> __device__ __forceinline__ void rp_load_pair(const void* src, size_t pixel, bool ids, float& r0, float& r1);
template <> __device__ __forceinline__ void rp_load_pair<RpPacked>(const void* src, size_t pixel, bool ids, float& r0, float& r1) {
  const uint8_t* b = reinterpret_cast<const uint8_t*>(src) + (pixel >> 1) * 3;
  rp_unpack(b[0], b[1], b[2], ids, r0, r1);
}
template <> __device__ __forceinline__ void rp_load_pair<uint16_t>(const void* src, size_t pixel, bool, float& r0, float& r1) {
  const uint16_t* s = reinterpret_cast<const uint16_t*>(src) + pixel;
  r0 = (float)s[0];
  r1 = (float)s[1];
}
template <> __device__ __forceinline__ void rp_load_pair<float>(const void* src, size_t pixel, bool, float& r0, float& r1) {
  const float* s = reinterpret_cast<const float*>(src) + pixel;
  r0 = s[0];
  r1 = s[1];
}
template <> __device__ __forceinline__ void rp_load_pair<__half>(const void* src, size_t pixel, bool, float& r0, float& r1) {
  const __half* s = reinterpret_cast<const __half*>(src) + pixel;
  r0 = __half2float(s[0]);
  r1 = __half2float(s[1]);
}

// eight adjacent pixels of an aligned frame (RpArgs::vec_in): three dwords, or 16-byte loads
template <typename IN> __device__ __forceinline__ void rp_load8(const void* src, size_t pixel, bool ids, float* raw);
template <> __device__ __forceinline__ void rp_load8<RpPacked>(const void* src, size_t pixel, bool ids, float* raw) {
  const uint32_t* q = reinterpret_cast<const uint32_t*>(reinterpret_cast<const uint8_t*>(src) + (pixel >> 1) * 3);
  const uint32_t w[3] = {q[0], q[1], q[2]};
  uint32_t by[12];
#pragma unroll
  for (int k = 0; k < 12; k++) by[k] = (w[k >> 2] >> (8 * (k & 3))) & 0xffu;
#pragma unroll
  for (int k = 0; k < 4; k++) rp_unpack(by[3 * k], by[3 * k + 1], by[3 * k + 2], ids, raw[2 * k], raw[2 * k + 1]);
}
template <> __device__ __forceinline__ void rp_load8<uint16_t>(const void* src, size_t pixel, bool, float* raw) {
  const uint4 u = *reinterpret_cast<const uint4*>(reinterpret_cast<const uint16_t*>(src) + pixel);
  const uint32_t w[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
  for (int k = 0; k < 4; k++) {
    raw[2 * k] = (float)(w[k] & 0xffffu);
    raw[2 * k + 1] = (float)(w[k] >> 16);
  }
}
template <> __device__ __forceinline__ void rp_load8<float>(const void* src, size_t pixel, bool, float* raw) {
  const float4* q = reinterpret_cast<const float4*>(reinterpret_cast<const float*>(src) + pixel);
  const float4 a = q[0], b = q[1];
  raw[0] = a.x; raw[1] = a.y; raw[2] = a.z; raw[3] = a.w; raw[4] = b.x; raw[5] = b.y; raw[6] = b.z; raw[7] = b.w;
}
template <> __device__ __forceinline__ void rp_load8<__half>(const void* src, size_t pixel, bool, float* raw) {
  uint4 u = *reinterpret_cast<const uint4*>(reinterpret_cast<const __half*>(src) + pixel);
  const __half2* h = reinterpret_cast<const __half2*>(&u);
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const float2 f = __half22float2(h[k]);
    raw[2 * k] = f.x;
    raw[2 * k + 1] = f.y;
  }
}

__device__ __forceinline__ float rp_linear(float raw, float black, float scale) { return (raw - black) * scale; }

// the defect rules on L and its neighbours (up, down, left, right); a NaN neighbour (missing, or a NaN of the input) never counts
__device__ __forceinline__ float rp_defect(const RpArgs& a, float L, const float* n, int& mask) {
  float v = L;
  mask = 0;
  if (a.hot) {
    const float lim = L * a.ratio;
    int count = 0;
    float best = 0.0f;
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const bool in = n[k] < lim;
      best = in && (count == 0 || n[k] > best) ? n[k] : best;
      count += in ? 1 : 0;
    }
    if (L > a.threshold && count >= a.min_count) {
      v = best;
      mask = 1;
    }
  }
  if (a.dead) {
    int count = 0;
    float best = 0.0f;
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const bool in = n[k] > a.threshold && L < n[k] * a.ratio;
      best = in && (count == 0 || n[k] < best) ? n[k] : best;
      count += in ? 1 : 0;
    }
    if (mask == 0 && count >= a.min_count) {
      v = best;
      mask = 2;
    }
  }
  return v;
}

template <typename IN, typename OUT, bool DEFECT>
__global__ __launch_bounds__(RP_THREADS) void raw_prepare_kernel(const void* __restrict__ src, OUT* __restrict__ dst, uint8_t* __restrict__ mask,
                                                                   const float* __restrict__ shading, const float* __restrict__ gains, RpArgs a) {
  extern __shared__ __attribute__((aligned(16))) float rp_lds[];
  float* pix = rp_lds;                                        // DEFECT: the staged tile
  float* shade = rp_lds + (DEFECT ? RP_PIX_FLOATS : 0);       // shading: records and nodes
  int* colq = reinterpret_cast<int*>(shade + RP_OFF_COLQ);
  float* cola = shade + RP_OFF_COLA;
  int* rowq = reinterpret_cast<int*>(shade + RP_OFF_ROWQ);
  float* rowa = shade + RP_OFF_ROWA;
  float* nodes = shade + RP_OFF_NODES;

  const int tid = threadIdx.x;
  const int x0 = (int)blockIdx.x * RP_TW, y0 = (int)blockIdx.y * RP_TH;
  const int tr = tid / RP_GROUPS, tc = (tid % RP_GROUPS) * RP_PIX;   // the thread's row and first column inside the tile
  const int i = y0 + tr, j0 = x0 + tc;
  const bool shaded = a.gw > 0, ids = a.ids != 0;

  // ---- lens shading, 1: the records of the tile's columns (threads 0..127) and rows (threads 128..143)
  if (shaded) {
    if (tid < RP_TW + RP_TH) {
      const bool col = tid < RP_TW;
      const int pos = col ? min(x0 + tid, a.w - 1) : min(y0 + tid - RP_TW, a.h - 1);
      const unsigned span = (unsigned)((col ? a.w : a.h) - 1), t = (unsigned)pos * (unsigned)((col ? a.gw : a.gh) - 1);
      const unsigned q = t / span, r = t - q * span;
      const float f = (float)r / (float)span;
      if (col) {
        colq[tid] = (int)q;
        cola[tid] = f;
      } else {
        rowq[tid - RP_TW] = (int)q;
        rowa[tid - RP_TW] = f;
      }
    }
    __syncthreads();
  }
  // ---- 2: the nodes under the tile; (qx0, qy0) is the first
  int qx0 = 0, qy0 = 0;
  if (shaded) {
    qx0 = colq[0], qy0 = rowq[0];
    const int nx = min(min(colq[RP_TW - 1] + 2, a.gw) - qx0, RP_NX), ny = min(min(rowq[RP_TH - 1] + 2, a.gh) - qy0, RP_NY);
    for (int e = tid; e < ny * nx * 4; e += RP_THREADS) {
      const int yy = e / (nx * 4), rest = e - yy * (nx * 4);
      nodes[yy * (RP_NX * 4) + rest] = shading[((size_t)(qy0 + yy) * a.gw + qx0) * 4 + rest];
    }
  }

  const bool odd_row = (i & 1) != 0;
  float v[RP_PIX];
  int m[RP_PIX];
  const bool row_live = i < a.h;
  if constexpr (DEFECT) {
    // ---- the tile and its apron as L, a pixel pair per lane; NaN outside the frame
    const bool interior = x0 >= RP_APRON && x0 + RP_TW + RP_APRON <= a.w && y0 >= RP_APRON && y0 + RP_TH + RP_APRON <= a.h;
    if (interior) {
#pragma unroll 2
      for (int e = tid; e < RP_SROWS * RP_PAIRS; e += RP_THREADS) {
        const int r = e / RP_PAIRS, c = (e - r * RP_PAIRS) * 2;
        const int gi = y0 - RP_APRON + r, gj = x0 - RP_APRON + c;
        float r0, r1;
        rp_load_pair<IN>(src, (size_t)gi * a.w + gj, ids, r0, r1);
        const bool odd = (gi & 1) != 0;
        pix[r * RP_PITCH + c] = rp_linear(r0, odd ? a.black[2] : a.black[0], odd ? a.scale[2] : a.scale[0]);
        pix[r * RP_PITCH + c + 1] = rp_linear(r1, odd ? a.black[3] : a.black[1], odd ? a.scale[3] : a.scale[1]);
      }
    } else {
      for (int e = tid; e < RP_SROWS * RP_PAIRS; e += RP_THREADS) {
        const int r = e / RP_PAIRS, c = (e - r * RP_PAIRS) * 2;
        const int gi = y0 - RP_APRON + r, gj = x0 - RP_APRON + c;
        float l0 = NAN, l1 = NAN;
        if (gi >= 0 && gi < a.h && gj >= 0 && gj < a.w) {   // width is even and gj is: the pair is inside or outside as one
          float r0, r1;
          rp_load_pair<IN>(src, (size_t)gi * a.w + gj, ids, r0, r1);
          const bool odd = (gi & 1) != 0;
          l0 = rp_linear(r0, odd ? a.black[2] : a.black[0], odd ? a.scale[2] : a.scale[0]);
          l1 = rp_linear(r1, odd ? a.black[3] : a.black[1], odd ? a.scale[3] : a.scale[1]);
        }
        pix[r * RP_PITCH + c] = l0;
        pix[r * RP_PITCH + c + 1] = l1;
      }
    }
    __syncthreads();   // (also orders the node staging above before its readers)
    const float* up = pix + tr * RP_PITCH + tc + RP_APRON;          // row i - 2, column j0
    const float* mid = pix + (tr + RP_APRON) * RP_PITCH + tc;        // row i, column j0 - 2
    const float* down = pix + (tr + 2 * RP_APRON) * RP_PITCH + tc + RP_APRON;
    float c[RP_PIX + 2 * RP_APRON];
#pragma unroll
    for (int k = 0; k < RP_PIX + 2 * RP_APRON; k++) c[k] = mid[k];
#pragma unroll
    for (int k = 0; k < RP_PIX; k++) {
      const float n[4] = {up[k], down[k], c[k], c[k + 2 * RP_APRON]};
      v[k] = rp_defect(a, c[k + RP_APRON], n, m[k]);
    }
  } else {
    if (shaded) __syncthreads();
    // black level and scale of the thread's row: even and odd columns
    const float black_e = odd_row ? a.black[2] : a.black[0], black_o = odd_row ? a.black[3] : a.black[1];
    const float scale_e = odd_row ? a.scale[2] : a.scale[0], scale_o = odd_row ? a.scale[3] : a.scale[1];
    if (row_live && j0 < a.w) {
      float raw[RP_PIX];
      const size_t pixel = (size_t)i * a.w + j0;
      if (a.vec_in) {
        rp_load8<IN>(src, pixel, ids, raw);
      } else {
#pragma unroll
        for (int k = 0; k < RP_PIX; k += 2) {
          raw[k] = raw[k + 1] = 0.0f;
          if (j0 + k < a.w) rp_load_pair<IN>(src, pixel + k, ids, raw[k], raw[k + 1]);
        }
      }
#pragma unroll
      for (int k = 0; k < RP_PIX; k++) v[k] = rp_linear(raw[k], (k & 1) ? black_o : black_e, (k & 1) ? scale_o : scale_e);
    } else {
#pragma unroll
      for (int k = 0; k < RP_PIX; k++) v[k] = 0.0f;
    }
#pragma unroll
    for (int k = 0; k < RP_PIX; k++) m[k] = 0;
  }

  // ---- lens shading, 3: the gain of every pixel from the staged nodes
  if (shaded) {
    const int qy = rowq[tr], qy1 = min(qy + 1, a.gh - 1);
    const float ay = rowa[tr], by = 1.0f - ay;
    const float* top = nodes + min(qy - qy0, RP_NY - 1) * (RP_NX * 4) + (odd_row ? 2 : 0);
    const float* bottom = nodes + min(qy1 - qy0, RP_NY - 1) * (RP_NX * 4) + (odd_row ? 2 : 0);
#pragma unroll
    for (int k = 0; k < RP_PIX; k++) {
      const int qx = colq[tc + k], qx1 = min(qx + 1, a.gw - 1);
      const float ax = cola[tc + k], bx = 1.0f - ax;
      const int n0 = min(qx - qx0, RP_NX - 1) * 4 + (k & 1), n1 = min(qx1 - qx0, RP_NX - 1) * 4 + (k & 1);
      const float g0 = top[n0] * bx + top[n1] * ax;
      const float g1 = bottom[n0] * bx + bottom[n1] * ax;
      const float g = g0 * by + g1 * ay;
      v[k] = v[k] * g;
    }
  }

  // ---- white balance and clip, the operation order of tdk_apply_white_balance
  if (gains != nullptr) {
    const float gr = gains[0], gg = gains[1], gb = gains[2];
    const int ce = cfa_color(i, 0, a.pattern), co = cfa_color(i, 1, a.pattern);
    const float gain_e = ce == 0 ? gr : (ce == 2 ? gb : gg), gain_o = co == 0 ? gr : (co == 2 ? gb : gg);
#pragma unroll
    for (int k = 0; k < RP_PIX; k++) v[k] = clampf(v[k] * ((k & 1) ? gain_o : gain_e), 0.0f, 1.0f);
  } else if (a.clip) {
#pragma unroll
    for (int k = 0; k < RP_PIX; k++) v[k] = clampf(v[k], 0.0f, 1.0f);
  }

  // ---- store: eight adjacent pixels as 16-byte stores where the frame is aligned, per element otherwise
  if (!row_live || j0 >= a.w) return;
  const size_t o = (size_t)i * a.w + j0;
  if (a.vec_out) {
    if constexpr (sizeof(OUT) == 4) {
      float4* q = reinterpret_cast<float4*>(dst + o);
      q[0] = make_float4(v[0], v[1], v[2], v[3]);
      q[1] = make_float4(v[4], v[5], v[6], v[7]);
    } else {
      uint4 u;
      __half2* h = reinterpret_cast<__half2*>(&u);
#pragma unroll
      for (int k = 0; k < 4; k++) h[k] = __floats2half2_rn(v[2 * k], v[2 * k + 1]);
      *reinterpret_cast<uint4*>(dst + o) = u;
    }
  } else {
#pragma unroll
    for (int k = 0; k < RP_PIX; k++)
      if (j0 + k < a.w) st<OUT>(dst, o + k, v[k]);
  }
  if (DEFECT && mask != nullptr) {
    if (a.vec_mask) {
      uint2 u;
      u.x = (uint32_t)m[0] | ((uint32_t)m[1] << 8) | ((uint32_t)m[2] << 16) | ((uint32_t)m[3] << 24);
      u.y = (uint32_t)m[4] | ((uint32_t)m[5] << 8) | ((uint32_t)m[6] << 16) | ((uint32_t)m[7] << 24);
      *reinterpret_cast<uint2*>(mask + o) = u;
    } else {
#pragma unroll
      for (int k = 0; k < RP_PIX; k++)
        if (j0 + k < a.w) mask[o + k] = (uint8_t)m[k];
    }
  }
}

inline size_t rp_lds_bytes(bool defect, bool shaded) { return sizeof(float) * ((defect ? RP_PIX_FLOATS : 0) + (shaded ? RP_SHADE_FLOATS : 0)); }

template <typename IN, typename OUT, bool DEFECT>
int launch(const void* src, void* dst, uint8_t* mask, const float* shading, const float* gains, const RpArgs& a, hipStream_t st) {
  const dim3 grid((unsigned)tdk_div_up(a.w, RP_TW), (unsigned)tdk_div_up(a.h, RP_TH));
  TDK_LAUNCH("tdk_raw_prepare", (raw_prepare_kernel<IN, OUT, DEFECT>), grid, dim3(RP_THREADS), rp_lds_bytes(DEFECT, a.gw > 0), st, src, reinterpret_cast<OUT*>(dst), mask,
             shading, gains, a);
  return TDK_OK;
}

template <typename IN> int dispatch(const void* src, void* dst, int dst_dtype, bool defect, uint8_t* mask, const float* shading, const float* gains, const RpArgs& a,
                                    hipStream_t st) {
  if (dst_dtype == TDK_F32) return defect ? launch<IN, float, true>(src, dst, mask, shading, gains, a, st) : launch<IN, float, false>(src, dst, mask, shading, gains, a, st);
  return defect ? launch<IN, __half, true>(src, dst, mask, shading, gains, a, st) : launch<IN, __half, false>(src, dst, mask, shading, gains, a, st);
}

}  // namespace

TDK_EXPORT int tdk_raw_abi_version(void) { return TDK_RAW_ABI_VERSION; }

TDK_EXPORT size_t tdk_raw_prepare_lds_bytes(int defects, int shading) { return rp_lds_bytes(defects != 0, shading != 0); }

TDK_EXPORT int tdk_raw_prepare(const void* src, int src_format, void* dst, int dst_dtype, unsigned char* mask, int width, int height, uint32_t pattern,
                               const float* black, const float* scale, int defects, float threshold, float ratio, int min_count, const float* shading,
                               int grid_width, int grid_height, const float* gains, int clip, tdk_stream_t stream) {
  TDK_REQUIRE(src && dst, "tdk_raw_prepare: null pointer (src or dst)");
  TDK_REQUIRE(black && scale, "tdk_raw_prepare: null pointer (black or scale)");
  TDK_REQUIRE(tdk_mosaic_size_ok(width, height), "tdk_raw_prepare: frame size %dx%d outside 2..%d", width, height, TDK_MOSAIC_MAX_SIZE);
  TDK_REQUIRE(width % 2 == 0 && height % 2 == 0, "tdk_raw_prepare: frame size %dx%d must be even in both axes (whole CFA cells)", width, height);
  TDK_REQUIRE(src_format >= TDK_RAW_PACKED12 && src_format <= TDK_RAW_F16, "tdk_raw_prepare: unknown src_format %d", src_format);
  TDK_REQUIRE(dst_dtype == TDK_F32 || dst_dtype == TDK_F16, "tdk_raw_prepare: unsupported dtype tag %d", dst_dtype);
  TDK_REQUIRE(tdk_pattern_ok(pattern), "tdk_raw_prepare: unknown Bayer pattern 0x%08x", pattern);
  for (int p = 0; p < 4; p++) {
    TDK_REQUIRE(isfinite(black[p]), "tdk_raw_prepare: black[%d] is not finite", p);
    TDK_REQUIRE(isfinite(scale[p]), "tdk_raw_prepare: scale[%d] is not finite", p);
  }
  TDK_REQUIRE(defects >= 0 && defects <= (TDK_RAW_HOT | TDK_RAW_DEAD), "tdk_raw_prepare: defects must be a combination of TDK_RAW_HOT and TDK_RAW_DEAD, got %d", defects);
  TDK_REQUIRE(isfinite(threshold) && threshold >= 0.0f, "tdk_raw_prepare: threshold must be finite and >= 0");
  TDK_REQUIRE(ratio > 0.0f && ratio <= 1.0f, "tdk_raw_prepare: ratio must lie in (0, 1]");
  TDK_REQUIRE(min_count >= 1 && min_count <= 4, "tdk_raw_prepare: min_count must be 1..4, got %d", min_count);
  TDK_REQUIRE(clip == 0 || clip == 1, "tdk_raw_prepare: clip must be 0 or 1, got %d", clip);
  if (shading) {
    TDK_REQUIRE(grid_width >= 2 && grid_height >= 2 && grid_width <= RP_MAX_GRID && grid_height <= RP_MAX_GRID, "tdk_raw_prepare: shading grid %dx%d outside 2..%d",
                grid_width, grid_height, RP_MAX_GRID);
    TDK_REQUIRE(4 * (grid_width - 1) <= width - 1 && 4 * (grid_height - 1) <= height - 1,
                "tdk_raw_prepare: shading grid %dx%d too dense for a %dx%d frame (nodes must be at least 4 pixels apart)", grid_width, grid_height, width, height);
  } else {
    TDK_REQUIRE(grid_width == 0 && grid_height == 0, "tdk_raw_prepare: shading grid %dx%d given without shading", grid_width, grid_height);
  }
  const size_t n = (size_t)width * height;
  const size_t src_bytes = src_format <= TDK_RAW_PACKED12_IDS ? n / 2 * 3 : src_format == TDK_RAW_F32 ? n * 4 : n * 2;
  const size_t dst_bytes = n * tdk_dtype_bytes(dst_dtype);
  const size_t grid_bytes = shading ? (size_t)grid_width * grid_height * 4 * sizeof(float) : 0;
  TDK_REQUIRE(tdk_disjoint(src, src_bytes, dst, dst_bytes), "tdk_raw_prepare: src and dst overlap (every output reads other positions)");
  TDK_REQUIRE(!shading || tdk_disjoint(shading, grid_bytes, dst, dst_bytes), "tdk_raw_prepare: shading and dst overlap");
  TDK_REQUIRE(!gains || tdk_disjoint(gains, 3 * sizeof(float), dst, dst_bytes), "tdk_raw_prepare: gains and dst overlap");
  if (mask) {
    TDK_REQUIRE(tdk_disjoint(mask, n, dst, dst_bytes), "tdk_raw_prepare: mask and dst overlap");
    TDK_REQUIRE(tdk_disjoint(mask, n, src, src_bytes), "tdk_raw_prepare: mask and src overlap");
    TDK_REQUIRE(!shading || tdk_disjoint(shading, grid_bytes, mask, n), "tdk_raw_prepare: mask and shading overlap");
    TDK_REQUIRE(!gains || tdk_disjoint(gains, 3 * sizeof(float), mask, n), "tdk_raw_prepare: mask and gains overlap");
  }

  RpArgs a{};
  for (int p = 0; p < 4; p++) a.black[p] = black[p], a.scale[p] = scale[p];
  a.threshold = threshold, a.ratio = ratio, a.min_count = min_count;
  a.hot = (defects & TDK_RAW_HOT) != 0, a.dead = (defects & TDK_RAW_DEAD) != 0;
  a.w = width, a.h = height, a.gw = shading ? grid_width : 0, a.gh = shading ? grid_height : 0;
  a.pattern = pattern;
  a.ids = src_format == TDK_RAW_PACKED12_IDS, a.clip = clip;
  // a thread's eight pixels as whole vectors: rows must start on the vector's alignment and hold whole groups of eight
  const bool rows8 = width % RP_PIX == 0;
  a.vec_in = rows8 && tdk_aligned(src, src_format <= TDK_RAW_PACKED12_IDS ? 4 : 16);
  a.vec_out = rows8 && tdk_aligned(dst, 16);
  a.vec_mask = rows8 && mask && tdk_aligned(mask, 8);
  const bool defect = defects != 0 || mask != nullptr;
  hipStream_t st = tdk_stream(stream);
  switch (src_format) {
    case TDK_RAW_U16: return dispatch<uint16_t>(src, dst, dst_dtype, defect, mask, shading, gains, a, st);
    case TDK_RAW_F32: return dispatch<float>(src, dst, dst_dtype, defect, mask, shading, gains, a, st);
    case TDK_RAW_F16: return dispatch<__half>(src, dst, dst_dtype, defect, mask, shading, gains, a, st);
    default: return dispatch<RpPacked>(src, dst, dst_dtype, defect, mask, shading, gains, a, st);
  }
}
