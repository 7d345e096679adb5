// rawcodec.hip -- lossless raw codec "TDKR" (include/tdk_hip_rawcodec.h is the normative text of the format).
//
// One wave per segment of 512 sites, four steps of 128: lane l of step s holds the sites x, x + 1 with x = 512*g + 128*s + 2*l, one
// sample of each parity.  Lanes 0..31 are one span, lanes 32..63 the next; the same-parity neighbour on the left is the lane before,
// and lane 63 carries into the next step.
//
//   rc_measure   z of every sample, the OR over each 32-lane half (its bit length is the group's width), anchors, width bytes, and the
//                segment's word count into its slot of offsets
//   rc_scan      one workgroup: counts -> exclusive prefix sum in place, header, padding of widths, *length
//   rc_pack      z again; plane word j of two groups is one 64-lane ballot; lane j keeps it and lanes 0..b-1 store a group's words
//   rc_unpack    stages the segment's payload in LDS (16 words a group), rebuilds z bit by bit, wave-wide inclusive scan, store in the output form.
//                Workgroup 0 decodes nothing: it reads every table and writes *status, so that no two workgroups write one word.
//
// Memory safety of rc_unpack: every table index is formed from the call's width and height, the tables are read only when
// table_bytes <= data_bytes, and a segment's payload only when its width bytes are <= 16 and offset + count fits data_bytes.
#include "tdk_common.h"
#include "tdk_frame.h"

#include "../../include/tdk_hip_rawcodec.h"

namespace {

constexpr int RC_WAVES = 4;             // waves (segments) of a workgroup of measure and pack
constexpr int RC_UNPACK_WAVES = 16;     // ... of unpack; its workgroup 0 is the checker
constexpr int RC_SCAN_THREADS = 1024;
constexpr int RC_SEG_WORDS = 256;       // 16 groups of at most 16 words
constexpr uint32_t RC_MAGIC = 0x524B4454u;   // 'T' 'D' 'K' 'R'

struct RcGeom {
  int w, h;
  int spans, segs;          // S, G
  uint32_t nseg;            // H*G
  uint32_t anchors_at, offsets_at, widths_at, table_bytes;   // byte offsets into the stream
};

RcGeom rc_geom(int w, int h) {
  RcGeom g{};
  g.w = w, g.h = h;
  g.spans = (w + 63) / 64, g.segs = (w + 511) / 512;
  g.nseg = (uint32_t)h * (uint32_t)g.segs;
  g.anchors_at = TDK_RAWCODEC_HEADER_BYTES;
  g.offsets_at = g.anchors_at + 4u * g.nseg;
  g.widths_at = g.offsets_at + 4u * g.nseg;
  g.table_bytes = g.widths_at + ((2u * (uint32_t)h * (uint32_t)g.spans + 3u) & ~3u);
  return g;
}

__device__ __forceinline__ uint32_t rc_zigzag(uint32_t v, uint32_t prev) {
  const uint32_t d = (v - prev) & 0xffffu;
  return ((d << 1) ^ ((d & 0x8000u) ? 0xffffu : 0u)) & 0xffffu;
}
__device__ __forceinline__ uint32_t rc_unzigzag(uint32_t z) { return ((z >> 1) ^ (0u - (z & 1u))) & 0xffffu; }
__device__ __forceinline__ int rc_bit_length(uint32_t v) { return v ? 32 - __clz((int)v) : 0; }

// one sample of a packed frame by its flat site index: the first or the second of the pair site / 2 (csrc/codec.hip: unpack)
__device__ __forceinline__ uint32_t rc_load_site12(const uint8_t* src, size_t site, bool ids) {
  const uint8_t* p = src + 3 * (site >> 1);
  if (ids) return site & 1 ? ((uint32_t)p[1] << 4) | (p[2] >> 4) : ((uint32_t)p[0] << 4) | (p[2] & 0xfu);
  return site & 1 ? ((uint32_t)p[2] << 4) | (p[1] >> 4) : (((uint32_t)p[1] & 0xfu) << 8) | p[0];
}

// the two samples of a lane; a site past the row reads nothing and gives 0
template <int FMT> __device__ __forceinline__ void rc_load_pair(const void* src, int w, int y, int x, uint32_t& v0, uint32_t& v1) {
  v0 = v1 = 0;
  if (x >= w) return;
  const size_t site = (size_t)y * (size_t)w + (size_t)x;
  if constexpr (FMT == TDK_RAW_U16) {
    const uint16_t* p = reinterpret_cast<const uint16_t*>(src) + site;
    if (x + 1 < w && (reinterpret_cast<uintptr_t>(p) & 3u) == 0) {
      const uint32_t u = *reinterpret_cast<const uint32_t*>(p);
      v0 = u & 0xffffu, v1 = u >> 16;
    } else {
      v0 = p[0];
      if (x + 1 < w) v1 = p[1];
    }
  } else if ((site & 1) == 0 && x + 1 < w) {   // packed, and the lane's two sites are one pair (every lane of a frame of even width)
    const uint8_t* p = reinterpret_cast<const uint8_t*>(src) + 3 * (site >> 1);
    const uint32_t b0 = p[0], b1 = p[1], b2 = p[2];
    if (FMT == TDK_RAW_PACKED12_IDS) {
      v0 = (b0 << 4) | (b2 & 0xfu), v1 = (b1 << 4) | (b2 >> 4);
    } else {
      v0 = ((b1 & 0xfu) << 8) | b0, v1 = (b2 << 4) | (b1 >> 4);
    }
  } else {   // an odd width: a site is read singly from the triple of its pair (the frame has an even number of sites: the pair is whole)
    v0 = rc_load_site12(reinterpret_cast<const uint8_t*>(src), site, FMT == TDK_RAW_PACKED12_IDS);
    if (x + 1 < w) v1 = rc_load_site12(reinterpret_cast<const uint8_t*>(src), site + 1, FMT == TDK_RAW_PACKED12_IDS);
  }
}

// z of the lane's two samples, low and high half of a word.  carry: the samples of lane 63 of the step before.
__device__ __forceinline__ uint32_t rc_step_z(uint32_t v0, uint32_t v1, int lane, int step, int x, int w, uint32_t& carry) {
  const uint32_t mine = v0 | (v1 << 16);
  uint32_t prev = (uint32_t)__shfl_up((int)mine, 1, 64);
  if (lane == 0) prev = step == 0 ? mine : carry;
  carry = (uint32_t)__shfl((int)mine, 63, 64);
  const uint32_t z0 = x < w ? rc_zigzag(v0, prev & 0xffffu) : 0u;
  const uint32_t z1 = x + 1 < w ? rc_zigzag(v1, prev >> 16) : 0u;
  return z0 | (z1 << 16);
}

// Cross-lane moves inside the VALU (DPP) in place of LDS-path shuffles.  A lane whose source lies outside its row of 16 (row_shr) or
// whose row is not in ROWS (row_bcast) gets 0, the identity of both uses below.
constexpr int RC_ROW_SHR = 0x110, RC_ROW_BCAST15 = 0x142, RC_ROW_BCAST31 = 0x143;
template <int CTRL, int ROWS = 0xf> __device__ __forceinline__ uint32_t rc_dpp(uint32_t v) {
  return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, ROWS, 0xf, false);
}

// inclusive sum over the wave's 64 lanes (mod 2^32)
__device__ __forceinline__ uint32_t rc_wave_scan(uint32_t v) {
  v += rc_dpp<RC_ROW_SHR + 1>(v);
  v += rc_dpp<RC_ROW_SHR + 2>(v);
  v += rc_dpp<RC_ROW_SHR + 4>(v);
  v += rc_dpp<RC_ROW_SHR + 8>(v);          // every row of 16 holds its own inclusive sums
  v += rc_dpp<RC_ROW_BCAST15, 0xa>(v);     // rows 1 and 3 add the total of the row before
  v += rc_dpp<RC_ROW_BCAST31, 0xc>(v);     // rows 2 and 3 add the total of lanes 0..31
  return v;
}

// OR over each 32-lane half, as wave-uniform values: lo of lanes 0..31, hi of lanes 32..63
__device__ __forceinline__ void rc_half_or(uint32_t v, uint32_t& lo, uint32_t& hi) {
  v |= rc_dpp<RC_ROW_SHR + 1>(v);
  v |= rc_dpp<RC_ROW_SHR + 2>(v);
  v |= rc_dpp<RC_ROW_SHR + 4>(v);
  v |= rc_dpp<RC_ROW_SHR + 8>(v);
  v |= rc_dpp<RC_ROW_BCAST15, 0xa>(v);     // lanes 31 and 63 hold the OR of their half
  lo = (uint32_t)__builtin_amdgcn_readlane((int)v, 31), hi = (uint32_t)__builtin_amdgcn_readlane((int)v, 63);
}

template <int FMT>
__global__ __launch_bounds__(RC_WAVES * 64) void rc_measure(const void* __restrict__ src, uint8_t* __restrict__ data, RcGeom g) {
  const int lane = threadIdx.x & 63;
  const uint32_t n = blockIdx.x * RC_WAVES + (threadIdx.x >> 6);
  if (n >= g.nseg) return;
  const int y = (int)(n / (uint32_t)g.segs), seg = (int)(n % (uint32_t)g.segs);
  uint8_t* widths = data + g.widths_at + 2 * ((size_t)y * g.spans + 8 * seg);
  uint32_t carry = 0, count = 0;
#pragma unroll
  for (int step = 0; step < 4; step++) {
    const int x = 512 * seg + 128 * step + 2 * lane;
    uint32_t v0, v1;
    rc_load_pair<FMT>(src, g.w, y, x, v0, v1);
    if (step == 0 && lane == 0) reinterpret_cast<uint32_t*>(data + g.anchors_at)[n] = v0 | (v1 << 16);
    uint32_t lo, hi;
    rc_half_or(rc_step_z(v0, v1, lane, step, x, g.w, carry), lo, hi);
    const int a0 = rc_bit_length(lo & 0xffffu), a1 = rc_bit_length(lo >> 16);   // the span of lanes 0..31, parity 0 and 1
    const int c0 = rc_bit_length(hi & 0xffffu), c1 = rc_bit_length(hi >> 16);   // the span of lanes 32..63
    if ((lane & 31) == 0 && x < g.w) reinterpret_cast<uint16_t*>(widths)[2 * step + (lane >> 5)] = (uint16_t)(lane ? c0 | (c1 << 8) : a0 | (a1 << 8));
    count += (uint32_t)(a0 + a1 + c0 + c1);
  }
  if (lane == 0) reinterpret_cast<uint32_t*>(data + g.offsets_at)[n] = count;
}

__global__ __launch_bounds__(RC_SCAN_THREADS) void rc_scan(uint8_t* __restrict__ data, RcGeom g, int bits, unsigned long long capacity, long long* __restrict__ length) {
  // One barrier per round: the wave totals alternate between two rows, and every thread keeps the running total itself.  The counts
  // of the next round are on their way while this one is summed.  A thread owns four consecutive counts, one 16-byte access where
  // the table lies so (a wave then moves 1 KB per instruction; four 4-byte accesses each touch the same eight lines again).
  constexpr int NW = RC_SCAN_THREADS / 64, PER = 4;
  __shared__ uint32_t wave_sums[2][NW];
  uint32_t* offsets = reinterpret_cast<uint32_t*>(data + g.offsets_at);
  const bool wide = (reinterpret_cast<uintptr_t>(offsets) & 15u) == 0;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  auto load = [&](uint32_t first, uint32_t (&v)[PER]) {
    if (wide && first + PER <= g.nseg) {
      const uint4 q = *reinterpret_cast<const uint4*>(offsets + first);
      v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
    } else {
#pragma unroll
      for (int k = 0; k < PER; k++) v[k] = first + k < g.nseg ? offsets[first + k] : 0u;
    }
  };
  uint32_t running = 0, c[PER], next[PER];
  load(PER * tid, c);
  int row = 0;
  for (uint32_t base = 0; base < g.nseg; base += PER * RC_SCAN_THREADS, row ^= 1) {
    const uint32_t first = base + PER * tid;
    load(first + PER * RC_SCAN_THREADS, next);   // (no slot of this round: nothing that is written below)
    const uint32_t mine = (c[0] + c[1]) + (c[2] + c[3]);
    const uint32_t incl = rc_wave_scan(mine);
    if (lane == 63) wave_sums[row][wave] = incl;
    __syncthreads();
    uint32_t before = running;
#pragma unroll
    for (int k = 0; k < NW; k++) {
      const uint32_t s = wave_sums[row][k];
      running += s;
      if (k < wave) before += s;
    }
    uint32_t at[PER];
    at[0] = before + incl - mine;
#pragma unroll
    for (int k = 1; k < PER; k++) at[k] = at[k - 1] + c[k - 1];
    if (wide && first + PER <= g.nseg) {
      *reinterpret_cast<uint4*>(offsets + first) = make_uint4(at[0], at[1], at[2], at[3]);
    } else {
#pragma unroll
      for (int k = 0; k < PER; k++)
        if (first + k < g.nseg) offsets[first + k] = at[k];
    }
#pragma unroll
    for (int k = 0; k < PER; k++) c[k] = next[k];
  }
  if (tid == 0) {
    const uint32_t words = running;
    const unsigned long long total = (unsigned long long)g.table_bytes + 4ull * words;
    uint32_t* header = reinterpret_cast<uint32_t*>(data);
    header[0] = RC_MAGIC;
    header[1] = (uint32_t)TDK_RAWCODEC_FORMAT_VERSION | ((uint32_t)bits << 16);
    header[2] = (uint32_t)g.w, header[3] = (uint32_t)g.h;
    header[4] = words, header[5] = (uint32_t)total;
    header[6] = 0, header[7] = 0;
    const uint32_t width_bytes = 2u * (uint32_t)g.h * (uint32_t)g.spans;
    if (width_bytes & 3u) *reinterpret_cast<uint16_t*>(data + g.widths_at + width_bytes) = 0;
    *length = total <= capacity ? (long long)total : -1ll;
  }
}

template <int FMT>
__global__ __launch_bounds__(RC_WAVES * 64) void rc_pack(const void* __restrict__ src, uint8_t* __restrict__ data, RcGeom g, unsigned long long capacity) {
  const int lane = threadIdx.x & 63;
  const uint32_t n = blockIdx.x * RC_WAVES + (threadIdx.x >> 6);
  if (n >= g.nseg) return;
  const int y = (int)(n / (uint32_t)g.segs), seg = (int)(n % (uint32_t)g.segs);
  const uint32_t* offsets = reinterpret_cast<const uint32_t*>(data + g.offsets_at);
  const uint32_t begin = offsets[n];
  const uint32_t end = n + 1 < g.nseg ? offsets[n + 1] : reinterpret_cast<const uint32_t*>(data)[4];   // (the header's payload_words)
  if ((unsigned long long)g.table_bytes + 4ull * end > capacity) return;   // the segment does not fit: nothing of it is written
  uint32_t* payload = reinterpret_cast<uint32_t*>(data + g.table_bytes);
  uint32_t carry = 0, at = begin;
#pragma unroll
  for (int step = 0; step < 4; step++) {
    const int x = 512 * seg + 128 * step + 2 * lane;
    uint32_t v0, v1;
    rc_load_pair<FMT>(src, g.w, y, x, v0, v1);
    const uint32_t z = rc_step_z(v0, v1, lane, step, x, g.w, carry);
    uint32_t lo, hi;
    rc_half_or(z, lo, hi);
    const int a0 = rc_bit_length(lo & 0xffffu), a1 = rc_bit_length(lo >> 16);   // the span of lanes 0..31, parity 0 and 1
    const int c0 = rc_bit_length(hi & 0xffffu), c1 = rc_bit_length(hi >> 16);   // the span of lanes 32..63
    const int planes = max(max(a0, a1), max(c0, c1));
    // Plane j of a parity is one ballot: its low word belongs to the first span, its high word to the second.  Lane j keeps them
    // so that afterwards lanes 0..b-1 store the b words of a group side by side.
    uint32_t ka = 0, kb = 0, kc = 0, kd = 0;
    for (int j = 0; j < planes; j++) {
      const unsigned long long p0 = __ballot(z & (1u << j)), p1 = __ballot(z & (0x10000u << j));
      if (lane == j) ka = (uint32_t)p0, kb = (uint32_t)p1, kc = (uint32_t)(p0 >> 32), kd = (uint32_t)(p1 >> 32);
    }
    if (lane < a0) payload[at + lane] = (uint32_t)ka;
    at += a0;
    if (lane < a1) payload[at + lane] = (uint32_t)kb;
    at += a1;
    if (lane < c0) payload[at + lane] = (uint32_t)kc;
    at += c0;
    if (lane < c1) payload[at + lane] = (uint32_t)kd;
    at += c1;
  }
}

// ---- decode
// The bytes tdk_decode12_u16 reads the samples from, saturated at 4095 as tdk_encode12_u16 does.  For the standard order these are the
// bytes of tdk_encode12_u16; for the IDS order that encoder puts the low nibbles the other way round than the decoder reads them
// (csrc/codec.hip, as the reference has it), and the codec follows the decoder: a packed frame comes back byte for byte.
__device__ __forceinline__ void rc_pack12(uint32_t p0, uint32_t p1, bool ids, uint8_t* o) {
  p0 = p0 < 4095u ? p0 : 4095u, p1 = p1 < 4095u ? p1 : 4095u;
  if (ids) {
    o[0] = (uint8_t)(p0 >> 4), o[1] = (uint8_t)(p1 >> 4), o[2] = (uint8_t)(((p1 & 0xfu) << 4) | (p0 & 0xfu));
  } else {
    o[0] = (uint8_t)(p0 & 0xffu), o[1] = (uint8_t)(((p1 & 0xfu) << 4) | (p0 >> 8)), o[2] = (uint8_t)(p1 >> 4);
  }
}

template <int FMT> __device__ __forceinline__ void rc_store_pair(void* out, int w, int y, int x, uint32_t v0, uint32_t v1) {
  if (x >= w) return;
  const bool both = x + 1 < w;
  const size_t site = (size_t)y * (size_t)w + (size_t)x;
  if constexpr (FMT == TDK_RAW_U16) {
    uint16_t* p = reinterpret_cast<uint16_t*>(out) + site;
    if (both && (reinterpret_cast<uintptr_t>(p) & 3u) == 0) {
      *reinterpret_cast<uint32_t*>(p) = v0 | (v1 << 16);
    } else {
      p[0] = (uint16_t)v0;
      if (both) p[1] = (uint16_t)v1;
    }
  } else if constexpr (FMT == TDK_RAW_F32) {
    float* p = reinterpret_cast<float*>(out) + site;
    const float f0 = (float)v0 * (1.0f / 4095.0f), f1 = (float)v1 * (1.0f / 4095.0f);
    if (both && (reinterpret_cast<uintptr_t>(p) & 7u) == 0) {
      *reinterpret_cast<float2*>(p) = make_float2(f0, f1);
    } else {
      p[0] = f0;
      if (both) p[1] = f1;
    }
  } else if constexpr (FMT == TDK_RAW_F16) {
    __half* p = reinterpret_cast<__half*>(out) + site;
    // tdk_decode12_f16 rounds the product to float32 and that to binary16.  Left alone, the compiler folds product and conversion into
    // one v_fma_mixlo_f16, which rounds once: the empty asm keeps the float32 product a value of its own.
    float f0 = (float)v0 * (1.0f / 4095.0f), f1 = (float)v1 * (1.0f / 4095.0f);
    asm volatile("" : "+v"(f0), "+v"(f1));
    const __half h0 = __float2half_rn(f0), h1 = __float2half_rn(f1);
    if (both && (reinterpret_cast<uintptr_t>(p) & 3u) == 0) {
      *reinterpret_cast<__half2*>(p) = __halves2half2(h0, h1);
    } else {
      p[0] = h0;
      if (both) p[1] = h1;
    }
  } else {   // packed, an even width: the lane's two sites are a pair (an odd width: rc_store_packed_odd)
    rc_pack12(v0, v1, FMT == TDK_RAW_PACKED12_IDS, reinterpret_cast<uint8_t*>(out) + 3 * (site >> 1));
  }
}

// Packed output of a frame of odd width (and an even count of sites).  A packed buffer knows no rows: the pair of flat sites (2q, 2q + 1)
// shares three bytes, and with an odd width every second row starts at an odd flat site.  In an even row a lane's two sites are a pair,
// except the row's last site, whose partner opens the next row.  In an odd row a lane's first site pairs with the site on its left (the
// lane before, or lane 63 of the step before: `carry`), the segment's first site is left to the wave in front of it, and lane 63 of a whole
// segment pairs its second site with the first site of the next segment.  `next`: that first sample of the segment that follows in
// the stream, which its owner decodes to the same value (its anchor, or 0 where it writes zeros).  Every triple has one writer.
template <int FMT>
__device__ __forceinline__ void rc_store_packed_odd(void* out, int w, int y, int seg, int x, int lane, uint32_t v0, uint32_t v1, uint32_t carry, uint32_t next) {
  constexpr bool ids = FMT == TDK_RAW_PACKED12_IDS;
  uint8_t* o = reinterpret_cast<uint8_t*>(out);
  uint32_t left = (uint32_t)__shfl_up((int)v1, 1, 64);
  if (lane == 0) left = carry;
  if (x >= w) return;
  const size_t site = (size_t)y * (size_t)w + (size_t)x;
  if ((y & 1) == 0) {   // site is even
    rc_pack12(v0, x + 1 < w ? v1 : next, ids, o + 3 * (site >> 1));
  } else {              // site is odd
    if (x > 512 * seg) rc_pack12(left, v0, ids, o + 3 * ((site - 1) >> 1));
    if (x + 1 == 512 * seg + 511 && x + 1 < w) rc_pack12(v1, next, ids, o + 3 * ((site + 1) >> 1));
  }
}

// bit 0 and bit 1 of the status, from the header alone
__device__ __forceinline__ int rc_header_status(const uint8_t* data, const RcGeom& g) {
  const uint32_t* header = reinterpret_cast<const uint32_t*>(data);
  int st = 0;
  if (header[0] != RC_MAGIC || (header[1] & 0xffffu) != (uint32_t)TDK_RAWCODEC_FORMAT_VERSION) st |= TDK_RAWCODEC_BAD_MAGIC;
  if (header[2] != (uint32_t)g.w || header[3] != (uint32_t)g.h) st |= TDK_RAWCODEC_BAD_SIZE;
  return st;
}

// One segment's tables against the buffer: a width byte above 16, or a payload that passes data_bytes.  Only for table_bytes <= data_bytes.
__device__ __forceinline__ bool rc_segment_bad(const uint8_t* __restrict__ data, unsigned long long data_bytes, const RcGeom& g, uint32_t n) {
  const int y = (int)(n / (uint32_t)g.segs), seg = (int)(n % (uint32_t)g.segs);
  const uint16_t* widths = reinterpret_cast<const uint16_t*>(data + g.widths_at + 2 * ((size_t)y * g.spans + 8 * seg));
  const int spans = min(8, g.spans - 8 * seg);
  bool bad = false;
  uint32_t count = 0;
  for (int k = 0; k < spans; k++) {
    const uint32_t u = widths[k], b0 = u & 0xffu, b1 = u >> 8;
    bad |= b0 > 16u || b1 > 16u;
    count += b0 + b1;
  }
  const uint32_t begin = reinterpret_cast<const uint32_t*>(data + g.offsets_at)[n];
  return bad || (unsigned long long)g.table_bytes + 4ull * ((unsigned long long)begin + count) > data_bytes;
}

// Workgroup 0 of rc_unpack: the status of the whole stream.  One thread per segment and round.
__device__ void rc_check_stream(const uint8_t* __restrict__ data, unsigned long long data_bytes, const RcGeom& g, int* __restrict__ status) {
  int st = rc_header_status(data, g);
  const bool tables = st == 0 && g.table_bytes <= data_bytes;   // only then do the tables have a place inside the buffer
  int bad = st == 0 && !tables;
  const uint32_t* offsets = reinterpret_cast<const uint32_t*>(data + g.offsets_at);
  if (tables && g.spans % 8 == 0 && (reinterpret_cast<uintptr_t>(data + g.widths_at) & 7u) == 0) {
    // Whole segments only (the width is a multiple of 512): segment n owns bytes 16n .. 16n + 15 of widths, two 8-byte reads at
    // consecutive addresses across the lanes.  Four segments per thread and round, so that four rounds of loads are in flight.
    const uint2* widths = reinterpret_cast<const uint2*>(data + g.widths_at);
    for (uint32_t base = 0; base < g.nseg; base += 4 * blockDim.x) {
      uint2 lo[4], hi[4];
      uint32_t at[4];
#pragma unroll
      for (int k = 0; k < 4; k++) {
        const uint32_t n = base + k * blockDim.x + threadIdx.x;
        const bool in = n < g.nseg;
        lo[k] = in ? widths[2 * (size_t)n] : make_uint2(0, 0), hi[k] = in ? widths[2 * (size_t)n + 1] : make_uint2(0, 0);
        at[k] = in ? offsets[n] : 0u;
      }
#pragma unroll
      for (int k = 0; k < 4; k++) {
        const uint32_t w[4] = {lo[k].x, lo[k].y, hi[k].x, hi[k].y};
        uint32_t count = 0;
#pragma unroll
        for (int i = 0; i < 4; i++) {   // a byte above 16: bit 7 of the byte itself, or of its low seven bits + 111
          bad |= ((w[i] | ((w[i] & 0x7f7f7f7fu) + 0x6f6f6f6fu)) & 0x80808080u) != 0;
          count = __builtin_amdgcn_sad_u8(w[i], 0u, count);   // + the sum of the four bytes
        }
        bad |= (unsigned long long)g.table_bytes + 4ull * ((unsigned long long)at[k] + count) > data_bytes;
      }
    }
  } else if (tables) {
#pragma unroll 2
    for (uint32_t n = threadIdx.x; n < g.nseg; n += blockDim.x) bad |= rc_segment_bad(data, data_bytes, g, n);
  }
  bad = __syncthreads_or(bad);
  if (threadIdx.x == 0) *status = st | (bad ? TDK_RAWCODEC_BAD_TABLES : 0);
}

template <int FMT>
__global__ __launch_bounds__(RC_UNPACK_WAVES * 64) void rc_unpack(const uint8_t* __restrict__ data, unsigned long long data_bytes, void* __restrict__ out, RcGeom g,
                                                                  int* __restrict__ status) {
  // A group owns 16 words of the wave's 1 KB whatever its width, the planes it does not have as zeros: a lane then reads four planes
  // with one 16-byte access at an address that depends on its group alone, and no plane needs a test of its own.
  __shared__ uint4 staged[RC_UNPACK_WAVES][RC_SEG_WORDS / 4];
  if (blockIdx.x == 0) {
    rc_check_stream(data, data_bytes, g, status);
    return;
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint32_t n = (blockIdx.x - 1) * RC_UNPACK_WAVES + wave;
  const bool live = n < g.nseg;   // (a wave without a segment still meets the barrier)
  const int y = live ? (int)(n / (uint32_t)g.segs) : 0, seg = live ? (int)(n % (uint32_t)g.segs) : 0;

  const bool tables = live && rc_header_status(data, g) == 0 && g.table_bytes <= data_bytes;
  bool ok = tables;
  uint32_t width = 0, anchors = 0;
  // packed output at an odd width: the first sample of the segment behind this one, where a pair reaches into it (rc_store_packed_odd)
  constexpr bool packed_out = FMT == TDK_RAW_PACKED12 || FMT == TDK_RAW_PACKED12_IDS;
  const bool odd_width = packed_out && (g.w & 1);
  uint32_t next = 0;
  if (odd_width && tables && ((y & 1) ? seg < g.segs - 1 : seg == g.segs - 1) && !rc_segment_bad(data, data_bytes, g, n + 1))
    next = reinterpret_cast<const uint32_t*>(data + g.anchors_at)[n + 1] & 0xffffu;   // (n + 1 exists: an even row is not the last)
  if (ok) {
    const int spans = min(8, g.spans - 8 * seg);
    const uint8_t* widths = data + g.widths_at + 2 * ((size_t)y * g.spans + 8 * seg);
    if (lane < 2 * spans) width = widths[lane];   // group `lane` of the segment: span lane / 2, parity lane & 1; 0 from lane 16 on
    ok = !__any(width > 16u);
    uint32_t incl = width;                        // lanes 0..15 are one row of 16
    incl += rc_dpp<RC_ROW_SHR + 1>(incl);
    incl += rc_dpp<RC_ROW_SHR + 2>(incl);
    incl += rc_dpp<RC_ROW_SHR + 4>(incl);
    incl += rc_dpp<RC_ROW_SHR + 8>(incl);
    const uint32_t start = incl - width;
    const uint32_t count = (uint32_t)__builtin_amdgcn_readlane((int)incl, 15);   // <= 256 once every width is <= 16
    const uint32_t begin = reinterpret_cast<const uint32_t*>(data + g.offsets_at)[n];
    ok = ok && (unsigned long long)g.table_bytes + 4ull * ((unsigned long long)begin + count) <= data_bytes;
    if (ok) {
      const uint32_t* payload = reinterpret_cast<const uint32_t*>(data + g.table_bytes) + begin;
      uint32_t* slots = reinterpret_cast<uint32_t*>(staged[wave]);
#pragma unroll
      for (int round = 0; round < 4; round++) {   // lane -> plane lane & 15 of group 4*round + lane / 16: word 64*round + lane of the 256
        const int group = 4 * round + (lane >> 4), plane = lane & 15;
        const int b = __shfl((int)width, group, 64), s = __shfl((int)start, group, 64);
        slots[64 * round + lane] = plane < b ? payload[s + plane] : 0u;   // (s + plane < count)
      }
      anchors = reinterpret_cast<const uint32_t*>(data + g.anchors_at)[n];
    }
  }
  __syncthreads();
  if (!live) return;

  const int half = lane >> 5, bit = lane & 31;
  uint32_t run0 = anchors & 0xffffu, run1 = anchors >> 16;   // the chain's value in front of the step
  [[maybe_unused]] uint32_t carry1 = 0;   // lane 63's second sample of the step before
#pragma unroll
  for (int step = 0; step < 4; step++) {
    const int x = 512 * seg + 128 * step + 2 * lane;
    uint32_t v0 = 0, v1 = 0;
    if (ok) {
      const int planes = max(max(__builtin_amdgcn_readlane((int)width, 4 * step), __builtin_amdgcn_readlane((int)width, 4 * step + 1)),
                             max(__builtin_amdgcn_readlane((int)width, 4 * step + 2), __builtin_amdgcn_readlane((int)width, 4 * step + 3)));
      const uint4* mine = &staged[wave][4 * (4 * step + 2 * half)];   // the lane's group of parity 0; parity 1 follows it
      uint32_t z0 = 0, z1 = 0;
#pragma unroll
      for (int m = 0; m < 4; m++) {
        if (4 * m < planes) {
          const uint4 p0 = mine[m], p1 = mine[4 + m];
          z0 |= (__builtin_amdgcn_ubfe(p0.x, bit, 1) << (4 * m)) | (__builtin_amdgcn_ubfe(p0.y, bit, 1) << (4 * m + 1)) |
                (__builtin_amdgcn_ubfe(p0.z, bit, 1) << (4 * m + 2)) | (__builtin_amdgcn_ubfe(p0.w, bit, 1) << (4 * m + 3));
          z1 |= (__builtin_amdgcn_ubfe(p1.x, bit, 1) << (4 * m)) | (__builtin_amdgcn_ubfe(p1.y, bit, 1) << (4 * m + 1)) |
                (__builtin_amdgcn_ubfe(p1.z, bit, 1) << (4 * m + 2)) | (__builtin_amdgcn_ubfe(p1.w, bit, 1) << (4 * m + 3));
        }
      }
      if (step == 0 && lane == 0) z0 = z1 = 0;   // the chain's first sample is its anchor whatever the stream holds there
      // parity 1 in the high half of its word: its sum wraps at 2^16 by itself
      const uint32_t t0 = rc_wave_scan(rc_unzigzag(z0)), t1 = rc_wave_scan(rc_unzigzag(z1) << 16);
      v0 = (run0 + t0) & 0xffffu, v1 = (run1 + (t1 >> 16)) & 0xffffu;
      run0 = (uint32_t)__builtin_amdgcn_readlane((int)v0, 63), run1 = (uint32_t)__builtin_amdgcn_readlane((int)v1, 63);
    }
    if constexpr (packed_out) {
      if (odd_width) {
        rc_store_packed_odd<FMT>(out, g.w, y, seg, x, lane, v0, v1, carry1, next);
        carry1 = (uint32_t)__builtin_amdgcn_readlane((int)v1, 63);
        continue;
      }
    }
    rc_store_pair<FMT>(out, g.w, y, x, v0, v1);
  }
}

bool rc_size_ok(int width, int height) {
  return width >= 1 && height >= 1 && width <= 65535 && height <= 65535 && (long long)width * height <= (long long)TDK_RAWCODEC_MAX_SITES;
}
bool rc_packed(int format) { return format == TDK_RAW_PACKED12 || format == TDK_RAW_PACKED12_IDS; }

size_t rc_frame_bytes(int format, int width, int height) {
  const size_t sites = (size_t)width * (size_t)height;
  return rc_packed(format) ? sites / 2 * 3 : format == TDK_RAW_F32 ? sites * 4 : sites * 2;
}
size_t rc_frame_align(int format) { return rc_packed(format) ? 1 : format == TDK_RAW_F32 ? 4 : 2; }

template <int FMT> int rc_launch_encode(const void* src, uint8_t* data, const RcGeom& g, int bits, size_t capacity, int64_t* length, hipStream_t st) {
  const dim3 grid((g.nseg + RC_WAVES - 1) / RC_WAVES), block(RC_WAVES * 64);
  TDK_LAUNCH("tdk_rawcodec_measure", rc_measure<FMT>, grid, block, 0, st, src, data, g);
  TDK_LAUNCH("tdk_rawcodec_scan", rc_scan, dim3(1), dim3(RC_SCAN_THREADS), 0, st, data, g, bits, (unsigned long long)capacity, reinterpret_cast<long long*>(length));
  TDK_LAUNCH("tdk_rawcodec_pack", rc_pack<FMT>, grid, block, 0, st, src, data, g, (unsigned long long)capacity);
  return TDK_OK;
}

template <int FMT> int rc_launch_decode(const uint8_t* data, size_t data_bytes, void* out, const RcGeom& g, int* status, hipStream_t st) {
  const dim3 grid(1 + (g.nseg + RC_UNPACK_WAVES - 1) / RC_UNPACK_WAVES), block(RC_UNPACK_WAVES * 64);
  TDK_LAUNCH("tdk_rawcodec_unpack", rc_unpack<FMT>, grid, block, 0, st, data, (unsigned long long)data_bytes, out, g, status);
  return TDK_OK;
}

}  // namespace

TDK_EXPORT int tdk_rawcodec_abi_version(void) { return TDK_RAWCODEC_ABI_VERSION; }

TDK_EXPORT size_t tdk_rawcodec_table_bytes(int width, int height) { return rc_size_ok(width, height) ? rc_geom(width, height).table_bytes : 0; }

TDK_EXPORT size_t tdk_rawcodec_max_stream_bytes(int width, int height) {
  if (!rc_size_ok(width, height)) return 0;
  const RcGeom g = rc_geom(width, height);
  return (size_t)g.table_bytes + (size_t)4 * 16 * 2 * (size_t)height * (size_t)g.spans;
}

TDK_EXPORT int tdk_rawcodec_encode(const void* src, int src_format, int width, int height, int bits, void* data, size_t capacity, int64_t* length,
                                   tdk_stream_t stream) {
  static const char* const who = "tdk_rawcodec_encode";
  TDK_REQUIRE(src && data && length, "%s: null pointer (src, data or length)", who);
  TDK_REQUIRE(src_format == TDK_RAW_U16 || rc_packed(src_format), "%s: unsupported source format %d (uint16 or packed 12-bit)", who, src_format);
  TDK_REQUIRE(rc_size_ok(width, height), "%s: frame size %dx%d outside 1..65535 or above 2^30 sites", who, width, height);
  TDK_REQUIRE(!rc_packed(src_format) || ((long long)width * height) % 2 == 0, "%s: a packed frame needs an even number of sites, got %dx%d", who, width, height);
  TDK_REQUIRE(bits >= 1 && bits <= 16, "%s: bits must be 1..16, got %d", who, bits);
  TDK_REQUIRE(!rc_packed(src_format) || bits == 12, "%s: bits must be 12 for packed input, got %d", who, bits);
  TDK_REQUIRE(tdk_aligned(src, rc_frame_align(src_format)) && tdk_aligned(data, 4) && tdk_aligned(length, 8),
              "%s: alignment (src at its element type, data at 4 bytes, length at 8)", who);
  const RcGeom g = rc_geom(width, height);
  TDK_REQUIRE(capacity >= g.table_bytes, "%s: capacity %zu is below the %u bytes of the tables", who, capacity, g.table_bytes);
  const size_t src_bytes = rc_frame_bytes(src_format, width, height);
  TDK_REQUIRE(tdk_disjoint(src, src_bytes, data, capacity), "%s: data overlaps src", who);
  TDK_REQUIRE(tdk_disjoint(length, 8, data, capacity) && tdk_disjoint(length, 8, src, src_bytes), "%s: length overlaps src or data", who);

  uint8_t* d = reinterpret_cast<uint8_t*>(data);
  hipStream_t st = tdk_stream(stream);
  if (src_format == TDK_RAW_U16) return rc_launch_encode<TDK_RAW_U16>(src, d, g, bits, capacity, length, st);
  if (src_format == TDK_RAW_PACKED12) return rc_launch_encode<TDK_RAW_PACKED12>(src, d, g, bits, capacity, length, st);
  return rc_launch_encode<TDK_RAW_PACKED12_IDS>(src, d, g, bits, capacity, length, st);
}

TDK_EXPORT int tdk_rawcodec_decode(const void* data, size_t data_bytes, void* out, int out_format, int width, int height, int* status, tdk_stream_t stream) {
  static const char* const who = "tdk_rawcodec_decode";
  TDK_REQUIRE(data && out && status, "%s: null pointer (data, out or status)", who);
  TDK_REQUIRE(out_format == TDK_RAW_U16 || out_format == TDK_RAW_F32 || out_format == TDK_RAW_F16 || rc_packed(out_format),
              "%s: unsupported output format %d", who, out_format);
  TDK_REQUIRE(rc_size_ok(width, height), "%s: frame size %dx%d outside 1..65535 or above 2^30 sites", who, width, height);
  TDK_REQUIRE(!rc_packed(out_format) || ((long long)width * height) % 2 == 0, "%s: a packed frame needs an even number of sites, got %dx%d", who, width, height);
  TDK_REQUIRE(data_bytes >= TDK_RAWCODEC_HEADER_BYTES, "%s: data_bytes %zu is below the %d bytes of the header", who, data_bytes, TDK_RAWCODEC_HEADER_BYTES);
  TDK_REQUIRE(tdk_aligned(data, 4) && tdk_aligned(out, rc_frame_align(out_format)) && tdk_aligned(status, 4),
              "%s: alignment (data at 4 bytes, out at its element type, status at 4)", who);
  const size_t out_bytes = rc_frame_bytes(out_format, width, height);
  TDK_REQUIRE(tdk_disjoint(data, data_bytes, out, out_bytes), "%s: out overlaps data", who);
  TDK_REQUIRE(tdk_disjoint(status, 4, out, out_bytes) && tdk_disjoint(status, 4, data, data_bytes), "%s: status overlaps data or out", who);

  const RcGeom g = rc_geom(width, height);
  const uint8_t* d = reinterpret_cast<const uint8_t*>(data);
  hipStream_t st = tdk_stream(stream);
  switch (out_format) {
    case TDK_RAW_U16: return rc_launch_decode<TDK_RAW_U16>(d, data_bytes, out, g, status, st);
    case TDK_RAW_F32: return rc_launch_decode<TDK_RAW_F32>(d, data_bytes, out, g, status, st);
    case TDK_RAW_F16: return rc_launch_decode<TDK_RAW_F16>(d, data_bytes, out, g, status, st);
    case TDK_RAW_PACKED12: return rc_launch_decode<TDK_RAW_PACKED12>(d, data_bytes, out, g, status, st);
    default: return rc_launch_decode<TDK_RAW_PACKED12_IDS>(d, data_bytes, out, g, status, st);
  }
}
