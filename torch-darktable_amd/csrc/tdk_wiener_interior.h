// tdk_wiener_interior.h -- the strip geometry of the Wiener strip kernel (tdk_wiener_ystream.h) that the kernel, its launch code
// and the host share: which workgroups are interior, the order the workgroups start in, and a lane's share of the staging block.
// Plain integer C++, no device builtins: included by tdk_wiener_ystream.h (inside wiener.hip's anonymous namespace) and, compiled
// for the host alone, by tests/hip_unit/wiener_interior_unit.cpp, which holds it to the per-sample definitions by brute force.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define TDK_YS_HD __host__ __device__
#else
#define TDK_YS_HD
#endif

namespace ys {

constexpr int K = 32, S = 8, NPC = 8;     // tile size, hop, tile PAIRS per strip
constexpr int NTC = 2 * NPC;              // tile columns per strip (Geom::G)
constexpr int SW = NTC * S + K - S;       // samples per strip row: 152
constexpr int GRP_PER_ROW = SW / 4;       // 16-B groups per staged row: 38
constexpr int GRP_PER_WAVE = 8 * GRP_PER_ROW / 4;  // 76

// ---- interior workgroups.  A workgroup (strip gx, segment gy) is INTERIOR when nothing it touches meets a frame edge:
//  * every sample column of the strip lies in the frame: 0 <= px0 and px0 + SW <= W, with px0 = S (16 gx - 3);
//  * all 16 tiles of the strip exist: 16 (gx + 1) <= ntx (implied by the line above: the last tile starts at px0 + 120 <= W - 32);
//  * every row of the segment's NB blocks lies in the frame without reflection: 0 <= S (t0 - 3) and S (t0 + NB - 3) <= H, with
//    t0 = gy TR and NB = min(TR, nty - t0) + 3.  S nty > H always, so the segment is a full one and the test is S TR (gy + 1) <= H;
//  * the plane is read with vector loads (W % 4 == 0, aligned, C == 1): `vec`.
// Both halves are intervals that start at 1 (strip 0 and segment 0 reach across the left / top edge), so the rule is stated as
// the two exclusive ends: interior <=> 1 <= gx < gx1 && 1 <= gy < gy1.  An interior workgroup runs the round loop's second
// instantiation, which carries no bounds test, no reflection, no per-sample edge loads and no tile-exists predicates; the bits
// are those of the general body (the two differ in integer addressing and control flow only).  The same function serves the
// kernel and the host query tdk_wiener_strip_interior (tests/test_wiener_interior.py holds it to a restatement from the tile
// geometry).
struct Interior {
  int gx1, gy1;
};
TDK_YS_HD inline Interior interior_range(int W, int H, int TR, bool vec) {
  Interior r = {0, 0};
  if (!vec || TR <= 0) return r;
  static_assert(SW - S * (K / S - 1) == NTC * S, "px0 + SW = 16 S (gx + 1)");
  r.gx1 = W / (NTC * S);  // S (16 gx - 3) + SW = 16 S (gx + 1) <= W
  r.gy1 = H / (S * TR);   // S TR (gy + 1) <= H
  return r;
}
TDK_YS_HD inline bool is_interior(const Interior& r, int gx, int gy) { return gx >= 1 && gx < r.gx1 && gy >= 1 && gy < r.gy1; }

// Launch order.  The edge workgroups keep the general body and are the slow ones, so they get the lowest workgroup numbers and
// start first: segment 0 (a whole row of strips), then per interior segment strip 0 and the strips right of the interior range,
// then the segments below it; the interior workgroups follow, row by row.  A permutation of the plane's (strip, segment) grid;
// slabs are addressed by the logical index gy * ngx + gx as before.  (Identity when the plane has no interior workgroup.)
TDK_YS_HD inline void launch_order(const Interior& r, int ngx, int ngy, int b, int& gx, int& gy) {
  const int iw = r.gx1 - 1, ih = r.gy1 - 1;
  if (iw <= 0 || ih <= 0) {
    gy = b / ngx;
    gx = b - gy * ngx;
    return;
  }
  const int edge = ngx * ngy - iw * ih, ew = ngx - iw;  // edge workgroups in all / per interior segment
  if (b >= edge) {
    const int k = b - edge;
    gy = 1 + k / iw;
    gx = 1 + (k - (gy - 1) * iw);
  } else if (b < ngx) {
    gy = 0;
    gx = b;
  } else if (b < ngx + ew * ih) {
    const int k = b - ngx, q = k / ew, rem = k - q * ew;
    gy = 1 + q;
    gx = rem == 0 ? 0 : r.gx1 + rem - 1;
  } else {
    const int k = b - ngx - ew * ih, q = k / ngx;
    gy = r.gy1 + q;
    gx = k - q * ngx;
  }
}

// A lane's share of the staging block.  The 8 x 152 block is 8 x 38 groups of 4 samples; wave w stages groups 76 w .. 76 w + 75 =
// block rows 2 w and 2 w + 1 whole.  Lane l takes group 76 w + l (the upper row for l >= 38) and, for l < 12, group 76 w + 64 + l
// (always the upper row).  col0 / col1: the strip column of the group's first sample.
struct StageLane {
  bool hi0, has1;
  int col0, col1;
};
TDK_YS_HD inline StageLane stage_lane(int lane) {
  static_assert(GRP_PER_WAVE == 2 * GRP_PER_ROW && GRP_PER_ROW < 64, "a wave stages two whole block rows");
  StageLane s;
  s.hi0 = lane >= GRP_PER_ROW;
  s.has1 = lane < GRP_PER_WAVE - 64;
  s.col0 = 4 * (s.hi0 ? lane - GRP_PER_ROW : lane);
  s.col1 = 4 * (lane + 64 - GRP_PER_ROW);
  return s;
}
// Interior body: element offsets of the two groups from the wave's row pointer (block row 2 w of the block, strip sample 0)
TDK_YS_HD inline unsigned interior_off0(const StageLane& s, int W) { return (s.hi0 ? (unsigned)W : 0u) + (unsigned)s.col0; }
TDK_YS_HD inline unsigned interior_off1(const StageLane& s, int W) { return (unsigned)W + (unsigned)s.col1; }

}  // namespace ys
