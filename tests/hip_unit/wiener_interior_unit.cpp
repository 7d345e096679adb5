// Stand-alone host program: csrc/tdk_wiener_interior.h against the per-sample definitions, by brute force.  No device code, no HIP.
//   * is_interior(interior_range(...)) == "every sample the workgroup reads lies in the frame unreflected, all 16 tiles exist, vec";
//   * launch_order is a permutation of the grid that puts every edge workgroup in front of every interior one;
//   * stage_lane / interior_off0 / interior_off1: for every wave, lane and block of an interior workgroup the interior body's address
//     (row pointer + constant offset, advanced by 8 W per block) is the general body's (group = 76 wave + lane [+ 64], block row =
//     group / 38, column = 4 (group % 38), row through reflect_index), and every lane's share covers the 8 x 152 block exactly once.
// Build and run, from the repository root (any host compiler; sanitizers optional):
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined tests/hip_unit/wiener_interior_unit.cpp -o wiener_interior_unit && ./wiener_interior_unit
#include <stdio.h>

#include <algorithm>
#include <vector>

#include "../../torch-darktable_amd/csrc/tdk_wiener_interior.h"

static int failures = 0;
#define CHECK(cond, ...)                  \
  do {                                    \
    if (!(cond)) {                        \
      if (failures++ < 20) {              \
        printf("FAIL %s: ", #cond);       \
        printf(__VA_ARGS__);              \
        printf("\n");                     \
      }                                   \
    }                                     \
  } while (0)

static int reflect_index(int x, int limit) {  // csrc/wiener.hip
  x = x < 0 ? -x : x;
  return std::min(x, 2 * limit - 1 - x);
}

struct G {
  int ntx, nty, ngx, ngy;
};
static G geometry(int W, int H, int TR) {  // geometry_ys of csrc/wiener.hip
  G g;
  g.ntx = (W - 1) / ys::S + 4;
  g.nty = (H - 1) / ys::S + 4;
  g.ngx = (g.ntx + ys::NTC - 1) / ys::NTC;
  g.ngy = (g.nty + TR - 1) / TR;
  return g;
}

static bool by_samples(int W, int H, int TR, const G& g, int gx, int gy) {
  if (W % 4 != 0) return false;
  const int t0 = gy * TR, NB = std::min(t0 + TR, g.nty) - t0 + 3, px0 = (gx * ys::NTC - 3) * ys::S;
  for (int q = 0; q < NB; q++)
    for (int r = 0; r < 8; r++) {
      const int y = 8 * (t0 + q) + r - 24;
      if (y < 0 || y >= H || reflect_index(y, H) != y) return false;
    }
  for (int c = 0; c < ys::SW; c++)
    if (px0 + c < 0 || px0 + c >= W) return false;
  return gx * ys::NTC + ys::NTC <= g.ntx;
}

int main() {
  long checked = 0, interior = 0, addresses = 0;
  // a lane's share covers the staging block exactly once
  {
    std::vector<int> hits(8 * ys::SW / 4, 0);
    for (int wave = 0; wave < 4; wave++)
      for (int lane = 0; lane < 64; lane++) {
        const ys::StageLane s = ys::stage_lane(lane);
        hits[(2 * wave + (s.hi0 ? 1 : 0)) * ys::GRP_PER_ROW + s.col0 / 4]++;
        if (s.has1) hits[(2 * wave + 1) * ys::GRP_PER_ROW + s.col1 / 4]++;
        CHECK(s.col0 >= 0 && s.col0 + 4 <= ys::SW && (!s.has1 || (s.col1 >= 0 && s.col1 + 4 <= ys::SW)), "lane %d", lane);
      }
    for (size_t k = 0; k < hits.size(); k++) CHECK(hits[k] == 1, "group %zu staged %d times", k, hits[k]);
  }
  const int TRS[] = {8, 9, 13, 26};
  for (int TR : TRS)
    for (int W = 32; W <= 700; W += (W < 200 ? 7 : 1))
      for (int H = 32; H <= 32 * TR + 40; H += (H > 16 * TR - 12 && H < 16 * TR + 12) || (H > 24 * TR - 10 && H < 24 * TR + 10) ? 1 : 5) {
        if (W > 400 && W % 4 != 0 && W % 64 > 8) continue;  // (keeps the run short: W % 4 != 0 never has an interior workgroup)
        const G g = geometry(W, H, TR);
        const ys::Interior ir = ys::interior_range(W, H, TR, W % 4 == 0);
        const int n = g.ngx * g.ngy;
        std::vector<int> seen(n, 0);
        int edge = 0;
        for (int gy = 0; gy < g.ngy; gy++)
          for (int gx = 0; gx < g.ngx; gx++) {
            const bool in = ys::is_interior(ir, gx, gy);
            CHECK(in == by_samples(W, H, TR, g, gx, gy), "W %d H %d TR %d (%d, %d): rule %d", W, H, TR, gx, gy, (int)in);
            checked++;
            edge += !in;
            if (!in) continue;
            interior++;
            // the interior body's addresses, per wave, lane and block
            const int t0 = gy * TR, NB = std::min(t0 + TR, g.nty) - t0 + 3, px0 = (gx * ys::NTC - 3) * ys::S;
            for (int wave = 0; wave < 4; wave++) {
              size_t rowp = (size_t)(unsigned)(ys::S * (t0 - 3) + 2 * wave) * (unsigned)W + (unsigned)px0;
              for (int q = 0; q < NB; q++, rowp += (size_t)(unsigned)(ys::S * W))
                for (int lane = 0; lane < 64; lane++) {
                  const ys::StageLane s = ys::stage_lane(lane);
                  for (int second = 0; second < (s.has1 ? 2 : 1); second++) {
                    const int grp = ys::GRP_PER_WAVE * wave + lane + 64 * second;
                    const int brow = grp / ys::GRP_PER_ROW, x = px0 + 4 * (grp - brow * ys::GRP_PER_ROW);
                    const size_t general = (size_t)(unsigned)reflect_index(8 * (t0 + q) + brow - 24, H) * (unsigned)W + x;
                    const size_t inner = rowp + (second ? ys::interior_off1(s, W) : ys::interior_off0(s, W));
                    CHECK(inner == general && inner + 4 <= (size_t)W * H, "W %d H %d TR %d (%d, %d) wave %d lane %d block %d", W, H, TR, gx, gy, wave, lane, q);
                    addresses++;
                  }
                }
            }
          }
        for (int b = 0; b < n; b++) {
          int gx = -1, gy = -1;
          ys::launch_order(ir, g.ngx, g.ngy, b, gx, gy);
          CHECK(gx >= 0 && gx < g.ngx && gy >= 0 && gy < g.ngy, "W %d H %d TR %d workgroup %d -> (%d, %d)", W, H, TR, b, gx, gy);
          if (gx < 0 || gx >= g.ngx || gy < 0 || gy >= g.ngy) continue;
          seen[gy * g.ngx + gx]++;
          CHECK(ys::is_interior(ir, gx, gy) == (b >= edge), "W %d H %d TR %d workgroup %d of %d (edge %d)", W, H, TR, b, n, edge);
        }
        for (int k = 0; k < n; k++) CHECK(seen[k] == 1, "W %d H %d TR %d: (strip %d, segment %d) taken %d times", W, H, TR, k % g.ngx, k / g.ngx, seen[k]);
      }
  // 12 MP
  {
    const G g = geometry(4096, 3072, 26);
    const ys::Interior ir = ys::interior_range(4096, 3072, 26, true);
    int count = 0;
    for (int gy = 0; gy < g.ngy; gy++)
      for (int gx = 0; gx < g.ngx; gx++) {
        CHECK(ys::is_interior(ir, gx, gy) == by_samples(4096, 3072, 26, g, gx, gy), "12 MP (%d, %d)", gx, gy);
        count += ys::is_interior(ir, gx, gy);
      }
    CHECK(g.ngx == 33 && g.ngy == 15 && count == 403, "12 MP: %d x %d, %d interior", g.ngx, g.ngy, count);
  }
  printf("%ld workgroups checked, %ld interior, %ld addresses, %d failures\n", checked, interior, addresses, failures);
  return failures ? 1 : 0;
}
