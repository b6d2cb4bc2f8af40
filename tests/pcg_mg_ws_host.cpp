// A stand-alone host program over fluidnet_amd/csrc/tfl_pcg_mg.hpp and the block tfl_pcg_ws.hpp appends for precondType = "mg":
// (a) the level geometry of mg_levels against its rule (2x per pooled axis, ceil, while every pooled axis is longer than
// kMgCoarsestExtent, at most kMgMaxLevels; the levels k_mg_coarse owns), (b) the child / parent maps: every fine cell's parent
// inside the coarse extent, every coarse cell's existing children inside the fine extent, each fine cell the child of exactly
// its parent, in the summation order, odd sizes included, (c) the workspace: with mg every earlier region keeps the offset it
// has without, the table without mg is the old one (total included), every mg region and every level's slice of the stacked
// arrays is written once into a buffer of exactly `total` floats (AddressSanitizer sees a slice that leaves it, the marks see
// two that overlap), and the arrays of level 0 that live in dg / y stay inside those. No GPU, no HIP call. Built and run by
// tests/test_pcg_mg_ws_cpu.py:
//   g++ -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all pcg_mg_ws_host.cpp
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../fluidnet_amd/csrc/tfl_pcg_ws.hpp"

#define CHECK(c) do { if (!(c)) { std::fprintf(stderr, "%s:%d: CHECK(%s) failed (%s)\n", __FILE__, __LINE__, #c, g_case); std::exit(1); } } while (0)

using namespace tfl;

static char g_case[160];

static bool same(WsRegion a, WsRegion b) { return a.off == b.off && a.floats == b.floats; }

// want_count / want_fb: the level count and first_block_level a shape is in the list for (-1: not stated)
static void check_levels(int Z, int Y, int X, bool is3d, int want_count = -1, int want_fb = -1) {
  const MgLevels m = mg_levels(Z, Y, X, is3d);
  if (want_count >= 0) CHECK(m.count == want_count);
  if (want_fb >= 0) CHECK(m.first_block_level == want_fb);
  // no level small enough for k_mg_coarse: first_block_level == count, and only then
  CHECK((m.first_block_level == m.count) == (m.count == 1 || m.lv[m.count - 1].n > kMgBlockCells));
  CHECK(m.count >= 1 && m.count <= kMgMaxLevels);
  CHECK(m.lv[0].Z == Z && m.lv[0].Y == Y && m.lv[0].X == X && m.lv[0].n == (long long)Z * Y * X);
  long long stacked = 0;
  for (int l = 0; l < m.count; l++) {
    const MgLevelGeom& g = m.lv[l];
    CHECK(g.n == (long long)g.Z * g.Y * g.X && g.n >= 1);
    const bool small = g.X <= kMgCoarsestExtent || g.Y <= kMgCoarsestExtent || (is3d && g.Z <= kMgCoarsestExtent);
    if (l + 1 < m.count) {
      CHECK(!small);
      const MgLevelGeom& c = m.lv[l + 1];
      CHECK(c.X == (g.X + 1) / 2 && c.Y == (g.Y + 1) / 2 && c.Z == (is3d ? (g.Z + 1) / 2 : g.Z));
      CHECK(c.off == stacked);
      stacked += c.n;
    } else {
      CHECK(small || m.count == kMgMaxLevels);
    }
  }
  CHECK(stacked == m.coarse_cells);
  CHECK(m.first_block_level >= 1 && m.first_block_level <= m.count);
  for (int l = m.first_block_level; l < m.count; l++) CHECK(m.lv[l].n <= kMgBlockCells);
  if (m.first_block_level > 1) CHECK(m.lv[m.first_block_level - 1].n > kMgBlockCells);

  // (b) the maps, level by level
  for (int l = 0; l + 1 < m.count; l++) {
    const MgLevelGeom &f = m.lv[l], &c = m.lv[l + 1];
    std::vector<int> seen(f.n, 0);
    for (int K = 0; K < c.Z; K++) for (int J = 0; J < c.Y; J++) for (int I = 0; I < c.X; I++) {
      const long long O = ((long long)K * c.Y + J) * c.X + I;
      long long last = -1;
      int existing = 0;
      for (int q = 0; q < mg_child_slots(is3d); q++) {
        int k, j, i;
        if (!mg_child(f, is3d, K, J, I, q, k, j, i)) continue;
        CHECK(k >= 0 && k < f.Z && j >= 0 && j < f.Y && i >= 0 && i < f.X);
        const long long o = ((long long)k * f.Y + j) * f.X + i;
        CHECK(o > last);                          // summation order: ascending cell index
        last = o;
        seen[o]++;
        CHECK(mg_parent(c, is3d, k, j, i) == O);
        existing++;
      }
      CHECK(existing >= 1);                        // child 0 always exists
    }
    for (long long o = 0; o < f.n; o++) CHECK(seen[o] == 1);
    for (int k = 0; k < f.Z; k++) for (int j = 0; j < f.Y; j++) for (int i = 0; i < f.X; i++) {
      const long long P = mg_parent(c, is3d, k, j, i);
      CHECK(P >= 0 && P < c.n);
    }
  }
}

static void check_ws(int Z, int Y, int X, bool is3d) {
  const long long n = (long long)Z * Y * X;
  const PcgWs a = pcg_ws(Z, Y, X, false), t = pcg_ws(Z, Y, X, false, true, is3d);
  // the old table is unchanged by the new arguments' defaults, with and without wavefronts
  for (int wf = 0; wf < (is3d ? 2 : 1); wf++) {
    const PcgWs o1 = pcg_ws(Z, Y, X, wf != 0), o2 = pcg_ws(Z, Y, X, wf != 0, false, is3d);
    CHECK(o1.total == o2.total && same(o1.counters, o2.counters) && same(o1.wf_err, o2.wf_err));
    CHECK(o1.mg_invd0.floats == 0 && o1.mg_c_zb.floats == 0);
  }
  // every old region keeps its offset under mg
  CHECK(same(a.partials, t.partials) && same(a.p_den, t.p_den) && same(a.p_rr, t.p_rr) && same(a.state, t.state));
  CHECK(same(a.label, t.label) && same(a.size_at, t.size_at) && same(a.x, t.x) && same(a.r, t.r) && same(a.z, t.z));
  CHECK(same(a.s, t.s) && same(a.w, t.w) && same(a.dg, t.dg) && same(a.y, t.y) && same(a.roots, t.roots) && same(a.counters, t.counters));
  CHECK(t.wf_cc.floats == 0 && t.wf_hk.floats == 0 && t.wf_clear.floats == 0);
  CHECK(t.mg_invd0.off == a.total);                // appended behind the existing table
  const MgLevels m = mg_levels(Z, Y, X, is3d);
  CHECK(t.total == a.total + 4 * n + 8 * m.coarse_cells);
  // walk it: one buffer of exactly `total` floats, every array of every level written once
  std::vector<float> ws(t.total, 0.0f);
  std::vector<unsigned char> mark(t.total, 0);
  auto touch = [&](long long off, long long floats) {
    CHECK(off >= a.total && off + floats <= t.total);
    for (long long e = 0; e < floats; e++) { ws[off + e] = 1.0f; CHECK(mark[off + e] == 0); mark[off + e] = 1; }
  };
  const WsRegion fine[4] = {t.mg_invd0, t.mg_cx0, t.mg_cy0, t.mg_cz0};
  for (const WsRegion& r : fine) { CHECK(r.floats == n); touch(r.off, n); }
  const WsRegion coarse[8] = {t.mg_c_diag, t.mg_c_invd, t.mg_c_cx, t.mg_c_cy, t.mg_c_cz, t.mg_c_r, t.mg_c_za, t.mg_c_zb};
  for (const WsRegion& r : coarse) {
    CHECK(r.floats == m.coarse_cells);
    for (int l = 1; l < m.count; l++) touch(r.off + m.lv[l].off, m.lv[l].n);
  }
  for (long long e = a.total; e < t.total; e++) CHECK(mark[e] == 1);       // nothing appended is left over
  // level 0 borrows dg (diag), y (its second iterate) and w (the right-hand side of a closed component's cycle): n floats each;
  // the set-up's "open" word lies in the counters' slot behind the words label_components uses
  CHECK(t.dg.floats == n && t.y.floats == n && t.w.floats == n);
  CHECK(t.counters.floats == kPcgCounterWords && kPcgMgOpenWord >= kPcgLabelWords && kPcgMgOpenWord < kPcgCounterWords);
}

int main() {
  const int sizes[][3] = {{1, 3, 3}, {1, 5, 5}, {1, 24, 28}, {1, 33, 47}, {1, 30, 34}, {1, 128, 128}, {1, 129, 65}, {1, 6, 1000}, {1, 1025, 9},
                          {3, 3, 3}, {5, 5, 5}, {9, 11, 13}, {8, 10, 16}, {12, 17, 20}, {36, 134, 22}, {64, 64, 64}, {65, 33, 17}, {5, 200, 7}};
  for (const auto& s : sizes) {
    const bool is3d = s[0] > 1;
    std::snprintf(g_case, sizeof(g_case), "mg %d x %d x %d", s[0], s[1], s[2]);
    check_levels(s[0], s[1], s[2], is3d);
    check_ws(s[0], s[1], s[2], is3d);
  }
  // the shapes whose coarse levels run one launch per operation (tests/pcg_mg_ref64.py WIDE_SHAPES): {Z, Y, X, count, first_block_level}.
  // Levels 1 and 2 as launches (a stacked offset > 0), even and odd; the thin grids, where no level is small enough for
  // k_mg_coarse (first_block_level == count); one level only.
  const int wide[][5] = {{1, 132, 136, 7, 2}, {1, 260, 264, 8, 3}, {1, 259, 263, 8, 3}, {24, 36, 40, 4, 2},
                         {1, 8, 2100, 2, 2}, {6, 6, 1000, 2, 2}, {1, 4, 60, 1, 1}, {4, 12, 14, 1, 1}};
  for (const auto& s : wide) {
    const bool is3d = s[0] > 1;
    std::snprintf(g_case, sizeof(g_case), "mg wide %d x %d x %d", s[0], s[1], s[2]);
    check_levels(s[0], s[1], s[2], is3d, s[3], s[4]);
    check_ws(s[0], s[1], s[2], is3d);
    const MgLevels m = mg_levels(s[0], s[1], s[2], is3d);
    if (s[4] == 3) CHECK(m.lv[2].off == m.lv[1].n && m.lv[2].n > kMgBlockCells);
    if (s[3] == 2 && s[4] == 2) CHECK(m.lv[1].n > kMgBlockCells);              // the thin shapes: the coarsest level as launches
  }
  // a 3-D call on a grid one plane thick pools z as well and must still fit the size of the 2-D table (what the library sizes for Z = 1)
  CHECK(pcg_ws(1, 40, 40, false, true, true).total <= pcg_ws(1, 40, 40, false, true, false).total);
  check_levels(1, 40, 40, true);
  // the level count stops at kMgMaxLevels
  CHECK(mg_levels(1, 1 << 14, 1 << 14, false).count == kMgMaxLevels);
  std::printf("pcg mg workspace OK\n");
  return 0;
}
