// A stand-alone host program over the workspace table of solveLinearSystemPCGBatched (fluidnet_amd/csrc/tfl_pcg_ws.hpp,
// pcg_batched_ws): for B = 1, 3, 16 at odd 2-D and 3-D sizes, with and without the multigrid block, (a) every region -- each
// array of each item's block, the states, the records, the labelling words and the component table -- is written once into a
// buffer of exactly `total` floats (AddressSanitizer sees a region that leaves it, the marks see two that overlap), (b) the
// stride is even (8-byte aligned) and holds an item's block, so every fp64 region of every item sits on 8 bytes, (c) the tables
// hold what the kernels index (B state slots of kPcgStateFloats, B records, kPcgCcWords words and kMaxComponents pairs per item),
// (d) pcg_ws is what it was: its offsets against the expressions written out here, its totals, with and without wavefronts.
// No GPU, no HIP call. Built and run by tests/test_pcg_batched_ws_cpu.py:
//   g++ -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all pcg_batched_ws_host.cpp
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../fluidnet_amd/csrc/tfl_pcg_ws.hpp"

#define CHECK(c) do { if (!(c)) { std::fprintf(stderr, "%s:%d: CHECK(%s) failed (%s)\n", __FILE__, __LINE__, #c, g_case); std::exit(1); } } while (0)

using namespace tfl;

static char g_case[160];

static void check_batched(int B, int Z, int Y, int X, bool mg, bool is3d) {
  const long long n = (long long)Z * Y * X;
  const PcgBatchedWs t = pcg_batched_ws(B, Z, Y, X, mg, is3d);
  const PcgWs one = pcg_ws(Z, Y, X, false, mg, is3d);
  CHECK(t.item.total == one.total && t.item.x.off == one.x.off && t.item.mg_c_zb.off == one.mg_c_zb.off);
  CHECK(t.item.wf_cc.floats == 0 && t.item.wf_hk.floats == 0 && t.item.wf_clear.floats == 0);      // no wavefront regions
  CHECK(t.stride % 2 == 0 && t.stride >= one.total && t.stride <= one.total + 1);
  CHECK(t.items.off == 0 && t.items.floats == B * t.stride);
  CHECK(t.states.floats == B * kPcgStateFloats && t.states.off % 2 == 0);
  CHECK(sizeof(PcgItemRec) == sizeof(float) * kPcgRecFloats && t.recs.floats == B * kPcgRecFloats);
  CHECK(t.cc.floats == (long long)B * kPcgCcWords && kPcgCcWords >= 3);
  CHECK(t.comps.floats == (long long)B * kMaxComponents * 2);

  std::vector<float> ws(t.total, 0.0f);
  std::vector<unsigned char> mark(t.total, 0);
  auto touch = [&](long long off, long long floats) {
    CHECK(off >= 0 && floats >= 0 && off + floats <= t.total);
    for (long long e = 0; e < floats; e++) { ws[off + e] = 1.0f; CHECK(mark[off + e] == 0); mark[off + e] = 1; }
  };
  const PcgWs& w = t.item;
  const WsRegion per_item[] = {w.partials, w.p_den, w.p_rr, w.state, w.label, w.size_at, w.x, w.r, w.z, w.s, w.w, w.dg, w.y, w.roots,
                               w.counters, w.mg_invd0, w.mg_cx0, w.mg_cy0, w.mg_cz0, w.mg_c_diag, w.mg_c_invd, w.mg_c_cx, w.mg_c_cy,
                               w.mg_c_cz, w.mg_c_r, w.mg_c_za, w.mg_c_zb};
  for (int b = 0; b < B; b++) {
    const long long base = t.items.off + b * t.stride;
    for (const WsRegion& r : per_item) touch(base + r.off, r.floats);
    // the fp64 regions of every item on 8 bytes (the workspace itself is 8-byte aligned)
    CHECK((base + w.partials.off) % 2 == 0 && (base + w.p_den.off) % 2 == 0 && (base + w.p_rr.off) % 2 == 0);
    CHECK(w.x.floats == n && w.label.floats == n && w.roots.floats == kMaxComponents);
    if (mg) CHECK(w.mg_invd0.floats == n && w.mg_c_zb.floats == mg_levels(Z, Y, X, is3d).coarse_cells);
    else CHECK(w.mg_invd0.floats == 0 && w.mg_c_zb.floats == 0);
  }
  for (int b = 0; b < B; b++) touch(t.states.off + b * kPcgStateFloats, kPcgStateFloats);
  touch(t.recs.off, t.recs.floats);
  touch(t.cc.off, t.cc.floats);
  touch(t.comps.off, t.comps.floats);
  // what is not marked is the padding of the stride alone
  long long idle = 0;
  for (long long e = 0; e < t.total; e++) idle += mark[e] == 0;
  CHECK(idle == B * (t.stride - one.total));
}

// pcg_ws as it was before the batched table: every offset against the expression written out
static void check_old(int Z, int Y, int X, bool is3d) {
  const long long n = (long long)Z * Y * X;
  for (int wf = 0; wf < (is3d ? 2 : 1); wf++) {
    const PcgWs t = pcg_ws(Z, Y, X, wf != 0);
    long long at = 0;
    CHECK(t.partials.off == at); at += 2 * kRedBlocks;
    CHECK(t.p_den.off == at); at += 2 * kRedBlocks;
    CHECK(t.p_rr.off == at); at += 2 * kRedBlocks;
    CHECK(t.state.off == at && t.state.floats == 128); at += 128;
    CHECK(t.label.off == at); at += n;
    CHECK(t.size_at.off == at); at += n;
    const WsRegion v[] = {t.x, t.r, t.z, t.s, t.w, t.dg, t.y};
    for (const WsRegion& r : v) { CHECK(r.off == at && r.floats == n); at += n; }
    CHECK(t.roots.off == at && t.roots.floats == 4096); at += 4096;
    CHECK(t.counters.off == at && t.counters.floats == 64); at += 64;
    if (wf) at += wf_floats(Z, Y, X) + kPcgWfSlack;
    CHECK(t.total == at);
    const PcgWs m = pcg_ws(Z, Y, X, false, true, is3d);
    CHECK(m.total == pcg_ws(Z, Y, X, false).total + 4 * n + 8 * mg_levels(Z, Y, X, is3d).coarse_cells);
  }
  const NpmWs q = npm_ws(Z, Y, X);
  CHECK(q.total == 4 * n + 16 + kMaxComponents);
}

int main() {
  const int sizes[][3] = {{1, 3, 3}, {1, 5, 7}, {1, 24, 28}, {1, 33, 47}, {1, 129, 65}, {3, 3, 3}, {9, 11, 13}, {5, 7, 9}, {13, 17, 21}, {24, 36, 40}};
  const int batches[] = {1, 3, 16};
  for (const auto& s : sizes) {
    const bool is3d = s[0] > 1;
    std::snprintf(g_case, sizeof(g_case), "old %d x %d x %d", s[0], s[1], s[2]);
    check_old(s[0], s[1], s[2], is3d);
    for (int B : batches)
      for (int mg = 0; mg < 2; mg++) {
        std::snprintf(g_case, sizeof(g_case), "B %d, %d x %d x %d, mg %d", B, s[0], s[1], s[2], mg);
        check_batched(B, s[0], s[1], s[2], mg != 0, is3d);
      }
  }
  std::printf("pcg batched workspace OK\n");
  return 0;
}
