// A stand-alone host program over fluidnet_amd/csrc/tfl_pcg_ws.hpp -- the workspace tables of solveLinearSystemPCG (pcg_solve)
// and normalizePressureMean. It is the record of what the layout was when the tables replaced the literals in pcg.hip: (a) every
// region's offset and length against the expression pcg_solve / normalize_pressure_mean used to write out, (b) the totals
// against the size formulas pcg_workspace_floats / npm_workspace_floats used to restate, every region inside them whatever the
// run-time alignment pad, (c) all regions pairwise disjoint, (d) the alignment of the fp64 regions and of the wavefront block,
// (e) the span the per-solve memset clears, (f) the guard pairs of the hand-off arrays. No GPU, no HIP call. Built and run by
// tests/test_pcg_ws_cpu.py:
//   g++ -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all pcg_ws_host.cpp
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../fluidnet_amd/csrc/tfl_pcg_ws.hpp"

#define CHECK(c) do { if (!(c)) { std::fprintf(stderr, "%s:%d: CHECK(%s) failed (%s)\n", __FILE__, __LINE__, #c, g_case); std::exit(1); } } while (0)

using namespace tfl;

static char g_case[160];

static bool is(WsRegion r, long long off, long long floats) { return r.off == off && r.floats == floats; }
static bool disjoint(WsRegion a, WsRegion b) { return a.off + a.floats <= b.off || b.off + b.floats <= a.off; }
static WsRegion moved(WsRegion r, long long by) { return {r.off + by, r.floats}; }

// (f) what the comment on kWfGuard promises. A helper wave reads the slab hand-off pairs [block][t / 4][row][t % 4] of the steps
// t in [-G, NT + G), G = kWfLag * (kWfPlanes - 1), without clamping: whole groups of four steps, 4 * kWfRows pairs each, on either
// side of a block's rows. It reads the strip hand-off pairs [block][plane][t] up to 63 steps, plus the steps of one interval, on
// either side, and its idle lanes store up to 64 pairs in front of the array.
constexpr long long kSlabReach = kWfLag * (kWfPlanes - 1);
static_assert(kWfGuard >= (kSlabReach + 3) / 4 * 4 * kWfRows, "slab hand-off guard");
static_assert(kWfGuard >= 63 + kWfLag && kWfGuard >= 64, "strip hand-off guard");
static_assert(kWfGuard % 2 == 0, "the first pair behind a guard stays on 16 bytes");

static void check_pcg(int Z, int Y, int X, bool wavefronts) {
  std::snprintf(g_case, sizeof(g_case), "pcg %d x %d x %d, wavefronts %d", Z, Y, X, (int)wavefronts);
  const long long n = (long long)Z * Y * X;
  const PcgWs t = pcg_ws(Z, Y, X, wavefronts);

  // ---- (a) the layout as pcg_solve wrote it out -----------------------------------------------------------------------------
  // double* partials = workspace; p_den = partials + kRedBlocks; p_rr = partials + 2 * kRedBlocks; S = partials + 3 * kRedBlocks
  CHECK(is(t.partials, 0, 2 * kRedBlocks) && is(t.p_den, 2 * kRedBlocks, 2 * kRedBlocks) && is(t.p_rr, 2 * 2 * kRedBlocks, 2 * kRedBlocks));
  CHECK(is(t.state, 2 * 3 * kRedBlocks, 2 * 64));
  // float* base = workspace + 2 * (3 * kRedBlocks + 64): label, size_at, x, r, z, s, w, dg, y at base + 0 .. 8 n
  const long long base = 2 * (3 * kRedBlocks + 64);
  CHECK(is(t.label, base, n) && is(t.size_at, base + n, n));
  CHECK(is(t.x, base + 2 * n, n) && is(t.r, base + 3 * n, n) && is(t.z, base + 4 * n, n) && is(t.s, base + 5 * n, n));
  CHECK(is(t.w, base + 6 * n, n) && is(t.dg, base + 7 * n, n) && is(t.y, base + 8 * n, n));
  // roots = base + 9 * n; counters = roots + kMaxComponents; 64 floats for them
  CHECK(is(t.roots, base + 9 * n, kMaxComponents) && is(t.counters, base + 9 * n + kMaxComponents, 64));
  // wfbase = base + 9 * n + kMaxComponents + 64 (then rounded up to 16 bytes); wtot = wg.sub * wg.ns * wg.nb;
  // cs = wfbase; rsk = cs + wtot; qsk = cs + 2 * wtot; zsk = cs + 3 * wtot; wf_hk = (float2*)(cs + 4 * wtot) + kWfGuard;
  // wf_hs = (float2*)(cs + 4 * wtot + wf_handoff_k(wg)) + kWfGuard; wferr = cs + 4 * wtot + wf_handoff_k(wg) + wf_handoff_s(wg)
  // the memset: from cs, tot * 4 + wf_handoff_k(wg) + wf_handoff_s(wg) + 16 floats
  long long wf_floats_parent = 0;
  if (wavefronts) {
    const long long wfbase = base + 9 * n + kMaxComponents + 64;
    const int ns = (Y - 2 + kWfRows - 1) / kWfRows, nb = (Z - 2 + kWfPlanes - 1) / kWfPlanes;
    const int NT = (((X - 2) + (kWfRows - 1) + kWfLag * (kWfPlanes - 1)) + kWfDepth - 1) / kWfDepth * kWfDepth;
    const long long sub = (long long)kWfPlanes * NT * kWfRows, wtot = sub * ns * nb;
    const long long hk = 2ll * ns * nb * NT * kWfRows + 4 * kWfGuard, hs = 2ll * ns * nb * kWfPlanes * NT + 4 * kWfGuard;
    CHECK(t.geom.X == X && t.geom.Y == Y && t.geom.Z == Z && t.geom.ns == ns && t.geom.nb == nb && t.geom.NT == NT && t.geom.sub == sub);
    CHECK(t.geom.b_lo == 0 && t.geom.b_cnt == nb && NT % kWfDepth == 0 && NT >= (X - 2) + (kWfRows - 1) + kWfLag * (kWfPlanes - 1));
    CHECK(is(t.wf_cc, wfbase, wtot) && is(t.wf_r, wfbase + wtot, wtot) && is(t.wf_q, wfbase + 2 * wtot, wtot) && is(t.wf_z, wfbase + 3 * wtot, wtot));
    CHECK(is(t.wf_hk, wfbase + 4 * wtot, hk) && is(t.wf_hs, wfbase + 4 * wtot + hk, hs));
    CHECK(is(t.wf_err, wfbase + 4 * wtot + hk + hs, 1));
    CHECK(is(t.wf_clear, wfbase, wtot * 4 + hk + hs + 16));
    wf_floats_parent = 4 * sub * ns * nb + hk + hs + 64;
    CHECK(wf_floats_parent == wf_floats(Z, Y, X));
    // (f) the hand-off arrays are their blocks' pairs with kWfGuard pairs in front and behind
    CHECK(t.wf_hk.floats == 2 * ((long long)ns * nb * NT * kWfRows + 2 * kWfGuard));
    CHECK(t.wf_hs.floats == 2 * ((long long)ns * nb * kWfPlanes * NT + 2 * kWfGuard));
  } else {
    for (WsRegion r : {t.wf_cc, t.wf_r, t.wf_q, t.wf_z, t.wf_hk, t.wf_hs, t.wf_err, t.wf_clear}) CHECK(is(r, 0, 0));
    CHECK(t.geom.ns == 0 && t.geom.nb == 0 && t.geom.NT == 0 && t.geom.sub == 0);
  }

  // ---- (b) the total: 2 (3 kRedBlocks + 64) + 9 n + kMaxComponents + 64 (+ wf_floats + 4) ------------------------------------
  CHECK(t.total == 2 * (3 * kRedBlocks + 64) + 9 * n + kMaxComponents + 64 + (wavefronts ? wf_floats_parent + 4 : 0));
  const std::vector<WsRegion> fixed = {t.partials, t.p_den, t.p_rr, t.state, t.label, t.size_at, t.x, t.r, t.z, t.s, t.w, t.dg, t.y, t.roots, t.counters};
  const std::vector<WsRegion> wf = {t.wf_cc, t.wf_r, t.wf_q, t.wf_z, t.wf_hk, t.wf_hs, t.wf_err};
  for (WsRegion r : fixed) CHECK(r.off >= 0 && r.floats > 0 && r.off + r.floats <= t.total);
  // ---- (d) fp64 regions on 8 bytes relative to the workspace
  for (WsRegion r : {t.partials, t.p_den, t.p_rr, t.state}) CHECK(r.off % 2 == 0);
  if (!wavefronts) {
    for (size_t a = 0; a < fixed.size(); a++) for (size_t b = a + 1; b < fixed.size(); b++) CHECK(disjoint(fixed[a], fixed[b]));
    return;
  }
  // the round-up as pcg_solve applies it, for an 8-byte aligned workspace on and off a 16-byte boundary
  for (uintptr_t addr : {(uintptr_t)0x7f0000001000ull, (uintptr_t)0x7f0000001008ull}) {
    const long long pad = pcg_wf_pad(reinterpret_cast<const float*>(addr), t);
    CHECK(pad >= 0 && pad <= 3 && (addr + 4 * (uintptr_t)(t.wf_cc.off + pad)) % 16 == 0);
    CHECK(pad == (long long)((4 - (((addr + 4 * (uintptr_t)t.wf_cc.off) >> 2) & 3)) & 3));      // the parent's line on the parent's pointer
  }
  for (long long pad = 0; pad <= 3; pad++) {
    std::vector<WsRegion> all = fixed;
    for (WsRegion r : wf) {
      CHECK(r.floats > 0);
      all.push_back(moved(r, pad));
      CHECK(r.off + pad + r.floats <= t.total);                                   // (b) inside the total for every pad
    }
    // ---- (c) nothing aliases
    for (size_t a = 0; a < all.size(); a++) for (size_t b = a + 1; b < all.size(); b++) CHECK(disjoint(all[a], all[b]));
    // ---- (e) the memset starts at cc, ends at or behind the error word and stays inside the total
    const WsRegion clear = moved(t.wf_clear, pad);
    CHECK(clear.off == t.wf_cc.off + pad && clear.off + clear.floats >= t.wf_err.off + pad + 1 && clear.off + clear.floats <= t.total);
    for (WsRegion r : fixed) CHECK(disjoint(clear, r));
  }
  // ---- (d) once cc sits on 16 bytes, so do the other skewed arrays and the first pair behind the guards of both hand-off arrays
  for (WsRegion r : {t.wf_r, t.wf_q, t.wf_z}) CHECK((r.off - t.wf_cc.off) % 4 == 0);
  CHECK((t.wf_hk.off + 2 * kWfGuard - t.wf_cc.off) % 4 == 0 && (t.wf_hs.off + 2 * kWfGuard - t.wf_cc.off) % 4 == 0);
}

static void check_npm(int Z, int Y, int X) {
  std::snprintf(g_case, sizeof(g_case), "npm %d x %d x %d", Z, Y, X);
  const long long n = (long long)Z * Y * X;
  const NpmWs t = npm_ws(Z, Y, X);
  // sum_at = (double*)workspace; label = workspace + 2 * n; size_at = workspace + 3 * n; counters = workspace + 4 * n with
  // [0] changed, [1] count, [2] border fluid, [3..] the roots sink (k_cc_count stores at most kMaxComponents roots)
  CHECK(is(t.sum_at, 0, 2 * n) && is(t.label, 2 * n, n) && is(t.size_at, 3 * n, n) && is(t.counters, 4 * n, 3));
  CHECK(is(t.roots, 4 * n + 3, kMaxComponents));
  CHECK(t.total == 4ll * Z * Y * X + 16 + kMaxComponents);
  CHECK(t.sum_at.off % 2 == 0);
  const std::vector<WsRegion> all = {t.sum_at, t.label, t.size_at, t.counters, t.roots};
  for (size_t a = 0; a < all.size(); a++) {
    CHECK(all[a].off >= 0 && all[a].floats > 0 && all[a].off + all[a].floats <= t.total);
    for (size_t b = a + 1; b < all.size(); b++) CHECK(disjoint(all[a], all[b]));
  }
}

int main() {
  static_assert(kWfRows == 64 && kWfPlanes == 8 && kWfLag == 2 && kWfDepth == 16 && kWfGuard == 1280, "the shapes below sit on the seams of these");
  const int shapes2[][3] = {{1, 3, 3}, {1, 16, 16}, {1, 128, 128}};
  const int shapes3[][3] = {
      {3, 3, 3},
      {10, 66, 5},      // one strip (Y - 2 = 64), one slab (Z - 2 = 8), NT = 3 + 77 = 80 on a multiple of kWfDepth
      {10, 67, 5},      // two strips
      {11, 66, 5},      // two slabs
      {10, 66, 6},      // NT one past: 81 -> 96
      {11, 67, 6}, {19, 131, 8}, {12, 20, 24},      // the suite's own
      {128, 128, 128}, {256, 256, 256}};
  int cases = 0;
  for (const auto& d : shapes2) {
    check_pcg(d[0], d[1], d[2], false); check_npm(d[0], d[1], d[2]); cases += 2;      // (no wavefronts on a 2-D grid: wf_usable)
  }
  for (const auto& d : shapes3)
    for (bool wavefronts : {false, true}) { check_pcg(d[0], d[1], d[2], wavefronts); check_npm(d[0], d[1], d[2]); cases += 2; }
  std::printf("pcg workspace OK (%d cases)\n", cases);
  return 0;
}
