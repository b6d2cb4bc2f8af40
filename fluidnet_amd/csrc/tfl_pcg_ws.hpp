// tfl_pcg_ws.hpp -- the workspaces of solveLinearSystemPCG and normalizePressureMean (pcg.hip) as ONE table each: every region
// of the caller's scratch array as {offset, floats} and the floats the whole table needs. pcg_solve and normalize_pressure_mean
// build all their views from it, and tfl_pcg_workspace_floats / tfl_normalize_workspace_floats take their sizes from it. Nothing
// aliases in these workspaces: every region is disjoint from every other. With it the plain data the host code and the kernels
// share: the solver's device state and the geometry of the pipelined wavefront sweeps with their compile-time shape.
// Held by a stand-alone host program (tests/pcg_ws_host.cpp: every offset against the expression pcg_solve used to write out,
// the totals, disjointness, alignment, the cleared span and the guard pairs). Plain C++ without a HIP header.
// pcg_batched_ws is the table of solveLinearSystemPCGBatched: B of pcg_ws's blocks and the per-item tables (held by
// tests/pcg_batched_ws_host.cpp).
#pragma once

#include <cstdint>

#include "tfl_pcg_mg.hpp"       // mg_levels: the hierarchy of precondType = "mg"
#include "tfl_step_ws.hpp"      // WsRegion

namespace tfl {

constexpr int kRedBlocks = 512;    // partial sums per dot product
constexpr int kMaxComponents = 4096;

// Device-resident solver state of one component solve.
struct PcgState {
  double rr1, rr0;         // current / previous ||r||^2
  double num, prev_num;    // r.z of this / the previous iteration (preconditioned form)
  double den;              // s.A s
  float alpha, beta;
  float tol2;
  int iter, max_iter, done, first, bad;   // bad: a NaN residual was seen
  int pending;                            // an update's r.r partials have not been folded into rr1 yet
  double sum_x;
};
constexpr long long kPcgStateFloats = 2 * 64;      // its slot: 64 doubles
static_assert(sizeof(PcgState) <= 64 * sizeof(double), "PcgState outgrew its slot in the workspace");

// ---- the shape of the pipelined wavefront sweeps (pcg.hip, "the triangular solves as TWO launches") ------------------------
#ifndef TFL_WF_PLANES
#define TFL_WF_PLANES 8
#endif
#ifndef TFL_WF_DEPTH
#define TFL_WF_DEPTH 16
#endif
// kWfDepth: steps the operands are prefetched ahead; kWfHelperAhead: exchange intervals the helper wave prefetches the
// predecessors' pairs ahead (a block can only run that far + the memory round trip behind its predecessor)
#ifndef TFL_WF_LAG
#define TFL_WF_LAG 2
#endif
#ifndef TFL_WF_HELPER_AHEAD
#define TFL_WF_HELPER_AHEAD 4
#endif
constexpr int kWfRows = 64, kWfPlanes = TFL_WF_PLANES, kWfLag = TFL_WF_LAG, kWfDepth = TFL_WF_DEPTH, kWfHelperAhead = TFL_WF_HELPER_AHEAD, kWfMaxBlocks = 240;
static_assert(kWfDepth % 4 == 0 && (kWfLag == 1 || kWfLag == 2 || kWfLag == 4), "operands in groups of four steps");
static_assert(kWfHelperAhead >= 1 && (kWfDepth / kWfLag) % kWfHelperAhead == 0, "the helper's rotating slots repeat with the unrolled loop");
static_assert(kWfPlanes * kWfLag <= 64, "one helper lane per (plane, step of the interval)");

struct WfGeom {
  int X, Y, Z, ns, nb, NT;     // strips, slabs, steps per sub-box (a multiple of kWfDepth)
  long long sub;               // cells of one sub-box in the skewed arrays = kWfPlanes * NT * kWfRows
  int b_lo, b_cnt;             // the slabs [b_lo, b_lo + b_cnt) this launch works on (all strips of them)
};
inline WfGeom wf_geom(int Z, int Y, int X) {
  WfGeom g;
  g.X = X; g.Y = Y; g.Z = Z;
  g.ns = (Y - 2 + kWfRows - 1) / kWfRows; g.nb = (Z - 2 + kWfPlanes - 1) / kWfPlanes;
  g.NT = (((X - 2) + (kWfRows - 1) + kWfLag * (kWfPlanes - 1)) + kWfDepth - 1) / kWfDepth * kWfDepth;
  g.sub = (long long)kWfPlanes * g.NT * kWfRows;
  g.b_lo = 0; g.b_cnt = g.nb;
  return g;
}
// floats of: cc, r, q, z (skewed) | the slab hand-off pairs [block][t / 4][row][t % 4] | the strip hand-off pairs
// [block][plane][t] | the error word
// (floats, including kWfGuard pairs of padding at either end: the helper wave reads up to kWfLag * (kWfPlanes - 1) resp. 63 steps
// past a block's rows without clamping)
constexpr long long kWfGuard = 4 * kWfRows * (kWfLag * (kWfPlanes - 1) / 4 + 2);        // pairs; >= 64 too
inline long long wf_handoff_k(const WfGeom& g) { return 2ll * g.ns * g.nb * g.NT * kWfRows + 4 * kWfGuard; }
inline long long wf_handoff_s(const WfGeom& g) { return 2ll * g.ns * g.nb * kWfPlanes * g.NT + 4 * kWfGuard; }
constexpr long long kWfErrFloats = 64;       // reserved from the error word on
constexpr long long kWfClearTail = 16;       // ... of which the per-solve memset clears this many
inline long long wf_floats(int Z, int Y, int X) {
  const WfGeom g = wf_geom(Z, Y, X);
  return 4 * g.sub * g.ns * g.nb + wf_handoff_k(g) + wf_handoff_s(g) + kWfErrFloats;
}

// ---- solveLinearSystemPCG ---------------------------------------------------------------------------------------------------
// n = Z * Y * X. The workspace is 8-byte aligned (the abi checks it); the fp64 regions come first, on even offsets.
struct PcgWs {
  WsRegion partials, p_den, p_rr;    // fp64 partial sums, kRedBlocks each: r.r of the set-up / r.z / sum of x | s.w | r.r of the update
  WsRegion state;                    // PcgState
  WsRegion label, size_at;           // int32 per cell
  WsRegion x, r, z, s, w, dg, y;     // fp32 per cell
  WsRegion roots;                    // int32, kMaxComponents
  WsRegion counters;                 // int32, 64 words: [0] changed, [1] count, [2] border fluid (label_components);
                                     // [kPcgMgOpenWord] the multigrid set-up's "open component" word
  // The pipelined wavefront sweeps (3-D; every floats = 0 and geom zeroed without them). These regions need 16 bytes (float4
  // rows, {value, tag} pairs) where the workspace promises 8: the offsets below are those of a workspace that happens to be
  // 16-byte aligned, pcg_wf_pad() gives the 0..3 floats to add to each of them for the array at hand, and kPcgWfSlack floats
  // behind the block pay for it.
  WfGeom geom;
  WsRegion wf_cc, wf_r, wf_q, wf_z;  // the skewed arrays, sub-boxes * geom.sub each (a multiple of 1024)
  WsRegion wf_hk, wf_hs;             // slab / strip hand-off arrays as floats, kWfGuard pairs of padding at either end: the
                                     // pairs of block 0 begin 2 * kWfGuard floats in
  WsRegion wf_err;                   // the error word
  WsRegion wf_clear;                 // what the per-solve memset clears: from cc to behind the error word
  // The multigrid hierarchy (precondType = "mg"; every floats = 0 without it), appended behind everything above. Level 0 keeps its
  // diag in dg and its second iterate in y (idle under mg) and adds invd, cx, cy, cz (n each); the coarser levels are stacked:
  // level l >= 1 begins mg_levels().lv[l].off floats into each of the eight mg_c_* arrays (mg_levels().coarse_cells each).
  WsRegion mg_invd0, mg_cx0, mg_cy0, mg_cz0;
  WsRegion mg_c_diag, mg_c_invd, mg_c_cx, mg_c_cy, mg_c_cz, mg_c_r, mg_c_za, mg_c_zb;
  long long total;                   // floats the table needs
};
constexpr long long kPcgWfSlack = 4;
// the word of the counters' slot that pcg_mg.hip's set-up owns: 1 when a cell of the component at hand has an empty neighbour
constexpr int kPcgCounterWords = 64, kPcgLabelWords = 3, kPcgMgOpenWord = 8;
static_assert(kPcgMgOpenWord >= kPcgLabelWords && kPcgMgOpenWord < kPcgCounterWords, "the open word lies in the counters' slot, behind label_components' words");

inline PcgWs pcg_ws(int Z, int Y, int X, bool wavefronts, bool mg = false, bool mg_is3d = false) {
  const long long n = (long long)Z * Y * X;
  PcgWs t{};
  long long at = 0;
  auto take = [&at](long long floats) { const WsRegion r{at, floats}; at += floats; return r; };
  t.partials = take(2 * kRedBlocks); t.p_den = take(2 * kRedBlocks); t.p_rr = take(2 * kRedBlocks);
  t.state = take(kPcgStateFloats);
  t.label = take(n); t.size_at = take(n);
  t.x = take(n); t.r = take(n); t.z = take(n); t.s = take(n); t.w = take(n); t.dg = take(n); t.y = take(n);
  t.roots = take(kMaxComponents);
  t.counters = take(kPcgCounterWords);
  if (wavefronts) {
    t.geom = wf_geom(Z, Y, X);
    const long long wtot = t.geom.sub * t.geom.ns * t.geom.nb;
    t.wf_cc = take(wtot); t.wf_r = take(wtot); t.wf_q = take(wtot); t.wf_z = take(wtot);
    t.wf_hk = take(wf_handoff_k(t.geom)); t.wf_hs = take(wf_handoff_s(t.geom));
    t.wf_err = {at, 1};
    t.wf_clear = {t.wf_cc.off, at + kWfClearTail - t.wf_cc.off};
    at += kWfErrFloats + kPcgWfSlack;
  }
  if (mg) {
    const long long cc = mg_levels(Z, Y, X, mg_is3d).coarse_cells;
    t.mg_invd0 = take(n); t.mg_cx0 = take(n); t.mg_cy0 = take(n); t.mg_cz0 = take(n);
    t.mg_c_diag = take(cc); t.mg_c_invd = take(cc); t.mg_c_cx = take(cc); t.mg_c_cy = take(cc); t.mg_c_cz = take(cc);
    t.mg_c_r = take(cc); t.mg_c_za = take(cc); t.mg_c_zb = take(cc);
  }
  t.total = at;
  return t;
}
// the run-time round-up of the wavefront block: floats to add to every wf_* offset so that it sits on 16 bytes in `workspace`
inline long long pcg_wf_pad(const float* workspace, const PcgWs& t) {
  return (4 - ((((uintptr_t)workspace >> 2) + (uintptr_t)t.wf_cc.off) & 3)) & 3;
}

// ---- solveLinearSystemPCGBatched (pcg_batched.inc) -----------------------------------------------------------------------------
// What a batched kernel reads of the system its item is on in this round: written on the device (k_pcgb_round, k_mg_level0_b),
// never by the host.
struct PcgItemRec {
  int root, size;      // the component at hand
  int pc;              // its preconditioner: 0 none (also: fewer than 5 cells), 3 mg
  int open;            // mg set-up: a cell of the component has an empty neighbour (0: closed, the cycle runs on r minus its mean)
  int active;          // 0: the item has no system in this round (no such component, or one of size 1)
  int pad[3];
};
constexpr long long kPcgRecFloats = sizeof(PcgItemRec) / sizeof(float);
constexpr int kPcgCcWords = 4;     // per item: [0] changed, [1] count, [2] border fluid, [3] spare
// The batch as a kernel sees it: item b's record, its state slot, and its arrays b * stride floats behind item 0's.
struct PcgBatch {
  PcgItemRec* rec;
  PcgState* S;         // slot 0; the slots are kPcgStateFloats apart
  long long stride;
};
TFL_MG_HD inline PcgState* pcg_state_of(const PcgBatch& bt, int b) {
  return reinterpret_cast<PcgState*>(reinterpret_cast<float*>(bt.S) + (long long)b * kPcgStateFloats);
}

// B copies of the per-item block (pcg_ws without wavefront regions; its state slot and its counters stay idle) at one even stride,
// then tables of B: the solver states (one read per chunk), the records, the labelling words (one read per round) and the
// components (root, size) in scan order, kMaxComponents pairs per item.
struct PcgBatchedWs {
  PcgWs item;          // offsets inside an item's block
  long long stride;    // floats from one item's block to the next: even, so every fp64 region stays on 8 bytes
  WsRegion items;
  WsRegion states;     // B slots of kPcgStateFloats
  WsRegion recs;       // B PcgItemRec
  WsRegion cc;         // B * kPcgCcWords int32
  WsRegion comps;      // B * kMaxComponents * 2 int32
  long long total;
};
inline PcgBatchedWs pcg_batched_ws(int B, int Z, int Y, int X, bool mg, bool is3d) {
  PcgBatchedWs t{};
  t.item = pcg_ws(Z, Y, X, false, mg, is3d);
  t.stride = (t.item.total + 1) & ~1ll;
  long long at = 0;
  auto take = [&at](long long floats) { const WsRegion r{at, floats}; at += floats; return r; };
  t.items = take(B * t.stride);
  t.states = take(B * kPcgStateFloats);
  t.recs = take(B * kPcgRecFloats);
  t.cc = take((long long)B * kPcgCcWords);
  t.comps = take((long long)B * kMaxComponents * 2);
  t.total = at;
  return t;
}

// ---- normalizePressureMean --------------------------------------------------------------------------------------------------
struct NpmWs {
  WsRegion sum_at;           // fp64 per cell (first, for alignment)
  WsRegion label, size_at;   // int32 per cell
  WsRegion counters;         // int32: [0] changed, [1] count, [2] border fluid
  WsRegion roots;            // the sink of k_cc_count's roots list (nobody reads it: means are looked up through the label)
  long long total;
};
inline NpmWs npm_ws(int Z, int Y, int X) {
  const long long n = (long long)Z * Y * X;
  NpmWs t{};
  t.sum_at = {0, 2 * n}; t.label = {2 * n, n}; t.size_at = {3 * n, n};
  t.counters = {4 * n, 3}; t.roots = {4 * n + 3, kMaxComponents};
  t.total = 4 * n + 16 + kMaxComponents;
  return t;
}

}  // namespace tfl
