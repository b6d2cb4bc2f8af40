// tfl_step_ws.hpp -- the workspace of the un-cut native step (tfl_simulate_step, simulate.cpp) as ONE table: every region of
// the caller's scratch array as {offset, floats}, with the time it is live, and the floats the whole table needs. The step
// builds all its views from it and tfl_simulate_workspace_floats takes its size from it; the regions alias each other on
// purpose (the step's phases follow one another), and the rules that keep the live ones apart are the comments below, held by
// a stand-alone host program (tests/step_ws_host.cpp: every offset, the total, and the live groups pairwise disjoint).
// Plain C++ without a HIP header. N = B * Z * Y * X, C = the velocity's channels (2: a 2-D grid, 3: a 3-D one).
#pragma once

namespace tfl {

struct WsRegion { long long off, floats; };

// the projection of a step (simMethod): the ConvNet (its workspace is the model's own, sized by tfl_model_workspace_floats),
// the Jacobi sweeps, PCG, or a name the step refuses once it gets there (no region of its own)
enum class StepProj { convnet, jacobi, pcg, unknown };

// the temporaries of one advectScalar call
struct StepScalWs { WsRegion fwd, bwd, fwdPos, bwdPos; };

struct StepWs {
  // ---- advectVel: live from its pass A until the velocity has left `Uadv` (a force, the projection or the copy into U)
  WsRegion vfwd;       // pass A -> pass B. Where pass A runs in front of the density channels it stays live across them
  WsRegion vbwd;       // (the operator does not touch it)
  WsRegion Uadv;       // written by pass B only, i.e. after the last scalar pass; then the step's velocity until it is delivered
  // ---- advectScalar, one channel at a time, each call complete before the next
  StepScalWs scal;     // in front of advectVel: the whole workspace is free
  // pass A of advectVel has run first (3-D only; floats = 0 in 2-D): `vfwd` is live, so nothing below sits on its planes. The
  // bounds, laid out as a three-channel field, take the `Uadv` planes (nothing writes those before pass B), fwd goes behind
  // them (the |curl| plane of later), and bwd / the min-max grid -- neither is used on this path -- share the `vbwd` planes
  StepScalWs scal_first;
  WsRegion sout;       // the advected channel of every method that cannot run in place, until it is copied back
  // ---- vorticity confinement, after the advection: may read its velocity from `Uadv` or `Utmp`, so disjoint from both (3-D)
  WsRegion curl;       // 3-D: the `vbwd` planes; 2-D: three planes from 0 (below `Uadv`: C = 2)
  WsRegion cnorm;      // 3-D: behind `Uadv`; 2-D: behind curl
  WsRegion Utmp;       // the `vfwd` planes as a scratch velocity: buoyancy's output where the fused confinement (3-D) reads next
  WsRegion centered, force;   // arguments of the public operator's signature; the kernels read neither
  // ---- the solver projections: everything above is dead (the velocity is in U)
  WsRegion div;        // divergence -> the solver
  WsRegion pPrev, pDelta, norm;   // Jacobi: the sweeps' second buffer, the residual's difference and its B norms
  WsRegion pcg;        // PCG: its own workspace (tfl_pcg_workspace_floats), on an 8-byte boundary behind div
  long long total;     // floats the table needs, its two floats of slack included
};

constexpr long long kStepWsSlack = 2;    // behind the last region (the model's workspace gets the same)

// pcg_floats: tfl_pcg_workspace_floats of the grid (read for StepProj::pcg only)
inline StepWs step_ws(int B, int Z, int Y, int X, int C, StepProj proj, long long pcg_floats) {
  const long long N = (long long)B * Z * Y * X;
  const bool is3d = C == 3;
  StepWs w{};
  w.vfwd = {0, C * N}; w.vbwd = {C * N, C * N}; w.Uadv = {2 * C * N, C * N};
  w.scal = {{0, N}, {N, N}, {2 * N, C * N}, {(2 + C) * N, C * N}};
  if (is3d) w.scal_first = {{9 * N, N}, {3 * N, N}, {6 * N, 3 * N}, {3 * N, 3 * N}};
  w.sout = {(2 + 2 * C) * N, N};
  w.curl = {is3d ? 3 * N : 0, 3 * N}; w.cnorm = {is3d ? 9 * N : 3 * N, N};
  w.Utmp = {0, C * N};
  w.centered = {4 * N, C * N}; w.force = {(4 + C) * N, C * N};
  w.div = {0, N};
  long long need = (3 + 2 * C) * N;                      // advectScalar: fwd, bwd, fwdPos, bwdPos, sout
  if (3 * C * N > need) need = 3 * C * N;                // advectVel
  if ((2 * C + 4) * N > need) need = (2 * C + 4) * N;    // vorticity confinement (and scal_first.fwd)
  if (proj == StepProj::jacobi) {
    w.pPrev = {N, N}; w.pDelta = {2 * N, N}; w.norm = {3 * N, B};
    if (3 * N + B > need) need = 3 * N + B;
  } else if (proj == StepProj::pcg) {
    w.pcg = {(N + 1) & ~1ll, pcg_floats};
    if (N + 2 + pcg_floats > need) need = N + 2 + pcg_floats;
  }
  w.total = need + kStepWsSlack;
  return w;
}

// The table of the step on batch items (tfl_simulate_step_items): the step's own, region for region -- the items are the batch,
// and no offset above moves -- with the PCG region sized for the solver that step runs: the batched one's table
// (tfl_pcg_ws.hpp pcg_batched_ws(B, ...).total: B item blocks and the per-item tables) where the preconditioner batches,
// batched_floats >= 0, else the sequential solver's as above. Held by tests/step_items_ws_host.cpp.
inline StepWs step_items_ws(int B, int Z, int Y, int X, int C, StepProj proj, long long pcg_floats, long long batched_floats) {
  return step_ws(B, Z, Y, X, C, proj, batched_floats >= 0 ? batched_floats : pcg_floats);
}

}  // namespace tfl
