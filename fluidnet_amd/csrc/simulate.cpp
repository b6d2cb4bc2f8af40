// simulate.cpp -- tfluids.simulate() (torch/lib/simulate.lua:175-327) as one native call, for hosts that are not
// Python. Orchestration of the operators behind include/tfluids_hip.h: the same sequence, temp layout and launch-saving
// rules as fluidnet_amd/simulate.py, which it is tested against bit for bit (tests/test_hip_simulate.py). This file: the BC
// plans (tfl_bc_plan_*), the brick-list policy of advectScalar, and the un-cut step (tfl_simulate_step: `Step`, phase by
// phase, over the workspace table of tfl_step_ws.hpp). It launches no kernel of its own except the one-time BC scan. The
// z-slab rank-step is simulate_slab.cpp; what the two share is tfl_step.hpp.
#include "../../include/tfluids_hip.h"
#include "tfl_abi.hpp"
#include "tfl_host.hpp"
#include "tfl_ops.hpp"
#include "tfl_step.hpp"
#include "tfl_step_ws.hpp"

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

namespace {

long long numel_of(const tfl_tensor* t) { return (long long)t->B * t->C * t->Z * t->Y * t->X; }

// ---- advectScalar over the list of non-empty bricks: the host policy (advect_scalar3_sparse.hip) -----------------
// What a step does with the in-place maccormackOurs advection of a 3-D density field: today's two launches (full), the same behind
// a brick scan (probe), or the scan and the two passes over the lists it builds (lists). All three give the same bits for any
// state of the field, so the choice is one of time only. It is made from the words the lists kernel of an EARLIER scan left in
// pinned memory, read without any synchronisation: a stale value can cost time, never bits.
// mode: TFL_SCAL3_SPARSE (EXPERIMENTS flavour; the product library always runs the policy, 1). known: a scan has published.
// listed / bricks: |L_B| and the brick count of that scan; fast: it found a velocity word with !(|u dt| <= 0.9), so it listed
// everything. since_scan: steps on the two full launches since the last scan.
enum class SparsePlan { full, probe, lists };
// (profiles/scal3_sparse.md: at 128^3 the lists save 6 us with a fifth of the bricks listed, their passes grow by 0.023 us per listed
// brick and meet the two full launches at about a third; a probe costs 16 us, 0.4 % of a step when paid every 16th)
constexpr double kSparseThreshold = 0.25;  // the lists as long as at most this share of the bricks is listed
constexpr unsigned kSparseProbe = 16;      // above it one step in 16 scans, so that the state can come back
SparsePlan scal3_sparse_plan(int mode, bool known, unsigned listed, unsigned bricks, bool fast, unsigned since_scan) {
  if (mode == 0) return SparsePlan::full;
  if (mode == 2 || !known) return SparsePlan::lists;
  if (!fast && (double)listed <= kSparseThreshold * (double)bricks) return SparsePlan::lists;
  return since_scan + 1 >= kSparseProbe ? SparsePlan::probe : SparsePlan::full;
}

// The request that goes with the advection of density field `rho` (tfl_host.hpp Scal3SparseAsk; run == 0: none) and the field's
// state. Only for the whole un-cut array -- no z-window, stage mask or origin -- advected in place with a finite strength (the
// proof's border cells need hs * 0 = 0), on a shape the brick map holds. While the stream is capturing: no request and no state
// change (a graph replays one decision for ever, and nothing may be allocated), the wall plan's rule.
tfl::Scal3SparseAsk scal3_sparse_ask(tfl_ctx* c, const tfl_sim_params* prm, const tfl::Scope& sc, const Sizes& z, bool in_place,
                                     const tfl_tensor* rho, Scal3SparseState** state) {
  *state = nullptr;
  tfl::Scal3SparseAsk ask;
  const int mode = tfl::sw::num(tfl::Sw::SCAL3_SPARSE, 1);
  if (mode == 0 || !z.is3d || !in_place || sc.windowed() || sc.stages != 0 || sc.origin.total != 0 || !std::isfinite(prm->maccormackStrength)) return ask;
  if (!tfl::scal3_sparse_fits(tfl::whole_dom(z.Z, z.Y, z.X))) return ask;
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(c->stream, &cs) != hipSuccess) { (void)hipGetLastError(); return ask; }
  if (cs != hipStreamCaptureStatusNone) return ask;
  Scal3SparseState* st = tfl::scal3_sparse_state(c, rho->data, z.B, z.Z, z.Y, z.X, tfl::scal3_sparse_bricks(z.Z, z.Y, z.X));
  if (!st) return ask;
  bool known = true, fast = false;
  unsigned listed = 0, bricks = 0;
  const volatile unsigned* m = st->h_mirror;
  for (int b = 0; b < z.B; b++) { listed += m[8 * b]; bricks += m[8 * b + 1]; fast = fast || m[8 * b + 2] != 0; known = known && m[8 * b + 4] != 0; }
  const SparsePlan plan = scal3_sparse_plan(mode, known, listed, bricks, fast, st->since_scan);
  if (plan == SparsePlan::full) { *state = st; return ask; }
  // The scan's number tags the bricks and items it finds set (advect_scalar3_sparse.hip: nothing clears the tags between scans).
  // Before the number would come back to 0 the tags are cleared on the stream, ahead of the scan, and the count starts again: a
  // tag in memory is 0 or the number of a scan since the last clear, all below the current one.
  if (st->scans == 0xffffffffu) {
    const size_t n = (size_t)z.B * ((size_t)tfl::scal3_sparse_bricks(z.Z, z.Y, z.X) + 1);
    if (hipMemsetAsync(st->buf.nz, 0, sizeof(unsigned) * n, c->stream) != hipSuccess) { (void)hipGetLastError(); return ask; }
    st->scans = 0;
  }
  ask = st->buf;
  ask.run = plan == SparsePlan::lists ? 2 : 1;
  ask.took = 0;
  ask.scanned = 0;
  ask.seq = st->scans + 1;
  *state = st;
  return ask;
}
// what the operator did of the request (Scal3SparseAsk::took; a scan inside pass A of advectVel has used the number as well), into
// the field's state and the EXPERIMENTS flavour's counters
void scal3_sparse_done(tfl_ctx* c, Scal3SparseState* st, int took, bool scanned = false) {
  if (st && !took && scanned) st->scans++;
  if (st && took) { st->scans++; st->since_scan = 0; c->scal3_last = st; }
  else if (st) st->since_scan++;
#ifdef TFL_EXPERIMENTS
  c->scal3_counts[0] += took ? 1 : 0; c->scal3_counts[1] += took == 2 ? 1 : 0; c->scal3_counts[2] += took == 2 ? 0 : 1;
#endif
}

// ---- the un-cut step ---------------------------------------------------------------------------------------------------------
tfl::StepProj proj_of(const tfl_sim_params* p) {
  const char* m = p->simMethod && p->simMethod[0] ? p->simMethod : "convnet";
  return !std::strcmp(m, "convnet") ? tfl::StepProj::convnet : !std::strcmp(m, "jacobi") ? tfl::StepProj::jacobi
       : !std::strcmp(m, "pcg") ? tfl::StepProj::pcg : tfl::StepProj::unknown;
}
// the preconditioners tfl_solveLinearSystemPCGBatched takes: the step on items (tfl_simulate_step_items) solves all items at once
bool pcg_batches(const tfl_sim_params* prm) {
  return prm->pcgPrecond && (!std::strcmp(prm->pcgPrecond, "mg") || !std::strcmp(prm->pcgPrecond, "none"));
}
// the workspace table of a step (tfl_step_ws.hpp), and the floats the step needs: the table's, or the model's own workspace
// (the PCG region is sized for params->pcgPrecond; a name the solver does not know gets the common size and is refused there)
// items: the table of the step on items, whose PCG region holds the batched solver's workspace where that solver runs
tfl::StepWs step_ws_of(const tfl_sim_params* prm, const Sizes& z, tfl::StepProj proj, bool items = false) {
  long long pcg = 0;
  if (proj == tfl::StepProj::pcg) {
    pcg = tfl_pcg_workspace_floats_for(z.Z, z.Y, z.X, prm->pcgPrecond && prm->pcgPrecond[0] ? prm->pcgPrecond : "ic0");
    if (pcg < 0) pcg = tfl_pcg_workspace_floats(z.Z, z.Y, z.X);
  }
  if (!items) return tfl::step_ws(z.B, z.Z, z.Y, z.X, (int)z.C, proj, pcg);
  const long long batched = proj == tfl::StepProj::pcg && pcg_batches(prm) ? tfl_pcg_batched_workspace_floats(z.B, z.Z, z.Y, z.X, prm->pcgPrecond) : -1;
  return tfl::step_items_ws(z.B, z.Z, z.Y, z.X, (int)z.C, proj, pcg, batched);
}
long long step_ws_floats(const tfl_sim_state* s, const Sizes& z, tfl::StepProj proj, const tfl::StepWs& W) {
  if (proj != tfl::StepProj::convnet || !s->model) return W.total;
  return std::max<long long>(W.total, tfl_model_workspace_floats(s->model, z.B, z.Z, z.Y, z.X) + tfl::kStepWsSlack);
}

// One un-cut step, phase by phase. The phases share the call's arguments, what validate() resolved of them, the workspace views
// and what one phase hands to the next (which pairs and forces a kernel has applied already, where the velocity lives).
struct Step {
  tfl_ctx* c; const tfl_sim_params* prm; const tfl_sim_state* s; float* ws; int64_t ws_floats;
  Sizes z; int is3D;
  // whatever window / stage mask / origin / advect mode the host left on the context: every windowed operator of the step runs
  // under it (and the ConvNet projection refuses a set window or mask)
  tfl::Scope sc;
  const char* method; bool ours;       // the advection method; it is maccormackOurs (runs in place, no copy back)
  tfl::StepProj proj;                  // simMethod
  bool buoyant, gravity_on, vort;      // the forces of this step
  bool vfused;                         // ... the confinement as the fused kernel (it cannot run in place: reads one array, writes U)
  double dx;
  float bg[3];                         // the buoyancy force (scaled_gravity)
  // the workspace, every view from the table of tfl_step_ws.hpp, which says what aliases what and when each is live. The scalar
  // temporaries twice: [0] in front of advectVel, [1] behind its pass A (vel_first)
  tfl_tensor vfwd, vbwd, Uadv, sfwd[2], sbwd[2], sfwdPos[2], sbwdPos[2], sout, curl, cnorm, Utmp, centered, force;
  tfl_tensor div, pPrev, pDelta, norm;
  float* pws;                          // PCG's workspace
  // Where the first channel's advection goes over the brick lists (or probes them: scal3_sparse_ask), PASS A OF advectVel RUNS
  // FIRST and leaves the brick scan of that channel as a by-product of the words of U it stages anyway (tfl_host.hpp Vel3ScanAsk,
  // DESIGN.md 3.17): advectVel stage A with the request, the density channels, advectVel stage B. The two operators read the same
  // pre-advection U and pass A writes nothing but its own temporary, so the results are what they were in the other order. That
  // temporary is then live while the scalar passes run: their temporaries move (StepWs::scal_first).
  Scal3SparseState* sparse0 = nullptr; // the brick-list state of density channel 0 and the request made from it
  tfl::Scal3SparseAsk ask0;
  bool vel_first = false;              // (only ever in place on the whole un-cut 3-D array, never while capturing)
  unsigned density_done = 0;           // bit i: the kernel that advected density channel i applied the channel's setConstVals pair
  bool Uadv_done = false;              // pass B of advectVel applied the U pair of the first setConstVals
  bool buoy_folded = false;            // ... and added the buoyancy force behind it
  bool U_folded = false;               // the last force applied the U pair of the second setConstVals
  // U:copy(advected) (init.lua:216-218) costs nothing: the velocity stays in the advection's scratch array (`cur`) until an
  // operator that writes every cell of its output delivers it into U -- addBuoyancy (tfl_addBuoyancyFrom), the vorticity
  // confinement (tfl_vorticityConfinementFrom: the fused kernel cannot run in place anyway, the two-launch form reads one
  // array and writes the other since round 5) or the ConvNet projection (UDiv = cur, UOut = U); a copy only where none does.
  const tfl_tensor* cur = nullptr;     // where the velocity of the step currently lives
  // The step on batch items (tfl_simulate_step_items): every item has forces of its own. The advection and the
  // solver projection are the phases above, batch-wide; the forces run as the per-item operators, one launch per force (a force
  // runs where ANY item has it), and PCG as the batched solver where the preconditioner batches. `buoyant`, `gravity_on` and
  // `vort` stay off, so the advection folds no force.
  const tfl_sim_item* items = nullptr; // [z.B], set by validate_items
  bool on_items = false;               // the workspace table is the items step's
  bool pcg_batched = false;            // PCG runs tfl_solveLinearSystemPCGBatched
  tfl_sim_item own_items[TFL_MAX_ITEMS];   // items == NULL: params' forces for every item

  int validate_items(const tfl_sim_item* it, int n_items, const char* who);   // the items step's refusals, then validate()
  int forces_items();                  // the per-item forces, the velocity into U

  int validate(const char* who = "simulate_step");      // every refusal, before anything is enqueued, under the entry's name; the methods, the views, the forces
  int advect();                        // [advectVel pass A,] the density channels, advectVel, the first setConstVals
  int forces();                        // buoyancy (unless folded), gravity, confinement, the velocity into U where nobody delivered it
  int project_net();                   // the second setConstVals, the ConvNet projection, the last setConstVals
  int project_solver();                // setWallBcs, the second setConstVals, divergence, Jacobi / PCG, velocity update, BCs, clamp

  int advect_pass_a();
  int advect_scalars();
  tfl_tensor view(tfl::WsRegion r, int C) const { tfl_tensor t = *s->flags; t.data = ws + r.off; t.C = C; return t; }
};

int Step::validate(const char* who) {
  if (s->n_density < 0 || s->n_density > 8) return TFL_EINVAL;
  z = sizes_of(s);
  is3D = z.is3d ? 1 : 0;
  proj = proj_of(prm);
  const tfl::StepWs W = step_ws_of(prm, z, proj, on_items);
  if (!ws || ((uintptr_t)ws & 15) != 0 || ws_floats < step_ws_floats(s, z, proj, W)) return TFL_EINVAL;
  method = (prm->advectionMethod && prm->advectionMethod[0]) ? prm->advectionMethod : "maccormackOurs";
  ours = std::strcmp(method, "maccormackOurs") == 0;
  sc = tfl::scope_of(c);
  const bool net = s->model && proj == tfl::StepProj::convnet;
  // an earlier step's projection left the fp16 range of the default 3-D conv path (no sync: the word the projection kernel
  // wrote to pinned memory): refuse to step on from a clamped pressure, before anything of this step has been written
  if (net && tfl_model_range_flag(c, s->model) > 0) return range_refusal(c, who);
  // a banked / batch-norm / max-pool model refuses a grid its pyramid and pooling cannot halve evenly: here, before the
  // advection writes anything (tfl_model_begin would refuse the same grid half-way through the step)
  if (net && tfl::model_is_graph(s->model)) {
    const int f = tfl::model_grid_factor(s->model);
    if ((z.is3d && z.Z % f) || z.Y % f || z.X % f) {
      c->err = std::string(who) + ": the grid is not divisible by the model's downsampling factor " + std::to_string(f) + " (banks x pooling)";
      return TFL_EINVAL;
    }
  }
  const int C = (int)z.C;
  vfwd = view(W.vfwd, C); vbwd = view(W.vbwd, C); Uadv = view(W.Uadv, C);
  for (int k = 0; k < 2; k++) {
    const tfl::StepScalWs& t = k ? W.scal_first : W.scal;
    sfwd[k] = view(t.fwd, 1); sbwd[k] = view(t.bwd, 1); sfwdPos[k] = view(t.fwdPos, C); sbwdPos[k] = view(t.bwdPos, C);
  }
  sout = view(W.sout, 1);
  curl = view(W.curl, 3); cnorm = view(W.cnorm, 1); Utmp = view(W.Utmp, C);
  centered = view(W.centered, C); force = view(W.force, C);
  div = view(W.div, 1); pPrev = view(W.pPrev, 1); pDelta = view(W.pDelta, 1);
  norm = view(W.norm, 1); norm.B = z.B; norm.Z = norm.Y = norm.X = 1;
  pws = ws + W.pcg.off;
  buoyant = s->n_density > 0 && prm->buoyancyScale > 0.0;
  gravity_on = prm->gravityScale > 0.0;
  vort = prm->vorticityConfinementAmp > 0.0;
  vfused = vort && tfl::vorticity_confinement_fused_ok(is3D != 0, (int)z.Z, (int)z.Y, (int)z.X);
  dx = tfl::get_dx_double(c, sc, s->flags);
  scaled_gravity(prm, dx, prm->buoyancyScale, bg);
  return TFL_OK;
}

// advectVel stage A in front of the density channels, with the brick scan of channel 0 (Step::vel_first)
int Step::advect_pass_a() {
  if (s->n_density > 0) ask0 = scal3_sparse_ask(c, prm, sc, z, ours, s->density[0], &sparse0);
  vel_first = ask0.run != 0;
  if (!vel_first) return TFL_OK;
  tfl::Scope sa = sc;
  sa.stages = 2;
  tfl::Ask a = step_ask(nullptr);
  a.scan.s = s->density[0]->data; a.scan.nz = ask0.nz; a.scan.seq = ask0.seq;
  TRY(tfl::advectVel(c, prm->dt, s->U, s->flags, &vfwd, &vbwd, is3D, method, 1, prm->maccormackStrength, &Uadv, sa, a));
  ask0.scanned = a.scan.took ? 1 : 0;      // not taken (a gather path): advectScalar runs k_scal3_scan itself
  return TFL_OK;
}

// every density channel with the pre-advection U
int Step::advect_scalars() {
  const int k = vel_first ? 1 : 0;
  for (int i = 0; i < s->n_density; i++) {
    const tfl_tensor* dst = ours ? s->density[i] : &sout;      // maccormackOurs runs in place (no copy back)
    // the first setConstVals follows the advection directly: the kernel that writes the advected field applies
    // the field's pair itself where it can (step_ask; the sparse launch covers the rest)
    tfl::Ask a = step_ask(s->densityBC[i]);
    // ... and, where most of the field is +0.0, only over the bricks around the words that are not (scal3_sparse_ask)
    Scal3SparseState* sparse = sparse0;
    if (i == 0) a.sparse = ask0;
    else a.sparse = scal3_sparse_ask(c, prm, sc, z, ours, s->density[i], &sparse);
    const int rc = tfl::advectScalar(c, prm->dt, s->density[i], s->U, s->flags, &sfwd[k], &sbwd[k], is3D, method, &sfwdPos[k], &sbwdPos[k],
                                     1, 0, prm->maccormackStrength, dst, sc, a);
    if (ours && z.is3d) scal3_sparse_done(c, sparse, a.sparse.took, a.sparse.scanned != 0);
    if (a.fold.bc_took) density_done |= 1u << i;
    if (rc) return rc;
    if (!ours) TRY(tfl_copy(c, s->density[i], &sout));
  }
  return TFL_OK;
}

// ---- advection (simulate.lua:183-200): every density channel with the pre-advection U, then U ----------------
int Step::advect() {
  TRY(advect_pass_a());
  TRY(advect_scalars());
  tfl::Ask adv = step_ask(s->UBC);
  // addBuoyancy follows advectVel and the first setConstVals directly and needs nothing but the advected density, which is
  // final by now: pass B of advectVel may add the force itself behind the folded U pair (tfl_host.hpp BuoyFold; round 5).
  // Asked for only when the density's own pair has been applied already (or there is none) and the U pair travels with the
  // same kernel (or there is none); TFL_BUOY_FOLD=0 keeps the force in its own launch (A/B switch).
  const bool rho_final = buoyant && (!s->densityBC[0] || (density_done & 1u));
  if (rho_final && ours && is3D && tfl::sw::num(tfl::Sw::BUOY_FOLD, 1) != 0 && (!s->UBC || adv.fold.bc.dev)) {
    // strength = -gravity * (dt / dx) in float, exactly as tfl_addBuoyancyFrom forms it (tfluids.cc:1190-1192)
    const float bs = prm->dt / tfl::get_dx(c, sc, s->flags);
    adv.fold.buoy = tfl::BuoyFold{s->density[0]->data, -bg[0] * bs, -bg[1] * bs, -bg[2] * bs};
  }
  tfl::Scope sb = sc;
  if (vel_first) sb.stages = 4;      // pass A has run, in front of the density channels
  const int rc = tfl::advectVel(c, prm->dt, s->U, s->flags, &vfwd, &vbwd, is3D, method, 1, prm->maccormackStrength, &Uadv, sb, adv);
  Uadv_done = adv.fold.bc_took; buoy_folded = adv.fold.buoy_took;
  if (rc) return rc;
  cur = &Uadv;
  return set_const_vals(c, s, cur, !Uadv_done, Unchanged{false, false, false}, density_done);
}

// ---- forces (simulate.lua:204-239) -------------------------------------------------------------------------
int Step::forces() {
  // The setConstVals that follows the forces touches only U (nothing else has been written since the first one):
  // with the ConvNet projection nothing comes between the last force and it, so the LAST force's kernel applies the U pair
  // itself where it can (step_ask; the other projections run setWallBcs first, outputDiv skips the call).
  const bool to_net = proj == tfl::StepProj::convnet;
  const bool fold_forces = !prm->outputDiv && to_net;
  if (buoyant && !buoy_folded) {
    // (with the fused confinement next, or the vorticity operator / the ConvNet projection to move it later, the force may
    // stay in scratch: in place on `cur` when nothing needs the velocity in U yet -- but every cell of U must be written by
    // SOMEONE, and addBuoyancyFrom does that for free, so it delivers into U unless the fused confinement reads next)
    const tfl_tensor* dst = vfused ? &Utmp : s->U;
    const bool last = fold_forces && !gravity_on && !vort;
    tfl::Ask a = step_ask(last ? s->UBC : nullptr);
    const int rc = tfl::addBuoyancyFrom(c, cur, dst, s->flags, s->density[0], bg, prm->dt, is3D, sc, a);
    U_folded = a.fold.bc_took;
    if (rc) return rc;
    cur = dst;
  }
  if (gravity_on) {
    float g[3];
    scaled_gravity(prm, dx, prm->gravityScale, g);
    TRY(tfl::addGravity(c, cur, s->flags, g, prm->dt, is3D, sc));
  }
  if (vort) {
    const float strength = (float)(dx * prm->vorticityConfinementAmp);
    tfl::Ask a = step_ask(fold_forces ? s->UBC : nullptr);
    int rc;
    if (cur != s->U) {
      a.two_launch = !vfused;     // below the fused kernel's size the two launches read `cur` and write U
      rc = tfl::vorticityConfinementFrom(c, cur, s->U, s->flags, strength, &curl, &cnorm, is3D, sc, a);
    } else {
      rc = tfl::vorticityConfinement(c, s->U, s->flags, strength, &centered, &curl, &cnorm, &force, is3D, sc, a);
    }
    U_folded = a.fold.bc_took;
    if (rc) return rc;
    cur = s->U;
  }
  // the ConvNet projection reads its velocity from one array and writes the other; everything else wants it in U now
  if (cur != s->U && (prm->outputDiv || !to_net)) {
    TRY(tfl_copy(c, s->U, cur));
    cur = s->U;
  }
  return TFL_OK;
}

// ---- projection (simulate.lua:247-304) ---------------------------------------------------------------------
int Step::project_net() {
  // only U has been written since the first setConstVals
  TRY(set_const_vals(c, s, cur, !U_folded, Unchanged{true, false, true}));
  if (!s->model) return TFL_EINVAL;
  const LateUbc lu = late_ubc_of(s);
  tfl::Ask a = step_ask(lu.late ? s->UBC : nullptr);
  TRY(tfl::model_forward(c, s->model, s->p, cur, s->flags, s->p, s->U, ws, ws_floats, lu.bc, lu.mask, 1, -1e6f, 1e6f, sc, a));
  // p was rewritten by the model, density has not changed since the second setConstVals
  return set_const_vals(c, s, s->U, lu.late && !a.fold.bc_took, Unchanged{false, false, true});
}

int Step::project_solver() {
  TRY(tfl_setWallBcsForward(c, s->U, s->flags, is3D));
  // only U has been written since the first setConstVals
  TRY(set_const_vals(c, s, cur, !U_folded, Unchanged{true, false, true}));
  const int max_iter = prm->maxIter > 0 ? prm->maxIter : 100;
  TRY(tfl_velocityDivergenceForward(c, s->U, s->flags, &div, is3D));
  if (proj == tfl::StepProj::jacobi) {
    TRY(tfl_solveLinearSystemJacobi(c, s->p, s->flags, &div, &pPrev, &pDelta, &norm, is3D, 0.0f, max_iter, 0, nullptr));
  } else if (proj == tfl::StepProj::pcg) {
    float res = 0.0f;
    // simulate.lua:283 hard-codes 'ic0', and so does this step unless pcgPrecond says otherwise. The lexicographic
    // IC(0) / ILU(0) solves run as pipelined wavefronts (pcg.hip, two launches per application); the preconditioned
    // solve takes ~1.7x the time of the unpreconditioned one at 128^3 on this machine and 0.7x at 256^3 (a third of the
    // iterations, each with two latency-bound sweeps): pcgPrecond = "none" trades that for more iterations within maxIter.
    if (pcg_batched) {    // (the step on items: every item in the launches of one, each with the bits it gets alone)
      TRY(tfl_solveLinearSystemPCGBatched(c, s->p, s->flags, &div, is3D, prm->pcgPrecond, 1e-4f, max_iter, pws, ws_floats - (pws - ws), nullptr, nullptr));
    } else {
      TRY(tfl_solveLinearSystemPCG(c, s->p, s->flags, &div, is3D, prm->pcgPrecond && prm->pcgPrecond[0] ? prm->pcgPrecond : "ic0",
                                   1e-4f, max_iter, 0, pws, ws_floats - (pws - ws), &res));
    }
  } else {
    return TFL_EINVAL;   // mconf.simMethod is not a valid option
  }
  TRY(tfl_velocityUpdateForward(c, s->U, s->flags, s->p, is3D));
  TRY(set_const_vals(c, s, s->U, true, Unchanged{false, false, true}));
  return tfl_applyBCs(c, s->U, nullptr, nullptr, 1, -1e6f, 1e6f);
}

// ---- the step on batch items ---------------------------------------------------------------------------------------------------
// Every refusal of the items entries, by name, before anything is enqueued; then the step's own validate() on the items table.
int Step::validate_items(const tfl_sim_item* it, int n_items, const char* who) {
  auto refuse = [&](int code, const std::string& why) { c->err = std::string(who) + ": " + why; return code; };
  if (!s->flags->data || !s->U->data || !s->p->data) return refuse(TFL_EINVAL, "a state tensor is null");
  z = sizes_of(s);
  if (n_items > TFL_MAX_ITEMS || z.B > TFL_MAX_ITEMS)
    return refuse(TFL_EINVAL, std::to_string(std::max(n_items, z.B)) + " items, at most " + std::to_string(TFL_MAX_ITEMS) + " fit the force kernels' arguments");
  if (n_items != z.B) return refuse(TFL_EINVAL, "n_items = " + std::to_string(n_items) + ", the batch holds " + std::to_string(z.B));
  proj = proj_of(prm);
  if (proj == tfl::StepProj::convnet)
    return refuse(TFL_EUNSUPPORTED, "simMethod convnet is not stepped on items (the training rollouts share one mconf: tfl_simulate_step)");
  if (proj == tfl::StepProj::unknown) return refuse(TFL_EINVAL, "mconf.simMethod is not a valid option");
  const char* pc = prm->pcgPrecond && prm->pcgPrecond[0] ? prm->pcgPrecond : "ic0";
  if (proj == tfl::StepProj::pcg && tfl_pcg_workspace_floats_for(z.Z, z.Y, z.X, pc) < 0)
    return refuse(TFL_EINVAL, std::string("pcgPrecond '") + pc + "' is not a preconditioner");
  const tfl::Scope here = tfl::scope_of(c);
  if (here.windowed() || here.stages != 0) return refuse(TFL_EUNSUPPORTED, "a z-window or stage mask is set on the context");
  if (s->n_density < 0 || s->n_density > 8) return refuse(TFL_EINVAL, "0 to 8 density channels");
  if (!it) {
    for (int b = 0; b < z.B; b++) {
      tfl_sim_item& o = own_items[b];
      for (int a = 0; a < 3; a++) o.gravity[a] = prm->gravity[a];
      o.buoyancyScale = prm->buoyancyScale; o.gravityScale = prm->gravityScale; o.vorticityConfinementAmp = prm->vorticityConfinementAmp;
    }
    it = own_items;
  }
  for (int b = 0; b < z.B; b++) {
    const tfl_sim_item& o = it[b];
    if (!std::isfinite(o.gravity[0]) || !std::isfinite(o.gravity[1]) || !std::isfinite(o.gravity[2]) || !std::isfinite(o.buoyancyScale) ||
        !std::isfinite(o.gravityScale) || !std::isfinite(o.vorticityConfinementAmp))
      return refuse(TFL_EINVAL, "a force field of item " + std::to_string(b) + " is not finite");
  }
  items = it;
  on_items = true;
  pcg_batched = proj == tfl::StepProj::pcg && pcg_batches(prm);
  const long long need = step_ws_of(prm, z, proj, true).total;
  if (!ws || ((uintptr_t)ws & 15) != 0) return refuse(TFL_EINVAL, "the workspace is null or not 16-byte aligned");
  if (ws_floats < need)
    return refuse(TFL_EINVAL, "the workspace holds " + std::to_string((long long)ws_floats) + " floats, the step needs " + std::to_string(need) +
                                  " (tfl_simulate_items_workspace_floats)");
  TRY(validate(who));
  buoyant = gravity_on = vort = vfused = false;      // params' own force fields are not read: the items carry them
  return TFL_OK;
}

// forces (simulate.lua:204-239), each as ONE launch (the confinement: its two) for the whole batch. An item takes a force where the
// single-item step would: buoyancyScale > 0 with a density, gravityScale > 0, vorticityConfinementAmp > 0, with the strengths
// formed by the functions that step uses. The velocity reaches U through addBuoyancyItems where any item is buoyant (it writes
// every cell of U: the items without the force are copied), else by a copy; gravity and the confinement then run in place on U,
// and leave the items without them alone.
int Step::forces_items() {
  const int B = z.B;
  float g[3 * TFL_MAX_ITEMS], amp[TFL_MAX_ITEMS];
  int32_t on[TFL_MAX_ITEMS];
  auto fill = [&](auto scale_of, bool extra) {
    bool any = false;
    for (int b = 0; b < B; b++) {
      tfl_sim_params q = *prm;
      for (int a = 0; a < 3; a++) q.gravity[a] = items[b].gravity[a];
      const double scale = scale_of(items[b]);
      on[b] = extra && scale > 0.0;
      any = any || on[b];
      scaled_gravity(&q, dx, scale, g + 3 * b);
    }
    return any;
  };
  if (fill([](const tfl_sim_item& o) { return o.buoyancyScale; }, s->n_density > 0)) {
    TRY(tfl::addBuoyancyItems(c, cur, s->U, s->flags, s->density[0], g, on, B, prm->dt, is3D, sc));
    cur = s->U;
  }
  if (cur != s->U) {
    TRY(tfl_copy(c, s->U, cur));
    cur = s->U;
  }
  if (fill([](const tfl_sim_item& o) { return o.gravityScale; }, true))
    TRY(tfl::addGravityItems(c, s->U, s->flags, g, on, B, prm->dt, is3D, sc));
  bool any_vort = false;
  for (int b = 0; b < B; b++) {
    on[b] = items[b].vorticityConfinementAmp > 0.0;
    any_vort = any_vort || on[b];
    amp[b] = (float)(dx * items[b].vorticityConfinementAmp);
  }
  if (any_vort) TRY(tfl::vorticityConfinementItems(c, s->U, s->flags, amp, on, B, &curl, &cnorm, is3D, sc));
  return TFL_OK;
}

}  // namespace

extern "C" {

tfl_bc_plan* tfl_bc_plan_create(tfl_ctx* c, const tfl_tensor* bc, const tfl_tensor* invMask) {
  if (!c || !bc || !invMask || !bc->data || !invMask->data) return nullptr;
  if (numel_of(bc) != numel_of(invMask) || numel_of(bc) >= (1ll << 31)) return nullptr;
  tfl_bc_plan* p = new tfl_bc_plan();
  p->bc = *bc; p->inv = *invMask; p->numel = numel_of(bc);
  int* d_cnt = nullptr;
  int h_cnt[2] = {0, 0};
  (void)hipDeviceSynchronize();   // one-time set-up: whoever filled the BC tensors (any stream) is done
  if (hipMalloc((void**)&d_cnt, 2 * sizeof(int)) != hipSuccess) { delete p; return nullptr; }
  (void)hipMemset(d_cnt, 0, 2 * sizeof(int));
  tfl::bc_scan(nullptr, p->numel, bc->data, invMask->data, d_cnt, nullptr);
  (void)hipMemcpy(h_cnt, d_cnt, 2 * sizeof(int), hipMemcpyDeviceToHost);
  p->n_idx = h_cnt[0];
  p->idem = h_cnt[1] == 0;
  p->sparse = p->n_idx * 4 < p->numel;
  if (p->sparse && p->n_idx > 0) {
    if (hipMalloc((void**)&p->d_idx, sizeof(int) * (size_t)p->n_idx) != hipSuccess) { (void)hipFree(d_cnt); delete p; return nullptr; }
    (void)hipMemset(d_cnt, 0, 2 * sizeof(int));
    tfl::bc_scan(nullptr, p->numel, bc->data, invMask->data, d_cnt, p->d_idx);
    (void)hipDeviceSynchronize();
    // the listed elements' bounding box (one-time, on the host): what lets a producing kernel apply the pair itself
    std::vector<int> h((size_t)p->n_idx);
    if (hipMemcpy(h.data(), p->d_idx, sizeof(int) * h.size(), hipMemcpyDeviceToHost) == hipSuccess) {
      int lo[3] = {bc->X, bc->Y, bc->Z}, hi[3] = {-1, -1, -1};
      for (int e : h) {
        const int x = e % bc->X, y = (e / bc->X) % bc->Y, z = (int)((e / ((long long)bc->X * bc->Y)) % bc->Z);
        lo[0] = std::min(lo[0], x); hi[0] = std::max(hi[0], x);
        lo[1] = std::min(lo[1], y); hi[1] = std::max(hi[1], y);
        lo[2] = std::min(lo[2], z); hi[2] = std::max(hi[2], z);
      }
      for (int a = 0; a < 3; a++) { p->box[2 * a] = lo[a]; p->box[2 * a + 1] = hi[a]; }
      p->boxed = true;
      // the device descriptor (vector loads of the pair need 16-byte aligned tensors)
      const tfl::BcFold hf = {bc->data, invMask->data, lo[0], hi[0], lo[1], hi[1], lo[2], hi[2]};
      if ((((uintptr_t)bc->data | (uintptr_t)invMask->data) & 15) == 0 && bc->Y < 65536 && bc->Z < 65536 && hipMalloc((void**)&p->d_fold, sizeof(hf)) == hipSuccess &&
          hipMemcpy(p->d_fold, &hf, sizeof(hf), hipMemcpyHostToDevice) != hipSuccess) { (void)hipFree(p->d_fold); p->d_fold = nullptr; }
    }
  }
  (void)hipFree(d_cnt);
  return p;
}

void tfl_bc_plan_destroy(tfl_ctx* c, tfl_bc_plan* p) {
  (void)c;
  if (!p) return;
  if (p->d_idx) (void)hipFree(p->d_idx);
  if (p->d_fold) (void)hipFree(p->d_fold);
  delete p;
}

int64_t tfl_simulate_workspace_floats(tfl_ctx* c, const tfl_sim_params* prm, const tfl_sim_state* s) {
  if (!c || !prm || !s || !s->flags || !s->U) return 0;
  const Sizes z = sizes_of(s);
  const tfl::StepProj proj = proj_of(prm);
  return step_ws_floats(s, z, proj, step_ws_of(prm, z, proj));
}

int tfl_simulate_step(tfl_ctx* c, const tfl_sim_params* prm, const tfl_sim_state* s, float* ws, int64_t ws_floats) {
  if (!c || !prm || !s || !s->p || !s->U || !s->flags) return TFL_EINVAL;
  Step S{c, prm, s, ws, ws_floats};
  TRY(S.validate());
  TRY(S.advect());
  TRY(S.forces());
  if (prm->outputDiv) return TFL_OK;
  return S.proj == tfl::StepProj::convnet ? S.project_net() : S.project_solver();
}

// The projection phase alone, behind an outputDiv step. That step has delivered the velocity into U (forces(): `cur` is copied
// where no force wrote U) and applied no pair since the first setConstVals (fold_forces is off under outputDiv), so the phase
// starts from cur = U with nothing folded: the second setConstVals runs as its own launch, where the full ConvNet step may
// have let the last force's kernel apply the U pair -- the same values in the same cells -- and the ConvNet projection reads
// and writes U in place, as fluidnet_amd/simulate.py's does.
int tfl_simulate_project(tfl_ctx* c, const tfl_sim_params* prm, const tfl_sim_state* s, float* ws, int64_t ws_floats) {
  if (!c || !prm || !s || !s->p || !s->U || !s->flags) return TFL_EINVAL;
  Step S{c, prm, s, ws, ws_floats};
  TRY(S.validate("simulate_project"));
  if (S.proj == tfl::StepProj::unknown) { c->err = "simulate_project: mconf.simMethod is not a valid option"; return TFL_EINVAL; }
  if (S.proj == tfl::StepProj::convnet && !s->model) { c->err = "simulate_project: simMethod convnet needs a model"; return TFL_EINVAL; }
  S.cur = s->U;
  return S.proj == tfl::StepProj::convnet ? S.project_net() : S.project_solver();
}

int64_t tfl_simulate_items_workspace_floats(tfl_ctx* c, const tfl_sim_params* prm, const tfl_sim_state* s) {
  if (!c || !prm || !s || !s->flags || !s->U) return 0;
  const Sizes z = sizes_of(s);
  return step_ws_of(prm, z, proj_of(prm), true).total;
}

int tfl_simulate_step_items(tfl_ctx* c, const tfl_sim_params* prm, const tfl_sim_item* items, int32_t n_items, const tfl_sim_state* s,
                            float* ws, int64_t ws_floats) {
  if (!c || !prm || !s || !s->p || !s->U || !s->flags) return TFL_EINVAL;
  Step S{c, prm, s, ws, ws_floats};
  TRY(S.validate_items(items, n_items, "simulate_step_items"));
  TRY(S.advect());
  TRY(S.forces_items());
  if (prm->outputDiv) return TFL_OK;
  return S.project_solver();
}

// the projection phase alone, behind an outputDiv items step (which has delivered the velocity into U and applied no pair since
// the first setConstVals): tfl_simulate_project's contract, on items
int tfl_simulate_project_items(tfl_ctx* c, const tfl_sim_params* prm, const tfl_sim_item* items, int32_t n_items, const tfl_sim_state* s,
                               float* ws, int64_t ws_floats) {
  if (!c || !prm || !s || !s->p || !s->U || !s->flags) return TFL_EINVAL;
  Step S{c, prm, s, ws, ws_floats};
  TRY(S.validate_items(items, n_items, "simulate_project_items"));
  S.cur = s->U;
  return S.project_solver();
}

}  // extern "C"
