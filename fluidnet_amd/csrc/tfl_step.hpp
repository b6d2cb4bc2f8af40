// tfl_step.hpp -- what the two native steps share (simulate.cpp: the un-cut step; simulate_slab.cpp: the z-slab rank-step;
// private to them): the BC plan, setConstVals over plans, the requests a step makes of an operator call (tfl_ops.hpp Ask), and
// the small facts both read off the state and the parameters. All inline, for the reason tfl_abi.hpp gives: a step makes
// several of these calls, and as calls into another translation unit they cost 0.1 - 0.5 % of the step.
#pragma once
#include "../../include/tfluids_hip.h"
#include "tfl_abi.hpp"
#include "tfl_host.hpp"
#include "tfl_ops.hpp"

#include <cstdint>
#include <string>

struct tfl_bc_plan {
  tfl_tensor bc, inv;      // the dense pair (pointers kept, not owned)
  int* d_idx = nullptr;    // device list of non-identity elements
  long long n_idx = 0, numel = 0;
  bool sparse = false;     // worth using the list (fewer than a quarter of the elements)
  bool idem = false;       // every listed element has invMask == 0 and |bc| <= 1e6
  bool boxed = false;      // box[] = the listed elements' bounding box in (x, y, z), inclusive (any batch item / channel)
  int box[6] = {0, 0, 0, 0, 0, 0};
  tfl::BcFold* d_fold = nullptr;   // the device descriptor {bc, inv, box} a producing kernel reads (tfl_host.hpp BcFold)
};

struct Todo { const tfl_tensor* x; const tfl_bc_plan* plan; };

// setConstVals (simulate.lua:130-160) over the fields in `todo`: sparse plans in one launch, dense ones one each.
inline int apply_bcs(tfl_ctx* c, const Todo* todo, int n) {
  const tfl_tensor *xs[8], *bs[8], *ms[8];
  const int32_t* is[8];
  int64_t ns[8];
  int k = 0;
  for (int i = 0; i < n; i++) {
    const tfl_bc_plan* p = todo[i].plan;
    if (p->sparse) {
      if (p->n_idx == 0) continue;
      xs[k] = todo[i].x; bs[k] = &p->bc; ms[k] = &p->inv; is[k] = p->d_idx; ns[k] = p->n_idx; k++;
      if (k == 8) { int rc = tfl_applyBCsIndexedMulti(c, k, xs, bs, ms, is, ns); if (rc) return rc; k = 0; }
    } else {
      int rc = tfl_applyBCs(c, todo[i].x, &p->bc, &p->inv, 0, 0.0f, 0.0f);
      if (rc) return rc;
    }
  }
  if (k == 1) return tfl_applyBCsIndexed(c, xs[0], bs[0], ms[0], is[0], ns[0]);
  if (k > 1) return tfl_applyBCsIndexedMulti(c, k, xs, bs, ms, is, ns);
  return TFL_OK;
}

// which fields of the state a setConstVals call may skip: those nothing has written since the previous call AND
// whose pair is idempotent
struct Unchanged { bool p, U, density; };

// density_done: bit i = the pair of density channel i has been applied already (by the kernel that produced the field)
inline int set_const_vals(tfl_ctx* c, const tfl_sim_state* s, const tfl_tensor* U_now, bool with_U, Unchanged un, unsigned density_done = 0) {
  Todo todo[10];
  int n = 0;
  auto add = [&](const tfl_tensor* x, const tfl_bc_plan* p, bool unchanged) {
    if (!p) return;
    if (unchanged && p->sparse && p->idem) return;
    todo[n].x = x; todo[n].plan = p; n++;
  };
  add(s->p, s->pBC, un.p);
  if (with_U) add(U_now, s->UBC, un.U);
  for (int i = 0; i < s->n_density; i++)
    if (!((density_done >> i) & 1u)) add(s->density[i], s->densityBC[i], un.density);
  return apply_bcs(c, todo, n);
}

// Folding a sparse pair into the kernel that produces the field (tfl_host.hpp BcFold): fold_arg is the request as a value
// (the pair kernels of advect_pair3.hip take two of them as arguments). TFL_BC_FOLD=0 keeps every pair in its own launch
// (A/B switch).
inline tfl::BcFoldArg fold_arg(const tfl_bc_plan* p) {
  if (tfl::sw::num(tfl::Sw::BC_FOLD, 1) == 0 || !p || !p->sparse || !p->boxed || !p->d_fold || p->n_idx == 0) return tfl::no_fold();
  return tfl::BcFoldArg{p->d_fold, (unsigned)p->box[2] | ((unsigned)p->box[4] << 16), (unsigned)p->box[3] | ((unsigned)p->box[5] << 16)};
}
// What a step asks of an operator call (tfl_ops.hpp): the sparse pair of plan p (null: none) for the kernel that writes the
// result, and no fp16 range gate -- the step has taken it at its entry, nothing refuses half-way through.
inline tfl::Ask step_ask(const tfl_bc_plan* p) {
  tfl::Ask a;
  a.fold.bc = fold_arg(p);
  a.gated = false;
  return a;
}

struct Sizes { long long N, C; int B, Z, Y, X; bool is3d; };
inline Sizes sizes_of(const tfl_sim_state* s) {
  Sizes z;
  z.B = s->flags->B; z.Z = s->flags->Z; z.Y = s->flags->Y; z.X = s->flags->X;
  z.N = (long long)z.B * z.Z * z.Y * z.X; z.C = s->U->C; z.is3d = s->U->C == 3;
  return z;
}
inline std::string method_of(const tfl_sim_params* p) { return p->simMethod && p->simMethod[0] ? p->simMethod : "convnet"; }

// an earlier ConvNet projection left the fp16 range; `who` = the entry point, `some_rank` = the z-slab step's collective gate
inline int range_refusal(tfl_ctx* c, const char* who, bool some_rank = false) {
  c->err = std::string(who) + ": an earlier step's ConvNet projection clamped activations at the fp16 range" + (some_rank ? " on some rank" : "") +
           " (a blown-up simulation); read the count" + (some_rank ? "s" : "") +
           " with tfl_model_range_errors, or create the model under TFL_CONV_PATH=winograd (strict fp32)";
  return TFL_ERANGE;
}

// gravity * (-dx / 4) * scale (formed in double, rounded once): the force of addBuoyancy (buoyancyScale) / addGravity (gravityScale)
inline void scaled_gravity(const tfl_sim_params* prm, double dx, double scale, float out[3]) {
  const float sc = (float)(-(dx / 4.0) * scale);
  for (int i = 0; i < 3; i++) out[i] = prm->gravity[i] * sc;
}

// sparse idempotent U BCs go after the projection by index list instead of as two dense fields inside it (round 4: the
// projection kernel applies them itself on the rows inside their box -- step_ask -- and the launch goes too)
struct LateUbc { bool late; const tfl_tensor *bc, *mask; };
inline LateUbc late_ubc_of(const tfl_sim_state* s) {
  const bool late = s->UBC && s->UBC->sparse && s->UBC->idem;
  return LateUbc{late, (s->UBC && !late) ? &s->UBC->bc : nullptr, (s->UBC && !late) ? &s->UBC->inv : nullptr};
}
