// abi.cpp -- the fluid operators of the C ABI of libtfluids_hip.so (include/tfluids_hip.h): argument validation that
// mirrors torch/tfluids/init.lua's asserts, then kernel launches on the context's stream. The operators a native step calls
// come first in their tfl:: forms (tfl_ops.hpp), then every public tfl_* operator. The context is context.cpp's, the
// projection ConvNet model_build.cpp's, model_host.cpp's, model_train.cpp's and optim_host.cpp's (tfl_model.hpp).
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "tfl_abi.hpp"
#include "tfl_advect.hpp"
#include "tfl_ops.hpp"

using tfl::fail; using tfl::check_launch; using tfl::same_dims; using tfl::check_flags; using tfl::check_vel; using tfl::check_scalar;

namespace {

// generic/advect_type.cc:18-37
int parse_method(const char* m) {
  if (!m) return -1;
  static const char* names[] = {"euler", "maccormack", "eulerOurs", "rk2Ours", "rk3Ours", "maccormackOurs"};
  for (int i = 0; i < 6; i++) if (strcmp(m, names[i]) == 0) return i;
  return -1;
}

}  // namespace

// The operators a native step calls with a request (tfl_ops.hpp); the public tfl_* forms pass an empty one.
namespace tfl {
int advectScalar(tfl_ctx* c, float dt, const tfl_tensor* s, const tfl_tensor* U, const tfl_tensor* flags, const tfl_tensor* fwd,
                 const tfl_tensor* bwd, int is3D, const char* method, const tfl_tensor* fwdPos, const tfl_tensor* bwdPos,
                 int boundaryWidth, int sampleOutsideFluid, float maccormackStrength, const tfl_tensor* sDst, const Scope& sc, Ask& ask) {
  (void)bwd; (void)boundaryWidth;  // bnd = 1 like the reference (tfluids.cc:436,467)
  TRY(check_flags(c, "advectScalar", flags));
  TRY(check_vel(c, "advectScalar", "U", U, flags, is3D));
  TRY(check_scalar(c, "advectScalar", "s", s, flags));
  TRY(check_scalar(c, "advectScalar", "sDst", sDst, flags));
  const int m = parse_method(method);
  if (m < 0) return fail(c, TFL_EINVAL, "advectScalar: unknown advection method '%s'", method ? method : "(null)");
  // maccormackOurs' pass B reads `s` only at the cell it writes, so sDst may alias s (in-place, saves the
  // wrapper's copy-back); every other method gathers from s while writing sDst.
  if (sDst->data == s->data && m != tfl::kMacCormackOurs)
    return fail(c, TFL_EINVAL, "advectScalar: sDst must not alias s for method '%s'", method);
  float* fwd_p = nullptr;
  float* bounds_p = nullptr;
  float* mm_p = nullptr;
  if (m == tfl::kMacCormack || m == tfl::kMacCormackOurs) {
    TRY(check_scalar(c, "advectScalar", "fwd", fwd, flags));
    fwd_p = fwd->data;
  }
  if (m == tfl::kMacCormackOurs) {
    TRY(check_vel(c, "advectScalar", "fwdPos", fwdPos, flags, is3D));
    TRY(check_vel(c, "advectScalar", "bwdPos", bwdPos, flags, is3D));
    bounds_p = fwdPos->data;   // two planes: clamp bounds of each cell's forward position
    mm_p = bwdPos->data;       // two planes: 3^dim fluid min / max grid of s
  }
  tfl::advect_scalar(c->stream, sc, is3D != 0, m, flags->B, flags->Z, flags->Y, flags->X, dt, maccormackStrength,
                     sampleOutsideFluid != 0, c->d_trace_err, s->data, U->data, flags->data, fwd_p, bounds_p, mm_p,
                     sDst->data, ask.fold, &ask.sparse);
  return check_launch(c, "advectScalar");
}

int advectVel(tfl_ctx* c, float dt, const tfl_tensor* U, const tfl_tensor* flags, const tfl_tensor* fwd, const tfl_tensor* bwd,
              int is3D, const char* method, int boundaryWidth, float maccormackStrength, const tfl_tensor* UDst, const Scope& sc, Ask& ask) {
  (void)bwd; (void)boundaryWidth;
  TRY(check_flags(c, "advectVel", flags));
  TRY(check_vel(c, "advectVel", "U", U, flags, is3D));
  TRY(check_vel(c, "advectVel", "UDst", UDst, flags, is3D));
  int m = parse_method(method);
  if (m < 0) return fail(c, TFL_EINVAL, "advectVel: unknown advection method '%s'", method ? method : "(null)");
  if (UDst->data == U->data) return fail(c, TFL_EINVAL, "advectVel: UDst must not alias U");
  float* fwd_p = nullptr;
  if (m != tfl::kEuler && m != tfl::kEulerOurs) {
    TRY(check_vel(c, "advectVel", "fwd", fwd, flags, is3D));
    fwd_p = fwd->data;
  }
  tfl::advect_vel(c->stream, sc, is3D != 0, m, flags->B, flags->Z, flags->Y, flags->X, dt, maccormackStrength,
                  c->d_trace_err, U->data, flags->data, fwd_p, UDst->data, ask.fold, &ask.scan);
  return check_launch(c, "advectVel");
}

// (the z-slab step: both advections' passes A / passes B as one launch each, tfl_ops.hpp)
int advect_pair(tfl_ctx* c, float dt, float strength, const tfl_tensor* s, const tfl_tensor* U, const tfl_tensor* flags,
                const tfl_tensor* sfwd, const tfl_tensor* sbounds, const tfl_tensor* sDst, const tfl_tensor* vfwd, const tfl_tensor* UDst,
                const BcFoldArg& fold_s, const BcFoldArg& fold_v, const Scope& sc) {
  TRY(check_flags(c, "advectPair", flags));
  TRY(check_vel(c, "advectPair", "U", U, flags, 1));
  TRY(check_vel(c, "advectPair", "UDst", UDst, flags, 1));
  TRY(check_vel(c, "advectPair", "vfwd", vfwd, flags, 1));
  TRY(check_scalar(c, "advectPair", "s", s, flags));
  TRY(check_scalar(c, "advectPair", "sDst", sDst, flags));
  TRY(check_scalar(c, "advectPair", "sfwd", sfwd, flags));
  if (!sbounds || !sbounds->data || sbounds->C < 2 || !same_dims(sbounds, flags)) return fail(c, TFL_EINVAL, "advectPair: bounds needs two planes of the flags size");
  if (UDst->data == U->data) return fail(c, TFL_EINVAL, "advectPair: UDst must not alias U");
  AdvArgs a; a.d = make_dom(sc, flags->Z, flags->Y, flags->X); a.dt = dt; a.strength = strength; a.outside = 0; a.err = c->d_trace_err; a.fast = sc.advect_fast;
  a.ord = BlockOrder{};
  if (!advect_pair3(c->stream, a, flags->B, s->data, U->data, flags->data, sfwd->data, sbounds->data, sDst->data, vfwd->data, UDst->data,
                    sc.passes(), fold_s, fold_v))
    return TFL_EUNSUPPORTED;
  return check_launch(c, "advectPair");
}

int vorticityConfinement(tfl_ctx* c, const tfl_tensor* U, const tfl_tensor* flags, float strength, const tfl_tensor* centered,
                         const tfl_tensor* curl, const tfl_tensor* curlNorm, const tfl_tensor* force, int is3D, const Scope& sc, Ask& ask) {
  (void)centered; (void)force;  // fused away (vorticity.hip)
  TRY(check_flags(c, "vorticityConfinement", flags));
  TRY(check_vel(c, "vorticityConfinement", "U", U, flags, is3D));
  if (!curl || !curl->data || curl->C != 3 || !same_dims(curl, flags))
    return fail(c, TFL_EINVAL, "vorticityConfinement: curl must be a 3-channel grid of the flags size");
  TRY(check_scalar(c, "vorticityConfinement", "curlNorm", curlNorm, flags));
  const int stg = sc.passes();   // tfl_set_stages: 2 = pass A (curl), 4 = pass B (confinement force)
  tfl::vorticity_confinement(c->stream, sc, is3D != 0, flags->B, flags->Z, flags->Y, flags->X, U->data, flags->data,
                             strength, curl->data, curlNorm->data, ((stg & 2) ? 1 : 0) | ((stg & 4) ? 2 : 0), nullptr, ask.fold);
  return check_launch(c, "vorticityConfinement");
}

int vorticityConfinementFrom(tfl_ctx* c, const tfl_tensor* USrc, const tfl_tensor* U, const tfl_tensor* flags, float strength,
                             const tfl_tensor* curl, const tfl_tensor* curlNorm, int is3D, const Scope& sc, Ask& ask) {
  TRY(check_flags(c, "vorticityConfinementFrom", flags));
  TRY(check_vel(c, "vorticityConfinementFrom", "U", U, flags, is3D));
  TRY(check_vel(c, "vorticityConfinementFrom", "USrc", USrc, flags, is3D));
  if (USrc->data == U->data) return fail(c, TFL_EINVAL, "vorticityConfinementFrom: U must not alias USrc (use vorticityConfinement)");
  if (!curl || !curl->data || curl->C != 3 || !same_dims(curl, flags))
    return fail(c, TFL_EINVAL, "vorticityConfinementFrom: curl must be a 3-channel grid of the flags size");
  TRY(check_scalar(c, "vorticityConfinementFrom", "curlNorm", curlNorm, flags));
  if (is3D && !ask.two_launch && tfl::vorticity_confinement_fused_ok(true, flags->Z, flags->Y, flags->X) &&
      tfl::vorticity_confinement_fused(c->stream, sc, flags->B, flags->Z, flags->Y, flags->X, USrc->data, U->data, flags->data, strength, ask.fold))
    return check_launch(c, "vorticityConfinementFrom");
  // 2-D, a grid below the fused kernel's size, or TFL_VORT_FUSED=0: the two launches read USrc and write U (round 5) ...
  // Under a z-window pass A must cover what pass B taps: |curl| two planes below / one above, curl one below -- the
  // window widened by two planes either way, its two runs merged where they meet; pass B then runs on the window itself.
  const tfl::ZWin w0 = sc.win;
  const bool windowed = sc.windowed();
  if (windowed) {
    tfl::Scope sa = sc;
    tfl::ZWin& wa = sa.win;
    wa = {std::max(w0.a0 - 2, 0), std::min(w0.a1 + 2, (int)flags->Z), 0, 0};
    if (w0.b1 > w0.b0) { wa.b0 = std::max(w0.b0 - 2, 0); wa.b1 = std::min(w0.b1 + 2, (int)flags->Z); }
    if (w0.a1 <= w0.a0) { wa.a0 = wa.b0; wa.a1 = wa.b1; wa.b0 = wa.b1 = 0; }
    else if (wa.b1 > wa.b0 && wa.b0 <= wa.a1) { wa.a1 = wa.b1; wa.b0 = wa.b1 = 0; }
    const bool a_ok = tfl::vorticity_confinement(c->stream, sa, is3D != 0, flags->B, flags->Z, flags->Y, flags->X, U->data, flags->data, strength,
                                                 curl->data, curlNorm->data, 1, USrc->data, ask.fold);
    if (a_ok && tfl::vorticity_confinement(c->stream, sc, is3D != 0, flags->B, flags->Z, flags->Y, flags->X, U->data, flags->data, strength,
                                           curl->data, curlNorm->data, 2, USrc->data, ask.fold))
      return check_launch(c, "vorticityConfinementFrom");
    if (a_ok) return fail(c, TFL_EUNSUPPORTED, "vorticityConfinementFrom: pass B could not read USrc on this grid under a z-window");
  } else if (tfl::vorticity_confinement(c->stream, sc, is3D != 0, flags->B, flags->Z, flags->Y, flags->X, U->data, flags->data, strength,
                                        curl->data, curlNorm->data, 3, USrc->data, ask.fold))
    return check_launch(c, "vorticityConfinementFrom");
  if (windowed)      // (the one-cell kernels below run in place on a copy: the same two windows are needed there -- not built)
    return fail(c, TFL_EUNSUPPORTED, "vorticityConfinementFrom: this grid takes the one-cell kernels, which do not run from USrc under a z-window; "
                                     "copy USrc into U and call tfl_vorticityConfinement per pass (tfl_set_stages) with the passes' own windows");
  // ... or, where only the one-cell kernels apply (X % 4 != 0, misaligned views), the planes of the window are copied and the
  // two-launch form runs in place
  {
    const tfl::Dom d = tfl::make_dom(sc, flags->Z, flags->Y, flags->X);
    const size_t plane = sizeof(float) * (size_t)flags->Y * flags->X;
    const int C = is3D ? 3 : 2;
    for (int b = 0; b < flags->B; b++)
      for (int ch = 0; ch < C; ch++) {
        const size_t row = ((size_t)b * C + ch) * flags->Z;
        if (d.n0 > 0) HIP_TRY(c, hipMemcpyAsync(U->data + (row + d.w0) * (plane / 4), USrc->data + (row + d.w0) * (plane / 4), plane * d.n0, hipMemcpyDeviceToDevice, c->stream));
        if (d.nw > d.n0) HIP_TRY(c, hipMemcpyAsync(U->data + (row + d.w1) * (plane / 4), USrc->data + (row + d.w1) * (plane / 4), plane * (d.nw - d.n0), hipMemcpyDeviceToDevice, c->stream));
      }
  }
  tfl::vorticity_confinement(c->stream, sc, is3D != 0, flags->B, flags->Z, flags->Y, flags->X, U->data, flags->data, strength,
                             curl->data, curlNorm->data, 3, nullptr, ask.fold);
  return check_launch(c, "vorticityConfinementFrom");
}

int addBuoyancyFrom(tfl_ctx* c, const tfl_tensor* USrc, const tfl_tensor* U, const tfl_tensor* flags, const tfl_tensor* density,
                    const float gravity[3], float dt, int is3D, const Scope& sc, Ask& ask) {
  TRY(check_flags(c, "addBuoyancy", flags));
  TRY(check_vel(c, "addBuoyancy", "U", U, flags, is3D));
  TRY(check_vel(c, "addBuoyancy", "USrc", USrc, flags, is3D));
  TRY(check_scalar(c, "addBuoyancy", "density", density, flags));
  if (!gravity) return fail(c, TFL_EINVAL, "addBuoyancy: gravity is null");
  const float k = dt / get_dx(c, sc, flags);  // strength = -gravity * (dt / dx), tfluids.cc:1190-1192
  tfl::add_buoyancy(c->stream, sc, is3D != 0, flags->B, flags->Z, flags->Y, flags->X, USrc->data, U->data, flags->data,
                    density->data, -gravity[0] * k, -gravity[1] * k, -gravity[2] * k, ask.fold);
  return check_launch(c, "addBuoyancy");
}

int addGravity(tfl_ctx* c, const tfl_tensor* U, const tfl_tensor* flags, const float gravity[3], float dt, int is3D, const Scope& sc) {
  TRY(check_flags(c, "addGravity", flags));
  TRY(check_vel(c, "addGravity", "U", U, flags, is3D));
  if (!gravity) return fail(c, TFL_EINVAL, "addGravity: gravity is null");
  const float k = dt / get_dx(c, sc, flags);  // force = gravity * (dt / dx), tfluids.cc:1265-1267
  tfl::add_gravity(c->stream, sc, is3D != 0, flags->B, flags->Z, flags->Y, flags->X, U->data, flags->data,
                   gravity[0] * k, gravity[1] * k, gravity[2] * k);
  return check_launch(c, "addGravity");
}

// ---- the per-item force operators --------------------------------------------------------------------------
// what every one of them refuses, by name, before anything is enqueued
static int check_items(tfl_ctx* c, const char* op, const tfl_tensor* flags, const void* table, int n_items, const Scope& sc) {
  if (!table) return fail(c, TFL_EINVAL, "%s: the per-item table is null", op);
  if (n_items > TFL_MAX_ITEMS) return fail(c, TFL_EINVAL, "%s: %d items, at most %d fit the kernel arguments", op, n_items, TFL_MAX_ITEMS);
  if (n_items != flags->B) return fail(c, TFL_EINVAL, "%s: n_items = %d, the batch holds %d", op, n_items, flags->B);
  if (sc.windowed() || sc.stages != 0) return fail(c, TFL_EUNSUPPORTED, "%s: a z-window or stage mask is set on the context", op);
  return TFL_OK;
}
static bool item_on(const int32_t* on, int b) { return !on || on[b] != 0; }

int addBuoyancyItems(tfl_ctx* c, const tfl_tensor* USrc, const tfl_tensor* U, const tfl_tensor* flags, const tfl_tensor* density,
                     const float* gravity, const int32_t* on, int n_items, float dt, int is3D, const Scope& sc) {
  const char* op = "addBuoyancyItems";
  TRY(check_flags(c, op, flags));
  TRY(check_vel(c, op, "U", U, flags, is3D));
  if (USrc) TRY(check_vel(c, op, "USrc", USrc, flags, is3D));
  TRY(check_scalar(c, op, "density", density, flags));
  TRY(check_items(c, op, flags, gravity, n_items, sc));
  const float k = dt / get_dx(c, sc, flags);  // strength = -gravity * (dt / dx), as addBuoyancyFrom forms it
  tfl::ItemVec t{};
  for (int b = 0; b < n_items; b++) {
    if (!item_on(on, b)) continue;
    t.on |= 1u << b;
    t.x[b] = -gravity[3 * b] * k; t.y[b] = -gravity[3 * b + 1] * k; t.z[b] = -gravity[3 * b + 2] * k;
  }
  tfl::add_buoyancy_items(c->stream, sc, is3D != 0, flags->B, flags->Z, flags->Y, flags->X, USrc ? USrc->data : U->data, U->data, flags->data,
                          density->data, t);
  return check_launch(c, op);
}

int addGravityItems(tfl_ctx* c, const tfl_tensor* U, const tfl_tensor* flags, const float* gravity, const int32_t* on, int n_items,
                    float dt, int is3D, const Scope& sc) {
  const char* op = "addGravityItems";
  TRY(check_flags(c, op, flags));
  TRY(check_vel(c, op, "U", U, flags, is3D));
  TRY(check_items(c, op, flags, gravity, n_items, sc));
  const float k = dt / get_dx(c, sc, flags);  // force = gravity * (dt / dx), as addGravity forms it
  tfl::ItemVec t{};
  for (int b = 0; b < n_items; b++) {
    if (!item_on(on, b)) continue;
    t.on |= 1u << b;
    t.x[b] = gravity[3 * b] * k; t.y[b] = gravity[3 * b + 1] * k; t.z[b] = gravity[3 * b + 2] * k;
  }
  tfl::add_gravity_items(c->stream, sc, is3D != 0, flags->B, flags->Z, flags->Y, flags->X, U->data, flags->data, t);
  return check_launch(c, op);
}

int vorticityConfinementItems(tfl_ctx* c, const tfl_tensor* U, const tfl_tensor* flags, const float* strength, const int32_t* on,
                              int n_items, const tfl_tensor* curl, const tfl_tensor* curlNorm, int is3D, const Scope& sc) {
  const char* op = "vorticityConfinementItems";
  TRY(check_flags(c, op, flags));
  TRY(check_vel(c, op, "U", U, flags, is3D));
  if (!curl || !curl->data || curl->C != 3 || !same_dims(curl, flags))
    return fail(c, TFL_EINVAL, "%s: curl must be a 3-channel grid of the flags size", op);
  TRY(check_scalar(c, op, "curlNorm", curlNorm, flags));
  TRY(check_items(c, op, flags, strength, n_items, sc));
  tfl::ItemAmp t{};
  for (int b = 0; b < n_items; b++) {
    if (!item_on(on, b)) continue;
    t.on |= 1u << b;
    t.s[b] = strength[b];
  }
  tfl::vorticity_confinement_items(c->stream, sc, is3D != 0, flags->B, flags->Z, flags->Y, flags->X, U->data, flags->data, t,
                                   curl->data, curlNorm->data);
  return check_launch(c, op);
}
}  // namespace tfl

extern "C" {

int tfl_addBuoyancyItems(tfl_ctx* c, const tfl_tensor* USrc, const tfl_tensor* U, const tfl_tensor* flags, const tfl_tensor* density,
                         const float* gravity, const int32_t* on, int32_t n_items, float dt, int is3D) {
  if (!c) return TFL_EINVAL;
  return tfl::addBuoyancyItems(c, USrc, U, flags, density, gravity, on, n_items, dt, is3D, tfl::scope_of(c));
}
int tfl_addGravityItems(tfl_ctx* c, const tfl_tensor* U, const tfl_tensor* flags, const float* gravity, const int32_t* on,
                        int32_t n_items, float dt, int is3D) {
  if (!c) return TFL_EINVAL;
  return tfl::addGravityItems(c, U, flags, gravity, on, n_items, dt, is3D, tfl::scope_of(c));
}
int tfl_vorticityConfinementItems(tfl_ctx* c, const tfl_tensor* U, const tfl_tensor* flags, const float* strength,
                                  const int32_t* on, int32_t n_items, const tfl_tensor* curl, const tfl_tensor* curlNorm, int is3D) {
  if (!c) return TFL_EINVAL;
  return tfl::vorticityConfinementItems(c, U, flags, strength, on, n_items, curl, curlNorm, is3D, tfl::scope_of(c));
}

int tfl_advectScalar(tfl_ctx* c, float dt, const tfl_tensor* s, const tfl_tensor* U, const tfl_tensor* flags,
                     const tfl_tensor* fwd, const tfl_tensor* bwd, int is3D, const char* method,
                     const tfl_tensor* fwdPos, const tfl_tensor* bwdPos, int boundaryWidth, int sampleOutsideFluid,
                     float maccormackStrength, const tfl_tensor* sDst) {
  tfl::Ask none;
  return tfl::advectScalar(c, dt, s, U, flags, fwd, bwd, is3D, method, fwdPos, bwdPos, boundaryWidth, sampleOutsideFluid,
                           maccormackStrength, sDst, tfl::scope_of(c), none);
}

int tfl_advectVel(tfl_ctx* c, float dt, const tfl_tensor* U, const tfl_tensor* flags, const tfl_tensor* fwd,
                  const tfl_tensor* bwd, int is3D, const char* method, int boundaryWidth, float maccormackStrength,
                  const tfl_tensor* UDst) {
  tfl::Ask none;
  return tfl::advectVel(c, dt, U, flags, fwd, bwd, is3D, method, boundaryWidth, maccormackStrength, UDst, tfl::scope_of(c), none);
}

int tfl_setWallBcsForward(tfl_ctx* c, const tfl_tensor* U, const tfl_tensor* flags, int is3D) {
  TRY(check_flags(c, "setWallBcsForward", flags));
  TRY(check_vel(c, "setWallBcsForward", "U", U, flags, is3D));
  tfl::set_wall_bcs(c->stream, is3D != 0, flags->B, flags->Z, flags->Y, flags->X, U->data, flags->data);
  return check_launch(c, "setWallBcsForward");
}

int tfl_velocityDivergenceForward(tfl_ctx* c, const tfl_tensor* U, const tfl_tensor* flags, const tfl_tensor* UDiv,
                                  int is3D) {
  TRY(check_flags(c, "velocityDivergenceForward", flags));
  TRY(check_vel(c, "velocityDivergenceForward", "U", U, flags, is3D));
  TRY(check_scalar(c, "velocityDivergenceForward", "UDiv", UDiv, flags));
  tfl::velocity_divergence(c->stream, is3D != 0, flags->B, flags->Z, flags->Y, flags->X, U->data, flags->data,
                           UDiv->data);
  return check_launch(c, "velocityDivergenceForward");
}

int64_t tfl_divergence_norm_workspace_floats(int32_t B, int32_t Z, int32_t Y, int32_t X) {
  (void)Y; (void)X;
  if (B < 1 || Z < 1) return 0;
  return 2ll * B * Z;        // one double per (batch item, z-plane)
}

int tfl_velocityDivergenceNorm(tfl_ctx* c, const tfl_tensor* U, const tfl_tensor* flags, int is3D, double* norm, float* workspace,
                               int64_t workspace_floats) {
  TRY(check_flags(c, "velocityDivergenceNorm", flags));
  TRY(check_vel(c, "velocityDivergenceNorm", "U", U, flags, is3D));
  if (!norm || ((uintptr_t)norm & 7) != 0) return fail(c, TFL_EINVAL, "velocityDivergenceNorm: norm is null or not 8-byte aligned");
  if (!workspace || ((uintptr_t)workspace & 7) != 0 ||
      workspace_floats < tfl_divergence_norm_workspace_floats(flags->B, flags->Z, flags->Y, flags->X))
    return fail(c, TFL_EINVAL, "velocityDivergenceNorm: workspace too small or not 8-byte aligned (tfl_divergence_norm_workspace_floats)");
  double* sums = reinterpret_cast<double*>(workspace);
  // the whole array, like tfl_velocityDivergenceForward: the empty scope, whatever tfl_set_z_window / _z_origin left on the context
  tfl::divergence_norm_planes(c->stream, tfl::Scope{}, is3D != 0, flags->B, flags->Z, flags->Y, flags->X, U->data, flags->data, sums,
                              flags->Z, 0);
  tfl::divergence_norm_finish(c->stream, flags->B, flags->Z, sums, norm);
  return check_launch(c, "velocityDivergenceNorm");
}

int tfl_criterion_weight(tfl_ctx* c, const tfl_tensor* flags, double borderWidth, double borderWeight, int is3D,
                         const tfl_tensor* weight) {
  TRY(check_flags(c, "criterion_weight", flags));
  TRY(check_scalar(c, "criterion_weight", "weight", weight, flags));
  if (!(borderWidth > 1.0) || floor(borderWidth) != borderWidth)
    return fail(c, TFL_EINVAL, "criterion_weight: borderWidth must a positive integer > 1");      // fluid_criterion.lua:46
  if (borderWidth > 1024.0) return fail(c, TFL_EINVAL, "criterion_weight: borderWidth above 1024 is not supported");
  if (!(borderWeight > 1.0)) return fail(c, TFL_EINVAL, "criterion_weight: borderWeight must be > 1");      // :63
  if (!is3D && flags->Z != 1) return fail(c, TFL_EINVAL, "criterion_weight: 2D domain but zdepth > 1");
  if (weight->data == flags->data) return fail(c, TFL_EINVAL, "criterion_weight: weight must not alias flags");
  tfl::criterion_weight(c->stream, flags->B, flags->Z, flags->Y, flags->X, (int)borderWidth, (float)borderWidth,
                        (float)(-1.0 / (borderWidth - 1.0)), (float)(borderWeight - 1.0), flags->data, weight->data);
  return check_launch(c, "criterion_weight");
}

int64_t tfl_fluid_criterion_workspace_floats(int32_t B, int32_t Z, int32_t Y, int32_t X) {
  (void)Y; (void)X;
  if (B < 1 || Z < 1) return 0;
  return 6ll * B * Z;        // three doubles per (batch item, z-plane)
}

int tfl_fluidCriterion(tfl_ctx* c, const tfl_tensor* pPred, const tfl_tensor* UPred, const tfl_tensor* pTarget,
                       const tfl_tensor* UTarget, const tfl_tensor* flags, const tfl_tensor* weight, double pLambda,
                       double uLambda, double divLambda, int sizeAverage, int is3D, double* loss, const tfl_tensor* gradP,
                       const tfl_tensor* gradU, float* workspace, int64_t workspace_floats) {
  const char* op = "fluidCriterion";
  TRY(check_flags(c, op, flags));
  TRY(check_scalar(c, op, "pPred", pPred, flags));
  TRY(check_scalar(c, op, "pTarget", pTarget, flags));
  TRY(check_vel(c, op, "UPred", UPred, flags, is3D));
  TRY(check_vel(c, op, "UTarget", UTarget, flags, is3D));
  if (weight) TRY(check_scalar(c, op, "weight", weight, flags));
  if ((gradP != nullptr) != (gradU != nullptr)) return fail(c, TFL_EINVAL, "%s: gradP and gradU are given both or neither", op);
  const size_t cells = (size_t)flags->B * flags->Z * flags->Y * flags->X;
  if (gradP) {
    TRY(check_scalar(c, op, "gradP", gradP, flags));
    TRY(check_vel(c, op, "gradU", gradU, flags, is3D));
    // the kernel reads neighbours of what it writes: a gradient must not overlap any input, nor the other gradient
    auto overlap = [cells](const tfl_tensor* a, const tfl_tensor* b) {
      if (!a || !b) return false;
      const float *a0 = a->data, *a1 = a0 + cells * a->C, *b0 = b->data, *b1 = b0 + cells * b->C;
      return a0 < b1 && b0 < a1;
    };
    const tfl_tensor* ins[6] = {pPred, UPred, pTarget, UTarget, flags, weight};
    static const char* names[6] = {"pPred", "UPred", "pTarget", "UTarget", "flags", "weight"};
    for (int i = 0; i < 6; i++) {
      if (overlap(gradP, ins[i])) return fail(c, TFL_EINVAL, "%s: gradP must not alias %s", op, names[i]);
      if (overlap(gradU, ins[i])) return fail(c, TFL_EINVAL, "%s: gradU must not alias %s", op, names[i]);
    }
    if (overlap(gradP, gradU)) return fail(c, TFL_EINVAL, "%s: gradP must not alias gradU", op);
  }
  if (!loss || ((uintptr_t)loss & 7) != 0) return fail(c, TFL_EINVAL, "%s: loss is null or not 8-byte aligned", op);
  if (!workspace || ((uintptr_t)workspace & 7) != 0 ||
      workspace_floats < tfl_fluid_criterion_workspace_floats(flags->B, flags->Z, flags->Y, flags->X))
    return fail(c, TFL_EINVAL, "%s: workspace too small or not 8-byte aligned (tfl_fluid_criterion_workspace_floats)", op);
  const double n_p = (double)cells, n_u = (double)cells * UPred->C;
  tfl::CriterionArgs a{};
  a.p = pPred->data; a.pt = pTarget->data; a.U = UPred->data; a.Ut = UTarget->data; a.flags = flags->data;
  a.w = weight ? weight->data : nullptr;
  a.gP = gradP ? gradP->data : nullptr; a.gU = gradU ? gradU->data : nullptr;
  a.sums = reinterpret_cast<double*>(workspace);
  a.BZ = (long long)flags->B * flags->Z;
  a.normP = sizeAverage ? (float)(2.0 / n_p) : 2.0f;
  a.normU = sizeAverage ? (float)(2.0 / n_u) : 2.0f;
  a.lamP = (float)pLambda; a.lamU = (float)uLambda; a.lamD = (float)divLambda;
  a.pOn = pLambda > 0.0; a.uOn = uLambda > 0.0; a.dOn = divLambda > 0.0;
  tfl::CriterionFinish f{};
  f.lambda[0] = pLambda; f.lambda[1] = uLambda; f.lambda[2] = divLambda;
  f.n[0] = sizeAverage ? n_p : 1.0; f.n[1] = sizeAverage ? n_u : 1.0; f.n[2] = sizeAverage ? n_p : 1.0;
  f.on[0] = a.pOn; f.on[1] = a.uOn; f.on[2] = a.dOn;
  tfl::criterion_planes(c->stream, is3D != 0, flags->B, flags->Z, flags->Y, flags->X, a);
  tfl::criterion_finish(c->stream, a.BZ, a.sums, f, loss);
  return check_launch(c, op);
}

int tfl_closure_fold(tfl_ctx* c, const double* loss4, double* sums5, int32_t* guard, int longTerm, double errLimit) {
  const char* op = "closure_fold";
  if (!c) return TFL_EINVAL;
  if (!loss4 || !sums5 || (((uintptr_t)loss4 | (uintptr_t)sums5) & 7) != 0)
    return fail(c, TFL_EINVAL, "%s: loss4 or sums5 is null or not 8-byte aligned", op);
  if (!guard || ((uintptr_t)guard & 3) != 0) return fail(c, TFL_EINVAL, "%s: guard is null or not 4-byte aligned", op);
  if (errLimit != errLimit) return fail(c, TFL_EINVAL, "%s: errLimit is NaN", op);
  tfl::closure_fold(c->stream, loss4, sums5, guard, longTerm != 0, errLimit);
  return check_launch(c, op);
}

int tfl_velocityUpdateForward(tfl_ctx* c, const tfl_tensor* U, const tfl_tensor* flags, const tfl_tensor* p,
                              int is3D) {
  TRY(check_flags(c, "velocityUpdateForward", flags));
  TRY(check_vel(c, "velocityUpdateForward", "U", U, flags, is3D));
  TRY(check_scalar(c, "velocityUpdateForward", "p", p, flags));
  tfl::velocity_update(c->stream, is3D != 0, flags->B, flags->Z, flags->Y, flags->X, U->data, flags->data, p->data);
  return check_launch(c, "velocityUpdateForward");
}

int tfl_vorticityConfinement(tfl_ctx* c, const tfl_tensor* U, const tfl_tensor* flags, float strength,
                             const tfl_tensor* centered, const tfl_tensor* curl, const tfl_tensor* curlNorm,
                             const tfl_tensor* force, int is3D) {
  tfl::Ask none;
  return tfl::vorticityConfinement(c, U, flags, strength, centered, curl, curlNorm, force, is3D, tfl::scope_of(c), none);
}

int tfl_vorticityConfinementFrom(tfl_ctx* c, const tfl_tensor* USrc, const tfl_tensor* U, const tfl_tensor* flags, float strength,
                                 const tfl_tensor* curl, const tfl_tensor* curlNorm, int is3D) {
  tfl::Ask none;
  return tfl::vorticityConfinementFrom(c, USrc, U, flags, strength, curl, curlNorm, is3D, tfl::scope_of(c), none);
}

int tfl_addBuoyancyFrom(tfl_ctx* c, const tfl_tensor* USrc, const tfl_tensor* U, const tfl_tensor* flags,
                        const tfl_tensor* density, const float gravity[3], float dt, int is3D) {
  tfl::Ask none;
  return tfl::addBuoyancyFrom(c, USrc, U, flags, density, gravity, dt, is3D, tfl::scope_of(c), none);
}

int tfl_addBuoyancy(tfl_ctx* c, const tfl_tensor* U, const tfl_tensor* flags, const tfl_tensor* density,
                    const float gravity[3], float* strengthTmp, float dt, int is3D) {
  (void)strengthTmp;
  return tfl_addBuoyancyFrom(c, U, U, flags, density, gravity, dt, is3D);
}

int tfl_addGravity(tfl_ctx* c, const tfl_tensor* U, const tfl_tensor* flags, const float gravity[3], float dt,
                   int is3D, float* forceTmp) {
  (void)forceTmp;
  return tfl::addGravity(c, U, flags, gravity, dt, is3D, tfl::scope_of(c));
}

int tfl_emptyDomain(tfl_ctx* c, const tfl_tensor* flags, int is3D, int bnd) {
  TRY(check_flags(c, "emptyDomain", flags));
  if (!is3D && flags->Z != 1) return fail(c, TFL_EINVAL, "emptyDomain: 2D domain but zdepth > 1");
  tfl::empty_domain(c->stream, is3D != 0, bnd, flags->B, flags->Z, flags->Y, flags->X, flags->data);
  return check_launch(c, "emptyDomain");
}

int tfl_flagsToOccupancy(tfl_ctx* c, const tfl_tensor* flags, const tfl_tensor* occupancy) {
  TRY(check_flags(c, "flagsToOccupancy", flags));
  TRY(check_scalar(c, "flagsToOccupancy", "occupancy", occupancy, flags));
  tfl::flags_to_occupancy(c->stream, (long long)flags->B * flags->Z * flags->Y * flags->X, flags->data,
                          occupancy->data);
  return check_launch(c, "flagsToOccupancy");
}

int tfl_rectangularBlur(tfl_ctx* c, const tfl_tensor* src, int blurRad, int is3D, const tfl_tensor* dst,
                        const tfl_tensor* tmp) {
  if (!c) return TFL_EINVAL;
  if (!src || !dst || !tmp || !src->data || !dst->data || !tmp->data) return fail(c, TFL_EINVAL, "rectangularBlur: null tensor");
  if (!same_dims(dst, src) || dst->C != src->C || !same_dims(tmp, src) || tmp->C != src->C)
    return fail(c, TFL_EINVAL, "rectangularBlur: src, dst and tmp must have the same size");
  if (blurRad <= 0) return fail(c, TFL_EINVAL, "rectangularBlur: blurRad must be a positive, non-zero integer");   // init.lua:586-587
  if (!is3D && src->Z != 1) return fail(c, TFL_EINVAL, "rectangularBlur: 2D field but zdepth > 1");
  if (dst->data == src->data || tmp->data == src->data || tmp->data == dst->data)
    return fail(c, TFL_EINVAL, "rectangularBlur: src, dst and tmp must not alias");
  tfl::rectangular_blur(c->stream, is3D != 0, src->B, src->C, src->Z, src->Y, src->X, blurRad, src->data, dst->data, tmp->data);
  return check_launch(c, "rectangularBlur");
}

int tfl_signedDistanceField(tfl_ctx* c, const tfl_tensor* flags, int searchRad, int is3D, const tfl_tensor* dst) {
  TRY(check_flags(c, "signedDistanceField", flags));
  TRY(check_scalar(c, "signedDistanceField", "dst", dst, flags));
  if (searchRad <= 0) return fail(c, TFL_EINVAL, "signedDistanceField: searchRad must be a positive, non-zero integer");
  if (!is3D && flags->Z != 1) return fail(c, TFL_EINVAL, "signedDistanceField: 2D domain but zdepth > 1");
  tfl::signed_distance_field(c->stream, flags->B, flags->Z, flags->Y, flags->X, searchRad, flags->data, dst->data);
  return check_launch(c, "signedDistanceField");
}

int64_t tfl_pcg_workspace_floats(int32_t Z, int32_t Y, int32_t X) { return tfl::pcg_workspace_floats(Z, Y, X); }

// "none" 0 | "ilu0" 1 | "ic0" 2 | "mg" 3; NULL = "ic0"; -1: not a preconditioner
static int pcg_precond_of(const char* precondType) {
  const std::string pt = precondType ? precondType : "ic0";
  return pt == "none" ? 0 : pt == "ilu0" ? 1 : pt == "ic0" ? 2 : pt == "mg" ? 3 : -1;
}
int64_t tfl_pcg_workspace_floats_for(int32_t Z, int32_t Y, int32_t X, const char* precondType) {
  return tfl::pcg_workspace_floats_for(Z, Y, X, pcg_precond_of(precondType));
}
int64_t tfl_pcg_last_iterations(tfl_ctx* c) { return c ? c->pcg_last_iterations : -1; }

int tfl_solveLinearSystemPCG(tfl_ctx* c, const tfl_tensor* p, const tfl_tensor* flags, const tfl_tensor* div, int is3D,
                             const char* precondType, float tol, int maxIter, int verbose, float* workspace,
                             int64_t workspace_floats, float* residual) {
  TRY(check_flags(c, "solveLinearSystemPCG", flags));
  TRY(check_scalar(c, "solveLinearSystemPCG", "p", p, flags));
  TRY(check_scalar(c, "solveLinearSystemPCG", "div", div, flags));
  if (!is3D && flags->Z != 1) return fail(c, TFL_EINVAL, "solveLinearSystemPCG: d > 1 for a 2D domain");
  const int pc = pcg_precond_of(precondType);
  if (pc < 0) return fail(c, TFL_EINVAL, "solveLinearSystemPCG: precondType is not supported.");
  if (!workspace || ((uintptr_t)workspace & 7) != 0) return fail(c, TFL_EINVAL, "solveLinearSystemPCG: workspace must be 8-byte aligned");
  if (workspace_floats < tfl::pcg_workspace_floats_for(flags->Z, flags->Y, flags->X, pc))
    return fail(c, TFL_EINVAL, "%s", pc == 3 ? "solveLinearSystemPCG: workspace too small (tfl_pcg_workspace_floats_for)"
                                       : "solveLinearSystemPCG: workspace too small (tfl_pcg_workspace_floats)");
  if ((long long)flags->Z * flags->Y * flags->X >= (1ll << 31)) return fail(c, TFL_EINVAL, "solveLinearSystemPCG: grid too large for 32-bit cell indices");
  char msg[256] = {0};
  // the pipelined sweeps need every sub-box resident at once: when something else holds part of the GPU they time out (~1 s)
  // and the solve is repeated with one launch per hyperplane -- remembered per context, so that only the FIRST solve pays
  const tfl::PcgProblem q{is3D != 0, flags->B, flags->Z, flags->Y, flags->X, p->data, flags->data, div->data, pc, tol, maxIter, verbose};
  long long iterations = 0;
  auto solve = [&](bool allow_wavefronts) {
    return tfl::pcg_solve(c->stream, q, workspace, residual, msg, sizeof(msg), allow_wavefronts, &iterations);
  };
  tfl::PcgResult rc = solve(c->wf_skip == 0);
  if (c->wf_skip > 0) c->wf_skip--;
  if (rc == tfl::PcgResult::wavefront_timeout) {
    // back off for 16, 32, ... 1024 solves, then try the pipelined sweeps again; say so once per latch
    c->wf_timeouts++;
    c->wf_skip = 16 << (c->wf_timeouts < 7 ? c->wf_timeouts - 1 : 6);
    fprintf(stderr, "[tfl] solveLinearSystemPCG: a pipelined triangular sweep timed out (something else holds part of the GPU?); "
                    "this solve and the next %d on this context use hyperplane sweeps (slower), then the pipelined form is retried\n", c->wf_skip);
    rc = solve(false);
  }
  switch (rc) {
    case tfl::PcgResult::ok: c->pcg_last_iterations = iterations; return check_launch(c, "solveLinearSystemPCG");
    case tfl::PcgResult::bad_flags:
    case tfl::PcgResult::nan_residual:
    case tfl::PcgResult::too_many_components: return fail(c, TFL_EINVAL, "%s", msg);
    default: return fail(c, TFL_EHIP, "%s", msg);
  }
}

int64_t tfl_pcg_batched_workspace_floats(int32_t B, int32_t Z, int32_t Y, int32_t X, const char* precondType) {
  const int pc = precondType ? pcg_precond_of(precondType) : -1;
  return B > 0 ? tfl::pcg_batched_workspace_floats(B, Z, Y, X, pc) : -1;
}

int tfl_solveLinearSystemPCGBatched(tfl_ctx* c, const tfl_tensor* p, const tfl_tensor* flags, const tfl_tensor* div, int is3D,
                                    const char* precondType, float tol, int maxIter, float* workspace, int64_t workspace_floats,
                                    float* residuals, int64_t* iterations) {
  const char* who = "solveLinearSystemPCGBatched";
  TRY(check_flags(c, who, flags));
  TRY(check_scalar(c, who, "p", p, flags));
  TRY(check_scalar(c, who, "div", div, flags));
  if (!is3D && flags->Z != 1) return fail(c, TFL_EINVAL, "%s: d > 1 for a 2D domain", who);
  const int pc = precondType ? pcg_precond_of(precondType) : -1;
  if (pc < 0) return fail(c, TFL_EINVAL, "%s: precondType is not supported.", who);
  if (pc == 1 || pc == 2)
    return fail(c, TFL_EUNSUPPORTED, "%s: precondType '%s' does not batch (its wavefront sweeps wait for each other): 'mg' or 'none'", who,
                precondType);
  if (!workspace || ((uintptr_t)workspace & 7) != 0) return fail(c, TFL_EINVAL, "%s: workspace must be 8-byte aligned", who);
  if (workspace_floats < tfl::pcg_batched_workspace_floats(flags->B, flags->Z, flags->Y, flags->X, pc))
    return fail(c, TFL_EINVAL, "%s: workspace too small (tfl_pcg_batched_workspace_floats)", who);
  if ((long long)flags->Z * flags->Y * flags->X >= (1ll << 31)) return fail(c, TFL_EINVAL, "%s: grid too large for 32-bit cell indices", who);
  if (flags->B > 65535) return fail(c, TFL_EINVAL, "%s: more than 65535 batch items (the item is a launch's y index)", who);
  char msg[256] = {0};
  const tfl::PcgProblem q{is3D != 0, flags->B, flags->Z, flags->Y, flags->X, p->data, flags->data, div->data, pc, tol, maxIter, 0};
  std::vector<long long> its(flags->B, 0);
  long long total = 0;
  switch (tfl::pcg_solve_batched(c->stream, q, workspace, residuals, its.data(), &total, msg, sizeof(msg))) {
    case tfl::PcgResult::ok: break;
    case tfl::PcgResult::bad_flags:
    case tfl::PcgResult::nan_residual:
    case tfl::PcgResult::too_many_components: return fail(c, TFL_EINVAL, "%s", msg);
    default: return fail(c, TFL_EHIP, "%s", msg);
  }
  if (iterations) for (int b = 0; b < flags->B; b++) iterations[b] = its[b];
  c->pcg_last_iterations = total;
  return check_launch(c, who);
}

int64_t tfl_normalize_workspace_floats(int32_t Z, int32_t Y, int32_t X) { return tfl::npm_workspace_floats(Z, Y, X); }

int tfl_normalizePressureMean(tfl_ctx* c, const tfl_tensor* p, const tfl_tensor* flags, int is3D, float* workspace,
                              int64_t workspace_floats) {
  TRY(check_flags(c, "normalizePressureMean", flags));
  TRY(check_scalar(c, "normalizePressureMean", "p", p, flags));
  if (!is3D && flags->Z != 1) return fail(c, TFL_EINVAL, "normalizePressureMean: 2D domain but zdepth > 1");
  if (!workspace || ((uintptr_t)workspace & 7) != 0) return fail(c, TFL_EINVAL, "normalizePressureMean: workspace must be 8-byte aligned");
  if (workspace_floats < tfl::npm_workspace_floats(flags->Z, flags->Y, flags->X))
    return fail(c, TFL_EINVAL, "normalizePressureMean: workspace too small (tfl_normalize_workspace_floats)");
  if ((long long)flags->Z * flags->Y * flags->X >= (1ll << 31)) return fail(c, TFL_EINVAL, "normalizePressureMean: grid too large for 32-bit cell indices");
  char msg[256] = {0};
  const tfl::PcgResult rc = tfl::normalize_pressure_mean(c->stream, is3D != 0, flags->B, flags->Z, flags->Y, flags->X, p->data,
                                                         flags->data, workspace, msg, sizeof(msg));
  if (rc != tfl::PcgResult::ok) return fail(c, TFL_EHIP, "%s", msg);
  return check_launch(c, "normalizePressureMean");
}

int tfl_solveLinearSystemJacobi(tfl_ctx* c, const tfl_tensor* p, const tfl_tensor* flags, const tfl_tensor* div,
                                const tfl_tensor* pPrev, const tfl_tensor* pDelta, const tfl_tensor* pDeltaNorm,
                                int is3D, float pTol, int maxIter, int verbose, float* residual) {
  (void)pDelta; (void)pDeltaNorm;
  TRY(check_flags(c, "solveLinearSystemJacobi", flags));
  TRY(check_scalar(c, "solveLinearSystemJacobi", "p", p, flags));
  TRY(check_scalar(c, "solveLinearSystemJacobi", "div", div, flags));
  TRY(check_scalar(c, "solveLinearSystemJacobi", "pPrev", pPrev, flags));
  if (!is3D && flags->Z != 1) return fail(c, TFL_EINVAL, "solveLinearSystemJacobi: 2D domain but zdepth > 1");
  if (maxIter < 1) return fail(c, TFL_EINVAL, "solveLinearSystemJacobi: At least 1 iteration is needed (maxIter < 1)");
  const int B = flags->B;
  if (B > kMaxBatch) return fail(c, TFL_EINVAL, "solveLinearSystemJacobi: batch size above %d", kMaxBatch);
  const size_t bytes = sizeof(float) * (size_t)B * flags->Z * flags->Y * flags->X;
  // a small 2-D grid with a fixed iteration count (BASELINE config 1): one launch for the whole solve (jacobi.hip)
  if (!is3D && flags->Z == 1 && !(pTol > 0.0f) && !verbose) {
    const bool want = residual != nullptr;
    if (tfl::jacobi_solve_lds(c->stream, B, flags->Y, flags->X, flags->data, div->data, p->data, pPrev->data, maxIter,
                              want ? c->d_resid : nullptr)) {
      if (want) {
        HIP_TRY(c, hipMemcpyAsync(c->h_resid, c->d_resid, sizeof(double) * B, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        float res = 0.0f;
        for (int b = 0; b < B; b++) res = std::max(res, (float)std::sqrt(c->h_resid[b]));
        *residual = res;
      }
      return check_launch(c, "solveLinearSystemJacobi");
    }
  }
  // generic/tfluids.cu:1869-1872: both buffers start at zero
  HIP_TRY(c, hipMemsetAsync(p->data, 0, bytes, c->stream));
  HIP_TRY(c, hipMemsetAsync(pPrev->data, 0, bytes, c->stream));
  float* cur = p->data;
  float* prev = pPrev->data;
  float res = 0.0f;
  const bool every = pTol > 0.0f;  // the reference reads the residual back every iteration (:1886);
                                   // with pTol <= 0 it can never stop early, so only the last one matters
  int iter = 0;
  for (;;) {
    const bool last = (iter + 1 >= maxIter);
    const bool want = every || (last && residual != nullptr);
    if (want) HIP_TRY(c, hipMemsetAsync(c->d_resid, 0, sizeof(double) * B, c->stream));
    tfl::jacobi_iteration(c->stream, is3D != 0, B, flags->Z, flags->Y, flags->X, prev, flags->data, div->data, cur,
                          want ? c->d_resid : nullptr);
    if (want) {
      HIP_TRY(c, hipMemcpyAsync(c->h_resid, c->d_resid, sizeof(double) * B, hipMemcpyDeviceToHost, c->stream));
      HIP_TRY(c, hipStreamSynchronize(c->stream));
      res = 0.0f;
      for (int b = 0; b < B; b++) {
        const float r = (float)std::sqrt(c->h_resid[b]);
        if (r > res) res = r;
      }
      if (verbose) printf("Jacobi iteration %d: residual %e\n", iter + 1, (double)res);
      if (every && res < pTol) break;
    }
    iter++;
    if (iter >= maxIter) break;
    float* t = cur; cur = prev; prev = t;
  }
  if (cur != p->data) HIP_TRY(c, hipMemcpyAsync(p->data, cur, bytes, hipMemcpyDeviceToDevice, c->stream));
  if (residual) *residual = res;
  return check_launch(c, "solveLinearSystemJacobi");
}

int tfl_copy(tfl_ctx* c, const tfl_tensor* dst, const tfl_tensor* src) {
  if (!c) return TFL_EINVAL;
  if (!dst || !src || !dst->data || !src->data) return fail(c, TFL_EINVAL, "copy: null tensor");
  const long long n = (long long)dst->B * dst->C * dst->Z * dst->Y * dst->X;
  if (n != (long long)src->B * src->C * src->Z * src->Y * src->X) return fail(c, TFL_EINVAL, "copy: size mismatch");
  HIP_TRY(c, hipMemcpyAsync(dst->data, src->data, sizeof(float) * (size_t)n, hipMemcpyDeviceToDevice, c->stream));
  return TFL_OK;
}

int tfl_stream_copy(tfl_ctx* c, float* dst, const float* src, int64_t n) {
  if (!c) return TFL_EINVAL;
  if (!dst || !src || n < 0 || (n & 3) || (((uintptr_t)dst | (uintptr_t)src) & 15))
    return fail(c, TFL_EINVAL, "stream_copy: needs 16-byte aligned pointers and a multiple of 4 floats");
  tfl::stream_copy(c->stream, n / 4, src, dst);
  return check_launch(c, "stream_copy");
}

int tfl_applyBCs(tfl_ctx* c, const tfl_tensor* x, const tfl_tensor* bc, const tfl_tensor* invMask, int doClamp,
                 float lo, float hi) {
  if (!c) return TFL_EINVAL;
  if (!x || !x->data) return fail(c, TFL_EINVAL, "applyBCs: x is null");
  if ((bc == nullptr) != (invMask == nullptr)) return fail(c, TFL_EINVAL, "applyBCs: bc and invMask go together");
  const long long n = (long long)x->B * x->C * x->Z * x->Y * x->X;
  if (bc) {
    const long long nb = (long long)bc->B * bc->C * bc->Z * bc->Y * bc->X;
    const long long nm = (long long)invMask->B * invMask->C * invMask->Z * invMask->Y * invMask->X;
    if (nb != n || nm != n || !bc->data || !invMask->data) return fail(c, TFL_EINVAL, "applyBCs: size mismatch");
  }
  tfl::apply_bcs(c->stream, n, x->data, bc ? bc->data : nullptr, bc ? invMask->data : nullptr, doClamp, lo, hi);
  return check_launch(c, "applyBCs");
}

int tfl_applyBCsIndexed(tfl_ctx* c, const tfl_tensor* x, const tfl_tensor* bc, const tfl_tensor* invMask,
                        const int32_t* idx, int64_t n) {
  if (!c) return TFL_EINVAL;
  if (!x || !x->data || !bc || !bc->data || !invMask || !invMask->data) return fail(c, TFL_EINVAL, "applyBCsIndexed: null tensor");
  const long long nx = (long long)x->B * x->C * x->Z * x->Y * x->X;
  const long long nb = (long long)bc->B * bc->C * bc->Z * bc->Y * bc->X;
  const long long nm = (long long)invMask->B * invMask->C * invMask->Z * invMask->Y * invMask->X;
  if (nb != nx || nm != nx) return fail(c, TFL_EINVAL, "applyBCsIndexed: size mismatch");
  if (nx >= (1ll << 31)) return fail(c, TFL_EINVAL, "applyBCsIndexed: tensor too large for 32-bit indices");
  if (n < 0 || (n > 0 && !idx)) return fail(c, TFL_EINVAL, "applyBCsIndexed: bad index list");
  tfl::apply_bcs_indexed(c->stream, n, idx, x->data, bc->data, invMask->data);
  return check_launch(c, "applyBCsIndexed");
}

int tfl_applyBCsIndexedMulti(tfl_ctx* c, int count, const tfl_tensor* const* x, const tfl_tensor* const* bc,
                             const tfl_tensor* const* invMask, const int32_t* const* idx, const int64_t* n) {
  if (!c) return TFL_EINVAL;
  if (count < 1 || count > 8 || !x || !bc || !invMask || !idx || !n)
    return fail(c, TFL_EINVAL, "applyBCsIndexedMulti: 1..8 (x, bc, invMask, idx) tuples are required");
  long long nn[8];
  const int* ii[8];
  float* xx[8];
  const float *bb[8], *mm[8];
  for (int i = 0; i < count; i++) {
    const tfl_tensor *xi = x[i], *bi = bc[i], *mi = invMask[i];
    if (!xi || !xi->data || !bi || !bi->data || !mi || !mi->data) return fail(c, TFL_EINVAL, "applyBCsIndexedMulti: null tensor in tuple %d", i);
    const long long nx = (long long)xi->B * xi->C * xi->Z * xi->Y * xi->X;
    const long long nb = (long long)bi->B * bi->C * bi->Z * bi->Y * bi->X;
    const long long nm = (long long)mi->B * mi->C * mi->Z * mi->Y * mi->X;
    if (nb != nx || nm != nx) return fail(c, TFL_EINVAL, "applyBCsIndexedMulti: size mismatch in tuple %d", i);
    if (nx >= (1ll << 31)) return fail(c, TFL_EINVAL, "applyBCsIndexedMulti: tensor %d too large for 32-bit indices", i);
    if (n[i] < 0 || (n[i] > 0 && !idx[i])) return fail(c, TFL_EINVAL, "applyBCsIndexedMulti: bad index list %d", i);
    nn[i] = n[i]; ii[i] = idx[i]; xx[i] = xi->data; bb[i] = bi->data; mm[i] = mi->data;
  }
  tfl::apply_bcs_indexed_multi(c->stream, count, nn, ii, xx, bb, mm);
  return check_launch(c, "applyBCsIndexedMulti");
}

int tfl_packPlanes(tfl_ctx* c, int n, const tfl_tensor* const* fields, int zlo, int zhi, float* buf, int unpack) {
  if (!c) return TFL_EINVAL;
  if (n < 1 || n > 8 || !fields || !buf) return fail(c, TFL_EINVAL, "packPlanes: 1..8 fields and a buffer are required");
  const tfl_tensor* f0 = fields[0];
  if (!f0 || zlo < 0 || zhi > f0->Z || zlo >= zhi) return fail(c, TFL_EINVAL, "packPlanes: bad plane range [%d, %d)", zlo, zhi);
  float* ptrs[8];
  int rows[8], los[8], nps[8];
  for (int i = 0; i < n; i++) {
    const tfl_tensor* f = fields[i];
    if (!f || !f->data || f->Z != f0->Z || f->Y != f0->Y || f->X != f0->X)
      return fail(c, TFL_EINVAL, "packPlanes: field %d does not match the grid of field 0", i);
    ptrs[i] = f->data;
    rows[i] = f->B * f->C;
    los[i] = zlo; nps[i] = zhi - zlo;
  }
  const long long yx = (long long)f0->Y * f0->X;
  tfl::pack_planes(c->stream, n, ptrs, rows, los, nps, yx * f0->Z, yx, buf, unpack);
  return check_launch(c, "packPlanes");
}

int tfl_setWallBcsBackward(tfl_ctx* c, const tfl_tensor* flags, const tfl_tensor* gradOutput, int is3D, const tfl_tensor* gradU) {
  TRY(check_flags(c, "setWallBcsBackward", flags));
  TRY(check_vel(c, "setWallBcsBackward", "gradOutput", gradOutput, flags, is3D));
  TRY(check_vel(c, "setWallBcsBackward", "gradU", gradU, flags, is3D));
  if (gradU->data != gradOutput->data)
    HIP_TRY(c, hipMemcpyAsync(gradU->data, gradOutput->data, sizeof(float) * (size_t)flags->B * gradU->C * flags->Z * flags->Y * flags->X,
                              hipMemcpyDeviceToDevice, c->stream));
  tfl::set_wall_bcs(c->stream, is3D != 0, flags->B, flags->Z, flags->Y, flags->X, gradU->data, flags->data);
  return check_launch(c, "setWallBcsBackward");
}

int tfl_velocityDivergenceBackward(tfl_ctx* c, const tfl_tensor* U, const tfl_tensor* flags, const tfl_tensor* gradOutput,
                                   int is3D, const tfl_tensor* gradU) {
  TRY(check_flags(c, "velocityDivergenceBackward", flags));
  TRY(check_vel(c, "velocityDivergenceBackward", "U", U, flags, is3D));
  TRY(check_vel(c, "velocityDivergenceBackward", "gradU", gradU, flags, is3D));
  TRY(check_scalar(c, "velocityDivergenceBackward", "gradOutput", gradOutput, flags));
  tfl::velocity_divergence_bwd(c->stream, is3D != 0, flags->B, flags->Z, flags->Y, flags->X, flags->data,
                               gradOutput->data, gradU->data);
  return check_launch(c, "velocityDivergenceBackward");
}

int tfl_velocityUpdateBackward(tfl_ctx* c, const tfl_tensor* U, const tfl_tensor* flags, const tfl_tensor* p,
                               const tfl_tensor* gradOutput, int is3D, const tfl_tensor* gradP) {
  TRY(check_flags(c, "velocityUpdateBackward", flags));
  TRY(check_vel(c, "velocityUpdateBackward", "U", U, flags, is3D));
  TRY(check_vel(c, "velocityUpdateBackward", "gradOutput", gradOutput, flags, is3D));
  TRY(check_scalar(c, "velocityUpdateBackward", "p", p, flags));
  TRY(check_scalar(c, "velocityUpdateBackward", "gradP", gradP, flags));
  tfl::velocity_update_bwd(c->stream, is3D != 0, flags->B, flags->Z, flags->Y, flags->X, flags->data, gradOutput->data,
                           gradP->data);
  return check_launch(c, "velocityUpdateBackward");
}

int tfl_volumetricUpSamplingNearestForward(tfl_ctx* c, int ratio, const tfl_tensor* input, const tfl_tensor* output) {
  if (!c) return TFL_EINVAL;
  if (!input || !output || !input->data || !output->data) return fail(c, TFL_EINVAL, "ERROR: input and output must be dim 5");
  if (ratio < 1 || output->B != input->B || output->C != input->C || output->Z != input->Z * ratio ||
      output->Y != input->Y * ratio || output->X != input->X * ratio)
    return fail(c, TFL_EINVAL, "ERROR: input : output size mismatch.");
  tfl::upsample_nearest_fwd(c->stream, ratio, (long long)input->B * input->C, output->Z, output->Y, output->X,
                            input->data, output->data);
  return check_launch(c, "volumetricUpSamplingNearestForward");
}

int tfl_volumetricUpSamplingNearestBackward(tfl_ctx* c, int ratio, const tfl_tensor* input, const tfl_tensor* gradOutput,
                                            const tfl_tensor* gradInput) {
  if (!c) return TFL_EINVAL;
  if (!input || !gradOutput || !gradInput || !gradOutput->data || !gradInput->data)
    return fail(c, TFL_EINVAL, "ERROR: input, gradOutput and gradInput must be dim 5");
  if (ratio < 1 || gradOutput->B != input->B || gradOutput->C != input->C || gradOutput->Z != input->Z * ratio ||
      gradOutput->Y != input->Y * ratio || gradOutput->X != input->X * ratio)
    return fail(c, TFL_EINVAL, "ERROR: input : gradOutput size mismatch.");
  if (gradInput->B != input->B || gradInput->C != input->C || gradInput->Z != input->Z || gradInput->Y != input->Y ||
      gradInput->X != input->X)
    return fail(c, TFL_EINVAL, "ERROR: input : gradInput size mismatch.");
  tfl::upsample_nearest_bwd(c->stream, ratio, (long long)input->B * input->C, input->Z, input->Y, input->X,
                            gradOutput->data, gradInput->data);
  return check_launch(c, "volumetricUpSamplingNearestBackward");
}

}  // extern "C"
