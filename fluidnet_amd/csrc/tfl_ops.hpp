// tfl_ops.hpp -- library-internal (C++ linkage) forms of the operators that the native steps call (simulate.cpp: the un-cut
// step; simulate_slab.cpp: the z-slab rank-step): each takes
// the public tfl_* operator's arguments plus where it computes and which passes run (tfl_host.hpp Scope) and a request (Ask).
// The public operator (abi.cpp, model_host.cpp, model_train.cpp) passes scope_of(its context) and an empty Ask; a native step passes scopes of its own.
#pragma once
#include "../../include/tfluids_hip.h"
#include "tfl_host.hpp"

namespace tfl {

// What a step asks of the one operator call meant to take it, and what that call reports back (out). Empty = the public operator.
struct Ask {
  Fold fold;                       // the setConstVals pair / buoyancy force for the kernel that writes the result, and what was taken
  Scal3SparseAsk sparse;           // advectScalar (tfl_simulate_step sets it): the passes over the list of non-empty bricks (tfl_host.hpp)
  Vel3ScanAsk scan;                // advectVel (tfl_simulate_step sets it): the brick scan of the advectScalar that follows, inside pass A
  bool two_launch = false;         // vorticityConfinementFrom: the two launches even where the fused kernel would run
  bool gated = true;               // model_begin / model_forward: take the fp16 range gate (a step takes it once, at its entry)
  bool conv1_sums_stats = false;   // model_begin / model_finish (model_forward sets it): the first conv layer sums the partials itself
  const float* project_reads = nullptr;   // model_forward sets it to UDiv where nothing but the projection would read SetWallBcs(UDiv):
                                   // model_begin then leaves UOut alone, model_finish's projection reads the velocity here
  bool reach_via_project = false;  // model_finish: the projection (stage 8) publishes the z-slab reach word (tfl_ctx.hpp d_reach) ...
  bool reach_published = false;    // ... out: it was launched so,
  bool reach_folded = false;       // ... out: and folded max|u_z| of the planes it wrote into the word
};

Scope scope_of(const tfl_ctx* c);     // what tfl_set_z_window / _z_origin / _stages / _advect_mode left on the context
// tfluids.getDx (grid.cc:37-40) in float, as the operators form dt / dx, and in double: the scope's dx_cells, else
// tfl_set_dx_override, else the array's own largest dimension
float get_dx(const tfl_ctx* c, const Scope& sc, const tfl_tensor* flags);
double get_dx_double(const tfl_ctx* c, const Scope& sc, const tfl_tensor* flags);

int advectScalar(tfl_ctx* c, float dt, const tfl_tensor* s, const tfl_tensor* U, const tfl_tensor* flags, const tfl_tensor* fwd,
                 const tfl_tensor* bwd, int is3D, const char* method, const tfl_tensor* fwdPos, const tfl_tensor* bwdPos,
                 int boundaryWidth, int sampleOutsideFluid, float maccormackStrength, const tfl_tensor* sDst, const Scope& sc,
                 Ask& ask);
int advectVel(tfl_ctx* c, float dt, const tfl_tensor* U, const tfl_tensor* flags, const tfl_tensor* fwd, const tfl_tensor* bwd,
              int is3D, const char* method, int boundaryWidth, float maccormackStrength, const tfl_tensor* UDst, const Scope& sc,
              Ask& ask);
int addBuoyancyFrom(tfl_ctx* c, const tfl_tensor* USrc, const tfl_tensor* U, const tfl_tensor* flags, const tfl_tensor* density,
                    const float gravity[3], float dt, int is3D, const Scope& sc, Ask& ask);
int addGravity(tfl_ctx* c, const tfl_tensor* U, const tfl_tensor* flags, const float gravity[3], float dt, int is3D, const Scope& sc);
// the per-item forms (tfl_addBuoyancyItems ...; include/tfluids_hip.h): whole array only, the scope gives dx
int addBuoyancyItems(tfl_ctx* c, const tfl_tensor* USrc, const tfl_tensor* U, const tfl_tensor* flags, const tfl_tensor* density,
                     const float* gravity, const int32_t* on, int n_items, float dt, int is3D, const Scope& sc);
int addGravityItems(tfl_ctx* c, const tfl_tensor* U, const tfl_tensor* flags, const float* gravity, const int32_t* on, int n_items,
                    float dt, int is3D, const Scope& sc);
int vorticityConfinementItems(tfl_ctx* c, const tfl_tensor* U, const tfl_tensor* flags, const float* strength, const int32_t* on,
                              int n_items, const tfl_tensor* curl, const tfl_tensor* curlNorm, int is3D, const Scope& sc);
int vorticityConfinement(tfl_ctx* c, const tfl_tensor* U, const tfl_tensor* flags, float strength, const tfl_tensor* centered,
                         const tfl_tensor* curl, const tfl_tensor* curlNorm, const tfl_tensor* force, int is3D, const Scope& sc,
                         Ask& ask);
int vorticityConfinementFrom(tfl_ctx* c, const tfl_tensor* USrc, const tfl_tensor* U, const tfl_tensor* flags, float strength,
                             const tfl_tensor* curl, const tfl_tensor* curlNorm, int is3D, const Scope& sc, Ask& ask);
int model_begin(tfl_ctx* c, tfl_model* m, const tfl_tensor* UDiv, const tfl_tensor* flags, const tfl_tensor* UOut, float* workspace,
                int64_t workspace_floats, int zlo, int zhi, double* stats, const Scope& sc, Ask& ask);
int model_finish(tfl_ctx* c, tfl_model* m, const tfl_tensor* pDiv, const tfl_tensor* flags, const tfl_tensor* pOut,
                 const tfl_tensor* UOut, float* workspace, int64_t workspace_floats, const double* stats, double count,
                 const tfl_tensor* UBC, const tfl_tensor* UBCInvMask, int doClamp, float lo, float hi, const Scope& sc, Ask& ask);
int model_forward(tfl_ctx* c, tfl_model* m, const tfl_tensor* pDiv, const tfl_tensor* UDiv, const tfl_tensor* flags,
                  const tfl_tensor* pOut, const tfl_tensor* UOut, float* workspace, int64_t workspace_floats, const tfl_tensor* UBC,
                  const tfl_tensor* UBCInvMask, int doClamp, float lo, float hi, const Scope& sc, Ask& ask);

// The MacCormack(Ours) advection of one density channel AND of the velocity on a 3-D grid (the z-slab step), their passes A as
// one launch (stage bit 2) and their passes B as one launch (stage bit 4) -- advect_pair3.hip. fold_s / fold_v: the
// setConstVals pairs the passes B apply (dev == nullptr: none). TFL_EUNSUPPORTED = not taken, nothing launched: the caller runs
// advectScalar and advectVel.
int advect_pair(tfl_ctx* c, float dt, float strength, const tfl_tensor* s, const tfl_tensor* U, const tfl_tensor* flags,
                const tfl_tensor* sfwd, const tfl_tensor* sbounds, const tfl_tensor* sDst, const tfl_tensor* vfwd, const tfl_tensor* UDst,
                const BcFoldArg& fold_s, const BcFoldArg& fold_v, const Scope& sc);
const unsigned long long* model_range_counter(const tfl_model* m);     // the model's fp16 range word (device)

}  // namespace tfl
