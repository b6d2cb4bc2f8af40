// tfl_ctx.hpp -- the context object behind the opaque tfl_ctx* of include/tfluids_hip.h (private to the library:
// context.cpp owns it, simulate.cpp and simulate_slab.cpp read the stream, simulate.cpp keeps the brick-list state of
// advectScalar and simulate_slab.cpp the z-slab reach-check words). It holds resources and what the
// host's tfl_set_* calls stored. Nothing per call lives here: what a native step asks of an operator call (tfl_ops.hpp Ask)
// and where that call computes (tfl_host.hpp Scope) travel as arguments.
#pragma once
#include <hip/hip_runtime.h>

#include <mutex>
#include <string>
#include <vector>

#include "tfl_host.hpp"

// the wall codes of one flags array (include/tfluids_hip.h tfl_wall_plan): found again by the array's address and shape
struct tfl_wall_plan {
  const float* flags = nullptr;
  unsigned short* code = nullptr;             // 16 bits per cell (model.hip k_wall_code)
  int B = 0, Z = 0, Y = 0, X = 0;
  bool is3d = false;
  struct tfl_ctx* owner = nullptr;            // the context it is registered with (cleared by tfl_destroy: the plan may outlive it)
};

// What tfl_simulate_step keeps per density field for the passes over the list of non-empty bricks (advect_scalar3_sparse.hip): the
// device buffers of a Scal3SparseAsk and the pinned words its lists kernel leaves for the policy of later steps. Found again by
// the field's address and shape; allocated once (context.cpp scal3_sparse_state), never while the stream is capturing.
struct Scal3SparseState {
  const float* key = nullptr;
  int B = 0, Z = 0, Y = 0, X = 0;
  tfl::Scal3SparseAsk buf;                    // nz (the tags), lists, counts, mirror (run / took / scanned / seq are per call)
  unsigned* h_mirror = nullptr;               // pinned, mapped: 8 words per batch item (|L_B|, bricks, fast, |L_A|, the scan's number)
  unsigned scans = 0;                         // scans launched for this field so far (the next scan's number - 1)
  unsigned since_scan = 0;                    // steps on the two full launches since the last scan
};

struct tfl_ctx {
  std::vector<tfl_wall_plan*> wall_plans;     // registered by tfl_wall_plan_create, looked up by tfl_model_begin
  std::mutex wall_mu;                         // (a binding may retire a plan from a finalizer thread while this context steps)
  int device = 0;
  hipStream_t stream = nullptr;
  std::string err;
  unsigned long long* d_trace_err = nullptr;  // device words: [0] traces that hit an invariant path, [1], [2] tfl_scal3_zero_blocks
  double* d_resid = nullptr;                  // Jacobi residual accumulators [kMaxBatch]
  double* h_resid = nullptr;                  // pinned mirror
  float dx_override = 0.0f;                   // > 0: use instead of 1/max(X,Y,Z) (z-slab ranks: global dx)
  // the next four: what scope_of (context.cpp) copies into a Scope, for the public operators that honour them and for
  // tfl_simulate_step; the z-slab step builds scopes of its own and takes the advect mode alone
  tfl::ZWin zwin = {0, 0, 0, 0};              // tfl_set_z_window: planes the next operators compute (all zero = all)
  tfl::ZOrigin zorigin = {0, 0};              // tfl_set_z_origin: where the arrays sit in the whole grid
  int advect_fast = 0;                        // tfl_set_advect_mode (initialised from TFL_ADVECT_MODE by tfl_create)
  int stages = 0;                             // tfl_set_stages: which passes of a multi-pass operator run (0 = all)
  float* d_reach = nullptr;                   // z-slab reach check: max|u_z| of the current step (device word)
  float* h_reach = nullptr;                   // pinned mirror (TWO words: the maximum, and the publication count), read by later calls
  // check_reach = 1 (round 6): the device word is a STICKY maximum (never reset by a step: a violation cannot be overwritten before
  // the host has seen it). The step's LAST kernel (k_project) copies it into the mapped pinned mirror -- an async 4-byte D2H copy
  // BLOCKS the host on this stack -- and, behind a system-scope fence, the count of such publications (a device word it
  // increments) beside it. The call for step n + 1 waits, spinning on that pinned count, for the publication of step n - 1:
  // there unless the host is more than two steps ahead, so the wait bounds the host's lead and costs nothing. No API call
  // and no event on either side: the hipEventRecord per step of the first form cost the device 4 us of a 0.1 ms rank-step.
  float* d_reach_host = nullptr;              // the device address of h_reach
  unsigned* d_reach_tick = nullptr;           // device word: publications made so far
  bool reach_folded = false;                  // the last projection launch of a slab step folded max|u_z| of the planes it wrote into d_reach: the next step's k_absmax is not needed
  unsigned reach_issued = 0;                  // publishing launches enqueued so far (host side)
  unsigned reach_hist[2] = {0, 0};            // reach_issued as it stood at the end of the step before last / of the last step
  double* h_reach_flags = nullptr;            // pinned [kReachFlags]: the all-reduced "reach >= r" counts of check_reach = 2 (created on first use)
  int needed_reach = 0;                       // what the last TFL_EREACH asked for (tfl_slab_needed_reach)
  int wf_skip = 0;                            // > 0: a pipelined PCG sweep timed out on this context: the next wf_skip solves go straight to
                                              // hyperplane sweeps, then the pipelined form is tried again (a transient stall must not latch for good)
  int wf_timeouts = 0;                        // how often that happened (the back-off doubles, one warning per latch)
  long long pcg_last_iterations = -1;         // tfl_pcg_last_iterations: CG iterations of the last tfl_solveLinearSystemPCG, summed over its component solves
  std::vector<Scal3SparseState*> scal3_sparse;   // one per density field tfl_simulate_step has advected over brick lists (at most kScal3SparseFields)
  Scal3SparseState* scal3_last = nullptr;        // the field of the last scan
  long long scal3_counts[3] = {0, 0, 0};         // EXPERIMENTS flavour (tfl_scal3_sparse_stats): scans, steps over the lists, steps on the two full launches
};

namespace tfl {
constexpr int kScal3SparseFields = 8;      // a step has at most 8 density channels
// the state of the density field at `key` ([B][1][Z][Y][X], `bricks` bricks per item), created on first use (allocates: never call
// it while the stream is capturing); null when an allocation fails
Scal3SparseState* scal3_sparse_state(tfl_ctx* c, const float* key, int B, int Z, int Y, int X, int bricks);
}  // namespace tfl
