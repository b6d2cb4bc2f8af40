/*
 * tfluids_hip.h -- C ABI of the MI355X-native tfluids hot path (libtfluids_hip.so).
 *
 * This is the drop-in boundary for FluidNet's native layer. In the reference every operator is a
 * Lua-C function `static int tfluids_<Real>Main_<op>(lua_State*)` registered on the tensor
 * metatable (torch/tfluids/generic/tfluids.cc:927-957, generic/tfluids.cu:1932-1962) and called
 * from torch/tfluids/init.lua as `X.tfluids.<op>(positional args)`. Each tfl_<op> below takes the
 * SAME positional arguments in the SAME order (the reference call site is cited per function),
 * with THTensor* replaced by `const tfl_tensor*` (raw device pointer + the five sizes; contiguous
 * [B][C][Z][Y][X] fp32, x fastest -- third_party/grid.h:68-78) and lua numbers/booleans replaced by
 * float/int. No torch, Lua or C++ types cross this boundary.
 *
 * Semantics shared by every entry point (mirroring the reference's CUDA path):
 *   - asynchronous: work is enqueued on the context's HIP stream and the call returns without
 *     synchronising (generic/tfluids.cu:106 uses THCState_getCurrentStream the same way); the
 *     only exception is tfl_solveLinearSystemJacobi with pTol > 0, which must read the residual
 *     back every iteration exactly like the reference (generic/tfluids.cu:1886);
 *   - the caller owns every buffer; nothing is allocated, freed, resized or retained;
 *   - "temp" tensors (fwd, bwd, fwdPos, bwdPos, centered, curl, ...) are accepted because the
 *     reference wrappers pass them (init.lua:35-64 getTempStorage); their contents are undefined
 *     on entry AND on exit, exactly as in the reference. This implementation fuses sweeps and does
 *     not touch all of them;
 *   - return value: 0 on success, a negative tfl_status on error; tfl_last_error(ctx) returns a
 *     message. Errors never longjmp/throw across the ABI (the reference raises luaL_error /
 *     THError: init.lua asserts, third_party/tfluids.cc:441-466).
 */
#ifndef TFLUIDS_HIP_H_
#define TFLUIDS_HIP_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TFL_ABI_VERSION 4   /* 3: tfl_comm starts with its own size; tfl_set_advect_mode, tfl_stream_copy. 4: tfl_comm.capturable,
                              tfl_slab_graph_* (the rank-step as one HIP-graph launch) */

typedef enum tfl_status {
  TFL_OK = 0,
  TFL_EINVAL = -1,       /* bad argument (shape / channel / null pointer / unknown method) */
  TFL_EHIP = -2,         /* HIP runtime error (message carries hipGetErrorString) */
  TFL_EUNSUPPORTED = -3, /* valid in the reference but not built here */
  TFL_EREACH = -5,       /* tfl_simulate_step_slab with check_reach = 2: the flow is faster than the slab's halo allows; NOTHING of
                            the step has been written -- lay the slab out for tfl_slab_needed_reach() and call again */
  TFL_ERANGE = -4        /* an earlier forward pass of the model left the fp16 range of the default 3-D conv path (see
                            tfl_model_range_errors): refused until that count has been read */
} tfl_status;

/* A contiguous fp32 5-D tensor resident in HBM: [B][C][Z][Y][X], x fastest.
 * Supported sizes: the elements of ONE batch item fit a signed 32-bit index, C*Z*Y*X < 2^31 (element strides are
 * int32 inside the kernels; the batch offset is applied in 64 bits), e.g. a 3-channel velocity up to 894^3. Larger
 * tensors are refused with TFL_EUNSUPPORTED, never computed wrongly. The LDS-tiled 3-D advection kernels further use
 * 24-bit plane strides (4*X*Y < 2^24, i.e. X*Y <= 2047^2) and 32-bit byte offsets over the three velocity channels
 * (12*Z*Y*X < 2^32, i.e. up to ~710^3) and fall back to the gather kernels beyond that. */
typedef struct tfl_tensor {
  float* data;
  int32_t B, C, Z, Y, X;
} tfl_tensor;

/* Manta cell types stored as floats in `flags` (third_party/cell_type.h:22-33; exported to Lua as
 * tfluids.CellType by init.cu:108-120). */
enum {
  TFL_TypeNone = 0, TFL_TypeFluid = 1, TFL_TypeObstacle = 2, TFL_TypeEmpty = 4,
  TFL_TypeInflow = 8, TFL_TypeOutflow = 16, TFL_TypeOpen = 32, TFL_TypeStick = 128
};

typedef struct tfl_ctx tfl_ctx;

/* ---- scratch memory: `workspace` and `tape` arguments ----------------------------------------------------------------------
 * Every `float* workspace, int64_t workspace_floats` pair (and the `tape` of the training entries) is device memory the caller
 * owns and the entry sizes with the tfl_*_workspace_floats / tfl_model_tape_floats query next to it. For all of them:
 *   contents   undefined on entry. No entry reads a word it has not written in the same call: results, residuals, iteration
 *              counts and error counters do not depend on what the array held before -- zeros, NaN, the leftovers of another
 *              operator or of the same entry on another scene or grid size. The entries add in a fixed order, so that means
 *              the same bits, with one exception: tfl_normalizePressureMean adds each component's cells with fp64 atomics,
 *              in whatever order the waves arrive. Its sum can differ in the last bits of a double from one call to the next
 *              (leftovers or not); the mean is rounded to fp32 before it is subtracted, so the pressure comes out different
 *              only when the mean lies within ~1e-16 (relative) of an fp32 rounding boundary.
 *              No region carries state from one call to the next, with two exceptions stated where they apply: the tape
 *              (written by tfl_model_forward_train, read by the two backward entries) and the message buffers at the head of
 *              the z-slab step's workspace while slab->in_flight is not 0 (the p / U halos in flight between two steps; a
 *              first step, with in_flight = 0, takes the whole array undefined, and the compute region behind the buffers is
 *              dead between steps).
 *   size       exactly the query's value is enough, and no word outside [workspace, workspace + workspace_floats) is written
 *              (the helper wave of the PCG wavefront sweeps READS without clamping, inside the guard pairs the query counts).
 *              A shorter array is TFL_EINVAL before anything is enqueued or written.
 *   alignment  8 bytes: tfl_solveLinearSystemPCG[Batched], tfl_normalizePressureMean, tfl_velocityDivergenceNorm,
 *              tfl_fluidCriterion, tfl_model_forward / _forward_train / _backward / _backward_input and the tape (regions
 *              that need 16 bytes are rounded up inside the array at run time, paid for by slack the query counts); such an
 *              array at 8 mod 16 gives the bits of one at 0 mod 16. 16 bytes: tfl_simulate_step / _project,
 *              tfl_simulate_step_items / _project_items, tfl_simulate_step_slab, tfl_slab_drain and tfl_slab_divergence_norm
 *              (and with them tfl_model_begin / _finish as the z-slab step calls them, inside its workspace); anything less
 *              is TFL_EINVAL with nothing written. Operators that take their temporaries as tfl_tensor arguments (advection,
 *              vorticity confinement, Jacobi, blur) fall under the first two rules; for alignment each temporary is a tensor
 *              like the operator's others.
 * Held by tests/test_hip_scratch_history.py for the entries of tests/scratch_cases.py. */

/* ---- context ------------------------------------------------------------------------------ */
/* Replaces THCState (device + current stream). `device` is a HIP device ordinal. */
tfl_ctx* tfl_create(int device);
void tfl_destroy(tfl_ctx* ctx);
/* `hip_stream` is a hipStream_t (NULL = the legacy default stream). */
int tfl_set_stream(tfl_ctx* ctx, void* hip_stream);
const char* tfl_last_error(const tfl_ctx* ctx);
int tfl_abi_version(void);
/* Arithmetic of the LDS-tiled 3-D advection kernels (advectVel / advectScalar, methods eulerOurs and maccormackOurs):
 *   TFL_ADVECT_EXACT (default)  every operation in the reference's order and rounding: results are bit-equal to the
 *                               reference CPU path (third_party/tfluids.cc:152-234,594-774), which the golden tests pin;
 *   TFL_ADVECT_FAST             the tolerance mode: trace end point = centre + displacement (no normalise / rescale round
 *                               trip), trilinear samples as contracted a + t (b - a), MacCormack correction in fp32.
 *                               Differs from the reference by a few ulp per cell; held to the north-star's rel-L2 <= 1e-5
 *                               by tests/test_hip_fullsize.py. Lanes off the fast path (obstacle neighbours, fast flow)
 *                               run the exact generic code in both modes. Per voxel: within the bound that
 *                               tests/advect_bound.py derives from this arithmetic (tens of 2^-24 of the LOCAL magnitude)
 *                               of the operator evaluated in fp64, and the exact mode's bits on the generic path
 *                               (tests/test_hip_advect_bound.py).
 * A context starts in the mode named by the environment variable TFL_ADVECT_MODE ("fast" | "exact"; unset = exact). */
enum { TFL_ADVECT_EXACT = 0, TFL_ADVECT_FAST = 1 };
int tfl_set_advect_mode(tfl_ctx* ctx, int mode);
int tfl_get_advect_mode(const tfl_ctx* ctx);
/* Blocks until the context's stream is idle (cutorch.synchronize(), simulate.lua:258). */
int tfl_synchronize(tfl_ctx* ctx);
/* Number of back-traces that hit one of calcLineTrace's invariant-violation paths since the last
 * call (the reference CPU build THErrors there, calc_line_trace.cc:325-330,410,421; its CUDA build
 * silently substitutes). Synchronises the stream. Diagnostic only. */
int64_t tfl_trace_errors(tfl_ctx* ctx);
/* EXPERIMENTS flavour of the library only (the product library counts nothing and reports 0, 0): blocks[0], blocks[1] = thread
 * blocks of pass A / pass B of the tiled 3-D advectScalar kernels whose staged tile held nothing but +0.0 and non-fluid cells
 * (they take the short path) since the last call. Synchronises the stream. Diagnostic only. */
int tfl_scal3_zero_blocks(tfl_ctx* ctx, int64_t* blocks);
/* EXPERIMENTS flavour of the library only (the product library reports zeros): what tfl_simulate_step did with the in-place
 * advectScalar of its density fields since the last call -- stats[0] = brick scans launched, stats[1] = steps
 * whose two passes ran over the lists of non-empty bricks, stats[2] = steps on the two full launches -- and, of the last scan,
 * stats[3] = |L_A| and stats[4] = |L_B| (bricks of 64 x 4 x 4 cells, summed over the batch). Synchronises the stream. Diagnostic only. */
int tfl_scal3_sparse_stats(tfl_ctx* ctx, int64_t* stats);

/* Built-in per-kernel timing, the analogue of tfluids.profilePressure (lib/simulate.lua:254-260,
 * 306-318) at kernel granularity: between begin and end every kernel this library launches from the
 * calling thread is bracketed by HIP events on its launch stream. tfl_profile_end synchronises,
 * writes a JSON object {"kernel": {"calls": n, "ms": total}, ...} into buf (truncated to cap) and
 * returns the number of distinct kernels, or a negative tfl_status. */
int tfl_profile_begin(tfl_ctx* ctx);
int tfl_profile_end(tfl_ctx* ctx, char* buf, int64_t cap);

/* ---- operators (one per row of SURVEY.md section 8b) ------------------------------------- */

/* init.lua:142-144 -> third_party/tfluids.cc:415-588 | tfluids.cu:524-633.
 * method: "euler" | "maccormack" | "eulerOurs" | "rk2Ours" | "rk3Ours" | "maccormackOurs"
 * (generic/advect_type.cc:18-37). boundaryWidth is parsed and ignored like the reference
 * (tfluids.cc:436,467: bnd = 1). s_dst must not alias s. */
int tfl_advectScalar(tfl_ctx* ctx, float dt, const tfl_tensor* s, const tfl_tensor* U,
                     const tfl_tensor* flags, const tfl_tensor* fwd, const tfl_tensor* bwd,
                     int is3D, const char* method, const tfl_tensor* fwdPos,
                     const tfl_tensor* bwdPos, int boundaryWidth, int sampleOutsideFluid,
                     float maccormackStrength, const tfl_tensor* sDst);

/* init.lua:212-213 -> third_party/tfluids.cc:776-920 | tfluids.cu:876-963.
 * rk2Ours / rk3Ours map to maccormackOurs like the reference (tfluids.cc:799-802). */
int tfl_advectVel(tfl_ctx* ctx, float dt, const tfl_tensor* U, const tfl_tensor* flags,
                  const tfl_tensor* fwd, const tfl_tensor* bwd, int is3D, const char* method,
                  int boundaryWidth, float maccormackStrength, const tfl_tensor* UDst);

/* init.lua:246 -> third_party/tfluids.cc:926-1002 | tfluids.cu:969-1046 (in place on U). */
int tfl_setWallBcsForward(tfl_ctx* ctx, const tfl_tensor* U, const tfl_tensor* flags, int is3D);

/* init.lua:278 -> third_party/tfluids.cc:1008-1066 | tfluids.cu:1052-1105. */
int tfl_velocityDivergenceForward(tfl_ctx* ctx, const tfl_tensor* U, const tfl_tensor* flags,
                                  const tfl_tensor* UDiv, int is3D);

/* norm[b] = || velocityDivergence(U, flags)[b] ||_2 for every batch item b, without the divergence field: what
 * lib/calc_stats.lua:98-118 records after every step of a rollout (div[i]:norm(), one host synchronisation per sample there).
 * Per cell the fp32 value is the bits tfl_velocityDivergenceForward writes; its square (exact in fp64) is accumulated in fp64
 * in a fixed order -- one sum per z-plane, then the planes in ascending z, then the root -- with no atomics, so a call gives
 * the same bits every time and batch item b's result does not depend on B. `norm` is DEVICE memory, B doubles; `workspace` is
 * device memory, 8-byte aligned, tfl_divergence_norm_workspace_floats(B, Z, Y, X) floats. Two launches on the context's
 * stream; no host read, no synchronisation, no allocation: the call can be captured into a HIP graph. Covers the whole array
 * like tfl_velocityDivergenceForward (tfl_set_z_window / tfl_set_z_origin are not read). No reference counterpart. */
int64_t tfl_divergence_norm_workspace_floats(int32_t B, int32_t Z, int32_t Y, int32_t X);
int tfl_velocityDivergenceNorm(tfl_ctx* ctx, const tfl_tensor* U, const tfl_tensor* flags, int is3D,
                               double* norm, float* workspace, int64_t workspace_floats);

/* ---- nn.FluidCriterion (lib/modules/fluid_criterion.lua, lib/modules/weighted_flat_mse_criterion.lua) ------------------------
 * tfl_criterion_weight: the border weight of fluid_criterion.lua:145-158 in one launch. Per cell it starts from the bits
 * tfl_signedDistanceField(flags, borderWidth) writes and applies, in fp32 with one rounding each and no contraction,
 *   c = min(max(sdf, 1), bw); c = c + (-1); c = c * (float)(-1.0 / (bw - 1)); c = c + 1; c = c * (float)(borderWeight - 1); w = c + 1.
 * A function of flags only: a scene computes it once. borderWidth must be an integer > 1 and borderWeight > 1 (:46, :63);
 * a borderWidth above 1024 is refused too (the search visits (2 borderWidth + 1)^3 cells per cell).
 *
 * tfl_fluidCriterion: loss[0..3] (DEVICE memory, 4 doubles) = {pLoss, uLoss, divLoss, (pLoss + uLoss) + divLoss} with
 *   term = lambda * (S / n),  S = the fp64 sum of z * z over the term's tensor,  n = its element count (1 when !sizeAverage),
 *   z = x - t (weight == NULL) or z = a - b, a = w * x, b = w * t in fp32 (the cell's weight for every channel of U); for the
 *   divergence term z = dv resp. w * dv, dv being the bits tfl_velocityDivergenceForward writes for the cell.
 * A term whose lambda is <= 0 is 0 and adds nothing to the gradients (fluid_criterion.lua:162-181, 199-235). The sums follow
 * tfl_velocityDivergenceNorm's discipline: one sum per (batch item, z-plane) in a fixed order, the planes in ascending (b, z),
 * no atomics -- the same bits every call, and batch item b's plane sums do not depend on B.
 * With gradP / gradU (both or neither) the same launch writes the gradients to pPred and UPred, in fp32:
 *   norm = sizeAverage ? (float)(2.0 / n) : 2.0f;  g = norm * z;  weighted: g = g * w;  g = g * (float)lambda;
 *   gradP = g_p;  gradU_c = (0.0f + g_u,c) + d_c,  d_c = what tfl_velocityDivergenceBackward gathers from gradOutput = g_div
 * (g_div is recomputed at the three -c neighbours from UPred, flags and weight: no divergence or gradOutput field is stored).
 * `workspace`: device memory, 8-byte aligned, tfl_fluid_criterion_workspace_floats(B, Z, Y, X) floats. Two launches on the
 * context's stream; no host read, no synchronisation, no allocation: the call can be captured into a HIP graph. Refused with
 * TFL_EINVAL before anything is written: shape mismatches (fluid_criterion.lua:86-99, 117-129), a gradient that overlaps an
 * input or the other gradient. Covers the whole array (tfl_set_z_window / tfl_set_z_origin are not read); there is no z-slab
 * form: it would need one 3-double all-reduce and is out of scope.
 * The MSE arithmetic of the reference lives in Torch7's nn / THNN, outside the reference tree: the element-wise order above is
 * this library's, chosen to follow the Lua call order; the tfluids pieces (SDF, divergence forward / backward) are the reference's. */
int tfl_criterion_weight(tfl_ctx* ctx, const tfl_tensor* flags, double borderWidth, double borderWeight, int is3D,
                         const tfl_tensor* weight);
int64_t tfl_fluid_criterion_workspace_floats(int32_t B, int32_t Z, int32_t Y, int32_t X);
int tfl_fluidCriterion(tfl_ctx* ctx, const tfl_tensor* pPred, const tfl_tensor* UPred, const tfl_tensor* pTarget,
                       const tfl_tensor* UTarget, const tfl_tensor* flags, const tfl_tensor* weight, double pLambda,
                       double uLambda, double divLambda, int sizeAverage, int is3D, double* loss, const tfl_tensor* gradP,
                       const tfl_tensor* gradU, float* workspace, int64_t workspace_floats);

/* The loss bookkeeping of the training closure (lib/run_epoch.lua:216-229, 287-291) without its host read. loss4: what
 * tfl_fluidCriterion wrote; sums5 (DEVICE memory, 5 doubles, zeroed by the caller at the start of an epoch) = the running sums
 * {pLoss, uLoss, divLoss, total, long-term total}; guard: one DEVICE word, zeroed by the caller.
 *   longTerm == 0 (the main pass):  sums5[0] += loss4[0]; sums5[1] += loss4[1]; sums5[2] += loss4[2]; sums5[3] += loss4[3]
 *   longTerm != 0:                  sums5[3] += loss4[3]; sums5[4] += loss4[3]
 * plain fp64 adds in this order, then *guard = 1 if loss4[3] is NaN or > errLimit (the reference: 1e9); a set guard is never
 * cleared here. One launch of one thread on the context's stream; no host read, no synchronisation: capturable. */
int tfl_closure_fold(tfl_ctx* ctx, const double* loss4, double* sums5, int32_t* guard, int longTerm, double errLimit);

/* init.lua:346 -> third_party/tfluids.cc:1072-1156 | tfluids.cu:1111-1195 (in place on U). */
int tfl_velocityUpdateForward(tfl_ctx* ctx, const tfl_tensor* U, const tfl_tensor* flags,
                              const tfl_tensor* p, int is3D);

/* init.lua:428-429 -> third_party/tfluids.cc:1341-1458 | tfluids.cu:1355-1497 (in place on U).
 * curl always has 3 channels (tfluids.cc:1363). */
int tfl_vorticityConfinement(tfl_ctx* ctx, const tfl_tensor* U, const tfl_tensor* flags,
                             float strength, const tfl_tensor* centered, const tfl_tensor* curl,
                             const tfl_tensor* curlNorm, const tfl_tensor* force, int is3D);
/* The same operator out of place: U = USrc + confinement(USrc), every cell of U (of the z-window) written; U must not alias
 * USrc. On a 3-D grid of 2 M cells per batch item or more (64+ planes deep) this is ONE fused z-marched launch that keeps the centred velocities,
 * curl and |curl| in LDS (vorticity.hip k_vort_pipe, or k_vort_fused where the device cannot hold its block: 72 -> ~30 bytes
 * per cell of HBM traffic; TFL_VORT_FUSED=1|0 in the environment forces the route), bit-equal to tfl_vorticityConfinement;
 * smaller and 2-D grids run the two launches reading USrc and writing U (or, misaligned, copy first), for which curl (3
 * channels) / curlNorm are the scratch -- under a z-window that route needs its curl on a window one plane wider each way,
 * which tfl_simulate_step_slab arranges with tfl_set_stages; a host of its own should window only the fused route.
 * tfl_simulate_step uses the entry to fold simulate()'s `U:copy(advected)` and the confinement into one pass. No reference
 * counterpart (the reference op is in place). */
int tfl_vorticityConfinementFrom(tfl_ctx* ctx, const tfl_tensor* USrc, const tfl_tensor* U, const tfl_tensor* flags,
                                 float strength, const tfl_tensor* curl, const tfl_tensor* curlNorm, int is3D);

/* init.lua:469 -> third_party/tfluids.cc:1162-1233 | tfluids.cu:1201-1273 (in place on U).
 * gravity: 3 floats in HOST memory (the Lua wrapper passes a 3-element tensor, init.lua:455-458);
 * strengthTmp (a 3-float device scratch in the reference, tfluids.cu:1261-1265) is accepted and
 * unused: the strength travels as kernel arguments. */
int tfl_addBuoyancy(tfl_ctx* ctx, const tfl_tensor* U, const tfl_tensor* flags,
                    const tfl_tensor* density, const float gravity[3], float* strengthTmp,
                    float dt, int is3D);

/* tfl_addBuoyancy out of place: U = USrc + buoyancy(flags, density), every cell of U written. simulate() uses it
 * with USrc = advectVel's output buffer, which makes the reference's `U:copy(UDst)` after the advection
 * (init.lua:216-218) part of this pass instead of a sweep of its own. USrc == U is tfl_addBuoyancy. */
int tfl_addBuoyancyFrom(tfl_ctx* ctx, const tfl_tensor* USrc, const tfl_tensor* U, const tfl_tensor* flags,
                        const tfl_tensor* density, const float gravity[3], float dt, int is3D);

/* init.lua:505 -> third_party/tfluids.cc:1239-1306 | tfluids.cu:1279-1349 (in place on U). */
int tfl_addGravity(tfl_ctx* ctx, const tfl_tensor* U, const tfl_tensor* flags,
                   const float gravity[3], float dt, int is3D, float* forceTmp);

/* The three force operators with PER-ITEM strengths (not in the reference; what tfl_simulate_step_items runs): batch item b gets
 * the force of the single-item operator called on item b alone with the b-th entry, in ONE launch per operator for the whole
 * batch (vorticityConfinement: its two). n_items must equal flags->B and be at most TFL_MAX_ITEMS: the strengths travel by value
 * in the kernel arguments. on: n_items words, non-zero = the item has the force (NULL: every item has). An item without it is
 * not touched, bit for bit (the operator is not run with a zero strength: x + 0 * f would turn -0 into +0 and a NaN force into
 * NaN) -- with one exception: tfl_addBuoyancyItems with USrc != U (USrc NULL or == U: in place) writes every cell of U like
 * tfl_addBuoyancyFrom, and copies such an item. gravity: n_items x 3 floats in HOST memory, each row what tfl_addBuoyancy /
 * tfl_addGravity take; strength: n_items floats in host memory, each what tfl_vorticityConfinement takes. The per-cell arithmetic
 * is the single-item kernels', operation for operation. tfl_vorticityConfinementItems always runs the two launches (curl, then the
 * force, which equal the fused forms bit for bit); curl (3 channels) / curlNorm are scratch of the flags' size. A z-window or
 * stage mask set on the context is refused by name. */
#define TFL_MAX_ITEMS 32
int tfl_addBuoyancyItems(tfl_ctx* ctx, const tfl_tensor* USrc, const tfl_tensor* U, const tfl_tensor* flags,
                         const tfl_tensor* density, const float* gravity, const int32_t* on, int32_t n_items, float dt, int is3D);
int tfl_addGravityItems(tfl_ctx* ctx, const tfl_tensor* U, const tfl_tensor* flags, const float* gravity, const int32_t* on,
                        int32_t n_items, float dt, int is3D);
int tfl_vorticityConfinementItems(tfl_ctx* ctx, const tfl_tensor* U, const tfl_tensor* flags, const float* strength,
                                  const int32_t* on, int32_t n_items, const tfl_tensor* curl, const tfl_tensor* curlNorm,
                                  int is3D);

/* init.lua:552 -> generic/tfluids.cc:136-167 | generic/tfluids.cu:314-353. */
int tfl_emptyDomain(tfl_ctx* ctx, const tfl_tensor* flags, int is3D, int bnd);

/* init.lua:574 -> generic/tfluids.cc:173-210 | generic/tfluids.cu:355-397. Cells that are neither
 * exactly Fluid nor Obstacle become -1 (the CUDA behaviour); the CPU reference raises there. */
int tfl_flagsToOccupancy(tfl_ctx* ctx, const tfl_tensor* flags, const tfl_tensor* occupancy);

/* init.lua:583-595 `tfluids.rectangularBlur(src, blurRad, is3D, dst)` -> generic/tfluids.cc:642-760 (CPU only in the
 * reference): separable box blur of radius blurRad with clamped edges over every [B][C] field, each line a running sum
 * in the reference's order (bit-exact). tmp: scratch of src's size (the Lua wrapper's getTempStorage). */
int tfl_rectangularBlur(tfl_ctx* ctx, const tfl_tensor* src, int blurRad, int is3D, const tfl_tensor* dst,
                        const tfl_tensor* tmp);
/* init.lua:603-613 `tfluids.signedDistanceField(flags, searchRad, is3D, dst)` -> generic/tfluids.cc:766-821 |
 * generic/tfluids.cu:690-747: distance to the nearest obstacle cell within a (2 searchRad + 1)^dim window, clamped to
 * searchRad, 0 inside obstacles (the loss weighting of lib/modules/fluid_criterion.lua:149). */
int tfl_signedDistanceField(tfl_ctx* ctx, const tfl_tensor* flags, int searchRad, int is3D, const tfl_tensor* dst);

/* init.lua:645-677 `tfluids.solveLinearSystemPCG(p, flags, div, is3D, tol, maxIter, precondType, verbose)` ->
 * tfluids_CudaMain_solveLinearSystemPCG, generic/tfluids.cu:1257-1759 (CUDA only in the reference; the baseline
 * "exact" pressure solver and the accuracy yard-stick of the paper). p is zeroed, then every connected fluid
 * component (generic/find_connected_fluid_components.cc) of every batch element is solved by (P)CG from x = 0 with
 * the Laplacian of setupLaplacian (generic/tfluids.cu:904-1093), the component's mean is removed and the result
 * scattered into p; components of one cell are skipped, of fewer than five use no preconditioner.
 * precondType: "none" | "ilu0" | "ic0" | "mg" (init.lua default "ic0"); tol (default 1e-6) on ||r||; maxIter (default
 * 1000); *residual = max over the solves of the final ||r|| (-inf if there was nothing to solve).
 * The reference keeps its temporaries in the tfluids._tmpPCG table; here the caller passes a workspace of
 * tfl_pcg_workspace_floats_for(Z, Y, X, precondType) floats (8-byte aligned; tfl_pcg_workspace_floats(Z, Y, X) is that number
 * for "none" | "ilu0" | "ic0", the _for form returns -1 for a name that is no preconditioner). Synchronises the stream (as the reference does after
 * every dot product). On 3-D grids the IC(0) / ILU(0) triangular solves run as pipelined wavefronts whose sub-boxes wait
 * for each other (all of them must be resident on the GPU at once); if one times out (~1 s: something else holds part of
 * the GPU) the solve is repeated with one launch per hyperplane. TFL_PCG_HYPERPLANES=1 in the environment selects that
 * schedule from the start. "mg" is not in the reference: one symmetric V-cycle of aggregation multigrid per CG iteration
 * (damped Jacobi, piecewise-constant prolongation, Galerkin coarse operators, matrix-free from the flags) in which no block
 * waits for another one, so it has no such fallback; deterministic. Iterations and times measured so far: profiles/pcg_mg.md.
 * tfl_pcg_last_iterations: the CG iterations of the last tfl_solveLinearSystemPCG on this context that returned TFL_OK, summed
 * over its component solves (the iteration counter of each at exit); -1 before any solve.
 * Returns TFL_EINVAL for a fluid cell on the domain border (the reference raises). */
int64_t tfl_pcg_workspace_floats(int32_t Z, int32_t Y, int32_t X);
int64_t tfl_pcg_workspace_floats_for(int32_t Z, int32_t Y, int32_t X, const char* precondType);
int64_t tfl_pcg_last_iterations(tfl_ctx* ctx);
int tfl_solveLinearSystemPCG(tfl_ctx* ctx, const tfl_tensor* p, const tfl_tensor* flags, const tfl_tensor* div,
                             int is3D, const char* precondType, float tol, int maxIter, int verbose,
                             float* workspace, int64_t workspace_floats, float* residual);

/* tfl_solveLinearSystemPCG with every batch element advancing in the SAME launches (not in the reference): the c-th connected
 * component of every element is solved at once, for c = 0 .. the largest component count - 1, so a CG iteration of the batch
 * is as many launches as a CG iteration of one element and the host waits for the stream once per chunk of iterations, not
 * once per element and component. For every element b, p[b], residuals[b] and iterations[b] are bit for bit what
 * tfl_solveLinearSystemPCG gives for that element alone with the same precondType, tol and maxIter (residuals[b] = -inf where
 * nothing was solved); tfl_pcg_last_iterations afterwards is the sum of iterations[]. residuals / iterations: host arrays
 * of B entries, either may be NULL. precondType: "mg" | "none"; "ilu0" and "ic0" are refused with TFL_EUNSUPPORTED (their
 * wavefront sweeps wait for each other and do not batch), any other name with TFL_EINVAL. workspace:
 * tfl_pcg_batched_workspace_floats(B, Z, Y, X, precondType) floats, 8-byte aligned (-1 for any name but "mg" | "none").
 * p is zeroed first; a fluid cell on the border of any element is refused with TFL_EINVAL before any CG launch (the message
 * names the first such element, counted from 0). Synchronises the stream. */
int64_t tfl_pcg_batched_workspace_floats(int32_t B, int32_t Z, int32_t Y, int32_t X, const char* precondType);
int tfl_solveLinearSystemPCGBatched(tfl_ctx* ctx, const tfl_tensor* p, const tfl_tensor* flags, const tfl_tensor* div,
                                    int is3D, const char* precondType, float tol, int maxIter, float* workspace,
                                    int64_t workspace_floats, float* residuals, int64_t* iterations);

/* init.lua:747-764 `tfluids.normalizePressureMean(p, flags, is3D)` -> tfluids_<Real>Main_normalizePressureMean,
 * generic/tfluids.cc:845-925 (CPU only in the reference: CUDA tensors are copied to the host and back): subtracts
 * from p, per batch element, the mean of p over each connected component of fluid cells (non-fluid cells untouched).
 * Runs on the device here (the component labelling of tfl_solveLinearSystemPCG). The reference's `inds` IntTensor
 * temp becomes a workspace of tfl_normalize_workspace_floats(Z, Y, X) floats, 8-byte aligned. */
int64_t tfl_normalize_workspace_floats(int32_t Z, int32_t Y, int32_t X);
int tfl_normalizePressureMean(tfl_ctx* ctx, const tfl_tensor* p, const tfl_tensor* flags, int is3D, float* workspace,
                              int64_t workspace_floats);

/* init.lua:726-727 -> generic/tfluids.cu:1765-1927 (the reference has no CPU version).
 * p is overwritten (initial guess is zero like the reference, :1869-1872). pPrev is scratch;
 * pDelta / pDeltaNorm are accepted and unused (the residual is reduced on the fly). The final
 * residual max_b ||p - pPrev||_2 is written to *residual when non-NULL (one host sync at the
 * end; every iteration when pTol > 0, like the reference's maxall at :1886). */
int tfl_solveLinearSystemJacobi(tfl_ctx* ctx, const tfl_tensor* p, const tfl_tensor* flags,
                                const tfl_tensor* div, const tfl_tensor* pPrev,
                                const tfl_tensor* pDelta, const tfl_tensor* pDeltaNorm, int is3D,
                                float pTol, int maxIter, int verbose, float* residual);

/* ---- training-side callers and the multi-resolution resampler --------------------- */
/* init.lua:310-313 -> generic/tfluids.cc:49-130 | generic/tfluids.cu:224-291. gradU is overwritten. */
int tfl_velocityDivergenceBackward(tfl_ctx* ctx, const tfl_tensor* U, const tfl_tensor* flags,
                                   const tfl_tensor* gradOutput, int is3D, const tfl_tensor* gradU);
/* init.lua:358-383 -> generic/tfluids.cc:216-344 | generic/tfluids.cu:407-513. gradP is overwritten; each word
 * gathers its contributions in the reference's serial order (deterministic; the reference scatters atomically). */
int tfl_velocityUpdateBackward(tfl_ctx* ctx, const tfl_tensor* U, const tfl_tensor* flags, const tfl_tensor* p,
                               const tfl_tensor* gradOutput, int is3D, const tfl_tensor* gradP);
/* tfluids.SetWallBcs:updateGradInput (tfluids/set_wall_bcs.lua:50-66): gradU = mask * gradOutput with mask =
 * setWallBcsForward(ones, flags), i.e. the forward operator applied to the incoming gradient (the module's own comment:
 * "copy the gradOutput and treat it as an input velocity and call the forward function"); the gradient w.r.t. flags is
 * zero. gradU may alias gradOutput. */
int tfl_setWallBcsBackward(tfl_ctx* ctx, const tfl_tensor* flags, const tfl_tensor* gradOutput, int is3D,
                           const tfl_tensor* gradU);
/* init.lua:618-627 -> generic/tfluids.cc:509-633 | generic/tfluids.cu:516-686. */
int tfl_volumetricUpSamplingNearestForward(tfl_ctx* ctx, int ratio, const tfl_tensor* input,
                                           const tfl_tensor* output);
int tfl_volumetricUpSamplingNearestBackward(tfl_ctx* ctx, int ratio, const tfl_tensor* input,
                                            const tfl_tensor* gradOutput, const tfl_tensor* gradInput);

/* ---- the pressure-projection ConvNet (lib/model.lua `default` model, forward only) ---------- */
/* In the reference the projection is `model:forward({pDiv, UDiv, flags})` on an nngraph of cudnn
 * convolutions and tfluids nn.Modules (lib/simulate.lua:262-272, lib/model.lua:27-401), not a
 * tfluids op, so the boundary here is one "model" object + one forward call. */
typedef struct tfl_model tfl_model;

/* Builds the `default` topology: nlayers convolutions (stride 1, zero pad (k-1)/2, cross-correlation,
 * lib/model_utils.lua:80-116), ReLU after all but the last; input channels {pDiv/scale, div/scale,
 * occupancy} (cin[0] must be 3; other input sets: tfl_model_create_opts), cout[nlayers-1] must be 1; at most 64 channels per layer. weights[l] is HOST memory laid out like
 * cudnn.{Spatial,Volumetric}Convolution.weight: [cout][cin][k(z)][k(y)][k(x)] (no z for 2-D);
 * biases[l] is [cout]. The model copies and re-lays-out the weights; the caller keeps ownership.
 * Returns NULL on error (see tfl_last_error). */
tfl_model* tfl_model_create(tfl_ctx* ctx, int is3D, int nlayers, const int32_t* cin, const int32_t* cout,
                            const int32_t* ksize, const float* const* weights,
                            const float* const* biases);
/* The same with the two extra per-layer knobs of lib/model.lua's layer tables (:163-178, :211-218): pool[l] = psize
 * (2: cudnn 2x average pooling after the layer's ReLU, model_utils.lua:184-208) and up[l] = usize (2: the layer is an
 * nn.{Spatial,Volumetric}ConvolutionUpsample, lib/modules/{spatial,volumetric}_convolution_upsample.lua -- weights[l] then has
 * cout[l] * 2^dim output channels, channel index = o * 2^dim + sub-position, and the result is pixel-shuffled to twice
 * the resolution). NULL = all 1. This covers the `tog` model types (2-D: 16,32,32,64,64,32,1 with k 5,5,5,5,1,1,3;
 * 3-D: 16,16,16,16,32,32,1 with k 3,3,3,3,1,1,3); such models run through the shape-generic kernels, and the grid
 * must be divisible by the product of the pooling factors. */
tfl_model* tfl_model_create_ex(tfl_ctx* ctx, int is3D, int nlayers, const int32_t* cin, const int32_t* cout,
                               const int32_t* ksize, const int32_t* pool, const int32_t* up,
                               const float* const* weights, const float* const* biases);
/* The mconf switches of lib/model.lua:27-160, 356-387 that change the FORWARD graph (fields of torch/lib/default_conf.lua:
 * 60-100 with the same meaning; the defaults there are what tfl_model_create[_ex] builds and what NULL means here):
 *   in_pDiv / in_UDiv / in_div  inputChannels (flags always feed the net, model.lua:81); the net input is the join, in this
 *                               order, of pDiv/scale, SetWallBcs(UDiv)/scale (2 or 3 channels), div/scale, occupancy
 *                               (model.lua:130-148), so cin[0] = in_pDiv + in_UDiv*(2|3) + in_div + 1
 *   normalize, norm_chan, norm_func  normalizeInput / normalizeInputChan / normalizeInputFunc: scale = per-sample 'std'
 *                               (n-1) or 'norm' (l2) of SetWallBcs(UDiv), pDiv or div; 0 = no scaling
 *   nonlin                      nonlinType after every layer but the last (model_utils.lua:20-34)
 *   pressure_skip               addPressureSkip: pDiv/scale joins the input of the LAST layer as its last channel
 *                               (model.lua:356-360): cin[nlayers-1] = cout[nlayers-2] + 1
 * Models with non-default options run through the shape-generic kernels and are not available to the z-slab step. */
enum { TFL_NORM_UDIV = 0, TFL_NORM_PDIV = 1, TFL_NORM_DIV = 2 };
enum { TFL_NORMFUNC_STD = 0, TFL_NORMFUNC_L2 = 1 };
enum { TFL_NONLIN_RELU = 0, TFL_NONLIN_RELU6 = 1, TFL_NONLIN_SIGMOID = 2 };
typedef struct tfl_model_opts {
  int32_t in_pDiv, in_UDiv, in_div;
  int32_t normalize;
  int32_t norm_chan;
  int32_t norm_func;
  int32_t nonlin;
  int32_t pressure_skip;
} tfl_model_opts;
tfl_model* tfl_model_create_opts(tfl_ctx* ctx, int is3D, int nlayers, const int32_t* cin, const int32_t* cout,
                                 const int32_t* ksize, const int32_t* pool, const int32_t* up,
                                 const float* const* weights, const float* const* biases, const tfl_model_opts* opts);
/* Every projection net lib/model.lua's defineModelGraph builds from mconf (model.lua:253-392): the knobs above plus
 * resolution or dilated banks, their join, batch norm and max pooling.
 *   Conv modules are listed in the reference's creation order: the stages before banksSplitStage, then for every banked
 *   stage lid in [split, join) bank 1..banks_num, then the remaining stages. pool / up are per conv module (NULL = all 1);
 *   every bank of a stage must have bank 1's shape.
 *   banks_num > 1 splits before stage `split_stage` and joins before `join_stage` (1-based, 1 <= split < join < #stages):
 *     TFL_BANKS_MRES: bank i starts from 2x average pooling of bank i-1 (a cascade), and is upsampled nearest by 2^(i-1)
 *                     at the join; TFL_BANKS_DILATE: every bank starts from the same tensor and bank i's convolutions
 *                     have dilation 2^(i-1), zero padding 2^(i-1)*(k-1)/2 (their up must be 1).
 *     TFL_AGG_CONCAT: nn.JoinTable -- bank 1's channels first, the join stage takes cout * banks_num inputs;
 *     TFL_AGG_ADD:    nn.CAddTable -- ((b1 + b2) + b3) ... in fp32, bank order.
 *   pool_type: the psize > 1 pooling is average (TFL_POOL_AVG) or max (TFL_POOL_MAX); the mres pyramid is average always.
 *   batch_norm (addBatchNorm): one inference-form BN module per hidden conv module (after its non-linearity and pooling),
 *     in the same order: y = (x - mean[c]) / sqrt(var[c] + eps) * weight[c] + bias[c]. bn_weight / bn_bias NULL (or a NULL
 *     entry) = not affine (weight 1, bias 0). The library folds each module on the host, in double, into one scale and
 *     one shift per channel, each rounded once to fp32, and applies y = fmaf(x, scale, shift) in the launch that writes
 *     the stage's output (the conv, or the pooling when the stage pools): no launch of its own.
 * graph = NULL, or one bank without BN and with average pooling, builds exactly what tfl_model_create_opts builds. Other
 * graphs run through the shape-generic kernels, un-sharded: tfl_simulate_step_slab refuses them (TFL_EUNSUPPORTED), and
 * the grid must be divisible by the model's largest downsampling factor (the mres pyramid times the pooling). */
enum { TFL_BANKS_MRES = 0, TFL_BANKS_DILATE = 1 };
enum { TFL_AGG_CONCAT = 0, TFL_AGG_ADD = 1 };
enum { TFL_POOL_AVG = 0, TFL_POOL_MAX = 1 };
typedef struct tfl_model_graph {
  int32_t banks_num;                 /* banksNum (1 = no banks; at most 8) */
  int32_t bank_type;                 /* banksType: TFL_BANKS_* */
  int32_t aggregate;                 /* banksAggregateMethod: TFL_AGG_* */
  int32_t split_stage, join_stage;   /* banksSplitStage / banksJoinStage (1-based) */
  int32_t pool_type;                 /* poolType: TFL_POOL_* */
  int32_t batch_norm;                /* addBatchNorm: 1 = the bn_* arrays hold one entry per hidden conv module */
  const float* const* bn_mean;       /* running_mean[cout] */
  const float* const* bn_var;        /* running_var[cout] */
  const float* const* bn_weight;     /* weight[cout], or NULL (batchNormAffine = false) */
  const float* const* bn_bias;       /* bias[cout], or NULL */
  const double* bn_eps;              /* eps of each module */
} tfl_model_graph;
tfl_model* tfl_model_create_graph(tfl_ctx* ctx, int is3D, int nconv, const int32_t* cin, const int32_t* cout,
                                  const int32_t* ksize, const int32_t* pool, const int32_t* up,
                                  const float* const* weights, const float* const* biases, const tfl_model_opts* opts,
                                  const tfl_model_graph* graph);
void tfl_model_destroy(tfl_ctx* ctx, tfl_model* model);
/* The 3-D default topology's convolution stack runs as a split-operand fp16 MFMA implicit GEMM (csrc/conv_mfma16.hip):
 * every fp32 operand travels as two fp16 halves, which ends at |x| = 65504. An activation above that is clamped and the
 * forward pass counts it; this returns the number of thread blocks that clamped since the last call and resets the
 * count (synchronises the context's stream). 0 for every working simulation: the net's input is divided by the
 * velocity's standard deviation. Always 0 on the fp32 paths (TFL_CONV_PATH=winograd|mfma|direct). -1 on error. */
int64_t tfl_model_range_errors(tfl_ctx* ctx, tfl_model* model);
/* The same count WITHOUT a stream synchronisation, as far as the device has reported it: the projection kernel at the end of
 * a forward pass copies a non-zero count into pinned host memory, and this reads that word (not reset; tfl_model_range_errors
 * resets it). While it is non-zero, tfl_model_forward / tfl_model_begin / tfl_simulate_step[_slab] return TFL_ERANGE instead
 * of stepping on from a clamped pressure -- the reference's fp32 cuDNN would have carried values up to 3e38; create the model
 * under TFL_CONV_PATH=winograd for a strict-fp32 stack without a range limit. 0 on the fp32 paths. -1 on error. */
int64_t tfl_model_range_flag(tfl_ctx* ctx, tfl_model* model);
/* Scratch floats tfl_model_forward needs for a [B][.][Z][Y][X] grid. */
int64_t tfl_model_workspace_floats(const tfl_model* model, int B, int Z, int Y, int X);
/* {pOut, UOut} = model:forward({pDiv, UDiv, flags}) (lib/model.lua:398, 421-450). Inputs are not
 * modified; pOut may alias pDiv and UOut may alias UDiv (simulate.lua:270-272 copies the prediction
 * back into the state, which this makes free). When UBC/UBCInvMask are non-NULL the tail of
 * simulate() -- U = U*UBCInvMask + UBC and, if doClamp, clamp(U, lo, hi) (simulate.lua:321-326) -- is
 * fused into the last kernel. UDiv is read again by that last kernel (unless it lies inside `workspace`): it must not be
 * written by anyone else while the call is in flight on the stream. */
int tfl_model_forward(tfl_ctx* ctx, tfl_model* model, const tfl_tensor* pDiv, const tfl_tensor* UDiv,
                      const tfl_tensor* flags, const tfl_tensor* pOut, const tfl_tensor* UOut,
                      float* workspace, int64_t workspace_floats, const tfl_tensor* UBC,
                      const tfl_tensor* UBCInvMask, int doClamp, float lo, float hi);

/* The same forward in two halves, for z-slab decomposition (BASELINE config 5): `begin` applies the
 * wall BCs, computes the divergence and reduces sum(u), sum(u^2) of SetWallBcs(UDiv) over the owned
 * z-planes [zlo, zhi) into stats[2*B] (device doubles; NULL = the model's internal buffer); the caller
 * all-reduces stats across ranks; `finish` runs the rest with `count` = the GLOBAL number of velocity
 * samples per batch item (C*Z*Y*X of the whole grid). tfl_model_forward == begin(0, Z) + finish.
 * Models created with non-default tfl_model_opts (another normaliser channel / function, normalisation off) form their
 * scale from statistics the model computes itself inside `finish` over the whole array when stats = NULL (`count` is then
 * not used). A caller that passes `stats` has formed the (sum, sum of squares | 0, sum of squares | 0, 1) pair and its
 * `count` itself (std | l2 norm with count 2 | none with count 2): a z-slab rank does so over its owned planes, and a
 * windowed / staged `finish` of such a model requires it. */
int tfl_model_begin(tfl_ctx* ctx, tfl_model* model, const tfl_tensor* UDiv, const tfl_tensor* flags,
                    const tfl_tensor* UOut, float* workspace, int64_t workspace_floats, int zlo, int zhi,
                    double* stats);
int tfl_model_finish(tfl_ctx* ctx, tfl_model* model, const tfl_tensor* pDiv, const tfl_tensor* flags,
                     const tfl_tensor* pOut, const tfl_tensor* UOut, float* workspace,
                     int64_t workspace_floats, const double* stats, double count, const tfl_tensor* UBC,
                     const tfl_tensor* UBCInvMask, int doClamp, float lo, float hi);

/* ---- the training side of the projection ConvNet: the reference's closure is model:forward, crit:forward / :backward,
 * model:backward (lib/run_epoch.lua:207-235, 269-293); tfl_fluidCriterion is the middle, these are the two ends. For linear
 * models (tfl_model_create[_ex|_opts]) whose layers neither pool nor upsample -- `default`, `yang`, custom layer tables, every
 * tfl_model_opts switch -- and for banked models (tfl_model_create_graph: banksNum 2 .. 8, 'mres' or 'dilate' banks, 'concat' or
 * 'add' joins, any legal split / join stage) that hold no batch norm and whose modules neither pool nor upsample. Graph models
 * with batch norm (it needs a training-mode forward), models with pooling / ConvolutionUpsample layers (`tog`, banked or not)
 * and a module the weight-gradient kernel's tile cannot hold at its tap spacing are refused with TFL_EUNSUPPORTED before
 * anything is written, and the size queries answer -1 for them -- a LINEAR model with pooling / ConvolutionUpsample layers
 * until tfl_model_enable_multires_training (below) has been called on it, from then on it trains like the others.
 * tfl_model_backward gives the parameter gradients (the reference computes a
 * gradInput and run_epoch.lua discards it); tfl_model_backward_input also gives the gradients to pDiv and UDiv, for training
 * through the net (an iterated projection, a loss behind a refinement pass, differentiable code in front of it). There is no
 * gradient to flags. */

/* New weights into an existing model: host pointers laid out as for tfl_model_create. Every re-layout the model's path holds
 * (the [tap][cin][cout] form, the MFMA fragments, the Winograd transform, the tail packs, the data-gradient forms) is redone into
 * the buffers it already has, by the code that filled them at creation. Synchronous: waits for the context's stream, copies,
 * and returns with the new weights in place -- what an optimiser step calls; legal between two tfl_simulate_step calls. A
 * tfl_slab_graph recorded with this model holds per-layer constants of the OLD weights by value: the model does not know its
 * graphs, so the caller destroys and re-records them after this call. */
int tfl_model_set_weights(tfl_ctx* ctx, tfl_model* model, const float* const* weights, const float* const* biases);
/* Opt-in: gives a linear model (tfl_model_create[_ex|_opts]) with 2x average pooling and / or ConvolutionUpsample layers -- the
 * `tog` layer tables, custom ones -- its training pass. Builds, from the weights the model holds, the data-gradient form of every
 * layer (an upsample layer's for each of its up^dim sub-positions), the first layer's padded form and the zero bias; afterwards
 * the three size queries, tfl_model_forward_train, tfl_model_backward, tfl_model_backward_input, tfl_model_set_weights[_device]
 * and the tfl_optim_* entries take the model as they take `default`. The tape then also keeps every pooling layer's pooled
 * output; in the backward a pooling layer's gradient goes back through the pool and its activation mask in one pass,
 * g_pre[fine] = act'(y[fine]) g[fine >> 1] / 2^dim, an upsample layer's weight gradient reads the gradient where the pixel
 * shuffle put it (the mask is taken behind the shuffle) and its data gradient adds the sub-positions' transposed convolutions in
 * one launch, in a fixed order. Until the call nothing changes: the model is refused as before. A model that has a training
 * pass already: TFL_OK, nothing done. Refused with TFL_EUNSUPPORTED, by name and before anything is allocated or written: graph
 * models (tfl_model_create_graph with banks, max pooling or batch norm), a layer the weight-gradient kernel's tile cannot hold,
 * more than 32 layers. Synchronous (waits for the context's stream and reads the weights back once); not capturable. */
int tfl_model_enable_multires_training(tfl_ctx* ctx, tfl_model* model);
/* Floats of the tape tfl_model_forward_train fills for a [B][.][Z][Y][X] grid (-1: the model has no training pass). */
int64_t tfl_model_tape_floats(const tfl_model* model, int B, int Z, int Y, int X);
/* tfl_model_forward (without its fused UBC / clamp tail) that also keeps what the backward pass reads in `tape` (device,
 * 8-byte aligned): the per-item input scale, the net input, every layer's post-activation output with the joined skip channel;
 * for a banked model every module's output at its bank's resolution, the 'mres' pyramid levels and the join's output (its
 * outputs are tfl_model_forward's of the same model, bit for bit).
 * Always evaluated on the shape-generic fp32 kernels -- the exact fmaf chain, no fp16 and hence no range gate -- whatever
 * path the model was created on: the outputs are those of the same model created under TFL_CONV_PATH=direct, bit for bit.
 * workspace: tfl_model_workspace_floats. A short tape or workspace is TFL_EINVAL with nothing written. */
int tfl_model_forward_train(tfl_ctx* ctx, tfl_model* model, const tfl_tensor* pDiv, const tfl_tensor* UDiv,
                            const tfl_tensor* flags, const tfl_tensor* pOut, const tfl_tensor* UOut, float* workspace,
                            int64_t workspace_floats, float* tape, int64_t tape_floats);
/* Scratch floats tfl_model_backward needs (-1: the model has no training pass). */
int64_t tfl_model_backward_workspace_floats(const tfl_model* model, int B, int Z, int Y, int X);
/* model:backward for the parameters: from gradP / gradU at the model's outputs (either may be NULL = zero) and the tape of
 * the forward pass, gradWeights[l] / gradBiases[l] (DEVICE arrays, laid out like the weights of tfl_model_create). At the
 * last layer's output, per batch item with its input scale,
 *   g = scale gradP + velocityUpdateBackward(scale setWallBcsBackward(gradU))
 * then per layer from the last to the first g_pre = g (.) act'(y), gradBias = sum g_pre, gradWeight[co][ci][tap] =
 * sum x[ci][pos + tap] g_pre[co][pos], and g = conv(g_pre, W transposed and mirrored) for the layer in front.
 * A banked model: at the join every bank gets its channel slice ('concat') or all channels ('add') of g, an 'mres' bank the sum
 * over the block of cells the nearest up-sample replicated; each bank runs the per-layer step on its own grid at its tap
 * spacing; at the split the banks' gradients are added, 'mres' through the transpose of the 2x average pooling. Fixed-order
 * sums, no atomics: the same inputs give the same bits.
 * accumulate = 0 overwrites; 1 adds the fresh gradient, rounded to fp32, onto what is there with one fp32 add per element
 * (Torch's accGradParameters). Sums over voxels run in a fixed order (fp32 fmaf inside a 32 x 8 tile, fp64 across tiles and
 * blocks, no atomics): the same inputs give the same bits on every call. No host read, no stream synchronisation; capturable.
 * Sizes are checked before the first launch: a short tape or workspace is TFL_EINVAL with nothing written. */
int tfl_model_backward(tfl_ctx* ctx, tfl_model* model, const tfl_tensor* flags, const tfl_tensor* gradP,
                       const tfl_tensor* gradU, const float* tape, int64_t tape_floats, float* workspace,
                       int64_t workspace_floats, float* const* gradWeights, float* const* gradBiases, int accumulate);
/* Scratch floats tfl_model_backward_input needs (-1: the model has no training pass): tfl_model_backward's and, behind them,
 * the first layer's data gradient, the skip channel's, and the partial sums of the scale's gradient. */
int64_t tfl_model_backward_input_workspace_floats(const tfl_model* model, int B, int Z, int Y, int X);
/* tfl_model_backward that also returns the gradients to the net's inputs: gradPDiv [B][1] and gradUDiv [B][C] (device,
 * overwritten; either may be NULL) from the same gradP / gradU and tape. pDiv and UDiv are the tensors the forward was given,
 * UOut the U it wrote. gradWeights and gradBiases may BOTH be NULL (input gradients only); where given, the parameter
 * gradients are bit for bit those of tfl_model_backward on the same tape. The tape is tfl_model_forward_train's, unchanged.
 * With s the item's input scale, q = 1 / s, U_bc = SetWallBcs(UDiv), d its divergence, h = s SetWallBcs(gradU):
 *   g_x     the first layer's data gradient (its weights transposed and mirrored), g_skip the joined skip channel's
 *   g_a     h where velocityUpdate keeps its velocity input, 0 where it overwrites it -- the true derivative (the reference's
 *           tfluids.VelocityUpdate module passes zero to its velocity input; the net's input gradient does not)
 *   g_s     sum gradP pPred + q sum gradU UOut - q [sum (g_x[p] + g_skip) q pDiv + sum (g_x[U] + g_a) q U_bc + sum g_x[d] q d],
 *           one fp64 number per item: the scale depends on the inputs, and for most models that is most of gradUDiv
 *   gradPDiv = q (g_x[p] + g_skip) [+ g_s ds/dpDiv]
 *   gradUDiv = SetWallBcs(q (g_x[U] + g_a) + D^T(q g_x[d] [+ g_s ds/dd]) [+ g_s ds/dU_bc])
 *   ds/dsrc = (src - mean) / ((n - 1) s) for std, src / s for the l2 norm, at the field normalizeInputChan names
 * gradPDiv is exactly zero for a model with neither the pDiv channel, nor the skip, nor a pDiv normaliser. The sums of g_s run
 * in a fixed order (fp32 products, fp64 sums, one partial per block at a fixed place, no atomics): the same inputs give the same
 * bits on every call. Four to five launches more than tfl_model_backward (three more where the scale is taken from the
 * divergence and the net has no div channel); no host read, no stream synchronisation; capturable. Sizes and shapes are checked
 * before the first launch: graph models and models with pooling / upsampling layers are TFL_EUNSUPPORTED, a short tape or
 * workspace TFL_EINVAL, each with nothing written. */
int tfl_model_backward_input(tfl_ctx* ctx, tfl_model* model, const tfl_tensor* flags, const tfl_tensor* pDiv,
                             const tfl_tensor* UDiv, const tfl_tensor* UOut, const tfl_tensor* gradP, const tfl_tensor* gradU,
                             const float* tape, int64_t tape_floats, float* workspace, int64_t workspace_floats,
                             float* const* gradWeights, float* const* gradBiases, int accumulate, const tfl_tensor* gradPDiv,
                             const tfl_tensor* gradUDiv);

/* tfl_model_set_weights with DEVICE pointers (cudnn layout, one weight and one bias array per layer, as tfl_model_create takes
 * them from the host): every weight form the model's path holds is rebuilt by kernels enqueued on the context's stream, into
 * the buffers it already has -- byte for byte what tfl_model_set_weights produces from the same values. No host read of a
 * parameter value, no stream synchronisation, capturable; launches that read the old weights were enqueued earlier on the same
 * stream and finish first. One gather launch covers the generic forms of all layers, one the fp32 forms of a default topology
 * (MFMA fragments, Winograd transform, tail packs), one the split-fp16 fragments: three launches at the most, none per layer.
 * The arrays must stay valid until those launches have run. Batch-norm folds are not parameters here and stay as they are.
 * ONE EXCEPTION: a 3-D default model on the split-fp16 MFMA path (TFL_CONV_PATH unset or "mfma16") hands its three per-layer
 * post-scales to its conv kernels by value, so on that path only the call ends by reading those three floats back: one 12-byte
 * copy and the wait for the stream it implies. There it is refused with TFL_EUNSUPPORTED, before anything is launched, while
 * the stream is capturing. As after tfl_model_set_weights, a tfl_slab_graph recorded with the model must be re-recorded.
 * Models of more than 32 layers are refused with TFL_EUNSUPPORTED (the pointers travel as kernel arguments). */
int tfl_model_set_weights_device(tfl_ctx* ctx, tfl_model* model, const float* const* d_weights, const float* const* d_biases);

/* ---- the optimiser step of the training closure: gradient clip (lib/run_epoch.lua:304-312), weight decay, lib/adam.lua or
 * lib/rmsprop.lua, and the refresh of the native model from the updated parameters, as ONE asynchronous call on device
 * arrays. (optim.sgd is Torch's own, not in the reference tree, and is not built.) */
enum { TFL_OPTIM_ADAM = 0, TFL_OPTIM_RMSPROP = 1 };
typedef struct tfl_optim tfl_optim;
typedef struct {
  int32_t method;            /* TFL_OPTIM_ADAM, TFL_OPTIM_RMSPROP */
  double learningRate, learningRateDecay, beta1, beta2, epsilon, weightDecay;   /* lib/adam.lua:28-34 */
  double alpha, initialMean;                                                    /* lib/rmsprop.lua:28-32 */
  double gradNormThreshold;  /* <= 0: no clip (run_epoch.lua:304-312) */
} tfl_optim_config;
/* State for the parameters of `model` (one weight and one bias array per layer, cudnn layout): the moments m and v -- RMSprop:
 * m alone, filled with initialMean -- and the step counter t, all on the device. NULL on error (tfl_last_error).
 * The optimiser keeps `model` and refreshes it in every step: the model must outlive the optimiser (destroy the optimiser
 * first; a tfl_optim_step after tfl_model_destroy of its model is undefined). */
tfl_optim* tfl_optim_create(tfl_ctx* ctx, tfl_model* model, const tfl_optim_config* config);
/* One step, in place on the DEVICE arrays, fp32 per element in the reference's operation order:
 *   clip     norm = the L2 norm over all gradients, summed in fp64 in a fixed order (per-block partials at fixed places, added
 *            in index order, no atomics) and rounded once; if norm > gradNormThreshold every gradient element is divided by
 *            (float)(norm / gradNormThreshold)
 *   decay    g += weightDecay x
 *   Adam     clr = lr / (1 + t lrd) with t before the increment; m = m beta1 + (1 - beta1) g; v = v beta2 + (1 - beta2) g g;
 *            x -= stepSize m / (sqrt(v) + epsilon), stepSize = clr sqrt(1 - beta2^t) / (1 - beta1^t) formed in fp64 from the
 *            new t and rounded once
 *   RMSprop  m = m alpha + (1 - alpha) g g; x -= lr g / (sqrt(m) + epsilon)
 * The gradient arrays hold the clipped and decayed gradients afterwards. A kernel advances t, so a captured step advances on
 * replay; the hyper-parameters travel by value with each call (tfl_optim_set_config changes them for the next one). At most
 * three launches, then tfl_model_set_weights_device from the updated parameters (its launches, its one exception, its limits).
 * The same inputs and state give the same bits on every call. */
int tfl_optim_step(tfl_ctx* ctx, tfl_optim* opt, float* const* d_weights, float* const* d_biases,
                   float* const* d_gradWeights, float* const* d_gradBiases);
/* tfl_optim_step whose update kernels read *d_guard (a DEVICE word: tfl_closure_fold's) when they RUN: where it is non-zero they
 * write nothing -- parameters, moments, gradients and the step counter stay as they are -- and the refresh that follows rebuilds
 * the native model's weight forms from the unchanged parameters, i.e. the same forms. The clip's norm launch and the refresh
 * run either way, so the call is the same sequence of launches whatever the word holds and can be captured. d_guard == NULL is
 * tfl_optim_step itself. */
int tfl_optim_step_guarded(tfl_ctx* ctx, tfl_optim* opt, float* const* d_weights, float* const* d_biases,
                           float* const* d_gradWeights, float* const* d_gradBiases, const int32_t* d_guard);
/* New hyper-parameters from the next step on; the method and the shapes are fixed (a changed method is TFL_EINVAL). */
int tfl_optim_set_config(tfl_ctx* ctx, tfl_optim* opt, const tfl_optim_config* config);
/* The step counter t (reads it back: synchronises the stream; for logging). -1 on error. */
int64_t tfl_optim_steps(tfl_ctx* ctx, tfl_optim* opt);
/* The moments, for a checkpoint: copies m into d_m and (Adam) v into d_v -- DEVICE arrays of the returned count of floats, in
 * parameter order (layer 0's weight, its bias, layer 1's weight, ...); either may be NULL (both NULL: the count alone).
 * Enqueued on the context's stream, no synchronisation. -1 on error. */
int64_t tfl_optim_get_state(tfl_ctx* ctx, tfl_optim* opt, float* d_m, float* d_v);
void tfl_optim_destroy(tfl_ctx* ctx, tfl_optim* opt);

/* A z-slab rank holds only part of the grid, but tfluids.getDx = 1/max(X,Y,Z) (grid.cc:37-40) is a
 * property of the WHOLE grid: dx > 0 overrides the value addBuoyancy / addGravity derive from the
 * local tensor sizes; 0 restores the default. */
int tfl_set_dx_override(tfl_ctx* ctx, float dx);

/* x = x*invMask + bc (both NULL: skip), then clamp to [lo, hi] if doClamp: one fused launch for
 * setConstVals' cmul+add pairs and the final U:clamp (lib/simulate.lua:130-160, 326), which the
 * reference issues as separate THC elementwise kernels. */
int tfl_applyBCs(tfl_ctx* ctx, const tfl_tensor* x, const tfl_tensor* bc, const tfl_tensor* invMask,
                 int doClamp, float lo, float hi);

/* tfl_applyBCs restricted to the element indices idx[0..n) (device int32, indices into the flattened
 * tensors): x[e] = x[e]*invMask[e] + bc[e]. For BC tensors that are the identity (invMask 1, bc 0)
 * almost everywhere -- the plume BCs touch 4 y-rows -- the host caches the non-identity indices once and
 * every setConstVals becomes O(|BC cells|) instead of three dense sweeps per field. */
int tfl_applyBCsIndexed(tfl_ctx* ctx, const tfl_tensor* x, const tfl_tensor* bc, const tfl_tensor* invMask,
                        const int32_t* idx, int64_t n);

/* count <= 8 tfl_applyBCsIndexed calls in ONE launch (setConstVals touches p, U and every density channel
 * back to back, lib/simulate.lua:130-160; each list is a few thousand cells, so the launches themselves were
 * the cost). x[i], bc[i], invMask[i] as in tfl_applyBCsIndexed; idx[i] / n[i] the device index list of pair i. */
int tfl_applyBCsIndexedMulti(tfl_ctx* ctx, int count, const tfl_tensor* const* x, const tfl_tensor* const* bc,
                             const tfl_tensor* const* invMask, const int32_t* const* idx, const int64_t* n);

/* init.lua:560-564 `tfluids.getDx(flags)`: 1 / max(X, Y, Z) as a double (a Lua number), or the override of
 * tfl_set_dx_override. */
double tfl_getDx(tfl_ctx* ctx, const tfl_tensor* flags);

/* `dst:copy(src)` on the context's stream (same element count). */
int tfl_copy(tfl_ctx* ctx, const tfl_tensor* dst, const tfl_tensor* src);
/* A plain streaming copy of n floats (16-byte aligned, n % 4 == 0) by the library's own float4 kernel: the measured
 * HBM yard-stick of bench.py (timed through tfl_profile_begin / _end as "k_stream_copy"). No reference counterpart. */
int tfl_stream_copy(tfl_ctx* ctx, float* dst, const float* src, int64_t n);

/* ---- the whole step as one call: lib/simulate.lua:175-327 in native code -------------------------------------
 * For hosts that are not Python (the LuaJIT binding): tfl_simulate_step runs tfluids.simulate() -- advectScalar
 * per density channel, advectVel, setConstVals, addBuoyancy / addGravity / vorticityConfinement, setConstVals, the
 * pressure projection (ConvNet | Jacobi | PCG), setConstVals, U:clamp(+-1e6) -- with the same launch-saving
 * orchestration as fluidnet_amd/simulate.py: index-list BCs, idempotent BC pairs skipped on fields nothing has
 * written, the U:copy after advectVel folded into addBuoyancy, setConstVals(U) + clamp fused into the projection.
 * State tensors are updated in place like the reference's batchGPU.
 *
 * tfl_bc_plan: the precomputed form of one (BC, BCInvMask) pair of lib/simulate.lua:130-160 (the list of cells where
 * the pair is not the identity; whether it is sparse; whether it is idempotent). Create once per pair, re-create
 * when the BC tensors change (createPlumeBCs, the 2-D demo's interactive edits). The plan keeps the two pointers. */
typedef struct tfl_bc_plan tfl_bc_plan;
tfl_bc_plan* tfl_bc_plan_create(tfl_ctx* ctx, const tfl_tensor* bc, const tfl_tensor* invMask);
void tfl_bc_plan_destroy(tfl_ctx* ctx, tfl_bc_plan* plan);

/* tfl_wall_plan (round 6, optional): what the projection asks of a scene's flags as one 16-bit code per cell (the setWallBcs
 * decisions: zero u_x / u_y / u_z; is-fluid, is-open, and the same of the three minus-neighbours), computed once. The flags of a simulation are set when the scene is built (lib/simulate.lua never writes them);
 * the projection's first and last kernel otherwise re-derive all that from up to ten rows of flag words per cell row, every step.
 * Create one per flags array ([B][1][Z][Y][X]) on the context that steps it: tfl_model_begin / tfl_model_forward /
 * tfl_simulate_step[_slab] find it again by the array's address and shape and read the bytes instead -- the same decisions,
 * the same bits out. Destroy it (and create a new one) whenever the flags change, and before the array is freed. */
typedef struct tfl_wall_plan tfl_wall_plan;
tfl_wall_plan* tfl_wall_plan_create(tfl_ctx* ctx, const tfl_tensor* flags);
void tfl_wall_plan_destroy(tfl_ctx* ctx, tfl_wall_plan* plan);
/* Unregister without freeing (no HIP call: safe from a garbage collector's finalizer, where a hipFree could invalidate a graph
 * capture in progress); tfl_wall_plan_destroy still has to follow. */
void tfl_wall_plan_retire(tfl_wall_plan* plan);

typedef struct tfl_sim_params {      /* mconf of lib/simulate.lua (defaults of lib/default_conf.lua in brackets) */
  float dt;
  const char* advectionMethod;       /* NULL = "maccormackOurs" */
  float maccormackStrength;
  double buoyancyScale;              /* 0 = off. Lua numbers: (dx/4)*scale is formed in double and rounded once, */
  double gravityScale;               /* 0 = off.  exactly like simulate.lua:204-239 does on its float tensors   */
  float gravity[3];                  /* direction, simulate.lua:204-211 [0, 1, 0] */
  double vorticityConfinementAmp;    /* 0 = off */
  const char* simMethod;             /* NULL | "convnet" | "jacobi" | "pcg" */
  int32_t maxIter;                   /* jacobi / pcg; <= 0 -> 100 */
  const char* pcgPrecond;            /* NULL = "ic0" like simulate.lua:283; "none" | "ilu0" | "ic0" | "mg". The unpreconditioned
                                        solve is ~1.7x faster per call at 128^3 here (slower at 256^3) and takes ~3x the iterations */
  int32_t outputDiv;                 /* 1: return before the projection (simulate.lua:241-245) */
} tfl_sim_params;

typedef struct tfl_sim_state {
  const tfl_tensor* p;               /* batch.pDiv   [B][1][Z][Y][X] */
  const tfl_tensor* U;               /* batch.UDiv   [B][C][Z][Y][X] */
  const tfl_tensor* flags;
  int32_t n_density;                 /* 0..8 scalar channels (the RGB table of the 2-D demo = 3) */
  const tfl_tensor* density[8];
  const tfl_bc_plan* pBC;            /* NULL = no such BC pair */
  const tfl_bc_plan* UBC;
  const tfl_bc_plan* densityBC[8];
  tfl_model* model;                  /* needed for simMethod convnet */
} tfl_sim_state;

int64_t tfl_simulate_workspace_floats(tfl_ctx* ctx, const tfl_sim_params* params, const tfl_sim_state* state);
int tfl_simulate_step(tfl_ctx* ctx, const tfl_sim_params* params, const tfl_sim_state* state, float* workspace,
                      int64_t workspace_floats);
/* The second half of the step as its own entry: the projection phase of tfl_simulate_step alone (simulate.lua:247-326: [setWallBcs,]
 * setConstVals, the ConvNet | Jacobi | PCG projection, setConstVals, U:clamp) on a state whose U already holds the post-force
 * velocity and whose p holds the previous pressure -- what a tfl_simulate_step call with params->outputDiv = 1 leaves.
 * Contract: an outputDiv = 1 step followed by tfl_simulate_project (same params but for outputDiv, which this entry does not read;
 * same state) leaves the bits of ONE tfl_simulate_step with outputDiv = 0 -- for pcg, jacobi and convnet, in 2-D and 3-D, with and
 * without BC pairs and density. Between the two calls the host may read the divergent state (the data-set generator stores it:
 * fluidnet_amd/datagen.py) but must not write it. The workspace is the step's: tfl_simulate_workspace_floats, same alignment.
 * tfl_simulate_step itself is not changed by this entry. */
int tfl_simulate_project(tfl_ctx* ctx, const tfl_sim_params* params, const tfl_sim_state* state, float* workspace,
                         int64_t workspace_floats);

/* The step on batch items with forces of their own (not in the reference): what the data-set generator steps R
 * runs at a time with. Contract: item b of the state ends with the VALUES of tfl_simulate_step (or of an outputDiv step followed
 * by tfl_simulate_project) on a B = 1 state that holds item b alone -- its slices of p, U, flags, density and of the BC tensors --
 * with params whose four force fields are items[b]'s. items == NULL: every item takes params' own forces. Values, not bits, in
 * one respect: the sign of a zero (a dense BC pair, or a pair folded into a producing kernel, computes x * 1 + 0 on the cells of
 * an item whose pair is the identity, which turns -0 into +0; DESIGN.md 3.25 lists the paths).
 * simMethod "pcg" | "jacobi"; "convnet" is refused by name with TFL_EUNSUPPORTED. pcgPrecond "mg" | "none" solve all items in the
 * launches of one (tfl_solveLinearSystemPCGBatched, tol 1e-4); "ic0" | "ilu0" | NULL run tfl_solveLinearSystemPCG, serial over the
 * items. tfl_pcg_last_iterations afterwards: the sum over the items. Every advection method, 0..8 density channels and BC plans
 * over [B]-wide tensors are taken as in tfl_simulate_step. n_items must equal state->flags->B and be at most TFL_MAX_ITEMS.
 * Refused by name before anything is enqueued: a wrong n_items, more than TFL_MAX_ITEMS items, a workspace shorter than
 * tfl_simulate_items_workspace_floats or not 16-byte aligned, "convnet", an unknown simMethod / pcgPrecond, a force field that is
 * not finite, a z-window or stage mask set on the context. tfl_simulate_project_items is the projection phase alone, as
 * tfl_simulate_project is of tfl_simulate_step: an outputDiv items step + project items = one items step. */
typedef struct tfl_sim_item {        /* the force fields of tfl_sim_params, for one batch item */
  float gravity[3];
  double buoyancyScale;
  double gravityScale;
  double vorticityConfinementAmp;
} tfl_sim_item;
int64_t tfl_simulate_items_workspace_floats(tfl_ctx* ctx, const tfl_sim_params* params, const tfl_sim_state* state);
int tfl_simulate_step_items(tfl_ctx* ctx, const tfl_sim_params* params, const tfl_sim_item* items, int32_t n_items,
                            const tfl_sim_state* state, float* workspace, int64_t workspace_floats);
int tfl_simulate_project_items(tfl_ctx* ctx, const tfl_sim_params* params, const tfl_sim_item* items, int32_t n_items,
                               const tfl_sim_state* state, float* workspace, int64_t workspace_floats);

/* ---- z-slab decomposition across the GPUs of a node (BASELINE config 5; no counterpart in the reference, which is
 * single-GPU). A rank holds planes [z_first, z_first + Zlocal) of a z_total-deep grid: the planes it OWNS,
 * [own_lo, own_hi) in local indices, plus `halo` planes of its neighbours on each side that has one (none at the domain
 * ends). Building blocks first, the assembled step last. ------------------------------------------------------- */

/* Gather planes [zlo, zhi) of n <= 8 fields (each with its own B and C; all with the same Z, Y, X) into one contiguous
 * buffer laid out [field][b][c][plane][Y][X] (unpack = 0), or scatter such a buffer back (unpack = 1): what RCCL
 * send/recv moves over xGMI. */
int tfl_packPlanes(tfl_ctx* ctx, int n, const tfl_tensor* const* fields, int zlo, int zhi, float* buf,
                   int unpack);

/* Compute window: until changed, advectScalar, advectVel, addBuoyancy[From], addGravity, vorticityConfinement,
 * tfl_model_begin and tfl_model_finish compute ONLY the z-planes [a0, a1) and [b0, b1) of their tensors (the two runs
 * go out as one launch; an empty second run is b0 == b1); reads still address the whole array. All zero = every plane
 * (the default). The other operators ignore the window. A slab rank uses it to run each phase of the step on exactly
 * the planes whose inputs are valid, and to split a phase into boundary strips (computed first, so their halo message
 * can leave) and interior (computed while the message is in flight). */
int tfl_set_z_window(tfl_ctx* ctx, int a0, int a1, int b0, int b1);

/* Where the tensors of the next advectScalar / advectVel calls sit inside the whole grid: local plane 0 is global plane
 * z_first of z_total. The back-traces then form their positions in GLOBAL z, so that a slab rounds every position
 * exactly like the unsplit grid does (a slab-relative coordinate lands in another binade and rounds differently);
 * the domain walls of the trace are those of the whole grid. (0, 0) = the tensors are the whole grid (default). */
int tfl_set_z_origin(tfl_ctx* ctx, int z_first, int z_total);

/* Pass selection for the multi-pass operators (0 = all passes, the default), so that each pass can get its own
 * window: advectScalar 1 = 3^dim min/max grid, 2 = pass A (forward), 4 = pass B (backward + correct + clamp);
 * advectVel 2 / 4 likewise; vorticityConfinement 2 = curl, 4 = confinement force; tfl_model_begin 2 = wall BCs +
 * divergence + partial sums, 4 = reduction over [zlo, zhi); tfl_model_finish on the 3-D default topology's fused kernels
 * 1 / 2 / 4 = first / second / third(+1x1x1) conv layer, 8 = velocity update + un-scale + wall BCs; on any other 3-D model
 * that is not a graph model 1 = the whole net, every launch on its layer's cone of the window's planes (the window names the
 * planes whose pressure must come out exact and is aligned to the model's downsampling factor), 8 = as above. Such a windowed
 * forward of a model with non-default tfl_model_opts takes its input-scale stats from the caller. */
int tfl_set_stages(tfl_ctx* ctx, int mask);

/* The divergence plane tfl_model_begin wrote inside `workspace` (a [B][1][Z][Y][X] field): a slab rank exchanges its
 * halo planes before the first conv layer. */
float* tfl_model_div(const tfl_model* model, int B, int Z, int Y, int X, float* workspace);

typedef struct tfl_slab {
  int32_t z_total;        /* planes of the whole grid */
  int32_t z_first;        /* global index of local plane 0 */
  int32_t own_lo, own_hi; /* owned planes [own_lo, own_hi), local indices; own_lo = 0 at the lower domain end, else the
                             stored halo depth (>= tfl_slab_halo(reach)); likewise above */
  int32_t reach;          /* R: the step is exact while max|u_z|*dt < R cells (the back-trace of the advection);
                             0 = 1. Halo depth needed = max(4, 2R + 1) */
  int32_t overlap;        /* 1: split the phases that feed a message into boundary strips + interior so that the
                             transfer overlaps compute (worth it when a slab holds >~ 1M cells); 0: one launch each */
  int32_t check_reach;    /* 1: every step reduces max|u_z| on the device into a sticky maximum and copies it to pinned
                             memory; a violation by the state step n starts from is reported by the call for step n+2
                             at the latest (that call waits for step n's copy, which has long landed unless the host is
                             more than two steps ahead of the device: round 6 -- waiting for step n+1's cost 60 us per
                             step); messages in flight are drained before the error is returned. The report is per
                             rank: stop every rank when one reports (or use 2). Where the planes fill the projection
                             kernel's blocks (X % 128 == 0, Y % 8 == 0, ConvNet projection) the maximum is taken by that
                             kernel over the planes it writes -- the rank's OWNED planes; its halo planes are their owners'
                             to report -- and the step launches no reduction of its own from the second step on; the report
                             then comes one call later still (round 6).
                             2 (round 6, "exact"): the check comes BEFORE the step's advection and is collective -- max|u_z|
                             of the state the step starts from, the reach it needs all-reduced over the ranks (8 doubles
                             through tfl_comm.allreduce_sum), one host synchronisation. A step that needs more than `reach`
                             returns TFL_EREACH on EVERY rank with nothing written; the host widens the halos
                             (tfl_slab_needed_reach, tfl_slab_exchange) and calls again, so the cut run stays the
                             un-cut run whatever the flow does (fluidnet_amd/dist.py SlabSimulation does it by itself).
                             The same all-reduce carries every rank's fp16 range word, so TFL_ERANGE is collective too
                             in this mode; with check_reach 0 / 1 a slab that has neighbours never returns TFL_ERANGE on
                             its own (the others would wait for its halos): poll tfl_model_range_flag on the host.
                             Costs the host its lead over the device (~10-30 us per step): opt-in */
  int32_t in_flight;      /* OUT/IN, initialise to 0 for a new run: bits 0-3 = halo messages started by the previous call and
                             not yet consumed (tfl_simulate_step_slab finishes them; tfl_slab_drain does so explicitly);
                             bit 8 = this run has reset the context's reach word (library-internal) */
} tfl_slab;

/* Transport supplied by the host (RCCL send/recv through torch.distributed in fluidnet_amd/dist.py; any MPI-like
 * layer works). All buffers are device memory inside the step's workspace. Every callback is called from the thread
 * that called tfl_simulate_step_slab, after the library has enqueued the packing kernels on the context's stream:
 *   exchange_start: begin sending send_lo[0..n_send_lo) to rank-1 and receiving recv_lo from it, send_hi / recv_hi with
 *                   rank+1 (n == 0 / NULL: no such neighbour). Must order the transfer after the work enqueued so far
 *                   on the stream; should not block the host.
 *   exchange_wait:  make the stream wait until the transfers of exchange_start(tag) have landed.
 *   allreduce_sum:  in-place sum of n device doubles over all ranks, ordered on the stream.
 * Return 0, or non-zero to abort the step (reported as TFL_EINVAL with "comm callback failed"). */
typedef struct tfl_comm_chunk {   /* n contiguous floats of device memory */
  float* ptr;
  int64_t n;
} tfl_comm_chunk;

typedef struct tfl_comm {
  int32_t size;   /* sizeof(tfl_comm) as the HOST compiled it: the library reads no member that lies beyond it, so a host built
                     against a header without the optional trailing callbacks keeps working (0 is refused) */
  void* user;
  int (*exchange_start)(void* user, int tag, const float* send_lo, int64_t n_send_lo, float* recv_lo, int64_t n_recv_lo,
                        const float* send_hi, int64_t n_send_hi, float* recv_hi, int64_t n_recv_hi);
  int (*exchange_wait)(void* user, int tag);
  int (*allreduce_sum)(void* user, double* dev, int64_t n);
  /* Optional (NULL: not offered). The same exchange WITHOUT staging buffers: the halo planes of a [C][Z][Y][X] field are
   * one contiguous run per (batch item, channel), so a message is a short list of chunks that a transport able to move
   * several pieces per neighbour (RCCL: several ncclSend / ncclRecv in one group) takes straight out of, and delivers
   * straight into, the fields -- the step then launches no pack / unpack kernels (6 of a middle rank's 22 launches per
   * step). Chunk i of send_hi pairs with chunk i of the upper neighbour's recv_lo (same order, same sizes); n_lo / n_hi = 0:
   * no such neighbour. The received planes are written while the transfer runs, i.e. any time between this call and
   * exchange_wait(tag); the step never reads them in that window. */
  int (*exchange_start_v)(void* user, int tag, int n_lo, const tfl_comm_chunk* send_lo, const tfl_comm_chunk* recv_lo,
                          int n_hi, const tfl_comm_chunk* send_hi, const tfl_comm_chunk* recv_hi);
  /* Optional (ABI 4; 0 or absent: no). Non-zero: every callback only ENQUEUES stream operations ordered against the
   * context's stream (kernels, copies, event record / wait, RCCL calls) and never waits on the host or reads device
   * results -- so a whole rank-step can be recorded into a HIP graph (tfl_slab_graph_create). The native RCCL transport
   * sets it; a transport that runs host code per message (the torch.distributed ones of fluidnet_amd/dist.py) must not. */
  int32_t capturable;
} tfl_comm;

/* Halo depth a slab must store next to each neighbour for reach R (>= 4). */
int32_t tfl_slab_halo(int32_t reach);
/* The same for a step that projects with `model` (NULL: the Jacobi projection, = tfl_slab_halo(reach)): max(tfl_slab_halo(reach),
 * the depth of net input the model's cone reads below / above the owned planes), rounded up to the model's downsampling factor F
 * (the pooling product along z). The 3-D default topology returns exactly tfl_slab_halo(reach); the 3-D `tog` table needs 16
 * (F = 4). With F > 1 the slab's z_first, owned boundaries and local depth must be multiples of F as well (the pooling windows of
 * the cut grid are then the un-cut grid's). TFL_EUNSUPPORTED (< 0) for the models the slab step refuses: graph models (banks,
 * batch norm, max pooling) and 2-D models. DESIGN.md 6d. */
int32_t tfl_slab_halo_model(const tfl_model* model, int32_t reach);
int64_t tfl_simulate_slab_workspace_floats(tfl_ctx* ctx, const tfl_sim_params* params, const tfl_sim_state* state,
                                           const tfl_slab* slab);

/* tfl_simulate_step on one z-slab: the owned planes of p, U and density come out as the single-GPU step would compute
 * them (bit for bit, except for the summation order of the std normaliser's all-reduce). State tensors are the LOCAL
 * extended arrays; BC plans are made on the local BC tensors; flags halos are static (filled by the caller once).
 * Preconditions: 3-D, any advectionMethod tfl_simulate_step takes (an unknown name: TFL_EINVAL before anything is written),
 * 0..8 density channels as in tfl_simulate_step (every channel travels in the advected-field message; buoyancy reads
 * channel 0), B*C layout as in tfl_simulate_step, and one of two
 * projections: the ConvNet (simMethod "convnet", state->model with the 3-D default topology) or Jacobi (simMethod "jacobi",
 * state->model = NULL, maxIter sweeps from p = 0 as in tfl_simulate_step; the workspace size follows state->model, so ask
 * for it with the state the step will get). PCG is refused (TFL_EUNSUPPORTED): its dot products need an all-reduce per
 * iteration and its IC(0) preconditioner is a lexicographic wavefront over the whole grid, which does not cut along z; on the first call every halo plane holds valid data (the caller cut its arrays
 * out of a global initial state); `workspace` must be the SAME buffer on every call (halo messages of p and U started
 * at the end of one step are consumed by the next).
 * Per step: three neighbour exchanges + one 2*B-double all-reduce --
 *   U(max(R+1, 2R) planes) + p(4 below, 3 above)   ONE message started at the end of the previous step, consumed at the start
 *   advected U(3 below, 4 above) + every density channel(max(4, 2R+1)) after the advection's last pass, overlapped with
 *                                         the interior of the velocity's last pass
 * (the same halos serve every advection method: DESIGN.md section 6c derives each method's dependency cone)
 *   divergence(4 below, 3 above)          overlapped with the interior of the first conv layer
 * and every phase runs under the narrowest z-window that keeps the owned planes exact, so the redundant compute is a
 * few planes per phase instead of a fixed wide halo. Those windows, stage masks and the slab's
 * origin are the step's own: it neither reads nor changes what tfl_set_z_window / tfl_set_stages / tfl_set_z_origin left
 * on the context (tfl_set_advect_mode is honoured).
 * Jacobi instead: the same U + p message and T2, then divergence(J-1 planes a side) once, and p(J planes a side) after every
 * J sweeps -- floor(maxIter / J) exchanges, none before the first sweep (p starts at zero) -- where J = the stored halo depth
 * (own_lo, or z_local - own_hi on the lowest rank; every rank must store the same depth). No all-reduce (check_reach = 2
 * all-reduces its 8 reach flags only), so the owned planes equal tfl_simulate_step's bit for bit at any world size. A host that
 * stores deeper halos gets fewer, longer exchanges. maxIter = 34 with 4-plane halos: 34 sweep launches, 8 p exchanges + div. */
int tfl_simulate_step_slab(tfl_ctx* ctx, const tfl_sim_params* params, const tfl_sim_state* state, tfl_slab* slab,
                           const tfl_comm* comm, float* workspace, int64_t workspace_floats);

/* The reach the last TFL_EREACH of this context asked for: the smallest R with max|u_z|*dt < R over ALL ranks (0: none yet). */
int32_t tfl_slab_needed_reach(const tfl_ctx* ctx);

/* One halo exchange of n <= 4 fields outside a step (what a host needs to widen a slab's halos after TFL_EREACH, or to
 * fill them at start-up without a global array): planes [own_lo - below[i], own_lo) of field i are received from the lower
 * neighbour and [own_hi, own_hi + above[i]) from the upper one; the matching owned planes are sent. Every field has the
 * slab's local depth (own_hi + halo). Staged through `scratch` (tfl_slab_exchange_floats of them); collective; returns with
 * the transfers ordered on the context's stream. */
int64_t tfl_slab_exchange_floats(int n, const tfl_tensor* const* fields, const int32_t* below, const int32_t* above, const tfl_slab* slab);
int tfl_slab_exchange(tfl_ctx* ctx, int n, const tfl_tensor* const* fields, const int32_t* below, const int32_t* above,
                      const tfl_slab* slab, const tfl_comm* comm, float* scratch, int64_t scratch_floats);

/* Finish the messages a previous tfl_simulate_step_slab left in flight: afterwards the halo planes of U and p are
 * valid too (call before reading halos on the host, or before freeing the workspace). */
int tfl_slab_drain(tfl_ctx* ctx, const tfl_sim_state* state, tfl_slab* slab, const tfl_comm* comm, float* workspace,
                   int64_t workspace_floats);

/* tfl_velocityDivergenceNorm of the WHOLE grid from its z-slabs: norm[b] (device, B doubles, the same on every rank) =
 * || velocityDivergence(U, flags)[b] ||_2 over all z_total planes. `workspace` is the step's workspace. The call first finishes
 * the U / p messages the last step left in flight (as tfl_slab_drain does: the plane above the owned range is valid then),
 * sums each OWNED plane into a zeroed [B][z_total] array of doubles at the plane's global index (in the compute region of the
 * workspace, which is dead between steps), makes ONE allreduce_sum of B * z_total doubles (none on a slab without neighbours)
 * and adds the planes on every rank. A plane's sum is formed by its owner exactly as the un-cut call forms it, every other
 * rank adds zeros to it, and the planes are added in the un-cut call's order: THE RESULT EQUALS tfl_velocityDivergenceNorm OF
 * THE UN-CUT GRID BIT FOR BIT AT ANY WORLD SIZE. Collective; no host read or synchronisation of its own (a transport with
 * `capturable` set only enqueues, so the call may be recorded; tfl_slab_graph_* does not record it). 2-D states are refused
 * like the step ("no z to cut"). */
int tfl_slab_divergence_norm(tfl_ctx* ctx, const tfl_sim_state* state, tfl_slab* slab, const tfl_comm* comm, float* workspace,
                             int64_t workspace_floats, double* norm);

/* ---- the rank-step as ONE host call (round 6). tfl_simulate_step_slab costs the host a dozen kernel launches plus the
 * transport's calls per step -- on a 16-plane slab about as long as the GPU needs to run them. tfl_slab_graph_create records
 * one step (same arguments; they, the tensors they point to and the workspace must stay where they are while the graph lives)
 * on a stream of its own into an executable HIP graph: kernels, the transport's sends / receives / all-reduce and the
 * stream forks between them. tfl_slab_graph_step replays it on the context's stream: it makes the two host-side checks of the
 * eager call first (the reach word and the fp16 range word the previous step left in pinned memory; same error codes), then
 * ONE hipGraphLaunch. Differences from the eager step: the U / p message is started AND finished inside the step (no message
 * in flight between calls: slab->in_flight stays 0, tfl_slab_drain is a no-op), and the scalar parameters are frozen.
 * Needs tfl_comm.capturable (or a slab without neighbours); call it after at least one eager tfl_simulate_step_slab on
 * the same arguments (allocations, RCCL's connection set-up). NULL + tfl_last_error when the step cannot be recorded --
 * the caller keeps stepping eagerly. Results are those of the eager step bit for bit. */
typedef struct tfl_slab_graph tfl_slab_graph;
tfl_slab_graph* tfl_slab_graph_create(tfl_ctx* ctx, const tfl_sim_params* params, const tfl_sim_state* state, tfl_slab* slab,
                                      const tfl_comm* comm, float* workspace, int64_t workspace_floats);
int tfl_slab_graph_step(tfl_ctx* ctx, tfl_slab_graph* graph);
int64_t tfl_slab_graph_nodes(const tfl_slab_graph* graph);   /* nodes of the recorded graph (kernels, copies, events) */
void tfl_slab_graph_destroy(tfl_ctx* ctx, tfl_slab_graph* graph);

/* ---- native transport for the z-slab step: RCCL send/recv over xGMI inside the library (csrc/comm_rccl.cpp) ------------
 * For hosts without a communication layer of their own (the LuaJIT loop, plain C): one process per GPU, ranks ordered
 * along z (rank r's upper neighbour is r+1). Rank 0 obtains a unique id and hands the 128 bytes to the other ranks by
 * any means it has (a file, a socket, MPI, the launcher's environment); every rank then creates its communicator and
 * passes tfl_rccl_comm_callbacks() as the `comm` of tfl_simulate_step_slab / tfl_slab_drain. RCCL is dlopen'ed on first
 * use ($TFL_RCCL_LIBRARY, else a copy already loaded in the process, else librccl.so.1): the library itself links
 * only the HIP runtime. Transfers run on a communication stream of the communicator, ordered against the context's
 * stream by events; no call blocks the host. The context must outlive the communicator and keep its device. */
#define TFL_RCCL_UNIQUE_ID_BYTES 128
typedef struct tfl_rccl_comm tfl_rccl_comm;
/* 1 when an RCCL could be bound (the reason is in tfl_last_error otherwise). */
int tfl_rccl_available(tfl_ctx* ctx);
/* which library was bound ("librccl.so.1 (already loaded)", a path, ...) */
const char* tfl_rccl_comm_origin(tfl_ctx* ctx);
/* ncclGetUniqueId: fills id[0..128). */
int tfl_rccl_get_unique_id(tfl_ctx* ctx, void* id);
/* ncclCommInitRank on the context's device (collective: every rank of `world` must call it). NULL on failure. */
tfl_rccl_comm* tfl_rccl_comm_create(tfl_ctx* ctx, const void* id, int rank, int world);
/* The same around a communicator the host already has (an ncclComm_t); it is not destroyed by tfl_rccl_comm_destroy. */
tfl_rccl_comm* tfl_rccl_comm_wrap(tfl_ctx* ctx, void* nccl_comm, int rank, int world);
const tfl_comm* tfl_rccl_comm_callbacks(tfl_rccl_comm* comm);
/* 1: issue every send / receive / all-reduce on the CONTEXT's stream instead of the communication stream (no events between the
 * two). For slabs run with tfl_slab.overlap = 0 -- nothing there for a transfer to overlap with, and an event hop between
 * two streams costs 12-15 us of device-side latency on this stack, eight of them per eager step. 0 (default): the
 * communication stream. Call between steps with no message in flight (after tfl_slab_drain). A recorded step
 * (tfl_slab_graph_create) does not care: inside a graph the hops are dependencies, not events. */
int tfl_rccl_comm_set_inline(tfl_rccl_comm* comm, int on);
void tfl_rccl_comm_destroy(tfl_ctx* ctx, tfl_rccl_comm* comm);

/* ---- data-parallel training: the optimiser step with ONE gradient all-reduce inside (csrc/optim.hip) -------
 * N ranks hold equal parameters and moments and each the gradient of its own mini-batch; the step averages the gradients over
 * the ranks and then updates, so every rank takes the step of the N-fold batch and ends with the same bits.
 * The reduce buffer is the CALLER's: tfl_optim_reduce_doubles() device doubles = P + 8, P the parameter count of
 * tfl_optim_get_state: slot i < P belongs to parameter element i in that call's order, slot P to the guard, the rest is reserved
 * (written as zeros). A transport that resolves pointers inside a bound array (fluidnet_amd/dist.py) is bound to it. */
int64_t tfl_optim_reduce_doubles(tfl_ctx* ctx, tfl_optim* opt);
/* comm == NULL: tfl_optim_step_guarded itself (same launches, same bits; world, d_reduce and reduce_doubles are not read).
 * With a comm (any world >= 1, a world of one included):
 *   pack     d_reduce[i] = (double) g[i]; d_reduce[P] = (*d_guard != 0), 0 for a NULL guard              (one launch)
 *   reduce   ONE comm->allreduce_sum(user, d_reduce, P + 1), ordered on the context's stream; a failing callback is
 *            TFL_EINVAL with "comm callback failed"
 *   unpack   g[i] = (float)(d_reduce[i] / (double) world): one fp64 division, one rounding -- the whole definition of the
 *            average; the REDUCED guard (d_reduce[P] != 0) goes into a word of the optimiser's (tfl_optim_reduced_guard).
 *            With a clip this is the clip's norm launch (the same fp64 partials at the same places as tfl_optim_step's, so the
 *            step that follows has the bits of tfl_optim_step_guarded on the averaged gradients); without, a launch of its own
 *   update   tfl_optim_step_guarded's update, counter and refresh launches, reading the reduced guard
 * i.e. at most two launches more than the guarded step of the same configuration, and one collective. Where the reduced guard
 * is set NOTHING is written on any rank: parameters, moments, counter and the gradient arrays (which keep the rank's local
 * gradients) stay. Otherwise the gradient arrays hold the averaged, clipped and decayed gradients afterwards. The reduced
 * guard is not sticky: a local guard is (tfl_closure_fold), which keeps the reduced one set from that step on.
 * No host read and no synchronisation: with a comm whose `capturable` is set the call can be captured into a graph. */
int tfl_optim_step_reduced(tfl_ctx* ctx, tfl_optim* opt, float* const* d_weights, float* const* d_biases,
                           float* const* d_gradWeights, float* const* d_gradBiases, const int32_t* d_guard,
                           const tfl_comm* comm, int32_t world, double* d_reduce, int64_t reduce_doubles);
/* Enqueues a copy of the last tfl_optim_step_reduced's reduced guard word (0 before the first) into the DEVICE word d_out. */
int tfl_optim_reduced_guard(tfl_ctx* ctx, tfl_optim* opt, int32_t* d_out);
/* Rank 0's parameters to every rank: d_reduce = the parameters on rank 0 and zeros elsewhere, ONE allreduce_sum of P doubles
 * (x + 0 is exact, so the values arrive bit for bit), unpacked into the parameter arrays of every rank; then
 * tfl_model_set_weights_device from them (its launches, its one exception, its limits). Moments and counter are not touched:
 * call it before the first step, or where they are equal anyway. comm == NULL: the refresh alone. */
int tfl_optim_sync_parameters(tfl_ctx* ctx, tfl_optim* opt, float* const* d_weights, float* const* d_biases,
                              const tfl_comm* comm, int32_t rank, double* d_reduce, int64_t reduce_doubles);

/* The inverse of tfl_optim_get_state, for resuming from a checkpoint: m from d_m and (Adam) v from d_v -- DEVICE arrays of
 * tfl_optim_get_state's count of floats in its order; either may be NULL and is then left as it is -- and the step counter set
 * to `steps` (>= 0). The counter lives on the device and is written by a launch that takes the value as an argument: the
 * call is enqueued on the context's stream and waits for nothing. The arrays must stay valid until the copies have run. */
int tfl_optim_set_state(tfl_ctx* ctx, tfl_optim* opt, const float* d_m, const float* d_v, int64_t steps);

/* ---- the resident frame store of the training loop and its one-launch mini-batch gather (csrc/frames.hip) ----
 * The data set of lib/data_binary.lua, kept where the training step runs. A store holds `capacity` slots of one record each:
 * 2 C + 5 fp32 planes of Z Y X cells (C = 3 in 3-D, 2 in 2-D) in the order
 *     pDiv, UDiv[C], flags, densityDiv, p, U[C], density
 * i.e. the divergent frame, the flags ONCE (the two files of a frame carry equal flags, data_binary.lua:77; the int32 words as
 * floats, as loadMantaFile delivers them) and the target frame. Every plane is padded to a multiple of 4 floats, so each plane
 * of each slot starts on 16 bytes: a record is tfl_frames_record_floats() = (2 C + 5) * ((Z Y X + 3) & ~3) floats, and plane k
 * starts at float k * ((Z Y X + 3) & ~3) of it (the padding floats are never read back).
 * Slots [0, device_frames) are ONE device allocation; slots [device_frames, capacity) are ONE pinned, device-mapped host
 * allocation that the gather kernel reads through its device address. device_frames may be 0 or capacity. A slot that was
 * never put holds undefined floats. NULL on error (tfl_last_error). */
typedef struct tfl_frames tfl_frames;
tfl_frames* tfl_frames_create(tfl_ctx* ctx, int is3D, int Z, int Y, int X, int64_t capacity, int64_t device_frames);
void tfl_frames_destroy(tfl_ctx* ctx, tfl_frames* frames);
int64_t tfl_frames_record_floats(const tfl_frames* frames);
/* One record from HOST memory into a slot. NOT a hot path: ingest happens once per data set, one call per frame. A device slot
 * is one host-to-device copy enqueued on the context's stream: h_record must stay valid and unchanged until the stream has
 * passed it. A host slot first waits for the stream -- a gather enqueued earlier may still be reading the slot -- and is then a
 * memcpy, done when the call returns. */
int tfl_frames_put(tfl_ctx* ctx, tfl_frames* frames, int64_t slot, const float* h_record);
/* One mini-batch: item i < n of every output tensor = the planes of slot h_slots[i], wherever the slot lies -- ONE launch
 * (k_frames_gather) for up to 128 items, one more per further 128. The outputs are contiguous [B][1 or C][Z][Y][X] device tensors
 * with n <= B; any of them may be NULL and is then skipped; items [n, B) are not touched. pTarget / UTarget / densityTarget
 * receive the record's p / U / density. A slot may appear more than once.
 * h_slots is a HOST array, read during the call only: the indices are validated here (range; n against every B; shapes; the
 * outputs are memory of the context's device), before anything is launched -- a refused call has written nothing -- and then
 * travel to the kernel BY VALUE. So there is no host read of device memory and no synchronisation, and a call captured into a
 * graph replays the slots it was recorded with (re-record, or call eagerly, for other slots).
 * The copy is bit-exact: NaN payloads, -0 and denormals arrive as they were put. */
int tfl_frames_gather(tfl_ctx* ctx, tfl_frames* frames, int n, const int32_t* h_slots,
                      const tfl_tensor* pDiv, const tfl_tensor* UDiv, const tfl_tensor* flags,
                      const tfl_tensor* densityDiv, const tfl_tensor* pTarget, const tfl_tensor* UTarget,
                      const tfl_tensor* densityTarget);
/* The mirror of tfl_frames_gather: item i < n of every non-NULL tensor is written into the plane(s) it feeds of slot h_slots[i],
 * device slots and host-mapped slots alike -- ONE launch (k_frames_scatter) per 128 items, 128-bit stores on the slot side. The
 * planes of a NULL tensor keep what they held, so a record can be filled in two calls: the divergent half (pDiv, UDiv, flags,
 * densityDiv) first, the target half (pTarget, UTarget, densityTarget -> the record's p, U, density) later. The padding floats of
 * a written plane are written as zero. The inputs are contiguous [B][1 or C][Z][Y][X] device tensors with n <= B.
 * Validation is tfl_frames_gather's (range; n against every B; shapes; device memory of the context's device), before anything is
 * launched -- a refused call has written nothing -- and a slot index that appears twice in one call is refused as well. The
 * indices travel BY VALUE: no host read of device memory, no synchronisation, and the call can be captured into a graph, which
 * then replays the slots it was recorded with. The write is ordered on the context's stream like any kernel: a gather
 * enqueued behind it reads the new planes. Bit-exact: NaN payloads, -0 and denormals arrive as they were. */
int tfl_frames_put_device(tfl_ctx* ctx, tfl_frames* frames, int n, const int32_t* h_slots,
                          const tfl_tensor* pDiv, const tfl_tensor* UDiv, const tfl_tensor* flags,
                          const tfl_tensor* densityDiv, const tfl_tensor* pTarget, const tfl_tensor* UTarget,
                          const tfl_tensor* densityTarget);

/* ---- the scene kernels of the data-set generator (csrc/datagen.hip, csrc/tfl_datagen.hpp) ---------------------
 * No counterpart in the reference, whose sets come from a Mantaflow scene script outside its tree: these build this project's
 * own random scenes. Every value is a function of the arguments alone, in fp32 / uint32 arithmetic of one stated order
 * (tfl_datagen.hpp), so a numpy restatement gives the same bits.
 *
 * One primitive in cell units, tested at the cell centres (i + 0.5, j + 0.5, k + 0.5), x first:
 *   kind 0, sphere: a = centre, b[0] = radius: inside where ((dx dx + dy dy) + dz dz) <= r r (2-D: no dz term)
 *   kind 1, box:    a = lo, b = hi: inside where lo <= centre <= hi on every axis (2-D: x and y)
 * val is the density of a blob; the obstacle table does not read it. */
typedef struct tfl_scene_prim {
  int32_t kind;
  float a[3];
  float b[3];
  float val;
} tfl_scene_prim;
/* flags ([B][1][Z][Y][X], every item alike) = emptyDomain(bnd = 1) with every cell whose centre lies in one of the n_obstacles
 * <= 32 primitives made an obstacle; density (same shape, or NULL) = the val of the LAST of the n_blobs <= 32 blobs that holds
 * the cell's centre, +0 outside all of them and in every non-fluid cell. One launch (k_scene_flags). */
int tfl_scene_flags(tfl_ctx* ctx, const tfl_scene_prim* obstacles, int n_obstacles, const tfl_scene_prim* blobs, int n_blobs,
                    int is3D, const tfl_tensor* flags, const tfl_tensor* density);
/* White noise into psi ([B][1][Z][Y][X] in 2-D, [B][3][Z][Y][X] in 3-D): the value of cell t of channel c of item b is
 * (int(h >> 8) - 2^23) * 2^-23 with h = mix(mix(mix(mix(seed + 0x9e3779b9) ^ (run + b)) ^ c) ^ t), mix a lowbias32-style uint32
 * mixer (tfl_datagen.hpp noise_mix): independent of the launch geometry, a multiple of 2^-23 in [-1, 1). (k_noise_potential) */
int tfl_noise_potential(tfl_ctx* ctx, uint32_t seed, uint32_t run, const tfl_tensor* psi);
/* U = amp * the MAC-staggered discrete curl of the edge-located potential psi (2-D: u = d_y psi, v = -(d_x psi); 3-D: the three
 * components d_y psi_z - d_z psi_y, d_z psi_x - d_x psi_z, d_x psi_y - d_y psi_x; d_a f = f(+1 along a) - f, the neighbour index
 * clamped at the grid's end). Its discrete MAC divergence is zero but for rounding. psi and U must not alias. (k_curl_mac) */
int tfl_curl_mac(tfl_ctx* ctx, const tfl_tensor* psi, float amp, int is3D, const tfl_tensor* U);

#ifdef __cplusplus
}
#endif
#endif /* TFLUIDS_HIP_H_ */
