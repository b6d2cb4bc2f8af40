-- tfluids_hip.lua -- LuaJIT FFI binding of libtfluids_hip.so (include/tfluids_hip.h).
--
-- Drop-in for the native half of torch/tfluids: after `require('tfluids')`, calling
--   local hip = require('tfluids_hip').install(tfluids)
-- (1) replaces the per-tensor-type C tables that torch/tfluids/init.lua dispatches through
--     (`X.tfluids.<op>(...)`, registered by generic/tfluids.cc:927-957 / generic/tfluids.cu:1932-1962) with functions of
--     the SAME positional signatures that forward to the MI355X library, so init.lua's wrappers (argument checks,
--     getTempStorage, copy-back) and lib/simulate.lua run unchanged;
-- (2) replaces tfluids.normalizePressureMean (init.lua:747-764, a host round trip in the reference) and
--     tfluids.simulate (lib/simulate.lua:175-327) by the device / one-call forms (tfl_normalizePressureMean,
--     tfl_simulate_step);
-- (3) offers hip.Model(gmodule): a table with the call shape of the nngraph model -- model:forward({pDiv, UDiv, flags})
--     -> {p, U} (lib/simulate.lua:262-272) -- backed by tfl_model_forward.
--
-- The ffi.cdef block below is GENERATED from include/tfluids_hip.h (tools/gen_lua_cdef.py) and the CPU test-suite
-- (tests/test_lua_binding.py) regenerates and diffs it, and checks every C call in this file against the declared
-- prototypes (name + argument count), so the binding cannot drift from the header.
-- NOTE: LuaJIT / Torch7 are not available in the build container, so this file is not EXECUTED by the test-suite;
-- the executed host mirror of the same calls is fluidnet_amd/{tfluids,simulate,model}.py. Tensors must be contiguous
-- float tensors whose storage is device memory (cutorch CudaTensor on a ROCm build of cutorch).
local ffi = require('ffi')
local bit = require('bit')

-- BEGIN generated cdef (tools/gen_lua_cdef.py)
ffi.cdef[[
typedef enum tfl_status {
  TFL_OK = 0,
  TFL_EINVAL = -1,
  TFL_EHIP = -2,
  TFL_EUNSUPPORTED = -3,
  TFL_EREACH = -5,
  TFL_ERANGE = -4
} tfl_status;
typedef struct tfl_tensor {
  float* data;
  int32_t B, C, Z, Y, X;
} tfl_tensor;
enum {
  TFL_TypeNone = 0, TFL_TypeFluid = 1, TFL_TypeObstacle = 2, TFL_TypeEmpty = 4,
  TFL_TypeInflow = 8, TFL_TypeOutflow = 16, TFL_TypeOpen = 32, TFL_TypeStick = 128
};
typedef struct tfl_ctx tfl_ctx;
tfl_ctx* tfl_create(int device);
void tfl_destroy(tfl_ctx* ctx);
int tfl_set_stream(tfl_ctx* ctx, void* hip_stream);
const char* tfl_last_error(const tfl_ctx* ctx);
int tfl_abi_version(void);
enum { TFL_ADVECT_EXACT = 0, TFL_ADVECT_FAST = 1 };
int tfl_set_advect_mode(tfl_ctx* ctx, int mode);
int tfl_get_advect_mode(const tfl_ctx* ctx);
int tfl_synchronize(tfl_ctx* ctx);
int64_t tfl_trace_errors(tfl_ctx* ctx);
int tfl_scal3_zero_blocks(tfl_ctx* ctx, int64_t* blocks);
int tfl_scal3_sparse_stats(tfl_ctx* ctx, int64_t* stats);
int tfl_profile_begin(tfl_ctx* ctx);
int tfl_profile_end(tfl_ctx* ctx, char* buf, int64_t cap);
int tfl_advectScalar(tfl_ctx* ctx, float dt, const tfl_tensor* s, const tfl_tensor* U,
                     const tfl_tensor* flags, const tfl_tensor* fwd, const tfl_tensor* bwd,
                     int is3D, const char* method, const tfl_tensor* fwdPos,
                     const tfl_tensor* bwdPos, int boundaryWidth, int sampleOutsideFluid,
                     float maccormackStrength, const tfl_tensor* sDst);
int tfl_advectVel(tfl_ctx* ctx, float dt, const tfl_tensor* U, const tfl_tensor* flags,
                  const tfl_tensor* fwd, const tfl_tensor* bwd, int is3D, const char* method,
                  int boundaryWidth, float maccormackStrength, const tfl_tensor* UDst);
int tfl_setWallBcsForward(tfl_ctx* ctx, const tfl_tensor* U, const tfl_tensor* flags, int is3D);
int tfl_velocityDivergenceForward(tfl_ctx* ctx, const tfl_tensor* U, const tfl_tensor* flags,
                                  const tfl_tensor* UDiv, int is3D);
int64_t tfl_divergence_norm_workspace_floats(int32_t B, int32_t Z, int32_t Y, int32_t X);
int tfl_velocityDivergenceNorm(tfl_ctx* ctx, const tfl_tensor* U, const tfl_tensor* flags, int is3D,
                               double* norm, float* workspace, int64_t workspace_floats);
int tfl_criterion_weight(tfl_ctx* ctx, const tfl_tensor* flags, double borderWidth, double borderWeight, int is3D,
                         const tfl_tensor* weight);
int64_t tfl_fluid_criterion_workspace_floats(int32_t B, int32_t Z, int32_t Y, int32_t X);
int tfl_fluidCriterion(tfl_ctx* ctx, const tfl_tensor* pPred, const tfl_tensor* UPred, const tfl_tensor* pTarget,
                       const tfl_tensor* UTarget, const tfl_tensor* flags, const tfl_tensor* weight, double pLambda,
                       double uLambda, double divLambda, int sizeAverage, int is3D, double* loss, const tfl_tensor* gradP,
                       const tfl_tensor* gradU, float* workspace, int64_t workspace_floats);
int tfl_closure_fold(tfl_ctx* ctx, const double* loss4, double* sums5, int32_t* guard, int longTerm, double errLimit);
int tfl_velocityUpdateForward(tfl_ctx* ctx, const tfl_tensor* U, const tfl_tensor* flags,
                              const tfl_tensor* p, int is3D);
int tfl_vorticityConfinement(tfl_ctx* ctx, const tfl_tensor* U, const tfl_tensor* flags,
                             float strength, const tfl_tensor* centered, const tfl_tensor* curl,
                             const tfl_tensor* curlNorm, const tfl_tensor* force, int is3D);
int tfl_vorticityConfinementFrom(tfl_ctx* ctx, const tfl_tensor* USrc, const tfl_tensor* U, const tfl_tensor* flags,
                                 float strength, const tfl_tensor* curl, const tfl_tensor* curlNorm, int is3D);
int tfl_addBuoyancy(tfl_ctx* ctx, const tfl_tensor* U, const tfl_tensor* flags,
                    const tfl_tensor* density, const float gravity[3], float* strengthTmp,
                    float dt, int is3D);
int tfl_addBuoyancyFrom(tfl_ctx* ctx, const tfl_tensor* USrc, const tfl_tensor* U, const tfl_tensor* flags,
                        const tfl_tensor* density, const float gravity[3], float dt, int is3D);
int tfl_addGravity(tfl_ctx* ctx, const tfl_tensor* U, const tfl_tensor* flags,
                   const float gravity[3], float dt, int is3D, float* forceTmp);
int tfl_addBuoyancyItems(tfl_ctx* ctx, const tfl_tensor* USrc, const tfl_tensor* U, const tfl_tensor* flags,
                         const tfl_tensor* density, const float* gravity, const int32_t* on, int32_t n_items, float dt, int is3D);
int tfl_addGravityItems(tfl_ctx* ctx, const tfl_tensor* U, const tfl_tensor* flags, const float* gravity, const int32_t* on,
                        int32_t n_items, float dt, int is3D);
int tfl_vorticityConfinementItems(tfl_ctx* ctx, const tfl_tensor* U, const tfl_tensor* flags, const float* strength,
                                  const int32_t* on, int32_t n_items, const tfl_tensor* curl, const tfl_tensor* curlNorm,
                                  int is3D);
int tfl_emptyDomain(tfl_ctx* ctx, const tfl_tensor* flags, int is3D, int bnd);
int tfl_flagsToOccupancy(tfl_ctx* ctx, const tfl_tensor* flags, const tfl_tensor* occupancy);
int tfl_rectangularBlur(tfl_ctx* ctx, const tfl_tensor* src, int blurRad, int is3D, const tfl_tensor* dst,
                        const tfl_tensor* tmp);
int tfl_signedDistanceField(tfl_ctx* ctx, const tfl_tensor* flags, int searchRad, int is3D, const tfl_tensor* dst);
int64_t tfl_pcg_workspace_floats(int32_t Z, int32_t Y, int32_t X);
int64_t tfl_pcg_workspace_floats_for(int32_t Z, int32_t Y, int32_t X, const char* precondType);
int64_t tfl_pcg_last_iterations(tfl_ctx* ctx);
int tfl_solveLinearSystemPCG(tfl_ctx* ctx, const tfl_tensor* p, const tfl_tensor* flags, const tfl_tensor* div,
                             int is3D, const char* precondType, float tol, int maxIter, int verbose,
                             float* workspace, int64_t workspace_floats, float* residual);
int64_t tfl_pcg_batched_workspace_floats(int32_t B, int32_t Z, int32_t Y, int32_t X, const char* precondType);
int tfl_solveLinearSystemPCGBatched(tfl_ctx* ctx, const tfl_tensor* p, const tfl_tensor* flags, const tfl_tensor* div,
                                    int is3D, const char* precondType, float tol, int maxIter, float* workspace,
                                    int64_t workspace_floats, float* residuals, int64_t* iterations);
int64_t tfl_normalize_workspace_floats(int32_t Z, int32_t Y, int32_t X);
int tfl_normalizePressureMean(tfl_ctx* ctx, const tfl_tensor* p, const tfl_tensor* flags, int is3D, float* workspace,
                              int64_t workspace_floats);
int tfl_solveLinearSystemJacobi(tfl_ctx* ctx, const tfl_tensor* p, const tfl_tensor* flags,
                                const tfl_tensor* div, const tfl_tensor* pPrev,
                                const tfl_tensor* pDelta, const tfl_tensor* pDeltaNorm, int is3D,
                                float pTol, int maxIter, int verbose, float* residual);
int tfl_velocityDivergenceBackward(tfl_ctx* ctx, const tfl_tensor* U, const tfl_tensor* flags,
                                   const tfl_tensor* gradOutput, int is3D, const tfl_tensor* gradU);
int tfl_velocityUpdateBackward(tfl_ctx* ctx, const tfl_tensor* U, const tfl_tensor* flags, const tfl_tensor* p,
                               const tfl_tensor* gradOutput, int is3D, const tfl_tensor* gradP);
int tfl_setWallBcsBackward(tfl_ctx* ctx, const tfl_tensor* flags, const tfl_tensor* gradOutput, int is3D,
                           const tfl_tensor* gradU);
int tfl_volumetricUpSamplingNearestForward(tfl_ctx* ctx, int ratio, const tfl_tensor* input,
                                           const tfl_tensor* output);
int tfl_volumetricUpSamplingNearestBackward(tfl_ctx* ctx, int ratio, const tfl_tensor* input,
                                            const tfl_tensor* gradOutput, const tfl_tensor* gradInput);
typedef struct tfl_model tfl_model;
tfl_model* tfl_model_create(tfl_ctx* ctx, int is3D, int nlayers, const int32_t* cin, const int32_t* cout,
                            const int32_t* ksize, const float* const* weights,
                            const float* const* biases);
tfl_model* tfl_model_create_ex(tfl_ctx* ctx, int is3D, int nlayers, const int32_t* cin, const int32_t* cout,
                               const int32_t* ksize, const int32_t* pool, const int32_t* up,
                               const float* const* weights, const float* const* biases);
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
enum { TFL_BANKS_MRES = 0, TFL_BANKS_DILATE = 1 };
enum { TFL_AGG_CONCAT = 0, TFL_AGG_ADD = 1 };
enum { TFL_POOL_AVG = 0, TFL_POOL_MAX = 1 };
typedef struct tfl_model_graph {
  int32_t banks_num;
  int32_t bank_type;
  int32_t aggregate;
  int32_t split_stage, join_stage;
  int32_t pool_type;
  int32_t batch_norm;
  const float* const* bn_mean;
  const float* const* bn_var;
  const float* const* bn_weight;
  const float* const* bn_bias;
  const double* bn_eps;
} tfl_model_graph;
tfl_model* tfl_model_create_graph(tfl_ctx* ctx, int is3D, int nconv, const int32_t* cin, const int32_t* cout,
                                  const int32_t* ksize, const int32_t* pool, const int32_t* up,
                                  const float* const* weights, const float* const* biases, const tfl_model_opts* opts,
                                  const tfl_model_graph* graph);
void tfl_model_destroy(tfl_ctx* ctx, tfl_model* model);
int64_t tfl_model_range_errors(tfl_ctx* ctx, tfl_model* model);
int64_t tfl_model_range_flag(tfl_ctx* ctx, tfl_model* model);
int64_t tfl_model_workspace_floats(const tfl_model* model, int B, int Z, int Y, int X);
int tfl_model_forward(tfl_ctx* ctx, tfl_model* model, const tfl_tensor* pDiv, const tfl_tensor* UDiv,
                      const tfl_tensor* flags, const tfl_tensor* pOut, const tfl_tensor* UOut,
                      float* workspace, int64_t workspace_floats, const tfl_tensor* UBC,
                      const tfl_tensor* UBCInvMask, int doClamp, float lo, float hi);
int tfl_model_begin(tfl_ctx* ctx, tfl_model* model, const tfl_tensor* UDiv, const tfl_tensor* flags,
                    const tfl_tensor* UOut, float* workspace, int64_t workspace_floats, int zlo, int zhi,
                    double* stats);
int tfl_model_finish(tfl_ctx* ctx, tfl_model* model, const tfl_tensor* pDiv, const tfl_tensor* flags,
                     const tfl_tensor* pOut, const tfl_tensor* UOut, float* workspace,
                     int64_t workspace_floats, const double* stats, double count, const tfl_tensor* UBC,
                     const tfl_tensor* UBCInvMask, int doClamp, float lo, float hi);
int tfl_model_set_weights(tfl_ctx* ctx, tfl_model* model, const float* const* weights, const float* const* biases);
int tfl_model_enable_multires_training(tfl_ctx* ctx, tfl_model* model);
int64_t tfl_model_tape_floats(const tfl_model* model, int B, int Z, int Y, int X);
int tfl_model_forward_train(tfl_ctx* ctx, tfl_model* model, const tfl_tensor* pDiv, const tfl_tensor* UDiv,
                            const tfl_tensor* flags, const tfl_tensor* pOut, const tfl_tensor* UOut, float* workspace,
                            int64_t workspace_floats, float* tape, int64_t tape_floats);
int64_t tfl_model_backward_workspace_floats(const tfl_model* model, int B, int Z, int Y, int X);
int tfl_model_backward(tfl_ctx* ctx, tfl_model* model, const tfl_tensor* flags, const tfl_tensor* gradP,
                       const tfl_tensor* gradU, const float* tape, int64_t tape_floats, float* workspace,
                       int64_t workspace_floats, float* const* gradWeights, float* const* gradBiases, int accumulate);
int64_t tfl_model_backward_input_workspace_floats(const tfl_model* model, int B, int Z, int Y, int X);
int tfl_model_backward_input(tfl_ctx* ctx, tfl_model* model, const tfl_tensor* flags, const tfl_tensor* pDiv,
                             const tfl_tensor* UDiv, const tfl_tensor* UOut, const tfl_tensor* gradP, const tfl_tensor* gradU,
                             const float* tape, int64_t tape_floats, float* workspace, int64_t workspace_floats,
                             float* const* gradWeights, float* const* gradBiases, int accumulate, const tfl_tensor* gradPDiv,
                             const tfl_tensor* gradUDiv);
int tfl_model_set_weights_device(tfl_ctx* ctx, tfl_model* model, const float* const* d_weights, const float* const* d_biases);
enum { TFL_OPTIM_ADAM = 0, TFL_OPTIM_RMSPROP = 1 };
typedef struct tfl_optim tfl_optim;
typedef struct {
  int32_t method;
  double learningRate, learningRateDecay, beta1, beta2, epsilon, weightDecay;
  double alpha, initialMean;
  double gradNormThreshold;
} tfl_optim_config;
tfl_optim* tfl_optim_create(tfl_ctx* ctx, tfl_model* model, const tfl_optim_config* config);
int tfl_optim_step(tfl_ctx* ctx, tfl_optim* opt, float* const* d_weights, float* const* d_biases,
                   float* const* d_gradWeights, float* const* d_gradBiases);
int tfl_optim_step_guarded(tfl_ctx* ctx, tfl_optim* opt, float* const* d_weights, float* const* d_biases,
                           float* const* d_gradWeights, float* const* d_gradBiases, const int32_t* d_guard);
int tfl_optim_set_config(tfl_ctx* ctx, tfl_optim* opt, const tfl_optim_config* config);
int64_t tfl_optim_steps(tfl_ctx* ctx, tfl_optim* opt);
int64_t tfl_optim_get_state(tfl_ctx* ctx, tfl_optim* opt, float* d_m, float* d_v);
void tfl_optim_destroy(tfl_ctx* ctx, tfl_optim* opt);
int tfl_set_dx_override(tfl_ctx* ctx, float dx);
int tfl_applyBCs(tfl_ctx* ctx, const tfl_tensor* x, const tfl_tensor* bc, const tfl_tensor* invMask,
                 int doClamp, float lo, float hi);
int tfl_applyBCsIndexed(tfl_ctx* ctx, const tfl_tensor* x, const tfl_tensor* bc, const tfl_tensor* invMask,
                        const int32_t* idx, int64_t n);
int tfl_applyBCsIndexedMulti(tfl_ctx* ctx, int count, const tfl_tensor* const* x, const tfl_tensor* const* bc,
                             const tfl_tensor* const* invMask, const int32_t* const* idx, const int64_t* n);
double tfl_getDx(tfl_ctx* ctx, const tfl_tensor* flags);
int tfl_copy(tfl_ctx* ctx, const tfl_tensor* dst, const tfl_tensor* src);
int tfl_stream_copy(tfl_ctx* ctx, float* dst, const float* src, int64_t n);
typedef struct tfl_bc_plan tfl_bc_plan;
tfl_bc_plan* tfl_bc_plan_create(tfl_ctx* ctx, const tfl_tensor* bc, const tfl_tensor* invMask);
void tfl_bc_plan_destroy(tfl_ctx* ctx, tfl_bc_plan* plan);
typedef struct tfl_wall_plan tfl_wall_plan;
tfl_wall_plan* tfl_wall_plan_create(tfl_ctx* ctx, const tfl_tensor* flags);
void tfl_wall_plan_destroy(tfl_ctx* ctx, tfl_wall_plan* plan);
void tfl_wall_plan_retire(tfl_wall_plan* plan);
typedef struct tfl_sim_params {
  float dt;
  const char* advectionMethod;
  float maccormackStrength;
  double buoyancyScale;
  double gravityScale;
  float gravity[3];
  double vorticityConfinementAmp;
  const char* simMethod;
  int32_t maxIter;
  const char* pcgPrecond;
  int32_t outputDiv;
} tfl_sim_params;
typedef struct tfl_sim_state {
  const tfl_tensor* p;
  const tfl_tensor* U;
  const tfl_tensor* flags;
  int32_t n_density;
  const tfl_tensor* density[8];
  const tfl_bc_plan* pBC;
  const tfl_bc_plan* UBC;
  const tfl_bc_plan* densityBC[8];
  tfl_model* model;
} tfl_sim_state;
int64_t tfl_simulate_workspace_floats(tfl_ctx* ctx, const tfl_sim_params* params, const tfl_sim_state* state);
int tfl_simulate_step(tfl_ctx* ctx, const tfl_sim_params* params, const tfl_sim_state* state, float* workspace,
                      int64_t workspace_floats);
int tfl_simulate_project(tfl_ctx* ctx, const tfl_sim_params* params, const tfl_sim_state* state, float* workspace,
                         int64_t workspace_floats);
typedef struct tfl_sim_item {
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
int tfl_packPlanes(tfl_ctx* ctx, int n, const tfl_tensor* const* fields, int zlo, int zhi, float* buf,
                   int unpack);
int tfl_set_z_window(tfl_ctx* ctx, int a0, int a1, int b0, int b1);
int tfl_set_z_origin(tfl_ctx* ctx, int z_first, int z_total);
int tfl_set_stages(tfl_ctx* ctx, int mask);
float* tfl_model_div(const tfl_model* model, int B, int Z, int Y, int X, float* workspace);
typedef struct tfl_slab {
  int32_t z_total;
  int32_t z_first;
  int32_t own_lo, own_hi;
  int32_t reach;
  int32_t overlap;
  int32_t check_reach;
  int32_t in_flight;
} tfl_slab;
typedef struct tfl_comm_chunk {
  float* ptr;
  int64_t n;
} tfl_comm_chunk;
typedef struct tfl_comm {
  int32_t size;
  void* user;
  int (*exchange_start)(void* user, int tag, const float* send_lo, int64_t n_send_lo, float* recv_lo, int64_t n_recv_lo,
                        const float* send_hi, int64_t n_send_hi, float* recv_hi, int64_t n_recv_hi);
  int (*exchange_wait)(void* user, int tag);
  int (*allreduce_sum)(void* user, double* dev, int64_t n);
  int (*exchange_start_v)(void* user, int tag, int n_lo, const tfl_comm_chunk* send_lo, const tfl_comm_chunk* recv_lo,
                          int n_hi, const tfl_comm_chunk* send_hi, const tfl_comm_chunk* recv_hi);
  int32_t capturable;
} tfl_comm;
int32_t tfl_slab_halo(int32_t reach);
int32_t tfl_slab_halo_model(const tfl_model* model, int32_t reach);
int64_t tfl_simulate_slab_workspace_floats(tfl_ctx* ctx, const tfl_sim_params* params, const tfl_sim_state* state,
                                           const tfl_slab* slab);
int tfl_simulate_step_slab(tfl_ctx* ctx, const tfl_sim_params* params, const tfl_sim_state* state, tfl_slab* slab,
                           const tfl_comm* comm, float* workspace, int64_t workspace_floats);
int32_t tfl_slab_needed_reach(const tfl_ctx* ctx);
int64_t tfl_slab_exchange_floats(int n, const tfl_tensor* const* fields, const int32_t* below, const int32_t* above, const tfl_slab* slab);
int tfl_slab_exchange(tfl_ctx* ctx, int n, const tfl_tensor* const* fields, const int32_t* below, const int32_t* above,
                      const tfl_slab* slab, const tfl_comm* comm, float* scratch, int64_t scratch_floats);
int tfl_slab_drain(tfl_ctx* ctx, const tfl_sim_state* state, tfl_slab* slab, const tfl_comm* comm, float* workspace,
                   int64_t workspace_floats);
int tfl_slab_divergence_norm(tfl_ctx* ctx, const tfl_sim_state* state, tfl_slab* slab, const tfl_comm* comm, float* workspace,
                             int64_t workspace_floats, double* norm);
typedef struct tfl_slab_graph tfl_slab_graph;
tfl_slab_graph* tfl_slab_graph_create(tfl_ctx* ctx, const tfl_sim_params* params, const tfl_sim_state* state, tfl_slab* slab,
                                      const tfl_comm* comm, float* workspace, int64_t workspace_floats);
int tfl_slab_graph_step(tfl_ctx* ctx, tfl_slab_graph* graph);
int64_t tfl_slab_graph_nodes(const tfl_slab_graph* graph);
void tfl_slab_graph_destroy(tfl_ctx* ctx, tfl_slab_graph* graph);
typedef struct tfl_rccl_comm tfl_rccl_comm;
int tfl_rccl_available(tfl_ctx* ctx);
const char* tfl_rccl_comm_origin(tfl_ctx* ctx);
int tfl_rccl_get_unique_id(tfl_ctx* ctx, void* id);
tfl_rccl_comm* tfl_rccl_comm_create(tfl_ctx* ctx, const void* id, int rank, int world);
tfl_rccl_comm* tfl_rccl_comm_wrap(tfl_ctx* ctx, void* nccl_comm, int rank, int world);
const tfl_comm* tfl_rccl_comm_callbacks(tfl_rccl_comm* comm);
int tfl_rccl_comm_set_inline(tfl_rccl_comm* comm, int on);
void tfl_rccl_comm_destroy(tfl_ctx* ctx, tfl_rccl_comm* comm);
int64_t tfl_optim_reduce_doubles(tfl_ctx* ctx, tfl_optim* opt);
int tfl_optim_step_reduced(tfl_ctx* ctx, tfl_optim* opt, float* const* d_weights, float* const* d_biases,
                           float* const* d_gradWeights, float* const* d_gradBiases, const int32_t* d_guard,
                           const tfl_comm* comm, int32_t world, double* d_reduce, int64_t reduce_doubles);
int tfl_optim_reduced_guard(tfl_ctx* ctx, tfl_optim* opt, int32_t* d_out);
int tfl_optim_sync_parameters(tfl_ctx* ctx, tfl_optim* opt, float* const* d_weights, float* const* d_biases,
                              const tfl_comm* comm, int32_t rank, double* d_reduce, int64_t reduce_doubles);
int tfl_optim_set_state(tfl_ctx* ctx, tfl_optim* opt, const float* d_m, const float* d_v, int64_t steps);
typedef struct tfl_frames tfl_frames;
tfl_frames* tfl_frames_create(tfl_ctx* ctx, int is3D, int Z, int Y, int X, int64_t capacity, int64_t device_frames);
void tfl_frames_destroy(tfl_ctx* ctx, tfl_frames* frames);
int64_t tfl_frames_record_floats(const tfl_frames* frames);
int tfl_frames_put(tfl_ctx* ctx, tfl_frames* frames, int64_t slot, const float* h_record);
int tfl_frames_gather(tfl_ctx* ctx, tfl_frames* frames, int n, const int32_t* h_slots,
                      const tfl_tensor* pDiv, const tfl_tensor* UDiv, const tfl_tensor* flags,
                      const tfl_tensor* densityDiv, const tfl_tensor* pTarget, const tfl_tensor* UTarget,
                      const tfl_tensor* densityTarget);
int tfl_frames_put_device(tfl_ctx* ctx, tfl_frames* frames, int n, const int32_t* h_slots,
                          const tfl_tensor* pDiv, const tfl_tensor* UDiv, const tfl_tensor* flags,
                          const tfl_tensor* densityDiv, const tfl_tensor* pTarget, const tfl_tensor* UTarget,
                          const tfl_tensor* densityTarget);
typedef struct tfl_scene_prim {
  int32_t kind;
  float a[3];
  float b[3];
  float val;
} tfl_scene_prim;
int tfl_scene_flags(tfl_ctx* ctx, const tfl_scene_prim* obstacles, int n_obstacles, const tfl_scene_prim* blobs, int n_blobs,
                    int is3D, const tfl_tensor* flags, const tfl_tensor* density);
int tfl_noise_potential(tfl_ctx* ctx, uint32_t seed, uint32_t run, const tfl_tensor* psi);
int tfl_curl_mac(tfl_ctx* ctx, const tfl_tensor* psi, float amp, int is3D, const tfl_tensor* U);
]]
-- END generated cdef

local M = {}
local lib, ctx

local function check(rc)
  if rc ~= 0 then error(ffi.string(lib.tfl_last_error(ctx)), 3) end
end

-- 5-D (or lower-rank: leading sizes padded with 1) contiguous float tensor -> tfl_tensor
local function T(t)
  assert(t:isContiguous(), 'Input is not contiguous')
  local d = ffi.new('tfl_tensor')
  d.data = ffi.cast('float*', torch.data(t))
  local n = t:dim()
  local sz = {1, 1, 1, 1, 1}
  for i = 1, n do sz[5 - n + i] = t:size(i) end
  d.B, d.C, d.Z, d.Y, d.X = sz[1], sz[2], sz[3], sz[4], sz[5]
  return d
end

local function vec3(t)  -- gravity arrives as a 3-element tensor (init.lua:455-458); the ABI wants host floats
  local h = t:float()
  return ffi.new('float[3]', h[1], h[2], h[3])
end

local function b2i(b) return b and 1 or 0 end

-- One grow-only device scratch (the analogue of init.lua:35-64's shared buffer) for the entry points that take a
-- caller workspace (PCG, normalizePressureMean, the model, the whole step).
local scratch
local function workspace(like, nfloats)
  nfloats = tonumber(nfloats)
  if scratch == nil or scratch:nElement() < nfloats then scratch = like.new():resize(nfloats) end
  return ffi.cast('float*', torch.data(scratch)), nfloats
end

-- ---- the native operator table (same positional signatures as tfluids_CudaMain_*) ----------------------------------
local ops = {}
function ops.advectScalar(dt, s, U, flags, fwd, bwd, is3D, method, fwdPos, bwdPos, bnd, outside, strength, sDst)
  check(lib.tfl_advectScalar(ctx, dt, T(s), T(U), T(flags), T(fwd), T(bwd), b2i(is3D), method,
                             T(fwdPos), T(bwdPos), bnd, b2i(outside), strength, T(sDst)))
end
function ops.advectVel(dt, U, flags, fwd, bwd, is3D, method, bnd, strength, UDst)
  check(lib.tfl_advectVel(ctx, dt, T(U), T(flags), T(fwd), T(bwd), b2i(is3D), method, bnd, strength, T(UDst)))
end
function ops.setWallBcsForward(U, flags, is3D)
  check(lib.tfl_setWallBcsForward(ctx, T(U), T(flags), b2i(is3D)))
end
function ops.velocityDivergenceForward(U, flags, UDiv, is3D)
  check(lib.tfl_velocityDivergenceForward(ctx, T(U), T(flags), T(UDiv), b2i(is3D)))
end
function ops.velocityUpdateForward(U, flags, p, is3D)
  check(lib.tfl_velocityUpdateForward(ctx, T(U), T(flags), T(p), b2i(is3D)))
end
function ops.vorticityConfinement(U, flags, strength, centered, curl, curlNorm, force, is3D)
  check(lib.tfl_vorticityConfinement(ctx, T(U), T(flags), strength, T(centered), T(curl), T(curlNorm), T(force), b2i(is3D)))
end
function ops.addBuoyancy(U, flags, density, gravity, strengthTmp, dt, is3D)
  check(lib.tfl_addBuoyancy(ctx, T(U), T(flags), T(density), vec3(gravity), nil, dt, b2i(is3D)))
end
function ops.addGravity(U, flags, gravity, dt, is3D, forceTmp)
  check(lib.tfl_addGravity(ctx, T(U), T(flags), vec3(gravity), dt, b2i(is3D), nil))
end
function ops.emptyDomain(flags, is3D, bnd)
  check(lib.tfl_emptyDomain(ctx, T(flags), b2i(is3D), bnd))
end
function ops.flagsToOccupancy(flags, occupancy)
  check(lib.tfl_flagsToOccupancy(ctx, T(flags), T(occupancy)))
end
function ops.rectangularBlur(src, blurRad, is3D, dst, tmp)
  check(lib.tfl_rectangularBlur(ctx, T(src), blurRad, b2i(is3D), T(dst), T(tmp)))
end
function ops.signedDistanceField(flags, searchRad, is3D, dst)
  check(lib.tfl_signedDistanceField(ctx, T(flags), searchRad, b2i(is3D), T(dst)))
end
function ops.velocityDivergenceBackward(U, flags, gradOutput, is3D, gradU)
  check(lib.tfl_velocityDivergenceBackward(ctx, T(U), T(flags), T(gradOutput), b2i(is3D), T(gradU)))
end
function ops.velocityUpdateBackward(U, flags, p, gradOutput, is3D, gradP)
  check(lib.tfl_velocityUpdateBackward(ctx, T(U), T(flags), T(p), T(gradOutput), b2i(is3D), T(gradP)))
end
-- not a native entry of the reference (tfluids.SetWallBcs:updateGradInput does it with a mask tensor,
-- set_wall_bcs.lua:50-66); exposed for a module override: gradInput[1] = hip.setWallBcsBackward(flags, gradOutput)
function M.setWallBcsBackward(flags, gradOutput, gradU)
  gradU = gradU or gradOutput.new():resizeAs(gradOutput)
  check(lib.tfl_setWallBcsBackward(ctx, T(flags), T(gradOutput), b2i(gradOutput:size(2) == 3), T(gradU)))
  return gradU
end
function ops.volumetricUpSamplingNearestForward(ratio, input, output)
  check(lib.tfl_volumetricUpSamplingNearestForward(ctx, ratio, T(input), T(output)))
end
function ops.volumetricUpSamplingNearestBackward(ratio, input, gradOutput, gradInput)
  check(lib.tfl_volumetricUpSamplingNearestBackward(ctx, ratio, T(input), T(gradOutput), T(gradInput)))
end
function ops.solveLinearSystemJacobi(p, flags, div, pPrev, pDelta, pDeltaNorm, is3D, pTol, maxIter, verbose)
  local res = ffi.new('float[1]')
  check(lib.tfl_solveLinearSystemJacobi(ctx, T(p), T(flags), T(div), T(pPrev), T(pDelta), T(pDeltaNorm),
                                        b2i(is3D), pTol, maxIter, b2i(verbose), res))
  return res[0]
end
-- init.lua:674-676: p.tfluids.solveLinearSystemPCG(tfluids._tmpPCG, p, flags, div, is3D, precondType, tol, maxIter,
-- verbose) -> residual. The reference's cache table of cuSPARSE temporaries is ignored: the workspace is ours.
function ops.solveLinearSystemPCG(tmpPCG, p, flags, div, is3D, precondType, tol, maxIter, verbose)
  -- sized for the preconditioner ('mg' adds its hierarchy); a name that is none gets the common size and is refused by the call
  local need = lib.tfl_pcg_workspace_floats_for(flags:size(3), flags:size(4), flags:size(5), precondType)
  if need < 0 then need = lib.tfl_pcg_workspace_floats(flags:size(3), flags:size(4), flags:size(5)) end
  local ws, n = workspace(p, need)
  local res = ffi.new('float[1]')
  check(lib.tfl_solveLinearSystemPCG(ctx, T(p), T(flags), T(div), b2i(is3D), precondType, tol, maxIter,
                                     b2i(verbose), ws, n, res))
  return res[0]
end
-- CG iterations of the last solveLinearSystemPCG, summed over its component solves (-1 before any solve)
function ops.pcgLastIterations()
  return tonumber(lib.tfl_pcg_last_iterations(ctx))
end

-- ---- tfluids.normalizePressureMean on the device (init.lua:747-764 copies to the host and back) ---------------------
function M.normalizePressureMean(p, flags, is3D)
  local ws, n = workspace(p, lib.tfl_normalize_workspace_floats(flags:size(3), flags:size(4), flags:size(5)))
  check(lib.tfl_normalizePressureMean(ctx, T(p), T(flags), b2i(is3D), ws, n))
end

-- ---- the projection ConvNet: hip.Model(gmodule) has the call shape of the nngraph model ------------------------------
-- Walks nn.gModule.forwardnodes in order and collects the convolution layers (cudnn / nn {Spatial,Volumetric}Convolution
-- built by lib/model_utils.lua:80-116), exactly what fluidnet_amd/torch7.py:conv_layers does for the Python binding.
local Model = {}
Model.__index = Model

-- The gModule walk of fluidnet_amd/torch7.py model_graph (lib/model.lua:253-392): the conv modules by their
-- `Bank i: conv stage N` annotation in the reference's creation order (stage, then bank; the unannotated output conv last),
-- and along each one's single consumer chain the pooling and batch norm that follow its non-linearity. Refuses by name
-- what the library does not build: gated (CMulTable) and low-rank (Sequential of convs) convolutions, a batch norm in
-- training mode, weight sharing. Returns {convs = {{module, stage, bank, pool, bn}}, poolType}.
local function is_conv(m) return m ~= nil and torch.type(m):find('Convolution') ~= nil end
local function graph_walk(gmodule, mconf)
  local nodes, users = {}, {}
  for _, node in ipairs(gmodule.forwardnodes) do
    local d = node.data
    local ins = {}
    for i, v in ipairs(d.mapindex or {}) do ins[i] = v.forwardNodeId end
    nodes[d.forwardNodeId] = {m = d.module, name = d.annotations and d.annotations.name, ins = ins}
  end
  for id, nd in pairs(nodes) do
    for _, i in ipairs(nd.ins) do users[i] = users[i] or {}; users[i][#users[i] + 1] = id end
  end
  if mconf.banksWeightShare then error('banksWeightShare: weight sharing is not supported (model.lua:326-328)', 3) end
  local convs, last = {}, nil
  for id, nd in pairs(nodes) do
    local tn = nd.m and torch.type(nd.m) or ''
    local what = tostring(nd.name or id)
    if tn == 'nn.CMulTable' then error('node ' .. what .. ': gated convolutions (CMulTable) are not supported', 3) end
    if tn == 'nn.Sequential' then
      for _, sm in ipairs(nd.m.modules) do
        if is_conv(sm) then error('node ' .. what .. ': low-rank convolutions (Sequential of convolutions) are not supported', 3) end
      end
    end
    if is_conv(nd.m) then
      local bank, stage = (nd.name or ''):match('^Bank (%d+): conv stage (%d+)$')
      if bank then convs[#convs + 1] = {m = nd.m, stage = tonumber(stage), bank = tonumber(bank) - 1, id = id}
      elseif last == nil then last = id
      else error('node ' .. what .. ': a convolution outside the layer stages', 3) end
    end
  end
  assert(last ~= nil and #convs > 0, 'no convolution stages found in the model')
  table.sort(convs, function(x, y) return x.stage < y.stage or (x.stage == y.stage and x.bank < y.bank) end)
  convs[#convs + 1] = {m = nodes[last].m, stage = convs[#convs].stage + 1, bank = 0, id = last, last = true}
  local pool_type = nil
  for _, c in ipairs(convs) do
    c.pool = 1
    local cur = c.id
    while not c.last and users[cur] ~= nil and #users[cur] == 1 do
      cur = users[cur][1]
      local m, name = nodes[cur].m, nodes[cur].name or ''
      local tn = m and torch.type(m) or ''
      if m == nil or is_conv(m) or tn:find('Table') or tn:find('UpSampling') or tn:find('Unsqueeze') or name:find('downsample') then break end
      if tn:find('MaxPooling') or tn:find('AveragePooling') then
        c.pool = m.kW
        local pt = tn:find('MaxPooling') and 'max' or 'avg'
        assert(pool_type == nil or pool_type == pt, 'both average and max pooling layers')
        pool_type = pt
      elseif tn:find('BatchNormalization') then
        if m.train then error('node ' .. tostring(nodes[cur].name or cur) .. ': batch norm in training mode (call model:evaluate() before saving)', 3) end
        c.bn = m
      end
    end
  end
  return {convs = convs, poolType = pool_type or mconf.poolType or 'avg'}
end

-- mconf (optional): the model's configuration table (torch.loadModel returns it next to the graph); its fields
-- inputChannels / normalizeInput* / nonlinType / addPressureSkip select the forward graph as lib/model.lua:27-160 does, and
-- with it the graph is walked as a whole (graph_walk: banks, dilation, pooling, batch norm; tfl_model_create_graph).
-- Without it, a graph holding batch-norm, dilated, pooling, upsampling or bank-join nodes is refused: the flat walk below
-- would drop them.
-- opts (optional): {train = true} gives a linear model with pooling / ConvolutionUpsample layers (`tog`) its training pass at
-- creation (tfl_model_enable_multires_training); a model that trains anyway is left as it is, a graph model (banks, max
-- pooling, batch norm) with such stages raises the library's refusal.
function M.Model(gmodule, mconf, opts_)
  if mconf == nil then
    for _, node in ipairs(gmodule.forwardnodes) do
      local tn = node.data.module and torch.type(node.data.module) or ''
      for _, h in ipairs({'BatchNormalization', 'Dilated', 'Pooling', 'UpSampling', 'ConvolutionUpsample', 'CAddTable', 'CMulTable'}) do
        if tn:find(h) then error('the model holds ' .. tn .. ' nodes: pass its mconf (torch.loadModel) to build it', 2) end
      end
    end
  end
  local cin, cout, ks, ws, bs, keep = {}, {}, {}, {}, {}, {}
  local pool, up = {}, {}
  local is3D = false
  local walk = mconf ~= nil and graph_walk(gmodule, mconf) or nil
  local function add_conv(m)
    local u = 1
    if torch.type(m):find('ConvolutionUpsample') then u = m.scaleW; m = m.modules[1] end
    is3D = torch.type(m):find('Volumetric') ~= nil
    local w, b = m.weight:float():contiguous(), m.bias:float():contiguous()   -- [nOut][nIn][k(z)][k(y)][k(x)]
    keep[#keep + 1] = w; keep[#keep + 1] = b
    cin[#cin + 1] = m.nInputPlane; cout[#cout + 1] = m.nOutputPlane / (u ^ (is3D and 3 or 2)); ks[#ks + 1] = m.kW
    ws[#ws + 1] = ffi.cast('const float*', torch.data(w)); bs[#bs + 1] = ffi.cast('const float*', torch.data(b))
    up[#up + 1] = u
    return m
  end
  if walk then
    for _, c in ipairs(walk.convs) do
      local m = add_conv(c.m)
      local dil = m.dilationW or 1
      local want = (mconf.banksNum or 1) > 1 and mconf.banksType == 'dilate' and 2 ^ c.bank or 1
      if dil ~= want then error('stage ' .. c.stage .. ' bank ' .. (c.bank + 1) .. ': dilation ' .. dil .. ' is not what banksType builds', 2) end
      pool[#pool + 1] = c.pool
    end
  else
    for _, node in ipairs(gmodule.forwardnodes) do
      local m = node.data.module
      if m and torch.type(m):find('Convolution') then add_conv(m); pool[#pool + 1] = 1 end
    end
  end
  local n = #cin
  assert(n > 0, 'no convolution layers found in the model')
  local self = setmetatable({is3D = is3D}, Model)
  local opts = nil
  if mconf ~= nil then
    local ic = mconf.inputChannels or {pDiv = true, UDiv = false, div = true, flags = true}
    assert(ic.flags ~= false, 'Are you sure you dont want flags?')
    local chan = ({UDiv = lib.TFL_NORM_UDIV, pDiv = lib.TFL_NORM_PDIV, div = lib.TFL_NORM_DIV})[mconf.normalizeInputChan or 'UDiv']
    local func = ({std = lib.TFL_NORMFUNC_STD, norm = lib.TFL_NORMFUNC_L2})[mconf.normalizeInputFunc or 'std']
    local nonlin = ({relu = lib.TFL_NONLIN_RELU, relu6 = lib.TFL_NONLIN_RELU6, sigmoid = lib.TFL_NONLIN_SIGMOID})[mconf.nonlinType or 'relu']
    assert(chan and func and nonlin, 'bad normalizeInputChan / normalizeInputFunc / nonlinType')
    opts = ffi.new('tfl_model_opts', {b2i(ic.pDiv), b2i(ic.UDiv), b2i(ic.div), b2i(mconf.normalizeInput ~= false), chan, func,
                                      nonlin, b2i(mconf.addPressureSkip == true)})
  end
  local c_cin, c_cout, c_ks = ffi.new('int32_t[?]', n, cin), ffi.new('int32_t[?]', n, cout), ffi.new('int32_t[?]', n, ks)
  local c_ws, c_bs = ffi.new('const float*[?]', n, ws), ffi.new('const float*[?]', n, bs)
  if walk then
    local g = ffi.new('tfl_model_graph')
    g.banks_num = mconf.banksNum or 1
    g.bank_type = (mconf.banksType == 'dilate') and lib.TFL_BANKS_DILATE or lib.TFL_BANKS_MRES
    g.aggregate = (mconf.banksAggregateMethod == 'add') and lib.TFL_AGG_ADD or lib.TFL_AGG_CONCAT
    g.split_stage, g.join_stage = mconf.banksSplitStage or 1, mconf.banksJoinStage or 3
    g.pool_type = walk.poolType == 'max' and lib.TFL_POOL_MAX or lib.TFL_POOL_AVG
    local nbn = 0
    for i = 1, n - 1 do if walk.convs[i].bn then nbn = nbn + 1 end end
    if nbn ~= 0 and nbn ~= n - 1 then error('batch norm after some hidden stages only', 2) end
    if (nbn > 0) ~= (mconf.addBatchNorm == true) then error('mconf.addBatchNorm does not match the graph\'s batch-norm nodes', 2) end
    if nbn > 0 then
      g.batch_norm = 1
      local mean, var = ffi.new('const float*[?]', n - 1), ffi.new('const float*[?]', n - 1)
      local wt, bi = ffi.new('const float*[?]', n - 1), ffi.new('const float*[?]', n - 1)
      local eps = ffi.new('double[?]', n - 1)
      local function ptr(t) if t == nil then return nil end; t = t:float():contiguous(); keep[#keep + 1] = t; return ffi.cast('const float*', torch.data(t)) end
      for i = 1, n - 1 do
        local bn = walk.convs[i].bn
        mean[i - 1], var[i - 1] = ptr(bn.running_mean), ptr(bn.running_var)
        wt[i - 1], bi[i - 1], eps[i - 1] = ptr(bn.weight), ptr(bn.bias), bn.eps
      end
      keep[#keep + 1] = {mean, var, wt, bi, eps}
      g.bn_mean, g.bn_var, g.bn_weight, g.bn_bias, g.bn_eps = mean, var, wt, bi, eps
    end
    self.handle = lib.tfl_model_create_graph(ctx, b2i(is3D), n, c_cin, c_cout, c_ks, ffi.new('int32_t[?]', n, pool),
                                             ffi.new('int32_t[?]', n, up), c_ws, c_bs, opts, g)
  elseif opts == nil then
    self.handle = lib.tfl_model_create(ctx, b2i(is3D), n, c_cin, c_cout, c_ks, c_ws, c_bs)
  else
    self.handle = lib.tfl_model_create_opts(ctx, b2i(is3D), n, c_cin, c_cout, c_ks, nil, nil, c_ws, c_bs, opts)
  end
  if self.handle == nil then error(ffi.string(lib.tfl_last_error(ctx)), 2) end
  ffi.gc(self.handle, function(h) lib.tfl_model_destroy(ctx, h) end)
  if opts_ and opts_.train then check(lib.tfl_model_enable_multires_training(ctx, self.handle)) end
  return self
end

-- model:forward({pDiv, UDiv, flags}) -> {p, U} (lib/model.lua:398, 421-450). The outputs are fresh tensors, like the
-- module outputs of the nngraph model; lib/simulate.lua:270-272 copies them into the state.
function Model:forward(input)
  local pDiv, UDiv, flags = input[1], input[2], input[3]
  self.p = self.p or pDiv.new(); self.U = self.U or UDiv.new()
  self.p:resizeAs(pDiv); self.U:resizeAs(UDiv)
  local ws, n = workspace(pDiv, lib.tfl_model_workspace_floats(self.handle, flags:size(1), flags:size(3), flags:size(4),
                                                               flags:size(5)))
  check(lib.tfl_model_forward(ctx, self.handle, T(pDiv), T(UDiv), T(flags), T(self.p), T(self.U), ws, n, nil, nil, 0, 0, 0))
  self.output = {self.p, self.U}
  return self.output
end
function Model:evaluate() return self end
function Model:cuda() return self end
-- The default 3-D conv path multiplies fp32 values as fp16 hi / lo pairs: an activation beyond 65504 (a blown-up simulation)
-- is clamped and counted, and the NEXT forward / simulate step is refused (check() raises, TFL_ERANGE) until the count has
-- been read. model:rangeErrors() reads and resets it (synchronises); model:rangeFlag() peeks at what the device has reported
-- so far (no synchronisation). TFL_CONV_PATH=winograd in the environment before hip.Model(...) is the strict-fp32 stack.
function Model:rangeErrors() return tonumber(lib.tfl_model_range_errors(ctx, self.handle)) end
function Model:rangeFlag() return tonumber(lib.tfl_model_range_flag(ctx, self.handle)) end

-- The training side (linear and banked models without batch norm, pooling / upsampling -- include/tfluids_hip.h; a linear model
-- with pooling / upsampling layers once it is created with {train = true}): the parameter gradients and, on
-- request, the gradients to pDiv and UDiv (model:backward's wantGradInput).
-- model:setWeights(weights, biases): tables of FloatTensors laid out like the convolutions' weight / bias, copied into the
-- model's own buffers (synchronous; re-record any slab graph built on the model).
function Model:setWeights(weights, biases)
  local n = #weights
  local ws, bs, hold = ffi.new('const float*[?]', n), ffi.new('const float*[?]', n), {}
  for i = 1, n do
    local w, b = weights[i]:float():contiguous(), biases[i]:float():contiguous()
    hold[#hold + 1] = w; hold[#hold + 1] = b
    ws[i - 1], bs[i - 1] = ffi.cast('const float*', torch.data(w)), ffi.cast('const float*', torch.data(b))
  end
  check(lib.tfl_model_set_weights(ctx, self.handle, ws, bs))
end
-- model:forwardTrain({pDiv, UDiv, flags}) -> {p, U}: the forward on the exact fp32 kernels that keeps the tape for model:backward
function Model:forwardTrain(input)
  local pDiv, UDiv, flags = input[1], input[2], input[3]
  self.p = self.p or pDiv.new(); self.U = self.U or UDiv.new()
  self.p:resizeAs(pDiv); self.U:resizeAs(UDiv)
  local B, Z, Y, X = flags:size(1), flags:size(3), flags:size(4), flags:size(5)
  local ws, n = workspace(pDiv, lib.tfl_model_workspace_floats(self.handle, B, Z, Y, X))
  local nt = tonumber(lib.tfl_model_tape_floats(self.handle, B, Z, Y, X))
  if nt < 0 then error('this model has no training pass (graph model; pooling or upsampling layers without {train = true})', 2) end
  self.tape = self.tape or pDiv.new()
  self.tape:resize(nt)
  check(lib.tfl_model_forward_train(ctx, self.handle, T(pDiv), T(UDiv), T(flags), T(self.p), T(self.U), ws, n,
                                    ffi.cast('float*', torch.data(self.tape)), nt))
  self.output = {self.p, self.U}
  self.trainInput = {pDiv, UDiv}       -- (what backward's wantGradInput reads again)
  return self.output
end
-- model:backward(flags, gradP, gradU, gradWeights, gradBiases, accumulate, wantGradInput): gradWeights / gradBiases are tables of
-- CudaTensors shaped like the convolutions' weight / bias; gradP or gradU may be nil; accumulate = true adds (accGradParameters).
-- wantGradInput = true: also returns {gradPDiv, gradUDiv} (tfl_model_backward_input; the tensors given to forwardTrain and its U
-- must be unchanged since). There is no gradient to flags.
function Model:backward(flags, gradP, gradU, gradWeights, gradBiases, accumulate, wantGradInput)
  assert(self.tape, 'model:forwardTrain first')
  local n = #gradWeights
  local gw, gb = ffi.new('float*[?]', n), ffi.new('float*[?]', n)
  for i = 1, n do
    gw[i - 1], gb[i - 1] = ffi.cast('float*', torch.data(gradWeights[i])), ffi.cast('float*', torch.data(gradBiases[i]))
  end
  local B, Z, Y, X = flags:size(1), flags:size(3), flags:size(4), flags:size(5)
  self.bwdWork = self.bwdWork or flags.new()
  if wantGradInput then
    local pDiv, UDiv = self.trainInput[1], self.trainInput[2]
    local need = tonumber(lib.tfl_model_backward_input_workspace_floats(self.handle, B, Z, Y, X))
    if self.bwdWork:nElement() < need then self.bwdWork:resize(need) end
    self.gradPDiv = self.gradPDiv or pDiv.new(); self.gradUDiv = self.gradUDiv or UDiv.new()
    self.gradPDiv:resizeAs(pDiv); self.gradUDiv:resizeAs(UDiv)
    check(lib.tfl_model_backward_input(ctx, self.handle, T(flags), T(pDiv), T(UDiv), T(self.U), gradP and T(gradP) or nil,
                                       gradU and T(gradU) or nil, ffi.cast('const float*', torch.data(self.tape)),
                                       self.tape:nElement(), ffi.cast('float*', torch.data(self.bwdWork)), self.bwdWork:nElement(),
                                       gw, gb, b2i(accumulate == true), T(self.gradPDiv), T(self.gradUDiv)))
    self.gradInput = {self.gradPDiv, self.gradUDiv}
    return self.gradInput
  end
  local need = tonumber(lib.tfl_model_backward_workspace_floats(self.handle, B, Z, Y, X))
  if self.bwdWork:nElement() < need then self.bwdWork:resize(need) end
  check(lib.tfl_model_backward(ctx, self.handle, T(flags), gradP and T(gradP) or nil, gradU and T(gradU) or nil,
                               ffi.cast('const float*', torch.data(self.tape)), self.tape:nElement(),
                               ffi.cast('float*', torch.data(self.bwdWork)), self.bwdWork:nElement(), gw, gb, b2i(accumulate == true)))
end

-- model:setWeightsDevice(weights, biases): the same from CudaTensors where they lie -- every weight form rebuilt by kernels on the
-- context's stream, no host copy and no synchronisation (the 3-D default model on its fp16 path reads 12 bytes back: header)
local function devptrs(ts, ctype)
  local p = ffi.new(ctype .. '[?]', #ts)
  for i = 1, #ts do
    assert(ts[i]:isContiguous(), 'parameter tensors must be contiguous')
    p[i - 1] = ffi.cast(ctype, torch.data(ts[i]))
  end
  return p
end
function Model:setWeightsDevice(weights, biases)
  check(lib.tfl_model_set_weights_device(ctx, self.handle, devptrs(weights, 'const float*'), devptrs(biases, 'const float*')))
end

-- ---- hip.Optim(model, method, config, gradNormThreshold): the closure's clip + optim.adam / optim.rmsprop + weight refresh as
-- ONE asynchronous call on the CudaTensors of the parameters and their gradients (tfl_optim_*). method: 'adam' | 'rmsprop';
-- config: the optimState table (learningRate, learningRateDecay, beta1, beta2, epsilon, weightDecay, alpha, initialMean; the
-- defaults of lib/adam.lua / lib/rmsprop.lua where absent); gradNormThreshold nil or <= 0: no clip.
--   local opt = hip.Optim(model, mconf.optimizationMethod, mconf.optimState, mconf.gradNormThreshold)
--   opt:step(weights, biases, gradWeights, gradBiases)      -- tables of CudaTensors, one per convolution
local Optim = {}
Optim.__index = Optim
local function optim_config(method, config, threshold)
  local c = ffi.new('tfl_optim_config')
  config = config or {}
  if method == 'adam' then
    c.method = lib.TFL_OPTIM_ADAM
    c.learningRate = config.learningRate or 0.001
    c.beta1, c.beta2 = config.beta1 or 0.9, config.beta2 or 0.999
    c.learningRateDecay = config.learningRateDecay or 0
  elseif method == 'rmsprop' then
    c.method = lib.TFL_OPTIM_RMSPROP
    c.learningRate = config.learningRate or 1e-2
    c.alpha, c.initialMean = config.alpha or 0.99, config.initialMean or 0
  else
    error("hip.Optim: optimizationMethod must be 'adam' or 'rmsprop' (optim.sgd is Torch's own)", 3)
  end
  c.epsilon, c.weightDecay = config.epsilon or 1e-8, config.weightDecay or 0
  c.gradNormThreshold = threshold or 0
  return c
end
function M.Optim(model, method, config, gradNormThreshold)
  local self = setmetatable({model = model, method = method}, Optim)
  local c = optim_config(method, config, gradNormThreshold)
  local h = lib.tfl_optim_create(ctx, model.handle, c)
  if h == nil then error(ffi.string(lib.tfl_last_error(ctx)), 2) end
  self.handle = ffi.gc(h, function(q) lib.tfl_optim_destroy(ctx, q) end)
  return self
end
function Optim:setConfig(config, gradNormThreshold)
  check(lib.tfl_optim_set_config(ctx, self.handle, optim_config(self.method, config, gradNormThreshold)))
end
function Optim:step(weights, biases, gradWeights, gradBiases)
  check(lib.tfl_optim_step(ctx, self.handle, devptrs(weights, 'float*'), devptrs(biases, 'float*'), devptrs(gradWeights, 'float*'),
                           devptrs(gradBiases, 'float*')))
end
function Optim:steps() return tonumber(lib.tfl_optim_steps(ctx, self.handle)) end
-- opt:state(m, v): copies the moments into the CudaTensors m and v (v: Adam only; either may be nil); returns their length
function Optim:state(m, v)
  return tonumber(lib.tfl_optim_get_state(ctx, self.handle, m and ffi.cast('float*', torch.data(m)) or nil,
                                          v and ffi.cast('float*', torch.data(v)) or nil))
end
-- hip.optimStepReduced(opt, weights, biases, gradWeights, gradBiases, guard, callbacks, world, reduce): the data-parallel step
-- (tfl_optim_step_reduced): the gradients averaged over `world` ranks by ONE all-reduce inside the step. guard: an IntTensor on
-- the device or nil; callbacks: a const tfl_comm* (lib.tfl_rccl_comm_callbacks(comm), as hip.Slab keeps it) or nil = the guarded
-- step; reduce: a CudaDoubleTensor of at least hip.optimReduceDoubles(opt) elements, the caller's and kept between steps.
function M.optimReduceDoubles(opt) return tonumber(lib.tfl_optim_reduce_doubles(ctx, opt.handle)) end
function M.optimStepReduced(opt, weights, biases, gradWeights, gradBiases, guard, callbacks, world, reduce)
  check(lib.tfl_optim_step_reduced(ctx, opt.handle, devptrs(weights, 'float*'), devptrs(biases, 'float*'), devptrs(gradWeights, 'float*'),
                                   devptrs(gradBiases, 'float*'), guard and ffi.cast('const int32_t*', torch.data(guard)) or nil,
                                   callbacks, world or 1, reduce and ffi.cast('double*', torch.data(reduce)) or nil,
                                   reduce and reduce:nElement() or 0))
end

-- ---- tfluids.simulate as ONE native call (lib/simulate.lua:175-327 = fluidnet_amd/csrc/simulate.cpp) -----------------
local plans = setmetatable({}, {__mode = 'k'})    -- BC tensor -> {mask tensor, tfl_bc_plan*}: created once per pair
local function plan(bc, mask)
  if bc == nil or mask == nil then return nil end
  local hit = plans[bc]
  if hit == nil or hit[1] ~= mask then
    local h = lib.tfl_bc_plan_create(ctx, T(bc), T(mask))
    if h == nil then error('tfl_bc_plan_create failed', 3) end
    -- (the finalizer ends in hipFree: a host that records HIP graphs ITSELF must keep collections out of its capture -- the
    -- Python binding learnt that in round 6; Slab:record() captures inside one library call, where no collection can run)
    ffi.gc(h, function(q) lib.tfl_bc_plan_destroy(ctx, q) end)
    hit = {mask, h}
    plans[bc] = hit
  end
  return hit[2]
end
--- Call after editing BC tensors in place (the 2-D demo's interactive edits): plans are keyed by tensor identity.
function M.invalidateBCs() plans = setmetatable({}, {__mode = 'k'}) end

-- the scene's flags as one code byte per cell (include/tfluids_hip.h tfl_wall_plan, round 6): registered once with the context, found
-- again by the flags' address inside tfl_model_begin. lib/simulate.lua never writes batch.flags; call M.invalidateFlags() after
-- editing them (a moving obstacle, the 2-D demo's mouse)
local wallPlans = setmetatable({}, {__mode = 'k'})    -- flags tensor -> tfl_wall_plan*
local function wallPlan(flags)
  local seen = wallPlans[flags]
  if seen == nil then
    wallPlans[flags] = false                           -- first sighting: only remembered (a plan costs an allocation and a device
  elseif seen == false then                            -- synchronisation: not for flags that come fresh with every call)
    local h = lib.tfl_wall_plan_create(ctx, T(flags))
    if h == nil then return end                        -- not fatal: the step decodes the flag words itself
    wallPlans[flags] = ffi.gc(h, function(q) lib.tfl_wall_plan_destroy(ctx, q) end)
  end
end
function M.invalidateFlags() wallPlans = setmetatable({}, {__mode = 'k'}); collectgarbage() end

-- `model` may be a hip.Model, or an nn.gModule (wrapped on first use), or nil for the Jacobi / PCG projections.
local wrapped = setmetatable({}, {__mode = 'k'})
local function sim_args(mconf, batch, model, outputDiv)
  local keep = {}
  local function D(t) local d = T(t); keep[#keep + 1] = d; return d end
  local prm = ffi.new('tfl_sim_params')
  prm.dt = mconf.dt
  prm.advectionMethod = mconf.advectionMethod          -- nil = maccormackOurs
  prm.maccormackStrength = mconf.maccormackStrength or 0.75
  prm.buoyancyScale = mconf.buoyancyScale or 0
  prm.gravityScale = mconf.gravityScale or 0
  local g = mconf.gravity or {0, 1, 0}                  -- lib/simulate.lua:204-211
  if torch.isTensor(g) then g = g:float():totable() end
  prm.gravity[0], prm.gravity[1], prm.gravity[2] = g[1], g[2], g[3]
  prm.vorticityConfinementAmp = mconf.vorticityConfinementAmp or 0
  prm.simMethod = mconf.simMethod                       -- nil = convnet
  prm.maxIter = mconf.maxIter or 0
  prm.pcgPrecond = mconf.pcgPrecond
  prm.outputDiv = b2i(outputDiv)
  local st = ffi.new('tfl_sim_state')
  st.p, st.U, st.flags = D(batch.pDiv), D(batch.UDiv), D(batch.flags)
  if model ~= nil and (mconf.simMethod or 'convnet') == 'convnet' then wallPlan(batch.flags) end
  local dens = batch.density
  local chans = (dens == nil) and {} or (torch.isTensor(dens) and {dens} or dens)   -- RGB table in the 2-D demo
  st.n_density = #chans
  for i, c in ipairs(chans) do st.density[i - 1] = D(c) end
  st.pBC = plan(batch.pBC, batch.pBCInvMask)
  st.UBC = plan(batch.UBC, batch.UBCInvMask)
  if batch.densityBC ~= nil then
    local bcs = torch.isTensor(batch.densityBC) and {batch.densityBC} or batch.densityBC
    local mks = torch.isTensor(batch.densityBCInvMask) and {batch.densityBCInvMask} or batch.densityBCInvMask
    assert(#bcs == #chans, 'density / densityBC channel mismatch')
    for i = 1, #chans do st.densityBC[i - 1] = plan(bcs[i], mks[i]) end
  end
  if model ~= nil and getmetatable(model) ~= Model then
    wrapped[model] = wrapped[model] or M.Model(model)
    model = wrapped[model]
  end
  st.model = model and model.handle or nil
  return prm, st, keep
end

function M.simulate(conf, mconf, batch, model, outputDiv)
  local prm, st, keep = sim_args(mconf, batch, model, outputDiv)
  local ws, n = workspace(batch.UDiv, lib.tfl_simulate_workspace_floats(ctx, prm, st))
  check(lib.tfl_simulate_step(ctx, prm, st, ws, n))
  return keep ~= nil
end

-- ---- z-slab ranks: one LuaJIT process per GPU, grid cut along z, halos over RCCL inside the library -----------------
-- (no counterpart in the reference, which is single-GPU; BASELINE config 5). Rank 0 calls M.rcclUniqueId() and hands
-- the 128-byte string to the other ranks (a file, the launcher's environment, a socket); every rank then builds
--   local slab = M.Slab{zTotal = 256, zFirst = lo, ownLo = c0, ownHi = c1, id = idString, rank = r, world = n}
-- on its LOCAL extended tensors (owned planes + M.slabHalo(reach, model) planes next to each neighbour) and steps with
--   slab:simulate(conf, mconf, batch, model)       -- tfluids.simulate on the slab, bit-equal on the owned planes
--                                                     (mconf.simMethod = 'jacobi': no model, bit-equal at any world size;
--                                                      any mconf.advectionMethod, batch.density a table of up to 8 channels)
--   slab:drain()                                   -- before reading halo planes / at the end
-- The halo planes a slab stores next to each neighbour for reach R when the step projects with `model` (an M.Model, or nil for
-- the Jacobi projection): tfl_slab_halo_model -- max(4, 2R + 1), widened to the depth the net's cone reads and rounded up to
-- its downsampling factor (16 for the 3-D tog table; DESIGN.md 6d). With a pooling net, zFirst / ownLo / ownHi and the local
-- depth go on that factor too. Graph and 2-D models: an error (the slab step refuses them).
function M.slabHalo(reach, model)
  local h = lib.tfl_slab_halo_model(model and model.handle or nil, reach or 1)
  if h < 0 then error('tfluids_hip: the z-slab step cannot run this model (graph or 2-D models run un-sharded only)', 2) end
  return h
end

function M.rcclUniqueId()
  local id = ffi.new('char[128]')
  check(lib.tfl_rccl_get_unique_id(ctx, id))
  return ffi.string(id, 128)
end

local Slab = {}
Slab.__index = Slab
function M.Slab(o)
  local self = setmetatable({}, Slab)
  self.desc = ffi.new('tfl_slab')
  self.desc.z_total, self.desc.z_first = o.zTotal, o.zFirst
  self.desc.own_lo, self.desc.own_hi = o.ownLo, o.ownHi
  self.desc.reach, self.desc.overlap = o.reach or 1, b2i(o.overlap)
  -- checkReach: true (default) = a violation is reported by the NEXT step; 'exact' = found before the step, collectively,
  -- nothing written (tfl_slab.check_reach = 2: the error names the reach to lay the slab out for); false = unchecked
  self.desc.check_reach, self.desc.in_flight = (o.checkReach == 'exact') and 2 or b2i(o.checkReach ~= false), 0
  if (o.world or 1) > 1 then
    assert(type(o.id) == 'string' and #o.id == 128, 'Slab: id = the 128 bytes of M.rcclUniqueId() of rank 0')
    self.comm = lib.tfl_rccl_comm_create(ctx, o.id, o.rank, o.world)
    if self.comm == nil then error('tfluids_hip: ' .. ffi.string(lib.tfl_last_error(ctx))) end
    self.comm = ffi.gc(self.comm, function(c) lib.tfl_rccl_comm_destroy(ctx, c) end)
    self.callbacks = lib.tfl_rccl_comm_callbacks(self.comm)
    -- a slab without the strip / interior split has nothing for a transfer to overlap with: RCCL on the step's own stream
    -- (an event hop between two streams costs 12-15 us on the device, eight of them per step)
    if not o.overlap then check(lib.tfl_rccl_comm_set_inline(self.comm, 1)) end
  end
  return self
end
-- Record the rank-step into a HIP graph (tfl_slab_graph_create): call after a few slab:simulate() steps; from then on
-- slab:simulate() is ONE hipGraphLaunch with mconf / batch / model frozen as they were. false + the reason when the step
-- cannot be recorded (the steps stay eager).
function Slab:record()
  if self.st == nil then return false, 'call slab:simulate() at least once first' end
  local g = lib.tfl_slab_graph_create(ctx, self.prm, self.st, self.desc, self.callbacks, self.ws, self.n)
  if g == nil then return false, ffi.string(lib.tfl_last_error(ctx)) end
  self.graph = ffi.gc(g, function(h) lib.tfl_slab_graph_destroy(ctx, h) end)
  return true
end
function Slab:simulate(conf, mconf, batch, model)
  if self.graph ~= nil then check(lib.tfl_slab_graph_step(ctx, self.graph)); return end
  if mconf.simMethod == 'jacobi' then model = nil end   -- the Jacobi slab step takes state->model = NULL (it reads none)
  local prm, st, keep = sim_args(mconf, batch, model, false)
  if self.ws == nil then   -- the SAME buffer on every call: messages started by one step are consumed by the next
    self.n = tonumber(lib.tfl_simulate_slab_workspace_floats(ctx, prm, st, self.desc))
    self.buf = batch.UDiv.new():resize(self.n):zero()     -- private: the shared scratch may be re-allocated by other operators
    self.ws = ffi.cast('float*', torch.data(self.buf))
  end
  self.prm, self.st, self.keep = prm, st, keep
  local rc = lib.tfl_simulate_step_slab(ctx, prm, st, self.desc, self.callbacks, self.ws, self.n)
  if rc == -5 then      -- TFL_EREACH (checkReach = 'exact'): every rank is here, nothing has been written
    local need = lib.tfl_slab_needed_reach(ctx)
    error(string.format('tfluids_hip: the flow needs a back-trace reach of %d planes: re-cut the local tensors with M.slabHalo(%d, model) = %d ' ..
                        'halo planes (tfl_slab_exchange fetches them) and create the Slab again with reach = %d', need, need,
                        lib.tfl_slab_halo_model(st.model, need), need))
  end
  check(rc)
end
function Slab:drain()
  if self.st ~= nil and bit.band(self.desc.in_flight, 15) ~= 0 then      -- (bits 0-3: messages in flight)
    check(lib.tfl_slab_drain(ctx, self.st, self.desc, self.callbacks, self.ws, self.n))
  end
end

-- The divergence norm of the WHOLE grid from its slabs (tfl_slab_divergence_norm): a torch.CudaDoubleTensor [B], the same on
-- every rank and bit-equal to M.velocityDivergenceNorm of the un-cut grid. Collective; call after slab:simulate().
function Slab:divergenceNorm()
  assert(self.st ~= nil, 'call slab:simulate() at least once first')
  local out = torch.CudaDoubleTensor(self.st.flags.B)
  check(lib.tfl_slab_divergence_norm(ctx, self.st, self.desc, self.callbacks, self.ws, self.n, ffi.cast('double*', torch.data(out))))
  return out
end

--- || velocityDivergence(U, flags)[b] ||_2 per batch item as a torch.CudaDoubleTensor [B] (what lib/calc_stats.lua:98-118 takes
--- with div[i]:norm(), one host synchronisation per sample): two launches, no divergence field, no host read.
function M.velocityDivergenceNorm(U, flags)
  local is3D = U:size(2) == 3
  local out = torch.CudaDoubleTensor(flags:size(1))
  local ws, n = workspace(flags, lib.tfl_divergence_norm_workspace_floats(flags:size(1), flags:size(3), flags:size(4), flags:size(5)))
  check(lib.tfl_velocityDivergenceNorm(ctx, T(U), T(flags), b2i(is3D), ffi.cast('double*', torch.data(out)), ws, n))
  return out
end

--- The border weight of nn.FluidCriterion (lib/modules/fluid_criterion.lua:145-158) in one launch: a function of flags only.
function M.criterionWeight(flags, borderWidth, borderWeight, out)
  local is3D = flags:size(3) > 1
  out = out or flags:clone()
  check(lib.tfl_criterion_weight(ctx, T(flags), borderWidth, borderWeight, b2i(is3D), T(out)))
  return out
end

--- nn.FluidCriterion's updateOutput and (with gradP / gradU, both or neither) updateGradInput in two launches: returns a
--- torch.CudaDoubleTensor [4] = {pLoss, uLoss, divLoss, total} on the device (no host read). weight: M.criterionWeight(flags,
--- ...) or nil (unweighted); a term whose lambda is <= 0 is 0 and adds nothing to the gradients.
function M.FluidCriterion(pPred, UPred, pTarget, UTarget, flags, weight, pLambda, uLambda, divLambda, sizeAverage, gradP, gradU)
  local is3D = UPred:size(2) == 3
  local loss = torch.CudaDoubleTensor(4)
  local ws, n = workspace(flags, lib.tfl_fluid_criterion_workspace_floats(flags:size(1), flags:size(3), flags:size(4), flags:size(5)))
  check(lib.tfl_fluidCriterion(ctx, T(pPred), T(UPred), T(pTarget), T(UTarget), T(flags), weight and T(weight) or nil, pLambda, uLambda, divLambda, b2i(sizeAverage ~= false), b2i(is3D), ffi.cast('double*', torch.data(loss)), gradP and T(gradP) or nil, gradU and T(gradU) or nil, ws, n))
  return loss
end

--- Arithmetic of the LDS-tiled 3-D advection kernels (include/tfluids_hip.h tfl_set_advect_mode): 'exact' (default; bit-equal
--- to the reference CPU path) or 'fast' (the tolerance mode: rel-L2 ~2e-8 against the reference, bar 1e-5).
function M.setAdvectMode(mode)
  assert(mode == 'exact' or mode == 'fast', "advect mode must be 'exact' or 'fast'")
  check(lib.tfl_set_advect_mode(ctx, mode == 'fast' and 1 or 0))
end

--- Route torch.CudaTensor's `.tfluids` method table, tfluids.normalizePressureMean and tfluids.simulate to the MI355X
--- library.
-- @param tfluids the table returned by require('tfluids')
-- @param opts {lib = path to libtfluids_hip.so, device = 0-based HIP device, stream = hipStream_t cdata, advectMode = 'exact' | 'fast',
--              keepLuaSimulate = true to leave lib/simulate.lua's tfluids.simulate in place}
function M.install(tfluids, opts)
  opts = opts or {}
  lib = ffi.load(opts.lib or 'tfluids_hip')
  assert(lib.tfl_abi_version() == 4, 'libtfluids_hip.so / tfluids_hip.lua ABI version mismatch')
  ctx = lib.tfl_create(opts.device or (cutorch.getDevice() - 1))
  assert(ctx ~= nil, 'tfl_create failed')
  if opts.stream then check(lib.tfl_set_stream(ctx, opts.stream)) end
  if opts.advectMode then M.setAdvectMode(opts.advectMode) end
  local mt = getmetatable(torch.CudaTensor)  -- luaT_registeratname(L, tbl, "tfluids") put the table here
  mt.tfluids = mt.tfluids or {}
  for name, fn in pairs(ops) do mt.tfluids[name] = fn end
  rawset(tfluids, 'normalizePressureMean', M.normalizePressureMean)
  rawset(tfluids, 'velocityDivergenceNorm', M.velocityDivergenceNorm)
  rawset(tfluids, 'criterionWeight', M.criterionWeight)
  rawset(tfluids, 'fluidCriterion', M.FluidCriterion)
  if not opts.keepLuaSimulate then rawset(tfluids, 'simulate', M.simulate) end
  tfluids.withHIP = true
  return M
end

function M.synchronize() check(lib.tfl_synchronize(ctx)) end
function M.traceErrors() return tonumber(lib.tfl_trace_errors(ctx)) end

M.ops = ops
return M
