// optim_host.cpp -- the optimiser step on the device: the tfl_optim object (state, the hyper-parameters by
// value) and every tfl_optim_* entry, the all-reduce path of data-parallel training included. The kernels are optim.hip's. Of
// the model it asks only the parameter counts and the refresh gate (tfl_model.hpp param_counts / refresh_gate) and ends every
// step with tfl_model_set_weights_device (model_build.cpp).
#include <cmath>
#include <cstddef>
#include <vector>

#include "tfl_model.hpp"

using tfl::fail; using tfl::check_launch; using tfl::model::refresh_gate;

struct tfl_optim {
  tfl_model* model = nullptr;
  tfl_optim_config cfg{};
  int ntens = 0;                 // 2 per layer: weight, bias
  long long total = 0;           // parameters
  long long* d_off = nullptr;    // [ntens + 1] prefix offsets of the tensors in the flat parameter space
  float* m = nullptr;            // [total] first moment (RMSprop: the mean square)
  float* v = nullptr;            // [total] second moment (Adam)
  long long* d_t = nullptr;      // the step counter
  double* d_partials = nullptr;  // [kOptimNormBlocks] partial sums of g^2
  int32_t* d_rguard = nullptr;   // the reduced guard word of the last tfl_optim_step_reduced (0 before the first)
};

namespace {
int optim_config_ok(tfl_ctx* c, const tfl_optim_config* k, const char* who) {
  if (!k) return fail(c, TFL_EINVAL, "%s: null config", who);
  if (k->method != TFL_OPTIM_ADAM && k->method != TFL_OPTIM_RMSPROP) return fail(c, TFL_EINVAL, "%s: unknown optimisation method", who);
  for (double x : {k->learningRate, k->learningRateDecay, k->beta1, k->beta2, k->epsilon, k->weightDecay, k->alpha, k->initialMean, k->gradNormThreshold})
    if (!std::isfinite(x)) return fail(c, TFL_EINVAL, "%s: a hyper-parameter is not finite", who);
  return TFL_OK;
}
// what a call with a transport needs of it and of the caller's reduce buffer
int optim_reduce_args_ok(tfl_ctx* c, const tfl_optim* o, const char* who, const tfl_comm* comm, const double* d_reduce, int64_t reduce_doubles) {
  if (comm->size < (int32_t)(offsetof(tfl_comm, allreduce_sum) + sizeof(comm->allreduce_sum)) || !comm->allreduce_sum)
    return fail(c, TFL_EINVAL, "%s: tfl_comm has no size or lacks allreduce_sum", who);
  if (!d_reduce || ((uintptr_t)d_reduce & 7) != 0) return fail(c, TFL_EINVAL, "%s: the reduce buffer is null or not 8-byte aligned", who);
  if (reduce_doubles < (int64_t)o->total + tfl::kOptimReduceTail)
    return fail(c, TFL_EINVAL, "%s: the reduce buffer holds %lld doubles, tfl_optim_reduce_doubles asks for %lld", who,
                (long long)reduce_doubles, (long long)(o->total + tfl::kOptimReduceTail));
  return TFL_OK;
}
// tfl_optim_step_guarded (comm == NULL) and tfl_optim_step_reduced: pack, all-reduce and unpack in front of the same update
int optim_step_any(tfl_ctx* c, tfl_optim* o, const char* who, float* const* d_weights, float* const* d_biases, float* const* d_gradWeights,
                   float* const* d_gradBiases, const int32_t* d_guard, const tfl_comm* comm, int32_t world, double* d_reduce,
                   int64_t reduce_doubles) {
  if (!c) return TFL_EINVAL;
  if (((uintptr_t)d_guard & 3) != 0) return fail(c, TFL_EINVAL, "%s: the guard word is not 4-byte aligned", who);
  if (!o || !d_weights || !d_biases || !d_gradWeights || !d_gradBiases) return fail(c, TFL_EINVAL, "%s: null optimiser or parameter table", who);
  const int n = o->ntens / 2;
  tfl::OptimPtrs p{};
  for (int l = 0; l < n; l++) {
    if (!d_weights[l] || !d_biases[l] || !d_gradWeights[l] || !d_gradBiases[l])
      return fail(c, TFL_EINVAL, "%s: layer %d lacks a parameter or a gradient array", who, l);
    p.x[2 * l] = d_weights[l]; p.x[2 * l + 1] = d_biases[l];
    p.g[2 * l] = d_gradWeights[l]; p.g[2 * l + 1] = d_gradBiases[l];
  }
  if (comm) {
    if (world < 1) return fail(c, TFL_EINVAL, "%s: a world of %d ranks", who, (int)world);
    TRY(optim_reduce_args_ok(c, o, who, comm, d_reduce, reduce_doubles));
  }
  TRY(refresh_gate(c, o->model, who));
  const tfl_optim_config& k = o->cfg;
  const bool adam = k.method == TFL_OPTIM_ADAM;
  tfl::OptimArgs a{};
  a.method = adam ? 0 : 1;
  a.b1 = (float)k.beta1; a.omb1 = (float)(1.0 - k.beta1);
  a.b2 = (float)(adam ? k.beta2 : k.alpha); a.omb2 = (float)(1.0 - (adam ? k.beta2 : k.alpha));
  a.eps = (float)k.epsilon; a.wd = (float)k.weightDecay;
  a.lr = k.learningRate; a.lrd = k.learningRateDecay; a.beta1 = k.beta1; a.beta2 = k.beta2;
  a.threshold = k.gradNormThreshold > 0.0 ? k.gradNormThreshold : 0.0;
  if (comm) {
    tfl::optim_pack(c->stream, p, o->d_off, o->ntens, o->total, d_guard, d_reduce, 0);
    TRY(check_launch(c, who));
    if (comm->allreduce_sum(comm->user, d_reduce, (int64_t)o->total + 1) != 0) { c->err = "optim_step_reduced: comm callback failed (allreduce_sum)"; return TFL_EINVAL; }
    tfl::optim_unpack(c->stream, p, o->d_off, o->ntens, o->total, d_reduce, world, a.threshold > 0.0 ? o->d_partials : nullptr, o->d_rguard, false);
    d_guard = o->d_rguard;
  }
  tfl::optim_step(c->stream, p, o->d_off, o->ntens, o->total, o->d_partials, o->m, o->v, o->d_t, a, d_guard, comm != nullptr);
  TRY(check_launch(c, who));
  return tfl_model_set_weights_device(c, o->model, d_weights, d_biases);
}
}  // namespace

extern "C" {

tfl_optim* tfl_optim_create(tfl_ctx* c, tfl_model* m, const tfl_optim_config* config) {
  if (!c) return nullptr;
  const char* who = "optim_create";
  if (!m) { fail(c, TFL_EINVAL, "%s: null model", who); return nullptr; }
  if (optim_config_ok(c, config, who) != TFL_OK) return nullptr;
  const std::vector<long long> counts = tfl::model::param_counts(m);      // {weight, bias} per layer
  if ((int)counts.size() / 2 > tfl::kRefreshMaxLayers) { fail(c, TFL_EUNSUPPORTED, "%s: more than %d layers", who, tfl::kRefreshMaxLayers); return nullptr; }
  tfl_optim* o = new tfl_optim();
  o->model = m; o->cfg = *config;
  std::vector<long long> off(1, 0);
  for (long long n : counts) off.push_back(off.back() + n);
  o->ntens = (int)off.size() - 1; o->total = off.back();
  const size_t bytes = sizeof(float) * (size_t)o->total;
  const bool adam = config->method == TFL_OPTIM_ADAM;
  bool ok = hipMalloc((void**)&o->d_off, off.size() * sizeof(long long)) == hipSuccess &&
            hipMemcpy(o->d_off, off.data(), off.size() * sizeof(long long), hipMemcpyHostToDevice) == hipSuccess &&
            hipMalloc((void**)&o->m, bytes) == hipSuccess && (!adam || hipMalloc((void**)&o->v, bytes) == hipSuccess) &&
            hipMalloc((void**)&o->d_t, sizeof(long long)) == hipSuccess &&
            hipMalloc((void**)&o->d_partials, sizeof(double) * tfl::kOptimNormBlocks) == hipSuccess &&
            hipMalloc((void**)&o->d_rguard, sizeof(int32_t)) == hipSuccess &&
            hipMemsetAsync(o->d_rguard, 0, sizeof(int32_t), c->stream) == hipSuccess &&
            hipMemsetAsync(o->d_t, 0, sizeof(long long), c->stream) == hipSuccess &&
            hipMemsetAsync(o->m, 0, bytes, c->stream) == hipSuccess && (!adam || hipMemsetAsync(o->v, 0, bytes, c->stream) == hipSuccess);
  if (ok && !adam && config->initialMean != 0.0) tfl::optim_fill(c->stream, o->m, o->total, (float)config->initialMean);
  if (!ok || check_launch(c, who) != TFL_OK) { if (!ok) fail(c, TFL_EHIP, "%s: hipMalloc failed", who); tfl_optim_destroy(c, o); return nullptr; }
  return o;
}

int tfl_optim_set_config(tfl_ctx* c, tfl_optim* o, const tfl_optim_config* config) {
  if (!c) return TFL_EINVAL;
  if (!o) return fail(c, TFL_EINVAL, "optim_set_config: null optimiser");
  TRY(optim_config_ok(c, config, "optim_set_config"));
  if (config->method != o->cfg.method) return fail(c, TFL_EINVAL, "optim_set_config: the method is fixed at creation");
  o->cfg = *config;
  return TFL_OK;
}

int tfl_optim_step(tfl_ctx* c, tfl_optim* o, float* const* d_weights, float* const* d_biases, float* const* d_gradWeights,
                   float* const* d_gradBiases) {
  return tfl_optim_step_guarded(c, o, d_weights, d_biases, d_gradWeights, d_gradBiases, nullptr);
}

int tfl_optim_step_guarded(tfl_ctx* c, tfl_optim* o, float* const* d_weights, float* const* d_biases, float* const* d_gradWeights,
                           float* const* d_gradBiases, const int32_t* d_guard) {
  return optim_step_any(c, o, d_guard ? "optim_step_guarded" : "optim_step", d_weights, d_biases, d_gradWeights, d_gradBiases, d_guard,
                        nullptr, 1, nullptr, 0);
}

int64_t tfl_optim_reduce_doubles(tfl_ctx* c, tfl_optim* o) {
  if (!c || !o) return -1;
  return (int64_t)o->total + tfl::kOptimReduceTail;
}

int tfl_optim_step_reduced(tfl_ctx* c, tfl_optim* o, float* const* d_weights, float* const* d_biases, float* const* d_gradWeights,
                           float* const* d_gradBiases, const int32_t* d_guard, const tfl_comm* comm, int32_t world, double* d_reduce,
                           int64_t reduce_doubles) {
  if (!comm) return tfl_optim_step_guarded(c, o, d_weights, d_biases, d_gradWeights, d_gradBiases, d_guard);
  return optim_step_any(c, o, "optim_step_reduced", d_weights, d_biases, d_gradWeights, d_gradBiases, d_guard, comm, world, d_reduce,
                        reduce_doubles);
}

int tfl_optim_reduced_guard(tfl_ctx* c, tfl_optim* o, int32_t* d_out) {
  if (!c) return TFL_EINVAL;
  if (!o || !d_out) return fail(c, TFL_EINVAL, "optim_reduced_guard: null optimiser or output word");
  if (hipMemcpyAsync(d_out, o->d_rguard, sizeof(int32_t), hipMemcpyDeviceToDevice, c->stream) != hipSuccess)
    return fail(c, TFL_EHIP, "optim_reduced_guard: the copy failed");
  return TFL_OK;
}

int tfl_optim_sync_parameters(tfl_ctx* c, tfl_optim* o, float* const* d_weights, float* const* d_biases, const tfl_comm* comm,
                              int32_t rank, double* d_reduce, int64_t reduce_doubles) {
  if (!c) return TFL_EINVAL;
  const char* who = "optim_sync_parameters";
  if (!o || !d_weights || !d_biases) return fail(c, TFL_EINVAL, "%s: null optimiser or parameter table", who);
  const int n = o->ntens / 2;
  tfl::OptimPtrs p{};
  for (int l = 0; l < n; l++) {
    if (!d_weights[l] || !d_biases[l]) return fail(c, TFL_EINVAL, "%s: layer %d lacks a parameter array", who, l);
    p.x[2 * l] = d_weights[l]; p.x[2 * l + 1] = d_biases[l];
  }
  TRY(refresh_gate(c, o->model, who));
  if (comm) {
    if (rank < 0) return fail(c, TFL_EINVAL, "%s: rank %d", who, (int)rank);
    TRY(optim_reduce_args_ok(c, o, who, comm, d_reduce, reduce_doubles));
    tfl::optim_pack(c->stream, p, o->d_off, o->ntens, o->total, nullptr, d_reduce, rank == 0 ? 1 : 2);
    TRY(check_launch(c, who));
    if (comm->allreduce_sum(comm->user, d_reduce, (int64_t)o->total) != 0) { c->err = "optim_sync_parameters: comm callback failed (allreduce_sum)"; return TFL_EINVAL; }
    tfl::optim_unpack(c->stream, p, o->d_off, o->ntens, o->total, d_reduce, 1, nullptr, nullptr, true);
    TRY(check_launch(c, who));
  }
  return tfl_model_set_weights_device(c, o->model, d_weights, d_biases);
}

int64_t tfl_optim_steps(tfl_ctx* c, tfl_optim* o) {
  if (!c || !o) return -1;
  long long t = 0;
  if (hipMemcpyAsync(&t, o->d_t, sizeof(t), hipMemcpyDeviceToHost, c->stream) != hipSuccess) return -1;
  if (hipStreamSynchronize(c->stream) != hipSuccess) return -1;
  return (int64_t)t;
}

int64_t tfl_optim_get_state(tfl_ctx* c, tfl_optim* o, float* d_m, float* d_v) {
  if (!c || !o) return -1;
  const size_t bytes = sizeof(float) * (size_t)o->total;
  if (d_m && hipMemcpyAsync(d_m, o->m, bytes, hipMemcpyDeviceToDevice, c->stream) != hipSuccess) return -1;
  if (d_v && o->v && hipMemcpyAsync(d_v, o->v, bytes, hipMemcpyDeviceToDevice, c->stream) != hipSuccess) return -1;
  return (int64_t)o->total;
}

int tfl_optim_set_state(tfl_ctx* c, tfl_optim* o, const float* d_m, const float* d_v, int64_t steps) {
  if (!c) return TFL_EINVAL;
  const char* who = "optim_set_state";
  if (!o) return fail(c, TFL_EINVAL, "%s: null optimiser", who);
  if (steps < 0) return fail(c, TFL_EINVAL, "%s: a step count of %lld", who, (long long)steps);
  const size_t bytes = sizeof(float) * (size_t)o->total;
  if (d_m) HIP_TRY(c, hipMemcpyAsync(o->m, d_m, bytes, hipMemcpyDeviceToDevice, c->stream));
  if (d_v && o->v) HIP_TRY(c, hipMemcpyAsync(o->v, d_v, bytes, hipMemcpyDeviceToDevice, c->stream));
  tfl::optim_set_steps(c->stream, o->d_t, (long long)steps);
  return check_launch(c, who);
}

void tfl_optim_destroy(tfl_ctx* c, tfl_optim* o) {
  (void)c;
  if (!o) return;
  if (o->d_off) (void)hipFree(o->d_off);
  if (o->m) (void)hipFree(o->m);
  if (o->v) (void)hipFree(o->v);
  if (o->d_t) (void)hipFree(o->d_t);
  if (o->d_partials) (void)hipFree(o->d_partials);
  if (o->d_rguard) (void)hipFree(o->d_rguard);
  delete o;
}

}  // extern "C"
