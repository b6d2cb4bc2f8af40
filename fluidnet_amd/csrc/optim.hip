// optim.hip -- the optimiser step of the training closure on the device (tfl_optim_step): the gradient clip of
// lib/run_epoch.lua:304-312, weight decay, and lib/adam.lua / lib/rmsprop.lua, over the flat parameter space of
// tfl_refresh.hpp (tensor 2 l = layer l's weight, 2 l + 1 = its bias; the caller's device pointers travel by value).
// Three launches at the most: k_optim_norm leaves one fp64 partial of sum g^2 per block at a fixed place, k_optim_update adds
// them in index order (every block the same sum: no atomics, the same bits every call), clips, decays and updates each
// element in fp32 in the reference's operation order, and k_optim_advance moves the step counter -- a kernel, so that a captured
// step advances on replay. With a guard word (tfl_optim_step_guarded) the update and the advance read it when they run and,
// where it is set, write nothing: parameters, moments and the counter stay as they are.
// The data-parallel step (tfl_optim_step_reduced) puts three things around that: k_optim_pack widens the gradients and the guard
// into the caller's fp64 reduce buffer, the transport sums it over the ranks, and k_optim_unpack_norm -- k_optim_norm with the
// average in front: (float)(sum / world), one division, one rounding -- writes the averaged gradients back and leaves the same
// partials at the same places (k_optim_unpack where there is no clip). Every output element has one writer.
#include <hip/hip_runtime.h>

#include "tfl_host.hpp"
#include "tfl_refresh.hpp"

namespace tfl {
namespace {

__global__ __launch_bounds__(kOptimThreads) void k_optim_norm(OptimPtrs p, const long long* __restrict__ off, int ntens, long long total,
                                                             double* __restrict__ partials) {
  __shared__ long long s_off[kOptimMaxTensors + 1];
  __shared__ double red[kOptimThreads];
  for (int i = threadIdx.x; i <= ntens; i += kOptimThreads) s_off[i] = off[i];
  __syncthreads();
  long long lo, hi;
  optim_chunk(total, gridDim.x, blockIdx.x, &lo, &hi);
  double s = 0.0;
  for (long long i = lo + threadIdx.x; i < hi; i += kOptimThreads) {
    const int t = optim_tensor_of(s_off, ntens, i);
    const double g = (double)p.g[t][i - s_off[t]];
    s += g * g;
  }
  red[threadIdx.x] = s;
  __syncthreads();
  for (int w = kOptimThreads / 2; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) partials[blockIdx.x] = red[0];
}

__global__ __launch_bounds__(kOptimThreads) void k_optim_update(OptimPtrs p, const long long* __restrict__ off, int ntens, long long total,
                                                               const double* __restrict__ partials, int npartials,
                                                               float* __restrict__ m, float* __restrict__ v,
                                                               const long long* __restrict__ t_ptr, OptimArgs c,
                                                               const int* __restrict__ guard) {
  __shared__ long long s_off[kOptimMaxTensors + 1];
  __shared__ float s_div, s_step;
  __shared__ int s_clip, s_skip;
  for (int i = threadIdx.x; i <= ntens; i += kOptimThreads) s_off[i] = off[i];
  if (threadIdx.x == 0) {
    s_skip = guard ? *guard : 0;
    s_clip = 0; s_div = 1.0f;
    if (partials) {
      double sum = 0.0;
      for (int b = 0; b < npartials; b++) sum += partials[b];
      const double norm = sqrt(sum);
      if (norm > c.threshold) { s_clip = 1; s_div = (float)(norm / c.threshold); }
    }
    if (c.method == 0) {     // Adam: clr from t before the increment, the bias corrections from the new t, in fp64, rounded once
      const double t0 = (double)*t_ptr, t1 = t0 + 1.0;
      const double clr = c.lr / (1.0 + t0 * c.lrd);
      s_step = (float)-(clr * sqrt(1.0 - pow(c.beta2, t1)) / (1.0 - pow(c.beta1, t1)));
    } else s_step = (float)-c.lr;
  }
  __syncthreads();
  const long long i = (long long)blockIdx.x * kOptimThreads + threadIdx.x;
  if (i >= total || s_skip) return;
  const int t = optim_tensor_of(s_off, ntens, i);
  const long long e = i - s_off[t];
  float x = p.x[t][e], g = p.g[t][e];
  if (s_clip) g = __fdiv_rn(g, s_div);
  if (c.wd != 0.0f) g = g + c.wd * x;
  if (s_clip || c.wd != 0.0f) p.g[t][e] = g;
  if (c.method == 0) {
    const float mi = m[i] * c.b1 + c.omb1 * g;
    const float vi = v[i] * c.b2 + (c.omb2 * g) * g;
    m[i] = mi; v[i] = vi;
    x = x + __fdiv_rn(s_step * mi, __fsqrt_rn(vi) + c.eps);
  } else {
    const float mi = m[i] * c.b2 + (c.omb2 * g) * g;
    m[i] = mi;
    x = x + __fdiv_rn(s_step * g, __fsqrt_rn(mi) + c.eps);
  }
  p.x[t][e] = x;
}

// flat element i < total -> slot i of the reduce buffer (what: 0 the gradient, 1 the parameter, 2 zero); slot total = the guard
// as 0 / 1; the reserved slots behind it = 0. One thread per slot.
__global__ __launch_bounds__(kOptimThreads) void k_optim_pack(OptimPtrs p, const long long* __restrict__ off, int ntens, long long total,
                                                             const int* __restrict__ guard, double* __restrict__ out, int what) {
  __shared__ long long s_off[kOptimMaxTensors + 1];
  for (int i = threadIdx.x; i <= ntens; i += kOptimThreads) s_off[i] = off[i];
  __syncthreads();
  const long long i = (long long)blockIdx.x * kOptimThreads + threadIdx.x;
  if (i >= total + kOptimReduceTail) return;
  double val = 0.0;
  if (i < total) {
    if (what != 2) {
      const int t = optim_tensor_of(s_off, ntens, i);
      val = (double)(what == 0 ? p.g[t][i - s_off[t]] : p.x[t][i - s_off[t]]);
    }
  } else if (i == total) val = (guard && *guard != 0) ? 1.0 : 0.0;
  out[i] = val;
}

// k_optim_norm over the averaged gradients, which it writes first: the chunks, the tree and the places of the partials are
// k_optim_norm's, so the sum the update forms is the one it would form from these gradient floats. A set reduced guard
// (r[total] != 0) keeps the gradient arrays as they are.
__global__ __launch_bounds__(kOptimThreads) void k_optim_unpack_norm(OptimPtrs p, const long long* __restrict__ off, int ntens, long long total,
                                                                    const double* __restrict__ r, double world,
                                                                    double* __restrict__ partials, int* __restrict__ rguard) {
  __shared__ long long s_off[kOptimMaxTensors + 1];
  __shared__ double red[kOptimThreads];
  for (int i = threadIdx.x; i <= ntens; i += kOptimThreads) s_off[i] = off[i];
  __syncthreads();
  const bool skip = r[total] != 0.0;
  long long lo, hi;
  optim_chunk(total, gridDim.x, blockIdx.x, &lo, &hi);
  double s = 0.0;
  for (long long i = lo + threadIdx.x; i < hi; i += kOptimThreads) {
    const int t = optim_tensor_of(s_off, ntens, i);
    const float gf = (float)(r[i] / world);
    if (!skip) p.g[t][i - s_off[t]] = gf;
    const double g = (double)gf;
    s += g * g;
  }
  red[threadIdx.x] = s;
  __syncthreads();
  for (int w = kOptimThreads / 2; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) partials[blockIdx.x] = red[0];
  if (threadIdx.x == 0 && blockIdx.x == 0) *rguard = skip ? 1 : 0;
}

// slot i -> flat element i of the gradients (to_params: of the parameters), one thread each; rguard (NULL: none, nothing skips)
// receives the reduced guard
__global__ __launch_bounds__(kOptimThreads) void k_optim_unpack(OptimPtrs p, const long long* __restrict__ off, int ntens, long long total,
                                                               const double* __restrict__ r, double world, int* __restrict__ rguard,
                                                               int to_params) {
  __shared__ long long s_off[kOptimMaxTensors + 1];
  for (int i = threadIdx.x; i <= ntens; i += kOptimThreads) s_off[i] = off[i];
  __syncthreads();
  const bool skip = rguard && r[total] != 0.0;
  const long long i = (long long)blockIdx.x * kOptimThreads + threadIdx.x;
  if (i == 0 && rguard) *rguard = skip ? 1 : 0;
  if (i >= total || skip) return;
  const int t = optim_tensor_of(s_off, ntens, i);
  const float val = (float)(r[i] / world);
  if (to_params) p.x[t][i - s_off[t]] = val;
  else p.g[t][i - s_off[t]] = val;
}

__global__ void k_optim_advance(long long* t, const int* __restrict__ guard) {
  if (guard && *guard) return;
  *t += 1;
}
// the counter of a restored checkpoint (tfl_optim_set_state): the value travels by value, so the call stays asynchronous
__global__ void k_optim_set_steps(long long* t, long long steps) { *t = steps; }
__global__ __launch_bounds__(kOptimThreads) void k_optim_fill(float* p, long long n, float val) {
  const long long i = (long long)blockIdx.x * kOptimThreads + threadIdx.x;
  if (i < n) p[i] = val;
}
}  // namespace

void optim_step(hipStream_t st, const OptimPtrs& p, const long long* d_off, int ntens, long long total, double* d_partials, float* m,
                float* v, long long* d_t, const OptimArgs& c, const int* d_guard, bool norm_done) {
  const bool clip = c.threshold > 0.0;
  if (clip && !norm_done) {
    TFL_TIMED("k_optim_norm", st);
    hipLaunchKernelGGL(k_optim_norm, dim3(kOptimNormBlocks), dim3(kOptimThreads), 0, st, p, d_off, ntens, total, d_partials);
  }
  const unsigned nb = (unsigned)((total + kOptimThreads - 1) / kOptimThreads);
  {
    TFL_TIMED("k_optim_update", st);
    hipLaunchKernelGGL(k_optim_update, dim3(nb), dim3(kOptimThreads), 0, st, p, d_off, ntens, total, clip ? (const double*)d_partials : nullptr,
                       kOptimNormBlocks, m, v, (const long long*)d_t, c, d_guard);
  }
  TFL_TIMED("k_optim_advance", st);
  hipLaunchKernelGGL(k_optim_advance, dim3(1), dim3(1), 0, st, d_t, d_guard);
}
void optim_pack(hipStream_t st, const OptimPtrs& p, const long long* d_off, int ntens, long long total, const int* d_guard,
                double* d_reduce, int what) {
  TFL_TIMED("k_optim_pack", st);
  const unsigned nb = (unsigned)((total + kOptimReduceTail + kOptimThreads - 1) / kOptimThreads);
  hipLaunchKernelGGL(k_optim_pack, dim3(nb), dim3(kOptimThreads), 0, st, p, d_off, ntens, total, d_guard, d_reduce, what);
}
void optim_unpack(hipStream_t st, const OptimPtrs& p, const long long* d_off, int ntens, long long total, const double* d_reduce,
                  int world, double* d_partials, int* d_rguard, bool to_params) {
  if (d_partials) {
    TFL_TIMED("k_optim_unpack_norm", st);
    hipLaunchKernelGGL(k_optim_unpack_norm, dim3(kOptimNormBlocks), dim3(kOptimThreads), 0, st, p, d_off, ntens, total, d_reduce,
                       (double)world, d_partials, d_rguard);
    return;
  }
  TFL_TIMED("k_optim_unpack", st);
  const unsigned nb = (unsigned)((total + kOptimThreads - 1) / kOptimThreads);
  hipLaunchKernelGGL(k_optim_unpack, dim3(nb), dim3(kOptimThreads), 0, st, p, d_off, ntens, total, d_reduce, (double)world, d_rguard,
                     to_params ? 1 : 0);
}
void optim_set_steps(hipStream_t st, long long* d_t, long long steps) {
  hipLaunchKernelGGL(k_optim_set_steps, dim3(1), dim3(1), 0, st, d_t, steps);
}
void optim_fill(hipStream_t st, float* p, long long n, float val) {
  if (n < 1) return;
  hipLaunchKernelGGL(k_optim_fill, dim3((unsigned)((n + kOptimThreads - 1) / kOptimThreads)), dim3(kOptimThreads), 0, st, p, n, val);
}

}  // namespace tfl
