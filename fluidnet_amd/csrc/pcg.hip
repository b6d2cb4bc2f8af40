// pcg.hip -- the reference's baseline pressure solver, solveLinearSystemPCG (gfx950).
//
// Replaces tfluids_CudaMain_solveLinearSystemPCG (generic/tfluids.cu:864-1759) and its helpers
// findConnectedFluidComponents (generic/find_connected_fluid_components.cc), createReducedSystemIndices /
// setupLaplacian (generic/tfluids.cu:864-1093), which build a CSR matrix on the CPU for every call and run CG
// through cuSPARSE / cuBLAS with a host read-back after every dot product.
//
// Here the solver is matrix-free and stays on the device:
//   * connected fluid components: union-find label propagation on the grid (hook + compress sweeps); a
//     component is named by its smallest cell index, so components come out in the reference's scan order;
//   * A = the 5/7-point Laplacian of setupLaplacian, applied straight from the flag grid: diagonal = number of
//     non-obstacle neighbours, -1 for every fluid neighbour; vectors are grid-shaped, masked by the component;
//   * CG is Golub & Van Loan alg. 10.3.1 exactly as the reference codes it (same update order, same
//     clampToEpsilon guards, same `r.r > tol^2 && iter <= maxIter` loop), with alpha / beta / the residual living
//     in a device struct: the host enqueues a chunk of iterations and reads one flag back per chunk; kernels of
//     iterations past convergence see `done` and return;
//   * preconditioners: for this stencil ILU(0) and IC(0) touch only the diagonal (every fill-in position is
//     outside the pattern): d(n) = a(n,n) - sum over lower fluid neighbours m of 1/d(m), in lexicographic order.
//     ilu0: L = unit lower with l(n,m) = -1/d(m), U = upper part of A with d on the diagonal.
//     ic0:  R upper with R(n,n) = sqrt(d(n)), R(n,q) = -1/R(n,n); M = R^T R.
//     Cells of one hyperplane i+j+k = const are independent (what cusparse's csrsv level analysis discovers at run
//     time). The factorisation (once per solve) runs one launch per hyperplane; the two triangular solves of every CG
//     iteration run as PIPELINED WAVEFRONTS on 3-D grids -- two launches instead of ~760 at 128^3 (k_wf_sweep below). 2-D grids keep the
//     launch-per-hyperplane sweeps; 3-D grids with more than 240 sub-boxes run the wavefronts one range of slabs per launch.
// Dot products are two-stage fp64 reductions with a fixed order (bit-reproducible run to run).
//
// The file: the kernels; then the host code. The caller's workspace is laid out by ONE table (tfl_pcg_ws.hpp: pcg_ws / npm_ws,
// which also size it), pcg_solve is the struct `Solve` -- the views of that table and the phases item / read_components /
// component / begin / factor / build_wavefront_operands / build_levels / precondition / vcycle / iteration / run_chunks /
// write_back -- and label_components is shared with normalize_pressure_mean. Results are named (PcgResult, tfl_host.hpp).
// precondType = "mg" (pc == 3) is one multigrid V-cycle per application: its kernels are pcg_mg.hip, its scheme tfl_pcg_mg.hpp;
// the wavefront machinery is not set up under it. The bodies of the k_cc_* / k_pcg_* kernels are __device__ functions (d_*):
// pcg_batched.inc, included at the end of the unnamed namespace, runs them once more with the batch item in blockIdx.y
// (solveLinearSystemPCGBatched, BatchedSolve).
#include "tfl_device.hpp"
#include "tfl_host.hpp"
#include "tfl_pcg_mg.hpp"
#include "tfl_pcg_ws.hpp"
#include "tfl_vec4.hpp"

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <optional>
#include <type_traits>
#include <vector>

namespace tfl {

namespace {

__device__ __forceinline__ float clamp_to_epsilon(float v) {   // generic/tfluids.cu:1203-1214
  const float eps = 1.17549435e-38f;
  if (fabsf(v) < eps) return v < 0.0f ? fminf(v, -eps) : fmaxf(v, eps);
  return v;
}

__device__ __forceinline__ bool cell_fluid(const float* __restrict__ flags, int o) { return (((int)flags[o]) & kFluid) != 0; }
__device__ __forceinline__ bool cell_obstacle(const float* __restrict__ flags, int o) { return (((int)flags[o]) & kObstacle) != 0; }

// ---- connected components -------------------------------------------------------------------------------
__device__ __forceinline__ void d_cc_init(Dom d, bool is3d, const float* __restrict__ flags, int* __restrict__ label,
                                                 int* __restrict__ border_fluid) {
  const int o = blockIdx.x * 256 + threadIdx.x;
  if (o >= d.sc) return;
  const bool f = cell_fluid(flags, o);
  label[o] = f ? o : -1;
  if (f) {
    const int i = o % d.X, j = (o / d.X) % d.Y, k = o / (d.X * d.Y);
    if (i < 1 || i > d.X - 2 || j < 1 || j > d.Y - 2 || (is3d && (k < 1 || k > d.Z - 2))) atomicAdd(border_fluid, 1);
  }
}

// hook: a cell that sees a smaller label next door pulls its own label AND its current root down to it
__device__ __forceinline__ void d_cc_hook(Dom d, bool is3d, int* __restrict__ label, int* __restrict__ changed) {
  const int o = blockIdx.x * 256 + threadIdx.x;
  if (o >= d.sc) return;
  const int l = label[o];
  if (l < 0) return;
  const int i = o % d.X, j = (o / d.X) % d.Y, k = o / (d.X * d.Y);
  int m = l;
  auto look = [&](int n) { const int ln = label[n]; if (ln >= 0 && ln < m) m = ln; };
  if (i > 0) look(o - 1);
  if (i < d.X - 1) look(o + 1);
  if (j > 0) look(o - d.sy);
  if (j < d.Y - 1) look(o + d.sy);
  if (is3d && k > 0) look(o - d.sz);
  if (is3d && k < d.Z - 1) look(o + d.sz);
  if (m < l) {
    atomicMin(&label[l], m);
    atomicMin(&label[o], m);
    *changed = 1;
  }
}
// compress: point every cell at the root of its tree
__device__ __forceinline__ void d_cc_compress(Dom d, int* __restrict__ label) {
  const int o = blockIdx.x * 256 + threadIdx.x;
  if (o >= d.sc) return;
  int l = label[o];
  if (l < 0) return;
  while (true) { const int p = label[l]; if (p == l) break; l = p; }
  label[o] = l;
}
// roots[0..count) = the cells that name a component; size_at[root] = cells in it
__device__ __forceinline__ void d_cc_count(Dom d, const int* __restrict__ label, int* __restrict__ size_at,
                                                  int* __restrict__ roots, int* __restrict__ count) {
  const int o = blockIdx.x * 256 + threadIdx.x;
  if (o >= d.sc) return;
  const int l = label[o];
  if (l < 0) return;
  // wave-aggregated: in the common case (one big component) all lanes carry the same label -> one atomic per wave
  const unsigned long long act = __ballot(1);
  const int leader = __ffsll((long long)act) - 1;
  const int l0 = __shfl(l, leader, 64);
  if (__ballot(l == l0) == act) { if ((int)(threadIdx.x & 63) == leader) atomicAdd(&size_at[l0], __popcll(act)); }
  else atomicAdd(&size_at[l], 1);
  if (l == o) { const int pos = atomicAdd(count, 1); if (pos < kMaxComponents) roots[pos] = o; }
}

// ---- reductions -----------------------------------------------------------------------------------------
__device__ __forceinline__ void block_partial(double v, double* __restrict__ partials) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  __shared__ double part[4];
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0) partials[blockIdx.x] = (part[0] + part[1]) + (part[2] + part[3]);
}
__device__ __forceinline__ double reduce_partials(const double* __restrict__ partials) {   // one block of 256
  double v = 0.0;
  for (int t = threadIdx.x; t < kRedBlocks; t += 256) v += partials[t];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  __shared__ double part[4];
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
  __syncthreads();
  return (part[0] + part[1]) + (part[2] + part[3]);   // valid in thread 0 (and everywhere: all read part[])
}

// ---- CG pieces ------------------------------------------------------------------------------------------
// x = 0, r = rhs on the component (0 elsewhere), partial r.r
__device__ __forceinline__ void d_pcg_setup(long long n, const int* __restrict__ label, int root,
                                                   const float* __restrict__ div, float* __restrict__ x,
                                                   float* __restrict__ r, float* __restrict__ s, double* __restrict__ partials) {
  double acc = 0.0;
  for (long long o = (long long)blockIdx.x * 256 + threadIdx.x; o < n; o += (long long)gridDim.x * 256) {
    const float v = (label[o] == root) ? div[o] : 0.0f;
    x[o] = 0.0f; r[o] = v; s[o] = 0.0f;
    acc += (double)v * v;
  }
  block_partial(acc, partials);
}
__device__ __forceinline__ void d_pcg_begin(PcgState* __restrict__ S, const double* __restrict__ partials, float tol,
                                                   int max_iter) {
  const double rr = reduce_partials(partials);
  if (threadIdx.x == 0) {
    S->rr1 = rr; S->rr0 = 0.0; S->num = 0.0; S->prev_num = 0.0; S->den = 0.0; S->alpha = 0.0f; S->beta = 0.0f;
    S->tol2 = tol * tol; S->iter = 0; S->max_iter = max_iter; S->first = 1; S->sum_x = 0.0; S->pending = 0;
    S->bad = (rr != rr) ? 1 : 0;
    S->done = (!((float)rr > S->tol2) || S->bad) ? 1 : 0;   // while (r_norm_sq1 > tol * tol && iter <= max_iter)
  }
}
// The scalar steps of an iteration (alpha, beta, the residual bookkeeping) ride at the head of the chip-wide kernel that
// needs them: every block folds the 512 partial sums itself, in the same fixed order, and block 0 records the result
// -- one launch per iteration for scalars (k_pcg_top) instead of four, which at 128^3 were a third of its time.
// Each reduction has its own partials buffer (a block may still be reading the previous one).
__device__ __forceinline__ void pcg_fold_residual(PcgState* __restrict__ S, double rr) {   // the end of an iteration
  S->prev_num = S->num;
  S->rr0 = S->rr1;
  S->rr1 = rr;
  S->first = 0;
  S->pending = 0;
  if (rr != rr) { S->bad = 1; S->done = 1; }
}
// end of the previous iteration (if one is pending), then the loop condition and iter++
__device__ __forceinline__ void d_pcg_top(PcgState* __restrict__ S, const double* __restrict__ p_rr, int test) {
  if (S->done) return;
  const int pending = S->pending;
  double rr = 0.0;
  if (pending) rr = reduce_partials(p_rr);
  if (threadIdx.x != 0) return;
  if (pending) pcg_fold_residual(S, rr);
  if (S->done || !test) return;
  if (!((float)S->rr1 > S->tol2) || S->iter > S->max_iter) { S->done = 1; return; }
  S->iter++;
}
// partial a.b over the grid (vectors are 0 off the component)
__device__ __forceinline__ void d_pcg_dot(const PcgState* __restrict__ S, long long n, const float* __restrict__ a,
                                                 const float* __restrict__ b, double* __restrict__ partials) {
  if (S->done) return;
  double acc = 0.0;
  for (long long o = (long long)blockIdx.x * 256 + threadIdx.x; o < n; o += (long long)gridDim.x * 256) acc += (double)a[o] * b[o];
  block_partial(acc, partials);
}
// beta (num = r.z from `p_num` when preconditioned, else r.r), then s = z + beta * s
// (iteration 1: s = z; the reference's scal-then-axpy order: (beta*s) + z)
__device__ __forceinline__ void d_pcg_dir(PcgState* __restrict__ S, long long n, const double* __restrict__ p_num, int precond,
                                                 const float* __restrict__ z, float* __restrict__ s) {
  if (S->done) return;
  const bool first = S->first != 0;
  double num = S->rr1;
  if (precond) num = reduce_partials(p_num);
  // beta_k = r_{k-1}.z_{k-1} / (r_{k-2}.z_{k-2}); the second is last iteration's numerator
  const float beta = first ? 0.0f : (float)num / clamp_to_epsilon((float)(precond ? S->prev_num : S->rr0));
  if (blockIdx.x == 0 && threadIdx.x == 0) { S->num = num; S->beta = beta; }
  for (long long o = (long long)blockIdx.x * 256 + threadIdx.x; o < n; o += (long long)gridDim.x * 256)
    s[o] = first ? z[o] : (beta * s[o] + 1.0f * z[o]);
}
// w = A s on the component, partial s.w
template <bool IS3D>
__device__ __forceinline__ void d_pcg_apply(const PcgState* __restrict__ S, Dom d, const float* __restrict__ flags,
                                                   const int* __restrict__ label, int root, const float* __restrict__ s,
                                                   float* __restrict__ w, double* __restrict__ partials) {
  if (S->done) return;
  double acc = 0.0;
  for (long long o = (long long)blockIdx.x * 256 + threadIdx.x; o < d.sc; o += (long long)gridDim.x * 256) {
    float v = 0.0f;
    // setupLaplacian, generic/tfluids.cu:938-1075: the row of an interior fluid cell. Every load is UNCONDITIONAL (round 4:
    // `if (f & kFluid) off += s[nb]` made each neighbour a branch whose join drains the load queue -- 14 memory round trips in
    // a row per cell); a cell outside the component reads its own index instead of its neighbours' and drops the values.
    const bool in = label[o] == root;
    const int nb[6] = {(int)o - d.sz, (int)o - d.sy, (int)o - 1, (int)o + 1, (int)o + d.sy, (int)o + d.sz};
    float fn[6], sn[6];
#pragma unroll
    for (int q = 0; q < 6; q++) {
      if (!IS3D && (q == 0 || q == 5)) { fn[q] = 0.0f; sn[q] = 0.0f; continue; }
      const long long e = in ? (long long)nb[q] : o;
      fn[q] = flags[e]; sn[q] = s[e];
    }
    const float so = s[o];
    if (in) {
      float diag = 0.0f, off = 0.0f;
#pragma unroll
      for (int q = 0; q < 6; q++) {
        if (!IS3D && (q == 0 || q == 5)) continue;
        const int f = (int)fn[q];
        if (!(f & kObstacle)) diag += 1.0f;
        if (f & kFluid) off += sn[q];
      }
      v = diag * so - off;
    }
    w[o] = v;
    acc += (double)so * v;
  }
  block_partial(acc, partials);
}
// alpha = num / s.w (from `p_den`), then x += alpha s; r -= alpha w; partial r.r
__device__ __forceinline__ void d_pcg_update(PcgState* __restrict__ S, long long n, const double* __restrict__ p_den,
                                                    const float* __restrict__ s, const float* __restrict__ w, float* __restrict__ x,
                                                    float* __restrict__ r, double* __restrict__ p_rr) {
  if (S->done) return;
  const double den = reduce_partials(p_den);
  const float alpha = (float)S->num / clamp_to_epsilon((float)den), nalpha = -alpha;
  if (blockIdx.x == 0 && threadIdx.x == 0) { S->den = den; S->alpha = alpha; S->pending = 1; }
  __syncthreads();      // reduce_partials' shared scratch is reused by block_partial below
  double acc = 0.0;
  for (long long o = (long long)blockIdx.x * 256 + threadIdx.x; o < n; o += (long long)gridDim.x * 256) {
    x[o] = alpha * s[o] + x[o];
    const float rv = nalpha * w[o] + r[o];
    r[o] = rv;
    acc += (double)rv * rv;
  }
  block_partial(acc, p_rr);
}
// sum of x over the component (for the mean), then p = x - mean on the component
__device__ __forceinline__ void d_pcg_sum(long long n, const float* __restrict__ x, double* __restrict__ partials) {
  double acc = 0.0;
  for (long long o = (long long)blockIdx.x * 256 + threadIdx.x; o < n; o += (long long)gridDim.x * 256) acc += (double)x[o];
  block_partial(acc, partials);
}
__device__ __forceinline__ void d_pcg_sum_end(PcgState* __restrict__ S, const double* __restrict__ partials) {
  const double v = reduce_partials(partials);
  if (threadIdx.x == 0) S->sum_x = v;
}
__device__ __forceinline__ void d_pcg_write(const PcgState* __restrict__ S, long long n, const int* __restrict__ label,
                                                   int root, int size, const float* __restrict__ x, float* __restrict__ p) {
  const float mean = (float)(S->sum_x / (double)size);
  for (long long o = (long long)blockIdx.x * 256 + threadIdx.x; o < n; o += (long long)gridDim.x * 256)
    if (label[o] == root) p[o] = x[o] - mean;      // copyPressureFromSystem, generic/tfluids.cu:1216-1240
}

// The bodies above (d_*) as the kernels of ONE system. pcg_batched.inc launches the same bodies with the batch item in blockIdx.y.
__global__ __launch_bounds__(256) void k_cc_init(Dom d, bool is3d, const float* __restrict__ flags, int* __restrict__ label,
                                                 int* __restrict__ border_fluid) { d_cc_init(d, is3d, flags, label, border_fluid); }
__global__ __launch_bounds__(256) void k_cc_hook(Dom d, bool is3d, int* __restrict__ label, int* __restrict__ changed) {
  d_cc_hook(d, is3d, label, changed);
}
__global__ __launch_bounds__(256) void k_cc_compress(Dom d, int* __restrict__ label) { d_cc_compress(d, label); }
__global__ __launch_bounds__(256) void k_cc_count(Dom d, const int* __restrict__ label, int* __restrict__ size_at,
                                                  int* __restrict__ roots, int* __restrict__ count) { d_cc_count(d, label, size_at, roots, count); }
__global__ __launch_bounds__(256) void k_pcg_setup(long long n, const int* __restrict__ label, int root,
                                                   const float* __restrict__ div, float* __restrict__ x,
                                                   float* __restrict__ r, float* __restrict__ s, double* __restrict__ partials) {
  d_pcg_setup(n, label, root, div, x, r, s, partials);
}
__global__ __launch_bounds__(256) void k_pcg_begin(PcgState* __restrict__ S, const double* __restrict__ partials, float tol,
                                                   int max_iter) { d_pcg_begin(S, partials, tol, max_iter); }
__global__ __launch_bounds__(256) void k_pcg_top(PcgState* __restrict__ S, const double* __restrict__ p_rr, int test) { d_pcg_top(S, p_rr, test); }
__global__ __launch_bounds__(256) void k_pcg_dot(const PcgState* __restrict__ S, long long n, const float* __restrict__ a,
                                                 const float* __restrict__ b, double* __restrict__ partials) { d_pcg_dot(S, n, a, b, partials); }
__global__ __launch_bounds__(256) void k_pcg_dir(PcgState* __restrict__ S, long long n, const double* __restrict__ p_num, int precond,
                                                 const float* __restrict__ z, float* __restrict__ s) { d_pcg_dir(S, n, p_num, precond, z, s); }
template <bool IS3D>
__global__ __launch_bounds__(256) void k_pcg_apply(const PcgState* __restrict__ S, Dom d, const float* __restrict__ flags,
                                                   const int* __restrict__ label, int root, const float* __restrict__ s,
                                                   float* __restrict__ w, double* __restrict__ partials) {
  d_pcg_apply<IS3D>(S, d, flags, label, root, s, w, partials);
}
__global__ __launch_bounds__(256) void k_pcg_update(PcgState* __restrict__ S, long long n, const double* __restrict__ p_den,
                                                    const float* __restrict__ s, const float* __restrict__ w, float* __restrict__ x,
                                                    float* __restrict__ r, double* __restrict__ p_rr) { d_pcg_update(S, n, p_den, s, w, x, r, p_rr); }
__global__ __launch_bounds__(256) void k_pcg_sum(long long n, const float* __restrict__ x, double* __restrict__ partials) { d_pcg_sum(n, x, partials); }
__global__ __launch_bounds__(256) void k_pcg_sum_end(PcgState* __restrict__ S, const double* __restrict__ partials) { d_pcg_sum_end(S, partials); }
__global__ __launch_bounds__(256) void k_pcg_write(const PcgState* __restrict__ S, long long n, const int* __restrict__ label,
                                                   int root, int size, const float* __restrict__ x, float* __restrict__ p) {
  d_pcg_write(S, n, label, root, size, x, p);
}

// ---- ILU(0) / IC(0) on the 5/7-point pattern: wavefront sweeps over hyperplanes h = i + j + k -------------
// thread -> (j, k) of the hyperplane, i = h - j - k
struct Wave { int i, j, k, o; bool ok; };
template <bool IS3D>
__device__ __forceinline__ Wave wave_cell(const Dom& d, int h, const int* __restrict__ label, int root) {
  Wave c;
  const int t = blockIdx.x * 256 + threadIdx.x;
  c.j = 1 + t % (d.Y - 2);
  c.k = IS3D ? 1 + t / (d.Y - 2) : 0;
  c.i = h - c.j - c.k;
  c.ok = c.i >= 1 && c.i <= d.X - 2 && (!IS3D || c.k <= d.Z - 2) && t < (d.Y - 2) * (IS3D ? d.Z - 2 : 1);
  c.o = c.ok ? TFL_AT(d, c.i, c.j, c.k) : 0;
  if (c.ok && label[c.o] != root) c.ok = false;
  return c;
}
// dg(n) = a(n,n) - sum_{lower fluid nbrs m} 1/dg(m)
template <bool IS3D>
__global__ __launch_bounds__(256) void k_ilu_factor(Dom d, int h, const float* __restrict__ flags, const int* __restrict__ label,
                                                    int root, float* __restrict__ dg) {
  const Wave c = wave_cell<IS3D>(d, h, label, root);
  if (!c.ok) return;
  const int nb[6] = {c.o - d.sz, c.o - d.sy, c.o - 1, c.o + 1, c.o + d.sy, c.o + d.sz};
  float diag = 0.0f;
#pragma unroll
  for (int q = 0; q < 6; q++) {
    if (!IS3D && (q == 0 || q == 5)) continue;
    if (!(((int)flags[nb[q]]) & kObstacle)) diag += 1.0f;
  }
#pragma unroll
  for (int q = 0; q < 3; q++) {       // lower neighbours in column order: z-1, y-1, x-1
    if (!IS3D && q == 0) continue;
    if (((int)flags[nb[q]]) & kFluid) diag -= 1.0f / dg[nb[q]];
  }
  dg[c.o] = diag;
}
// forward solve.  ilu0: y(n) = r(n) + sum_m y(m)/dg(m).   ic0: y(n) = (r(n) + sum_m y(m)/R(m,m)) / R(n,n)
template <bool IS3D, bool IC>
__global__ __launch_bounds__(256) void k_ilu_forward(const PcgState* __restrict__ S, Dom d, int h, const float* __restrict__ flags,
                                                     const int* __restrict__ label, int root, const float* __restrict__ dg,
                                                     const float* __restrict__ r, float* __restrict__ y) {
  if (S->done) return;
  const Wave c = wave_cell<IS3D>(d, h, label, root);
  if (!c.ok) return;
  const int nb[3] = {c.o - d.sz, c.o - d.sy, c.o - 1};
  float v = r[c.o];
#pragma unroll
  for (int q = 0; q < 3; q++) {
    if (!IS3D && q == 0) continue;
    if (((int)flags[nb[q]]) & kFluid) v += IC ? y[nb[q]] / sqrtf(dg[nb[q]]) : y[nb[q]] / dg[nb[q]];
  }
  y[c.o] = IC ? v / sqrtf(dg[c.o]) : v;
}
// backward solve. ilu0: z(n) = (y(n) + sum_q z(q)) / dg(n).   ic0: z(n) = (y(n) + (sum_q z(q)) / R(n,n)) / R(n,n)
template <bool IS3D, bool IC>
__global__ __launch_bounds__(256) void k_ilu_backward(const PcgState* __restrict__ S, Dom d, int h, const float* __restrict__ flags,
                                                      const int* __restrict__ label, int root, const float* __restrict__ dg,
                                                      const float* __restrict__ y, float* __restrict__ z) {
  if (S->done) return;
  const Wave c = wave_cell<IS3D>(d, h, label, root);
  if (!c.ok) return;
  const int nb[3] = {c.o + 1, c.o + d.sy, c.o + d.sz};
  float acc = 0.0f;
#pragma unroll
  for (int q = 0; q < 3; q++) {
    if (!IS3D && q == 2) continue;
    if (((int)flags[nb[q]]) & kFluid) acc += z[nb[q]];
  }
  if (IC) { const float rnn = sqrtf(dg[c.o]); z[c.o] = (y[c.o] + acc / rnn) / rnn; }
  else z[c.o] = (y[c.o] + acc) / dg[c.o];
}

// ---- the triangular solves as TWO launches: pipelined wavefronts (3-D) ------------------------------------------
// A lexicographic IC(0) / ILU(0) solve is a 3-D recurrence: cell (i, j, k) needs (i-1, j, k), (i, j-1, k), (i, j, k-1).
// One launch per hyperplane (above) is X+Y+Z-6 launches per solve, ~760 per CG iteration at 128^3: 2.7 ms of launch
// latency around ~20 us of arithmetic. Here a sweep is ONE launch:
//   * the interior is cut into sub-boxes of 64 rows (j) x kWfPlanes (8) planes (k) x all of x; a block of 8 COMPUTE waves
//     + 2 HELPER waves owns one: compute wave w <-> plane, lane l <-> row, and at step t the thread works on the cell
//     with (i-1) + l + kWfLag w = t. Its three predecessors were computed one step earlier by itself (x: a register),
//     one step earlier by the lane below (y: one DPP wave shift) and kWfLag (2) steps earlier by the wave below (z).
//     That lag lets the waves of a block exchange through LDS once per kWfLag steps ("interval"): one 8-byte read, one
//     8-byte write and one barrier. A step is a dependent chain of ~60 ns (tools/ubench/chain_latency.hip);
//   * a block's steps are bound by its CU: four waves per SIMD would take turns at ~12 instructions per step, and every
//     operand and result of the sub-box passes through one CU's 64 B/clk vector-memory pipe. Hence two waves per SIMD
//     (8 planes) and SKEWED arrays laid out [sub-box][plane][t / 4][row][t % 4]: per group of four steps a wave reads
//     cc and r and writes its results with ONE 16-byte access each. Two chip-wide kernels per solve copy r into, and
//     z out of, that layout (k_wf_skew);
//   * sub-boxes depend on their lower j / k neighbours through global memory, with no flags and no fences: the edge
//     plane and the edge lanes of a block are also stored as 8-byte {value, tag} pairs (tag = the launch's sequence
//     number) into hand-off arrays, and the consumer re-reads a pair until it carries this launch's tag (bounded; an
//     error word ends the solve instead of hanging the GPU). All of that is the HELPER waves' job (one for the slab
//     direction, one for the strips): they prefetch the predecessors' pairs a few intervals ahead, hand the values to
//     the compute waves through the same LDS slots a neighbouring plane would use, and publish the block's own edge
//     results out of those slots. The compute waves run a branch-free loop with nothing but their operand prefetch in
//     flight -- a wave's loads complete in issue order, and with the short-fused pair loads in the same queue every
//     operand prefetch had to arrive within their two groups (measured: memory latency / 8 per step, whatever the
//     block's size). A consumer settles by itself at the smallest lag behind its predecessor that memory latency allows.
// With c = 1/sqrt(d) (IC) or 1/d (ILU) and cc = c*c (IC) or c (ILU), both factorisations run the same recurrences:
//   forward    q = (((r + q_z) + q_y) + q_x) * cc          (q = y * c of the reference's forward solve)
//   backward   z = q + ((z_x + z_y) + z_z) * cc
// (the reference divides by R(m,m) / d(m) where this multiplies by reciprocals: inside the solver's tolerance).
// The shape constants (kWfRows, kWfPlanes, kWfLag, kWfDepth, kWfHelperAhead, kWfGuard), WfGeom / wf_geom and the sizes of the
// skewed and hand-off arrays are plain data shared with the host's workspace table: tfl_pcg_ws.hpp.

// the sub-box of a workgroup: blocks of one launch are numbered strip-major over the launch's slabs
__device__ __forceinline__ int wf_block(const WfGeom& g, int& sidx, int& bidx) {
  sidx = (int)blockIdx.x / g.b_cnt;
  bidx = g.b_lo + ((int)blockIdx.x - sidx * g.b_cnt);
  return sidx * g.nb + bidx;
}
inline bool wf_usable(bool is3d, int Z, int Y, int X) {
  if (!is3d || X < 3 || Y < 3 || Z < 3) return false;
  const bool off = sw::present(Sw::PCG_HYPERPLANES);     // A/B switch: the one-launch-per-hyperplane sweeps
  const WfGeom g = wf_geom(Z, Y, X);
  return !off && g.ns <= kWfMaxBlocks;      // (grids with more sub-boxes than fit the GPU at once run slab range by slab range)
}
__device__ __forceinline__ long long wf_at(const WfGeom& g, int i, int j, int k) {
  const int s = (j - 1) / kWfRows, l = (j - 1) % kWfRows, b = (k - 1) / kWfPlanes, w = (k - 1) % kWfPlanes;
  const int t = (i - 1) + l + kWfLag * w;
  return ((((long long)(s * g.nb + b) * kWfPlanes + w) * (g.NT / 4) + (t >> 2)) * kWfRows + l) * 4 + (t & 3);
}

// cc (skewed) from the factor's diagonal: one thread per interior cell
template <bool IC>
__global__ __launch_bounds__(256) void k_wf_build(WfGeom g, Dom d, const int* __restrict__ label, int root, const float* __restrict__ dg,
                                                  float* __restrict__ cs) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  const int nx = g.X - 2, ny = g.Y - 2, nz = g.Z - 2;
  if (t >= (long long)nx * ny * nz) return;
  const int i = 1 + (int)(t % nx), j = 1 + (int)((t / nx) % ny), k = 1 + (int)(t / ((long long)nx * ny));
  const int o = TFL_AT(d, i, j, k);
  float cc = 0.0f;
  if (label[o] == root) {
    if (IC) { const float c = 1.0f / sqrtf(dg[o]); cc = c * c; }
    else cc = 1.0f / dg[o];
  }
  cs[wf_at(g, i, j, k)] = cc;
}

// natural layout <-> skewed layout of a vector on the interior cells (chip-wide, one thread per cell: the sweeps
// themselves must not gather / scatter -- a wave's 64 rows are 64 cache lines per instruction)
template <bool TO_SKEWED>
__global__ __launch_bounds__(256) void k_wf_skew(const PcgState* __restrict__ S, WfGeom g, Dom d, float* __restrict__ nat, float* __restrict__ skw) {
  if (S->done) return;
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  const int nx = g.X - 2, ny = g.Y - 2, nz = g.Z - 2;
  if (t >= (long long)nx * ny * nz) return;
  const int i = 1 + (int)(t % nx), j = 1 + (int)((t / nx) % ny), k = 1 + (int)(t / ((long long)nx * ny));
  const int o = TFL_AT(d, i, j, k);
  const long long a = wf_at(g, i, j, k);
  if (TO_SKEWED) skw[a] = nat[o];
  else nat[o] = skw[a];
}

// {value, tag} pairs: one 8-byte access, coherent across the chip (sc1), so a tag never arrives before its value
__device__ __forceinline__ unsigned long long wf_load_pair(const float2* p) {
  return __hip_atomic_load(reinterpret_cast<const unsigned long long*>(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void wf_store_pair(float2* p, float v, int tag) {
  const unsigned long long u = (unsigned long long)__float_as_uint(v) | ((unsigned long long)(unsigned)tag << 32);
  __hip_atomic_store(reinterpret_cast<unsigned long long*>(p), u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// the same loads for the retry path, opaque to the compiler's wait-count bookkeeping (they complete before they return)
__device__ __forceinline__ unsigned long long wf_reload_pair(const float2* p) {
  unsigned long long v;
  asm volatile("global_load_dwordx2 %0, %1, off sc1\n\ts_waitcnt vmcnt(0)" : "=&v"(v) : "v"(p) : "memory");
  return v;
}
__device__ __forceinline__ int wf_reload_word(const int* p) {
  int v;
  asm volatile("global_load_dword %0, %1, off sc1\n\ts_waitcnt vmcnt(0)" : "=&v"(v) : "v"(p) : "memory");
  return v;
}
__device__ __forceinline__ float wf_value(unsigned long long u) { return __uint_as_float((unsigned)u); }
__device__ __forceinline__ int wf_tag(unsigned long long u) { return (int)(u >> 32); }

// kWfLag consecutive floats of one lane with one LDS access
__device__ __forceinline__ void wf_lds_read(const float* p, float* v) {
  if (kWfLag == 4) { const float4 t = *reinterpret_cast<const float4*>(p); v[0] = t.x; v[1] = t.y; v[2 % kWfLag] = t.z; v[3 % kWfLag] = t.w; }
  else if (kWfLag == 2) { const float2 t = *reinterpret_cast<const float2*>(p); v[0] = t.x; v[1 % kWfLag] = t.y; }
  else v[0] = *p;
}
__device__ __forceinline__ void wf_lds_write(float* p, const float* v) {
  if (kWfLag == 4) *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1 % kWfLag], v[2 % kWfLag], v[3 % kWfLag]);
  else if (kWfLag == 2) *reinterpret_cast<float2*>(p) = make_float2(v[0], v[1 % kWfLag]);
  else *p = v[0];
}

struct WfArrays {
  const float* cs;      // cc
  const float* in;      // forward: r; backward: q
  float* out;           // forward: q; backward: z
  float2* hk;           // slab hand-off pairs of this launch's results
  float2* hs;           // strip hand-off pairs
  int* err;
  long long* trace;     // TFL_WF_TRACE: [block][2] = wall clock (10 ns units) at a block's first and last step, else null
};

// A COMPUTE wave's share of a sweep (wave w < kWfPlanes <-> plane). DIR = +1 forward (lower neighbours), -1 backward
// (upper neighbours, steps run from the last to the first). It touches global memory only for its own operands and
// results: what it needs from other sub-boxes arrives through LDS from the block's HELPER wave (below), in the same
// slots and with the same lag as what it needs from the plane next door.
template <int DIR>
__device__ __forceinline__ void wf_compute(const WfGeom& g, const WfArrays& A, int tag, float (*ring)[2][kWfRows][kWfLag],
                                           float (*edge_s)[kWfPlanes + 1][kWfLag]) {
  constexpr int D = kWfDepth, G = D / 4;
  int sidx, bidx;
  const int blk = wf_block(g, sidx, bidx);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int NT = g.NT, NG = NT / 4;
  const long long base4 = ((long long)blk * kWfPlanes + w) * NG * kWfRows + lane;       // in float4 units; + group * 64
  const float4* c4 = reinterpret_cast<const float4*>(A.cs) + base4;
  const float4* i4 = reinterpret_cast<const float4*>(A.in) + base4;
  float4* o4 = reinterpret_cast<float4*>(A.out) + base4;
  // the wave whose results this one consumes with a lag: the plane below / above, or the helper (index kWfPlanes) for
  // the plane that borders the slab predecessor
  const int nbw = DIR > 0 ? (w > 0 ? w - 1 : kWfPlanes) : (w + 1 < kWfPlanes ? w + 1 : kWfPlanes);
  auto grp = [&](int ig) { return DIR > 0 ? ig : NG - 1 - ig; };           // memory group of the ig-th group in time

  // operands, prefetched G groups ahead into rotating registers (slot = group mod G; the loop below is unrolled by G)
  float4 cv[G], rv[G];
  auto issue = [&](int ig, int slot) {
    const int gm = grp(ig);
    cv[slot] = c4[(long long)gm * kWfRows];
    rv[slot] = i4[(long long)gm * kWfRows];
  };
  float q_prev = 0.0f;      // this thread's previous result (forward: q, backward: z)
  auto body = [&](int t0, auto more) {
#pragma unroll
    for (int c = 0; c < G; c++) {
      const int ig = t0 / 4 + c, gm = grp(ig);
      // in memory the group is ordered by t; backward walks it from its last element
      const float ccs[4] = {DIR > 0 ? cv[c].x : cv[c].w, DIR > 0 ? cv[c].y : cv[c].z, DIR > 0 ? cv[c].z : cv[c].y, DIR > 0 ? cv[c].w : cv[c].x};
      const float ins[4] = {DIR > 0 ? rv[c].x : rv[c].w, DIR > 0 ? rv[c].y : rv[c].z, DIR > 0 ? rv[c].z : rv[c].y, DIR > 0 ? rv[c].w : rv[c].x};
      float h4[4];
#pragma unroll
      for (int e = 0; e < 4 / kWfLag; e++) {       // LDS exchanges of this group: kWfLag steps each
        const int par = (c * (4 / kWfLag) + e) & 1;
        float below[kWfLag], edge[kWfLag];
        wf_lds_read(&ring[nbw][par ^ 1][lane][0], below);      // what the neighbour wave computed during the previous interval
        wf_lds_read(&edge_s[par ^ 1][w][0], edge);             // the strip predecessor's values for the edge lane (every lane reads them)
#pragma unroll
        for (int v = 0; v < kWfLag; v++) {
          const int u4 = e * kWfLag + v;
          // y neighbour: the lane below / above; the edge lane (0 forward, 63 backward) has no source lane and keeps `old`
          float nb_y = __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, edge[v]), __builtin_bit_cast(int, q_prev),
                                                                               DIR > 0 ? 0x138 /*wave_shr:1*/ : 0x130 /*wave_shl:1*/, 0xf, 0xf, false));
          asm volatile("" : "+v"(nb_y));
          float res;
          if (DIR > 0) res = (((ins[u4] + below[v]) + nb_y) + q_prev) * ccs[u4];
          else res = __builtin_fmaf((q_prev + nb_y) + below[v], ccs[u4], ins[u4]);
          h4[u4] = res;
          q_prev = res;
        }
        wf_lds_write(&ring[w][par][lane][0], &h4[e * kWfLag]);
        // workgroup barrier that waits for the LDS write only (__syncthreads() would also drain the operand prefetch)
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
      }
      const float m4[4] = {DIR > 0 ? h4[0] : h4[3], DIR > 0 ? h4[1] : h4[2], DIR > 0 ? h4[2] : h4[1], DIR > 0 ? h4[3] : h4[0]};   // by t
      o4[(long long)gm * kWfRows] = make_float4(m4[0], m4[1], m4[2], m4[3]);
      if constexpr (decltype(more)::value) issue(ig + G, c);
    }
  };
#pragma unroll
  for (int c = 0; c < G; c++) issue(c, c);
  if (A.trace && threadIdx.x == 0) A.trace[blk * 2] = wall_clock64();
  // the helper has to deliver the first interval's edge values before anyone starts (it is the "+1" of this barrier)
  asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
  int t0 = 0;
  for (; t0 + D < NT; t0 += D) body(t0, std::true_type{});
  body(t0, std::false_type{});
  if (A.trace && threadIdx.x == 0) A.trace[blk * 2 + 1] = wall_clock64();
}

// The HELPER wave of a block (wave index kWfPlanes): it alone reads what other sub-boxes hand over, and passes it on
// through LDS one exchange interval ahead of its use, in step with the block's barriers:
//   ring[kWfPlanes][.][lane][.]  the slab predecessor's edge-plane values  -> read by the bordering plane as its "plane next door"
//   edge_s[.][w][.]              the strip predecessor's edge-lane values of plane w -> the DPP `old` of every compute wave
// Its loads are the only ones in the block with a short fuse (the pairs exist only a few steps before they are needed),
// and a wave's loads complete in issue order: in a compute wave they made every operand prefetch issued before them
// wait in line (measured: each step of every block then cost memory latency / 8, whatever the block's size). Here they
// have a wave -- and a vmcnt -- of their own. Pairs are prefetched kWfHelperAhead intervals ahead, checked against this
// launch's tag and re-read until they carry it (bounded; an error word ends the solve instead of hanging the GPU).
template <int DIR, int ROLE>
__device__ __forceinline__ void wf_helper(const WfGeom& g, const WfArrays& A, int tag, float (*ring)[2][kWfRows][kWfLag],
                                          float (*edge_s)[kWfPlanes + 1][kWfLag]) {
  constexpr int P = kWfHelperAhead, NI = kWfDepth / kWfLag;     // the loop is unrolled by NI intervals (one compute body); NI % P == 0
  constexpr bool SLAB = ROLE == 0;
  int sidx, bidx;
  const int blk = wf_block(g, sidx, bidx);
  const int lane = threadIdx.x & 63;
  const int NT = g.NT, NG = NT / 4;
  const int ps = DIR > 0 ? (sidx > 0 ? blk - g.nb : -1) : (sidx + 1 < g.ns ? blk + g.nb : -1);
  const int pk = DIR > 0 ? (bidx > 0 ? blk - 1 : -1) : (bidx + 1 < g.nb ? blk + 1 : -1);
  const bool has_pred = SLAB ? pk >= 0 : ps >= 0;
  const bool has_succ = SLAB ? (DIR > 0 ? bidx + 1 < g.nb : bidx > 0) : (DIR > 0 ? sidx + 1 < g.ns : sidx > 0);     // someone reads what this block publishes
  // SLAB: lane <-> row of the edge plane, kWfLag pairs per interval. STRIP: lane = w * kWfLag + v <-> (plane w, step v in
  // memory order of the interval) of the edge lane; the lanes beyond that work on a spare row / the guard padding
  const int sw = min(lane / kWfLag, kWfPlanes), sv = lane % kWfLag;
  const bool live = SLAB || lane < kWfPlanes * kWfLag;
  const float2* from = SLAB ? A.hk + ((long long)(has_pred ? pk : blk) * NG * kWfRows + lane) * 4
                            : A.hs + ((long long)(has_pred ? ps : blk) * kWfPlanes + min(sw, kWfPlanes - 1)) * NT;
  float2* mine = SLAB ? A.hk + ((long long)blk * NG * kWfRows + lane) * 4 : A.hs + ((long long)blk * kWfPlanes + min(sw, kWfPlanes - 1)) * NT;
  constexpr int kOff = SLAB ? DIR * kWfLag * (kWfPlanes - 1) : DIR * (kWfRows - 1);
  constexpr int NV = SLAB ? kWfLag : 1;       // pairs per lane and interval
  // the first step IN MEMORY ORDER of interval iv (an interval's kWfLag steps are consecutive in t, and so are their pairs
  // in both hand-off arrays: kOff of the slab is a multiple of kWfLag and a group of four steps never splits an interval)
  auto t_lo = [&](int iv) { return DIR > 0 ? iv * kWfLag : NT - (iv + 1) * kWfLag; };
  // addresses are NOT clamped: both arrays carry kWfGuard pairs of padding at either end (wf_floats), a pair outside
  // [0, NT) is loaded from a neighbouring block's rows or the padding and never looked at
  auto at = [&](const float2* base, int t) { return SLAB ? base + (long long)(t >> 2) * (4 * kWfRows) + (t & 3) : base + (t + sv); };

  unsigned long long pv[P][NV];      // rotating: the pairs of interval (index mod P)
  bool dead = false;
  auto issue = [&](int iv, int slot) {
    const float2* src = at(from, t_lo(iv) + kOff);
#pragma unroll
    for (int v = 0; v < NV; v++) pv[slot][v] = wf_load_pair(src + v);
  };
  // deliver interval iv's values into the slots the compute waves read during interval iv (parity of iv, inverted). A
  // helper is one wave running a serial instruction stream in step with eight that do ~25 instructions per interval: its
  // fast path is straight-line (one test and branch for all the interval's pairs); re-reading is the rare path
  auto deliver = [&](int iv, int slot) {
    const int par = iv & 1;
    const int tp = t_lo(iv) + kOff + (SLAB ? 0 : sv);
    const bool want = has_pred && live && tp >= 0 && tp < NT;       // SLAB: wave-uniform, the same for the interval's steps
    bool stale = false;
#pragma unroll
    for (int v = 0; v < NV; v++) stale |= want && wf_tag(pv[slot][v]) != tag;
    if (__builtin_expect(__ballot(stale) != 0ull, 0) && !dead) {
      for (int spin = 0;; spin++) {
        bool again = false;
#pragma unroll
        for (int v = 0; v < NV; v++) {
          if (want && wf_tag(pv[slot][v]) != tag) pv[slot][v] = wf_reload_pair(at(from, t_lo(iv) + kOff) + v);
          again |= want && wf_tag(pv[slot][v]) != tag;
        }
        if (__ballot(again) == 0ull) break;
        // never hang the GPU: give up after ~1 s, or when another block already has (looked at every 64th retry only)
        if (spin > (1 << 17) || ((spin & 63) == 63 && wf_reload_word(A.err))) { atomicExch(A.err, 1); dead = true; break; }
      }
    }
    if (SLAB) {
      float kval[kWfLag];     // in TIME order of the interval's steps, like a compute wave's results
#pragma unroll
      for (int v = 0; v < kWfLag; v++) kval[v] = want ? wf_value(pv[slot][DIR > 0 ? v : kWfLag - 1 - v]) : 0.0f;
      wf_lds_write(&ring[kWfPlanes][par ^ 1][lane][0], kval);
    } else {
      edge_s[par ^ 1][sw][DIR > 0 ? sv : kWfLag - 1 - sv] = want ? wf_value(pv[slot][0]) : 0.0f;
    }
  };
  // publish interval iv's results of the block's edge plane (-> the slab successor) resp. of every plane's edge lane (->
  // the strip successor) as {value, tag} pairs, out of the LDS slots the compute waves wrote them to during interval iv
  // (stable until the barrier that ends interval iv + 1): the compute waves carry no hand-off code at all
  auto publish = [&](int iv, int ptag) {
    if (!has_succ) return;        // block-uniform
    const int par = iv & 1;
    float res[kWfLag];            // time order
    wf_lds_read(SLAB ? &ring[DIR > 0 ? kWfPlanes - 1 : 0][par][lane][0] : &ring[min(sw, kWfPlanes - 1)][par][DIR > 0 ? kWfRows - 1 : 0][0], res);
    float2* dst = live ? const_cast<float2*>(at(mine, t_lo(iv))) : A.hs - 1 - lane;       // idle lanes: into the guard padding
    if (SLAB) {
#pragma unroll
      for (int v = 0; v < kWfLag; v++) wf_store_pair(dst + v, res[DIR > 0 ? v : kWfLag - 1 - v], ptag);
    } else {
      float one = res[0];
#pragma unroll
      for (int v = 1; v < kWfLag; v++) one = (DIR > 0 ? sv : kWfLag - 1 - sv) == v ? res[v] : one;
      wf_store_pair(dst, one, live ? ptag : 0);
    }
  };
  const int n_iv = NT / kWfLag;
#pragma unroll
  for (int i = 0; i < P; i++) issue(i, i);
  deliver(0, 0);
  issue(P, 0);
  asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");      // the compute waves' start barrier
  // during interval iv a helper publishes interval iv - 1, delivers interval iv + 1 and prefetches interval iv + 1 + P
  for (int iv0 = 0; iv0 < n_iv; iv0 += NI) {
#pragma unroll
    for (int i = 0; i < NI; i++) {
      // no branch around the loads (hipcc sizes the loop's vmcnt waits for the path that issues fewest): past the end the
      // last interval is delivered again, into slots nobody reads any more
      const int iv = iv0 + i;
      publish(max(iv - 1, 0), iv > 0 ? tag : 0);          // (interval 0 has nothing behind it: a pair nobody will accept)
      deliver(min(iv + 1, n_iv - 1), (i + 1) % P);
      issue(min(iv + 1 + P, n_iv - 1), (i + 1) % P);
      asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    }
  }
  publish(n_iv - 1, tag);
}

template <int DIR>
__global__ __launch_bounds__((kWfPlanes + 2) * 64) void k_wf_sweep(const PcgState* __restrict__ S, WfGeom g, WfArrays A, int tag) {
  if (S->done) return;
  __shared__ __attribute__((aligned(16))) float ring[kWfPlanes + 1][2][kWfRows][kWfLag];   // results of a wave's last two exchange intervals
  __shared__ __attribute__((aligned(16))) float edge_s[2][kWfPlanes + 1][kWfLag];     // [.][kWfPlanes]: spare row for the helper's idle lanes
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  if (w <= kWfPlanes) {
#pragma unroll
    for (int v = 0; v < kWfLag; v++) ring[w][0][lane][v] = ring[w][1][lane][v] = 0.0f;
  }
  if (threadIdx.x < 2 * (kWfPlanes + 1) * kWfLag) (&edge_s[0][0][0])[threadIdx.x] = 0.0f;
  __syncthreads();
  if (w < kWfPlanes) wf_compute<DIR>(g, A, tag, ring, edge_s);
  else if (w == kWfPlanes) wf_helper<DIR, 0>(g, A, tag, ring, edge_s);
  else wf_helper<DIR, 1>(g, A, tag, ring, edge_s);
}

// ---- normalizePressureMean (generic/tfluids.cc:845-925): p -= mean of p over the cell's fluid component ----
__global__ __launch_bounds__(256) void k_npm_sum(Dom d, const int* __restrict__ label, const float* __restrict__ p,
                                                 double* __restrict__ sum_at) {
  const int o = blockIdx.x * 256 + threadIdx.x;
  const int l = o < d.sc ? label[o] : -1;
  const bool valid = l >= 0;
  const unsigned long long vm = __ballot(valid);
  if (!vm) return;                                   // wave-uniform
  // one fp64 atomic per wave when every fluid lane of the wave sits in the same component (the common case)
  const int l0 = __shfl(l, __ffsll((long long)vm) - 1, 64);
  double v = valid ? (double)p[o] : 0.0;
  if (__ballot(valid && l != l0) == 0ull) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    if ((threadIdx.x & 63) == 0) atomicAdd(&sum_at[l0], v);
  } else if (valid) {
    atomicAdd(&sum_at[l], v);
  }
}
__global__ __launch_bounds__(256) void k_npm_sub(Dom d, const int* __restrict__ label, const int* __restrict__ size_at,
                                                 const double* __restrict__ sum_at, float* __restrict__ p) {
  const int o = blockIdx.x * 256 + threadIdx.x;
  if (o >= d.sc) return;
  const int l = label[o];
  if (l < 0) return;
  p[o] = p[o] - (float)(sum_at[l] / (double)size_at[l]);
}

// ---- host code ------------------------------------------------------------------------------------------------------------
inline int cdiv(long long a, int b) { return (int)((a + b - 1) / b); }

template <class T>
T* view(float* workspace, WsRegion r) { return reinterpret_cast<T*>(workspace + r.off); }

// the caller's message buffer; a failed HIP call reads "<operator>: <what>: <the runtime's text>"
struct Report {
  const char* who;
  char* msg;
  size_t len;
  bool ok(hipError_t e, const char* what) const {
    if (e == hipSuccess) return true;
    snprintf(msg, len, "%s: %s: %s", who, what, hipGetErrorString(e));
    return false;
  }
};
#define HIP_TRY(call, what) do { if (!er.ok(call, what)) return PcgResult::hip_error; } while (0)
#define PCG_TRY(call) do { const PcgResult rc_ = (call); if (rc_ != PcgResult::ok) return rc_; } while (0)

// a "k_cc" scope, or none
struct CcTimer {
  std::optional<KernelTimer> t;
  CcTimer(bool on, hipStream_t st) { if (on) t.emplace("k_cc", st); }
};

// counters: [0] changed, [1] count, [2] border fluid
PcgResult clear_component_counts(hipStream_t st, const Report& er, int* counters, int* size_at, long long n) {
  HIP_TRY(hipMemsetAsync(counters, 0, 3 * sizeof(int), st), "memset");
  HIP_TRY(hipMemsetAsync(size_at, 0, sizeof(int) * (size_t)n, st), "memset");
  return PcgResult::ok;
}

// label[o] = the smallest cell index of o's fluid component (-1: no fluid): init, then hook + compress until a round changes
// nothing. h_cnt: the counters as the last round left them. timed: with "k_cc" scopes of its own (init | each round), as
// pcg_solve has them; normalize_pressure_mean keeps ONE scope around everything it launches for an item instead.
PcgResult label_components(hipStream_t st, const Report& er, const Dom& d, bool is3d, const float* fl, int* label, int* counters,
                           int h_cnt[3], bool timed) {
  const int gcell = cdiv(d.sc, 256);
  { CcTimer t(timed, st); k_cc_init<<<gcell, 256, 0, st>>>(d, is3d, fl, label, counters + 2); }
  for (int round = 0;; round++) {
    HIP_TRY(hipMemsetAsync(counters, 0, sizeof(int), st), "memset");
    { CcTimer t(timed, st);
      k_cc_hook<<<gcell, 256, 0, st>>>(d, is3d, label, counters);
      k_cc_compress<<<gcell, 256, 0, st>>>(d, label); }
    HIP_TRY(hipMemcpyAsync(h_cnt, counters, 3 * sizeof(int), hipMemcpyDeviceToHost, st), "memcpy");
    HIP_TRY(hipStreamSynchronize(st), "sync");
    if (!h_cnt[0]) return PcgResult::ok;
    if (round > 100000) { snprintf(er.msg, er.len, "%s: component labelling did not converge", er.who); return PcgResult::hip_error; }
  }
}

// One call of pcg_solve: the problem, the views of its workspace (tfl_pcg_ws.hpp), and what one phase hands to the next.
struct Solve {
  hipStream_t st;
  const PcgProblem& q;
  Report er;
  Dom d;
  long long n;
  // the workspace
  double *partials, *p_den, *p_rr;     // r.r of the set-up, r.z, the sum of x | s.w | r.r of the update
  PcgState* S;
  int *label, *size_at, *roots, *counters;
  float *x, *r, *z, *s, *w, *dg, *y;
  // pipelined wavefront sweeps (3-D): the skewed arrays (cc, r, q, z), the two hand-off arrays of {value, tag} pairs, an error word
  bool wf;
  WfGeom wg;
  float *cs = nullptr, *rsk = nullptr, *qsk = nullptr, *zsk = nullptr;
  float2 *wf_hk = nullptr, *wf_hs = nullptr;
  int* wferr = nullptr;
  size_t wf_clear_bytes = 0;
  int wf_slabs = 1;                    // slabs per launch
  int epoch = 0;                       // tag of the next sweep; the skewed arrays are zeroed with it
  long long* wf_trace = nullptr;       // TFL_WF_TRACE
  // the multigrid hierarchy (pc == 3): its levels' geometry and arrays
  bool mg;
  MgDev mgd{};
  int* mg_open = nullptr;              // device word: the component has a cell next to an empty one (its matrix is regular)
  bool mg_closed = false;              // ... read back at set-up: the component at hand is closed, its cycle runs on r minus its mean
  long long iterations = 0;            // the sum over the component solves of the iteration counter at exit
  // launch sizes: per cell, per hyperplane, per interior cell; the hyperplanes h = i + j + k of the interior
  int gcell, gwave, ginner = 0, hmin, hmax;
  // the item and the component at hand
  int b = 0, cidx = 0, root = 0, size = 0, pc = 0;
  const float *fl = nullptr, *dv = nullptr;
  float* pb = nullptr;
  float max_res = -std::numeric_limits<float>::infinity();

  Solve(hipStream_t st, const PcgProblem& q, float* workspace, char* msg, size_t msg_len, bool allow_wavefronts);
  ~Solve() { if (wf_trace) (void)hipFree(wf_trace); }      // every exit frees it
  PcgResult item(int b);
  PcgResult read_components(int h_cnt[3], std::vector<int>& h_roots, std::vector<int>& h_sizes);
  PcgResult component(int cidx, int root, int size);
  void begin();
  void factor();
  PcgResult build_wavefront_operands();
  PcgResult build_levels();
  void vcycle();
  template <bool IS3D, bool IC> void hyperplane_sweeps();
  void precondition();
  void iteration();
  PcgResult wavefront_error();
  PcgResult run_chunks();
  void write_back();
  void print_trace();
};

Solve::Solve(hipStream_t st_, const PcgProblem& q_, float* workspace, char* msg, size_t msg_len, bool allow_wavefronts)
    : st(st_), q(q_), er{"solveLinearSystemPCG", msg, msg_len}, d(whole_dom(q_.Z, q_.Y, q_.X)), n(d.sc) {
  mg = q.precond == 3;
  wf = !mg && allow_wavefronts && wf_usable(q.is3d, q.Z, q.Y, q.X);
  const PcgWs t = pcg_ws(q.Z, q.Y, q.X, wf, mg, q.is3d);
  partials = view<double>(workspace, t.partials); p_den = view<double>(workspace, t.p_den); p_rr = view<double>(workspace, t.p_rr);
  S = view<PcgState>(workspace, t.state);
  label = view<int>(workspace, t.label); size_at = view<int>(workspace, t.size_at);
  x = view<float>(workspace, t.x); r = view<float>(workspace, t.r); z = view<float>(workspace, t.z); s = view<float>(workspace, t.s);
  w = view<float>(workspace, t.w); dg = view<float>(workspace, t.dg); y = view<float>(workspace, t.y);
  roots = view<int>(workspace, t.roots); counters = view<int>(workspace, t.counters);
  wg = t.geom;
  if (wf) {
    float* wfb = workspace + pcg_wf_pad(workspace, t);      // 16-byte aligned (float4 rows, {value, tag} pairs)
    cs = view<float>(wfb, t.wf_cc); rsk = view<float>(wfb, t.wf_r); qsk = view<float>(wfb, t.wf_q); zsk = view<float>(wfb, t.wf_z);
    wf_hk = view<float2>(wfb, t.wf_hk) + kWfGuard; wf_hs = view<float2>(wfb, t.wf_hs) + kWfGuard;
    wferr = view<int>(wfb, t.wf_err);
    wf_clear_bytes = sizeof(float) * (size_t)t.wf_clear.floats;
    // every sub-box of a launch must be resident (they wait for each other): at most wf_cap of them per launch
    const int wf_cap = sw::present(Sw::WF_MAX_BLOCKS) ? std::max(1, sw::num(Sw::WF_MAX_BLOCKS, 0)) : kWfMaxBlocks;     // (tests: small launches)
    wf_slabs = std::max(1, std::min(wf_cap, kWfMaxBlocks) / std::max(wg.ns, 1));
    ginner = cdiv((long long)(q.X - 2) * (q.Y - 2) * (q.Z - 2), 256);
    // development aid: TFL_WF_TRACE=1 prints when every sub-box of the last forward / backward sweep started and finished
    if (sw::present(Sw::WF_TRACE) && q.precond && hipMalloc(&wf_trace, sizeof(long long) * 4 * wg.ns * wg.nb) != hipSuccess) wf_trace = nullptr;
  }
  if (mg) {
    const MgLevels ml = mg_levels(q.Z, q.Y, q.X, q.is3d);
    mgd.count = ml.count; mgd.first_block_level = ml.first_block_level;
    // level 0: z is the CG's, diag lives in dg, the second iterate in y and the cycle's right-hand side in w (all idle under mg,
    // w while the preconditioner runs)
    mgd.lv[0] = MgLv{ml.lv[0], (int)ml.lv[0].n, dg, view<float>(workspace, t.mg_invd0), view<float>(workspace, t.mg_cx0),
                     view<float>(workspace, t.mg_cy0), view<float>(workspace, t.mg_cz0), w, y, z};
    mg_open = counters + kPcgMgOpenWord;
    for (int l = 1; l < ml.count; l++) {
      const long long o = ml.lv[l].off;
      mgd.lv[l] = MgLv{ml.lv[l], (int)ml.lv[l].n, view<float>(workspace, t.mg_c_diag) + o, view<float>(workspace, t.mg_c_invd) + o,
                       view<float>(workspace, t.mg_c_cx) + o, view<float>(workspace, t.mg_c_cy) + o, view<float>(workspace, t.mg_c_cz) + o,
                       view<float>(workspace, t.mg_c_r) + o, view<float>(workspace, t.mg_c_za) + o, view<float>(workspace, t.mg_c_zb) + o};
    }
  }
  gcell = cdiv(n, 256);
  gwave = cdiv((long long)(q.Y - 2) * (q.is3d ? q.Z - 2 : 1), 256);
  hmin = q.is3d ? 3 : 2; hmax = (q.X - 2) + (q.Y - 2) + (q.is3d ? q.Z - 2 : 0);
}

// one batch element: its components, then one CG solve per component
PcgResult Solve::item(int b_) {
  b = b_;
  fl = q.flags + (long long)b * n; dv = q.div + (long long)b * n; pb = q.p + (long long)b * n;
  int h_cnt[3] = {0, 0, 0};
  PCG_TRY(clear_component_counts(st, er, counters, size_at, n));
  PCG_TRY(label_components(st, er, d, q.is3d, fl, label, counters, h_cnt, true));
  if (h_cnt[2] > 0) {   // generic/tfluids.cu:1083-1091 raises for a fluid cell on the border
    snprintf(er.msg, er.len, "solveLinearSystemPCG: Non fluid cell found in a connected component or fluid cell found on the "
             "domain border (%d fluid border cells)", h_cnt[2]);
    return PcgResult::bad_flags;
  }
  std::vector<int> h_roots, h_sizes;
  PCG_TRY(read_components(h_cnt, h_roots, h_sizes));
  for (size_t c = 0; c < h_roots.size(); c++) PCG_TRY(component((int)c, h_roots[c], h_sizes[c]));
  return PcgResult::ok;
}

// the components' count, their roots in scan order of the first cell (= the reference's numbering) and their sizes
PcgResult Solve::read_components(int h_cnt[3], std::vector<int>& h_roots, std::vector<int>& h_sizes) {
  { TFL_TIMED("k_cc", st); k_cc_count<<<gcell, 256, 0, st>>>(d, label, size_at, roots, counters + 1); }
  HIP_TRY(hipMemcpyAsync(h_cnt, counters, 3 * sizeof(int), hipMemcpyDeviceToHost, st), "memcpy");
  HIP_TRY(hipStreamSynchronize(st), "sync");
  const int ncomp = h_cnt[1];
  if (ncomp > kMaxComponents) {
    snprintf(er.msg, er.len, "solveLinearSystemPCG: %d fluid components (the solver handles %d)", ncomp, kMaxComponents);
    return PcgResult::too_many_components;
  }
  h_roots.resize(ncomp); h_sizes.resize(ncomp);
  if (!ncomp) return PcgResult::ok;
  HIP_TRY(hipMemcpy(h_roots.data(), roots, sizeof(int) * ncomp, hipMemcpyDeviceToHost), "memcpy roots");
  std::sort(h_roots.begin(), h_roots.end());
  for (int c = 0; c < ncomp; c++)
    HIP_TRY(hipMemcpy(&h_sizes[c], size_at + h_roots[c], sizeof(int), hipMemcpyDeviceToHost), "memcpy size");
  return PcgResult::ok;
}

PcgResult Solve::component(int cidx_, int root_, int size_) {
  cidx = cidx_; root = root_; size = size_;
  if (size == 1) {   // :1375-1383: no valid solution, pressure stays 0
    if (q.verbose) printf("PCG batch %d component %d has size 1, skipping.\n", b + 1, cidx + 1);
    return PcgResult::ok;
  }
  pc = q.precond;
  if (size < 5) pc = 0;   // :1390-1393
  if (q.verbose) printf("PCG batch %d component %d has size %d.\nPCG: %d component %d using precond type %s\n", b + 1, cidx + 1,
                        size, b + 1, cidx + 1, pc == 0 ? "none" : (pc == 1 ? "ilu0" : (pc == 2 ? "ic0" : "mg")));
  // z is only ever written on the component; its other cells must read as 0 in s = z and r.z
  if (pc) HIP_TRY(hipMemsetAsync(z, 0, sizeof(float) * (size_t)n, st), "memset z");
  begin();
  if (pc) {
    TFL_TIMED("k_pcg_precond", st);
    if (pc == 3) PCG_TRY(build_levels());
    else factor();
    if (wf) PCG_TRY(build_wavefront_operands());
  }
  PCG_TRY(run_chunks());
  write_back();
  return PcgResult::ok;
}

void Solve::begin() {
  TFL_TIMED("k_pcg", st);
  k_pcg_setup<<<kRedBlocks, 256, 0, st>>>(n, label, root, dv, x, r, s, partials);
  k_pcg_begin<<<1, 256, 0, st>>>(S, partials, q.tol, q.max_iter);
}

// the diagonal of ILU(0) / IC(0): one launch per hyperplane
void Solve::factor() {
  for (int h = hmin; h <= hmax; h++) {
    if (q.is3d) k_ilu_factor<true><<<gwave, 256, 0, st>>>(d, h, fl, label, root, dg);
    else k_ilu_factor<false><<<gwave, 256, 0, st>>>(d, h, fl, label, root, dg);
  }
}

// the skewed arrays and both hand-off arrays zeroed (with them the tags: epoch starts over), cc from the factor's diagonal
PcgResult Solve::build_wavefront_operands() {
  HIP_TRY(hipMemsetAsync(cs, 0, wf_clear_bytes, st), "memset skewed arrays");
  epoch = 0;
  if (pc == 2) k_wf_build<true><<<ginner, 256, 0, st>>>(wg, d, label, root, dg, cs);
  else k_wf_build<false><<<ginner, 256, 0, st>>>(wg, d, label, root, dg, cs);
  return PcgResult::ok;
}

// the multigrid hierarchy of the component: level 0 from the flags and the label, then one launch per coarser level
// (one word read back: whether the component is closed decides what the cycle launches)
PcgResult Solve::build_levels() {
  mg_build_levels(st, d, q.is3d, mgd, fl, label, root, mg_open);
  int h_open = 0;
  HIP_TRY(hipMemcpyAsync(&h_open, mg_open, sizeof(int), hipMemcpyDeviceToHost, st), "memcpy");
  HIP_TRY(hipStreamSynchronize(st), "sync");
  mg_closed = h_open == 0;
  mgd.lv[0].r = mg_closed ? w : r;     // closed: the right-hand side of the cycle is formed in the idle w
  return PcgResult::ok;
}

// z = M^-1 r, one V-cycle
void Solve::vcycle() { mg_vcycle(st, q.is3d, mgd, S, mg_closed, r, partials, size); }

// M^-1 r with one launch per hyperplane and sweep
template <bool IS3D, bool IC>
void Solve::hyperplane_sweeps() {
  for (int h = hmin; h <= hmax; h++) k_ilu_forward<IS3D, IC><<<gwave, 256, 0, st>>>(S, d, h, fl, label, root, dg, r, y);
  for (int h = hmax; h >= hmin; h--) k_ilu_backward<IS3D, IC><<<gwave, 256, 0, st>>>(S, d, h, fl, label, root, dg, y, z);
}

// z = M^-1 r
void Solve::precondition() {
  TFL_TIMED("k_pcg_precond", st);
  if (pc == 3) { vcycle(); return; }
  if (!wf) {
    if (q.is3d) { if (pc == 2) hyperplane_sweeps<true, true>(); else hyperplane_sweeps<true, false>(); }
    else { if (pc == 2) hyperplane_sweeps<false, true>(); else hyperplane_sweeps<false, false>(); }
    return;
  }
  // as two launches (pipelined wavefronts)
  const int nblk = wg.ns * wg.nb;
  k_wf_skew<true><<<ginner, 256, 0, st>>>(S, wg, d, r, rsk);
  // every sub-box of a launch must be resident (they wait for each other): at most wf_cap of them per launch,
  // all strips of a range of slabs, the ranges in sweep order -- a later launch finds its predecessors' pairs
  // waiting under the same tag
  ++epoch;
  for (int b0 = 0; b0 < wg.nb; b0 += wf_slabs) {
    WfGeom c = wg; c.b_lo = b0; c.b_cnt = std::min(wf_slabs, wg.nb - b0);
    k_wf_sweep<1><<<wg.ns * c.b_cnt, (kWfPlanes + 2) * 64, 0, st>>>(S, c, WfArrays{cs, rsk, qsk, wf_hk, wf_hs, wferr, wf_trace}, epoch);
  }
  ++epoch;
  for (int b1 = wg.nb; b1 > 0; b1 -= wf_slabs) {
    WfGeom c = wg; c.b_lo = std::max(b1 - wf_slabs, 0); c.b_cnt = b1 - c.b_lo;
    k_wf_sweep<-1><<<wg.ns * c.b_cnt, (kWfPlanes + 2) * 64, 0, st>>>(S, c, WfArrays{cs, qsk, zsk, wf_hk, wf_hs, wferr, wf_trace ? wf_trace + 2 * nblk : nullptr}, epoch);
  }
  k_wf_skew<false><<<ginner, 256, 0, st>>>(S, wg, d, z, zsk);
}

// one CG iteration, enqueued: every kernel returns at once when the state says `done`
void Solve::iteration() {
  k_pcg_top<<<1, 256, 0, st>>>(S, p_rr, 1);
  if (pc) precondition();
  TFL_TIMED("k_pcg", st);
  if (pc) k_pcg_dot<<<kRedBlocks, 256, 0, st>>>(S, n, r, z, partials);
  k_pcg_dir<<<kRedBlocks, 256, 0, st>>>(S, n, partials, pc ? 1 : 0, pc ? z : r, s);
  if (q.is3d) k_pcg_apply<true><<<kRedBlocks, 256, 0, st>>>(S, d, fl, label, root, s, w, p_den);
  else k_pcg_apply<false><<<kRedBlocks, 256, 0, st>>>(S, d, fl, label, root, s, w, p_den);
  k_pcg_update<<<kRedBlocks, 256, 0, st>>>(S, n, p_den, s, w, x, r, p_rr);
}

// the error word of the pipelined sweeps, read after a chunk
PcgResult Solve::wavefront_error() {
  int e = 0;
  HIP_TRY(hipMemcpy(&e, wferr, sizeof(int), hipMemcpyDeviceToHost), "memcpy");
  if (sw::present(Sw::WF_TEST_TIMEOUT)) e = 1;     // tests: exercise the caller's fallback
  // (its sub-boxes wait for each other, so all of them must be resident at once: not the case when something else holds
  // part of the GPU. The caller repeats the solve with one launch per hyperplane.)
  if (!e) return PcgResult::ok;
  snprintf(er.msg, er.len, "solveLinearSystemPCG: a block of the pipelined triangular solve never saw its predecessor");
  return PcgResult::wavefront_timeout;
}

// the iterations of one component: a chunk enqueued, then the state read back
PcgResult Solve::run_chunks() {
  PcgState hs;
  const int chunk = q.verbose ? 1 : (pc ? (wf ? 16 : (pc == 3 ? 8 : 4)) : 32);
  for (;;) {
    for (int it = 0; it < chunk; it++) iteration();
    { TFL_TIMED("k_pcg", st); k_pcg_top<<<1, 256, 0, st>>>(S, p_rr, 0); }     // fold the last update's residual for the host
    HIP_TRY(hipMemcpyAsync(&hs, S, sizeof(PcgState), hipMemcpyDeviceToHost, st), "memcpy state");
    HIP_TRY(hipStreamSynchronize(st), "sync");
    if (q.verbose && !hs.done)
      printf("PCG batch %d comp %d iter %d: residual %g (tol %g)\n", b + 1, cidx + 1, hs.iter, std::sqrt(hs.rr1), (double)q.tol);
    if (wf && pc) PCG_TRY(wavefront_error());
    if (hs.bad) { snprintf(er.msg, er.len, "solveLinearSystemPCG: ERROR: r_norm_sq1 is nan!"); return PcgResult::nan_residual; }
    // the loop ends when the NEXT top-of-loop test fails
    if (hs.done || !((float)hs.rr1 > q.tol * q.tol) || hs.iter > q.max_iter) break;
  }
  max_res = std::max(max_res, (float)std::sqrt((float)hs.rr1));
  iterations += hs.iter;
  return PcgResult::ok;
}

// p = x - mean of x on the component
void Solve::write_back() {
  TFL_TIMED("k_pcg", st);
  k_pcg_sum<<<kRedBlocks, 256, 0, st>>>(n, x, partials);
  k_pcg_sum_end<<<1, 256, 0, st>>>(S, partials);
  k_pcg_write<<<kRedBlocks, 256, 0, st>>>(S, n, label, root, size, x, pb);
}

void Solve::print_trace() {
  if (!wf_trace) return;
  const int nblk = wg.ns * wg.nb;
  std::vector<long long> t(4 * nblk);
  if (hipMemcpy(t.data(), wf_trace, sizeof(long long) * 4 * nblk, hipMemcpyDeviceToHost) != hipSuccess) return;
  long long t0 = t[0];
  for (int i = 0; i < 4 * nblk; i++) if (t[i] && t[i] < t0) t0 = t[i];
  for (int dir = 0; dir < 2; dir++)
    for (int b2 = 0; b2 < nblk; b2++)
      fprintf(stderr, "[tfl] wf %s strip %d slab %2d: start %8.2f us  end %8.2f us\n", dir ? "bwd" : "fwd", b2 / wg.nb, b2 % wg.nb,
              (t[dir * 2 * nblk + 2 * b2] - t0) * 0.01, (t[dir * 2 * nblk + 2 * b2 + 1] - t0) * 0.01);
}

#include "pcg_batched.inc"      // solveLinearSystemPCGBatched: the kernels above with the batch item in blockIdx.y, and its host code

}  // namespace

long long pcg_workspace_floats(int Z, int Y, int X) { return pcg_ws(Z, Y, X, wf_usable(Z > 1, Z, Y, X)).total; }
long long pcg_workspace_floats_for(int Z, int Y, int X, int precond) {
  if (precond >= 0 && precond <= 2) return pcg_workspace_floats(Z, Y, X);
  return precond == 3 ? pcg_ws(Z, Y, X, false, true, Z > 1).total : -1;
}

// Solves every component of every batch element. Anything but PcgResult::ok comes with `msg` filled; wavefront_timeout (the
// pipelined triangular solves timed out) only with allow_wavefronts: repeat without.
PcgResult pcg_solve(hipStream_t st, const PcgProblem& q, float* workspace, float* residual, char* msg, size_t msg_len,
                    bool allow_wavefronts, long long* iterations) {
  Solve v(st, q, workspace, msg, msg_len, allow_wavefronts);
  const Report& er = v.er;
  HIP_TRY(hipMemsetAsync(q.p, 0, sizeof(float) * (size_t)q.B * v.n, st), "memset p");   // :1341
  for (int b = 0; b < q.B; b++) PCG_TRY(v.item(b));
  v.print_trace();
  if (residual) *residual = v.max_res;
  if (iterations) *iterations = v.iterations;
  return PcgResult::ok;
}

long long pcg_batched_workspace_floats(int B, int Z, int Y, int X, int precond) {
  return (precond == 0 || precond == 3) ? pcg_batched_ws(B, Z, Y, X, precond == 3, Z > 1).total : -1;
}

// Every item's systems in the same launches, round by round (pcg_batched.inc). Anything but PcgResult::ok comes with `msg` filled.
PcgResult pcg_solve_batched(hipStream_t st, const PcgProblem& q, float* workspace, float* residuals, long long* iterations,
                            long long* total, char* msg, size_t msg_len) {
  BatchedSolve v(st, q, workspace, msg, msg_len);
  const Report& er = v.er;
  HIP_TRY(hipMemsetAsync(q.p, 0, sizeof(float) * (size_t)q.B * v.n, st), "memset p");   // :1341
  PCG_TRY(v.label_items());
  PCG_TRY(v.read_components());
  for (int c = 0; c < v.maxc; c++) PCG_TRY(v.round(c));
  long long sum = 0;
  for (int b = 0; b < q.B; b++) {
    if (residuals) residuals[b] = v.max_res[b];
    if (iterations) iterations[b] = v.iters[b];
    sum += v.iters[b];
  }
  if (total) *total = sum;
  return PcgResult::ok;
}

long long npm_workspace_floats(int Z, int Y, int X) { return npm_ws(Z, Y, X).total; }

// normalizePressureMean for every batch element.
PcgResult normalize_pressure_mean(hipStream_t st, bool is3d, int B, int Z, int Y, int X, float* p, const float* flags,
                                  float* workspace, char* msg, size_t msg_len) {
  const Dom d = whole_dom(Z, Y, X);
  const long long n = d.sc;
  const NpmWs t = npm_ws(Z, Y, X);
  double* sum_at = view<double>(workspace, t.sum_at);
  int* label = view<int>(workspace, t.label);
  int* size_at = view<int>(workspace, t.size_at);
  int* counters = view<int>(workspace, t.counters);
  const Report er{"normalizePressureMean", msg, msg_len};
  const int gcell = cdiv(n, 256);
  for (int b = 0; b < B; b++) {
    const float* fl = flags + (long long)b * n;
    float* pb = p + (long long)b * n;
    int h_cnt[3] = {0, 0, 0};
    PCG_TRY(clear_component_counts(st, er, counters, size_at, n));
    HIP_TRY(hipMemsetAsync(sum_at, 0, sizeof(double) * (size_t)n, st), "memset");
    TFL_TIMED("k_cc", st);
    PCG_TRY(label_components(st, er, d, is3d, fl, label, counters, h_cnt, false));
    // sizes only (the roots list is not needed: means are looked up through the label)
    k_cc_count<<<gcell, 256, 0, st>>>(d, label, size_at, view<int>(workspace, t.roots), counters + 1);
    k_npm_sum<<<gcell, 256, 0, st>>>(d, label, pb, sum_at);
    k_npm_sub<<<gcell, 256, 0, st>>>(d, label, size_at, sum_at, pb);
  }
  return PcgResult::ok;
}

}  // namespace tfl
