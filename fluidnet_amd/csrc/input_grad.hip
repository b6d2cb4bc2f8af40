// input_grad.hip -- the gradients of the projection ConvNet to its inputs pDiv and UDiv (tfl_model_backward_input, gfx950):
// what lies between the first layer's data gradient and the two tensors the caller gets. DESIGN.md 3.16 derives it; in short,
// per batch item with its input scale s, q = 1 / s:
//
//   forward   U_bc = keep (.) UDiv, d = D(U_bc), x = {q pDiv, q U_bc, q d, occupancy}, pPred = net(x; skip = q pDiv),
//             UPred = VU(q U_bc, pPred), p = s pPred, U = keep (.) s UPred;  s = std | l2 norm of U_bc | pDiv | d, or 1
//   given     g_x (the first layer's data gradient), g_skip (the joined skip channel's), h = s keep (.) gradU
//   g_a       = h where the velocity update keeps its velocity input, 0 where it overwrites it (empty, not outflow, interior
//               cells whose minus-neighbour is not fluid)
//   g_s       = sum gradP pPred + q sum gradU U - q [sum (g_x[p] + g_skip) q pDiv + sum (g_x[U] + g_a) q U_bc + sum g_x[d] q d]
//   gradPDiv  = q (g_x[p] + g_skip) [+ g_s ds/dpDiv]
//   g_d       = q g_x[d] [+ g_s ds/dd];   gradUDiv = keep (.) (q (g_x[U] + g_a) + D^T(g_d) [+ g_s ds/dU_bc])
//   ds/dsrc   = (src - mean) / ((n - 1) s) for std, src / s for the l2 norm
//
// k_input_grad_sums forms the five dot products of g_s in one pass over an item's cells -- fp32 products, fp64 sums, a wave64
// shuffle reduction, then LDS across the block's four waves in wave order -- and leaves one fp64 partial per (item, block, term)
// at a fixed place; k_input_grad_sums_finish adds the blocks in a fixed order and leaves g_s per item on the device. No atomics: the
// same inputs give the same bits. k_input_grad_head is the rest as one gather per cell: D is a one-sided difference, so D^T reads
// g_d at the cell and at its three minus-neighbours. keep, the divergence mask and the velocity update's cases are decoded by
// the helpers every other kernel uses (tfl_device.hpp wall_zero_mask, on_border).
#include "tfl_device.hpp"
#include "tfl_host.hpp"
#include "tfl_input_grad.hpp"

namespace tfl {
namespace {

// (model.hip scale_from_stats, restated as in conv_bwd.hip: the input scale of batch item b from its pair on the tape)
__device__ __forceinline__ float ig_scale(const double* __restrict__ stats, int b, double n) {
  const double s1 = stats[b * 2], s2 = stats[b * 2 + 1];
  return (float)sqrt(fmax(n * s2 - s1 * s1, 0.0) / (n * (n - 1.0)));
}

// What a cell's flags decide: z[c] = setWallBcs zeroes component c (keep = !z); over[c] = velocityUpdateForward overwrites
// component c instead of updating it (k_project's second branch with a non-fluid minus-neighbour); fc / fn = the cell's word and
// its minus-neighbours' (0 outside the grid).
template <bool IS3D>
struct CellFacts { bool z[3], over[3]; int fc, fn[3]; };
template <bool IS3D>
__device__ __forceinline__ CellFacts<IS3D> cell_facts(const Dom& d, const float* __restrict__ flags, int i, int j, int k, int o) {
  CellFacts<IS3D> f;
  wall_zero_mask<IS3D>(d, flags, i, j, k, o, f.z[0], f.z[1], f.z[2]);
  f.fc = (int)flags[o];
  f.fn[0] = i > 0 ? (int)flags[o - 1] : 0;
  f.fn[1] = j > 0 ? (int)flags[o - d.sy] : 0;
  f.fn[2] = (IS3D && k > 0) ? (int)flags[o - d.sz] : 0;
  const bool sets = !on_border<IS3D>(d, i, j, k) && !(f.fc & kFluid) && (f.fc & kEmpty) && !(f.fc & kOutflow);
#pragma unroll
  for (int c = 0; c < 3; c++) f.over[c] = sets && !(f.fn[c] & kFluid);
  return f;
}

}  // namespace

template <bool IS3D>
__global__ __launch_bounds__(kIgSumThreads) void k_input_grad_sums(Dom d, IgArgs a) {
  const int b = blockIdx.y, tid = threadIdx.x;
  const int C = IS3D ? 3 : 2;
  const long long cells = d.sc;
  const float q = 1.0f / ig_scale(a.stats, b, a.count);
  const float* flags = a.flags + b * cells;
  const float* pDiv = a.pDiv + b * cells;
  const float* UDiv = a.UDiv + b * cells * C;
  const float* UOut = a.UOut + b * cells * C;
  const float* gradP = a.gradP ? a.gradP + b * cells : nullptr;
  const float* gradU = a.gradU ? a.gradU + b * cells * C : nullptr;
  const float* h = a.h ? a.h + b * cells * C : nullptr;
  const float* gx = a.gx + b * cells * a.gxc;
  const float* gskip = a.gskip ? a.gskip + b * cells : nullptr;
  const float* x = a.x + b * cells * a.in_c;
  const float* pPred = a.pPred + b * cells;
  double acc[kIgTerms];
#pragma unroll
  for (int t = 0; t < kIgTerms; t++) acc[t] = 0.0;
  for (long long t = (long long)blockIdx.x * kIgSumThreads + tid; t < cells; t += (long long)gridDim.x * kIgSumThreads) {
    const int o = (int)t;
    const int i = o % d.X, j = (o / d.X) % d.Y, k = o / d.sz;
    if (gradP) acc[kIgP] += (double)(gradP[o] * pPred[o]);
    if (gradU) {
#pragma unroll
      for (int c = 0; c < C; c++) acc[kIgU] += (double)(gradU[o + c * d.sc] * UOut[o + c * d.sc]);
    }
    if (a.pch >= 0 || gskip) {
      float g = a.pch >= 0 ? gx[o + a.pch * d.sc] : 0.0f;
      if (gskip) g += gskip[o];
      acc[kIgQp] += (double)(g * (q * pDiv[o]));
    }
    if (a.uch >= 0 || h) {
      const CellFacts<IS3D> f = cell_facts<IS3D>(d, flags, i, j, k, o);
#pragma unroll
      for (int c = 0; c < C; c++) {
        if (f.z[c]) continue;          // q U_bc is zero there
        float g = a.uch >= 0 ? gx[o + (a.uch + c) * d.sc] : 0.0f;
        if (h && !f.over[c]) g += h[o + c * d.sc];
        acc[kIgQu] += (double)(g * (q * UDiv[o + c * d.sc]));
      }
    }
    if (a.dch >= 0) acc[kIgQd] += (double)(gx[o + a.dch * d.sc] * x[o + a.dch * d.sc]);
  }
  // the wave's 64 lanes, then the block's waves in wave order
#pragma unroll
  for (int t = 0; t < kIgTerms; t++)
    for (int off = 32; off > 0; off >>= 1) acc[t] += __shfl_down(acc[t], off, 64);
  __shared__ double sh[kIgSumThreads / 64][kIgTerms];
  if ((tid & 63) == 0) {
#pragma unroll
    for (int t = 0; t < kIgTerms; t++) sh[tid >> 6][t] = acc[t];
  }
  __syncthreads();
  if (tid < kIgTerms) {
    double s = sh[0][tid];
    for (int w = 1; w < kIgSumThreads / 64; w++) s += sh[w][tid];
    a.partials[ig_partial_slot(b, (int)gridDim.x, (int)blockIdx.x, tid)] = s;
  }
}

// g_s[b] = T_p + q T_U - q (T_qp + T_qU + T_qd). Thread (lane, t) adds term t's partials of the blocks lane, lane + 64, ... in
// ascending order; lane 0 then adds the 64 lanes in lane order: a fixed order whatever the block count.
__global__ __launch_bounds__(kIgFinishLanes * kIgTerms) void k_input_grad_sums_finish(const double* __restrict__ partials, int blocks,
                                                                                     const double* __restrict__ stats, double count,
                                                                                     double* __restrict__ gs) {
  __shared__ double sh[kIgTerms][kIgFinishLanes];
  __shared__ double T[kIgTerms];
  const int b = blockIdx.x, lane = threadIdx.x, t = threadIdx.y;
  double s = 0.0;
  for (int blk = lane; blk < blocks; blk += kIgFinishLanes) s += partials[ig_partial_slot(b, blocks, blk, t)];
  sh[t][lane] = s;
  __syncthreads();
  if (lane == 0) {
    for (int q = 1; q < kIgFinishLanes; q++) s += sh[t][q];
    T[t] = s;
  }
  __syncthreads();
  if (lane != 0 || t != 0) return;
  const double q = 1.0 / (double)ig_scale(stats, b, count);
  gs[b] = T[kIgP] + q * T[kIgU] - q * ((T[kIgQp] + T[kIgQu]) + T[kIgQd]);
}

template <bool IS3D>
__global__ __launch_bounds__(256) void k_input_grad_head(Dom d, IgArgs a) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const int j = blockIdx.y * blockDim.y + threadIdx.y;
  int b, k; dom_bk(d, b, k);
  if (i >= d.X || j >= d.Y) return;
  const int C = IS3D ? 3 : 2;
  const long long cells = d.sc;
  const float s = ig_scale(a.stats, b, a.count), q = 1.0f / s;
  // the scale's derivative at its source: g_s ds/dsrc = gsc (src - mean)
  float gsc = 0.0f, mean = 0.0f;
  if (a.nmode == 1) {
    mean = (float)(a.stats[b * 2] / a.count);
    gsc = (float)(a.gs[b] / ((a.count - 1.0) * (double)s));
  } else if (a.nmode == 2) {
    gsc = (float)(a.gs[b] / (double)s);
  }
  const float* flags = a.flags + b * cells;
  const float* gx = a.gx + b * cells * a.gxc;
  const int o = TFL_AT(d, i, j, k);
  if (a.gradPDiv) {
    float g = a.pch >= 0 ? gx[o + a.pch * d.sc] : 0.0f;
    if (a.gskip) g += a.gskip[b * cells + o];
    float v = q * g;
    if (a.nmode && a.nchan == 1) v += gsc * (a.pDiv[b * cells + o] - mean);
    a.gradPDiv[b * cells + o] = v;
  }
  if (!a.gradUDiv) return;
  const CellFacts<IS3D> f = cell_facts<IS3D>(d, flags, i, j, k, o);
  const bool div_norm = a.nmode && a.nchan == 2;
  const bool has_d = a.dch >= 0 || div_norm;
  const float* dsrc = div_norm ? a.dsrc + b * a.dstride : nullptr;
  // g_d of cell (ii, jj, kk) with the divergence's own mask folded in: zero outside the interior fluid cells
  auto gd = [&](int ii, int jj, int kk, int oo, int fw) -> float {
    if (on_border<IS3D>(d, ii, jj, kk) || !(fw & kFluid)) return 0.0f;
    float v = a.dch >= 0 ? q * gx[oo + a.dch * d.sc] : 0.0f;
    if (div_norm) v += gsc * ((a.dscaled ? dsrc[oo] * s : dsrc[oo]) - mean);
    return v;
  };
  const float g0 = has_d ? gd(i, j, k, o, f.fc) : 0.0f;
  const float* UDiv = a.UDiv + b * cells * C;
  const float* h = a.h ? a.h + b * cells * C : nullptr;
  float* out = a.gradUDiv + b * cells * C;
  const int st[3] = {1, d.sy, d.sz};
#pragma unroll
  for (int c = 0; c < C; c++) {
    float v = 0.0f;
    if (!f.z[c]) {
      float g = a.uch >= 0 ? gx[o + (a.uch + c) * d.sc] : 0.0f;
      if (h && !f.over[c]) g += h[o + c * d.sc];
      v = q * g;
      if (has_d) {
        // D^T: div(n) = sum_c U_c(n) - U_c(n + 1_c), so U_c(n) collects g_d(n) - g_d(n - 1_c)
        const bool nb = c == 0 ? i > 0 : (c == 1 ? j > 0 : k > 0);
        const float gm = nb ? gd(i - (c == 0), j - (c == 1), k - (c == 2), o - st[c], f.fn[c]) : 0.0f;
        v += g0 - gm;
      }
      if (a.nmode && a.nchan == 0) v += gsc * (UDiv[o + c * d.sc] - mean);
    }
    out[o + c * d.sc] = v;
  }
}

void input_grad_sums(hipStream_t st, bool is3d, int B, int Z, int Y, int X, const IgArgs& a) {
  const Dom d = whole_dom(Z, Y, X);
  {
    TFL_TIMED("k_input_grad_sums", st);
    const dim3 grd((unsigned)a.blocks, (unsigned)B);
    if (is3d) k_input_grad_sums<true><<<grd, kIgSumThreads, 0, st>>>(d, a);
    else k_input_grad_sums<false><<<grd, kIgSumThreads, 0, st>>>(d, a);
  }
  TFL_TIMED("k_input_grad_sums_finish", st);
  k_input_grad_sums_finish<<<B, dim3(kIgFinishLanes, kIgTerms), 0, st>>>(a.partials, a.blocks, a.stats, a.count, a.gs);
}

void input_grad_head(hipStream_t st, bool is3d, int B, int Z, int Y, int X, const IgArgs& a) {
  const Dom d = whole_dom(Z, Y, X);
  const dim3 blk(64, 4, 1), grd((X + 63) / 64, (Y + 3) / 4, (unsigned)(d.nw * B));
  TFL_TIMED("k_input_grad_head", st);
  if (is3d) k_input_grad_head<true><<<grd, blk, 0, st>>>(d, a);
  else k_input_grad_head<false><<<grd, blk, 0, st>>>(d, a);
}

}  // namespace tfl
