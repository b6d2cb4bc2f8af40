// multires_bwd.hip -- the backward of the two resolution-changing operations of a linear model with pooling / upsampling layers
// (the `tog` topologies), gfx950. The weight gradient of an upsample layer is conv_bwd.hip's k_conv_wgrad with a
// strided read of g; here are
//
//   k_pool_bwd_mask   the backward of 2x average pooling fused with the activation mask of the layer that pools:
//                     g_pre[b][c][fine] = act'(y[b][c][fine]) g_pooled[b][c][fine >> 1] / 2^dim -- one pass, no un-pooled array in
//                     between and no act_mask launch; what it writes feeds the layer's weight gradient and its data gradient
//   k_up_dgrad        the data gradient of an upsample layer, g_in = sum over the up^dim sub-positions of conv^T(g_sub, W_sub) at
//                     the layer's input resolution: one launch, the sub-positions as the outermost part of one thread's fmaf
//                     chain (sub, tap, channel: a fixed order), g read where the shuffle put it
//
// No atomics; every output element is written once by one thread: the same inputs give the same bits on every call.
#include "tfl_device.hpp"
#include "tfl_host.hpp"
#include "tfl_train.hpp"

namespace tfl {
namespace {

// act'(y) from the saved output (conv_bwd.hip act_grad): ReLU y > 0, ReLU6 0 < y < 6, sigmoid y (1 - y)
__device__ __forceinline__ float mr_act_grad(float g, float y, int act) {
  if (act == 1) return y > 0.0f ? g : 0.0f;
  if (act == 2) return (y > 0.0f && y < 6.0f) ? g : 0.0f;
  return g * (y * (1.0f - y));
}

template <int V> struct VecOf;
template <> struct VecOf<4> { using T = float4; };
template <> struct VecOf<2> { using T = float2; };
template <> struct VecOf<1> { using T = float; };

// blockIdx.y = plane (b, c); a thread owns V consecutive x-cells of one fine row [Z][Y][X]: V = 4, two coarse cells and one
// 16-byte load and store (X a multiple of 4 and the buffers 16-byte aligned), else V = 2 (one coarse cell, 8 bytes) or V = 1.
template <bool IS3D, int V>
__global__ __launch_bounds__(256) void k_pool_bwd_mask(int Z, int Y, int X, const float* __restrict__ y, const float* __restrict__ gc,
                                                       float* __restrict__ dst, int act) {
  using T = typename VecOf<V>::T;
  const int Xv = X / V;
  const long long n = (long long)Z * Y * Xv, t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t >= n) return;
  const int xv = (int)(t % Xv), yy = (int)((t / Xv) % Y), z = (int)(t / ((long long)Xv * Y));
  const long long cells = (long long)Z * Y * X, ccells = cells >> (IS3D ? 3 : 2);
  const float* __restrict__ gp = gc + (long long)blockIdx.y * ccells + pyr_bwd_parent(IS3D, z, yy, xv * V, Y, X);
  const long long o = (long long)blockIdx.y * cells + ((long long)z * Y + yy) * X + (long long)xv * V;
  const float sc = IS3D ? 0.125f : 0.25f;
  T yv = *reinterpret_cast<const T*>(y + o), out;
  const float* yf = reinterpret_cast<const float*>(&yv);
  float* of = reinterpret_cast<float*>(&out);
#pragma unroll
  for (int i = 0; i < V; i++) of[i] = mr_act_grad(gp[i >> 1] * sc, yf[i], act);
  *reinterpret_cast<T*>(dst + o) = out;
}

// One thread per cell (i, j, k) of the layer's input grid [Z][Y][X] and batch item, all NCI input planes in registers. g has gch
// planes at up times the resolution; wt = [sub][tap][gch][NCI], each sub-position's slice the data-gradient form of its weight
// (tfl_train.hpp relay_transposed). The loops are k_conv_direct's (conv.hip) inside a loop over the sub-positions.
template <bool IS3D, int NCI>
__global__ __launch_bounds__(256) void k_up_dgrad(int Z, int Y, int X, int up, int gch, int ksz, const float* __restrict__ g,
                                                  const float* __restrict__ wt, float* __restrict__ gin) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const int j = blockIdx.y * blockDim.y + threadIdx.y;
  const int b = blockIdx.z / Z, k = blockIdx.z - b * Z;
  if (i >= X || j >= Y) return;
  const long long cells = (long long)Z * Y * X;
  const int subs = IS3D ? up * up * up : up * up;
  const long long fcells = cells * subs;
  g += (long long)b * gch * fcells;
  float acc[NCI];
#pragma unroll
  for (int c = 0; c < NCI; c++) acc[c] = 0.0f;
  const int r = (ksz - 1) / 2, rz = IS3D ? r : 0;
  const int taps = IS3D ? ksz * ksz * ksz : ksz * ksz;
  for (int sub = 0; sub < subs; sub++) {
    int tap = 0;
    for (int dz = -rz; dz <= rz; dz++)
      for (int dy = -r; dy <= r; dy++)
        for (int dx = -r; dx <= r; dx++, tap++) {
          const int x = i + dx, y = j + dy, z = k + dz;
          const bool ok = x >= 0 && x < X && y >= 0 && y < Y && z >= 0 && z < Z;
          const long long o = ok ? up_fine_cell(IS3D, up, sub, z, y, x, Y, X) : 0;
          const float* __restrict__ w = wt + ((long long)sub * taps + tap) * gch * NCI;
          for (int co = 0; co < gch; co++) {
            const float v = ok ? g[o + co * fcells] : 0.0f;
#pragma unroll
            for (int c = 0; c < NCI; c++) acc[c] = fmaf(v, w[co * NCI + c], acc[c]);
          }
        }
  }
  const long long o = ((long long)k * Y + j) * X + i;
#pragma unroll
  for (int c = 0; c < NCI; c++) gin[((long long)b * NCI + c) * cells + o] = acc[c];
}
}  // namespace

void pool_bwd_mask(hipStream_t st, bool is3d, int rows, int Z, int Y, int X, const float* y, const float* gc, float* dst, int act) {
  const uintptr_t al = (uintptr_t)y | (uintptr_t)dst;
  const long long cells = (long long)Z * Y * X;
  // (rows of 16 or 8 bytes: every plane starts as aligned as the buffer where its cell count allows it)
  const int V = (X % 4 == 0 && (al & 15) == 0) ? 4 : (X % 2 == 0 && (al & 7) == 0 && cells % 2 == 0) ? 2 : 1;
  const long long n = cells / V;
  const dim3 grd((unsigned)((n + 255) / 256), (unsigned)rows);
  TFL_TIMED("k_pool_bwd_mask", st);
#define TFL_PBM(D3, W) k_pool_bwd_mask<D3, W><<<grd, 256, 0, st>>>(Z, Y, X, y, gc, dst, act)
  if (is3d) { if (V == 4) TFL_PBM(true, 4); else if (V == 2) TFL_PBM(true, 2); else TFL_PBM(true, 1); }
  else { if (V == 4) TFL_PBM(false, 4); else if (V == 2) TFL_PBM(false, 2); else TFL_PBM(false, 1); }
#undef TFL_PBM
}

bool up_dgrad(hipStream_t st, bool is3d, int B, int Z, int Y, int X, int up, int gch, int cin_t, int ksz, const float* g, const float* wt,
              float* gin) {
  const dim3 blk(64, 4), grd((unsigned)((X + 63) / 64), (unsigned)((Y + 3) / 4), (unsigned)(Z * B));
  TFL_TIMED("k_up_dgrad", st);
#define TFL_UDG(N)                                                                                  \
  case N:                                                                                           \
    if (is3d) k_up_dgrad<true, N><<<grd, blk, 0, st>>>(Z, Y, X, up, gch, ksz, g, wt, gin);          \
    else k_up_dgrad<false, N><<<grd, blk, 0, st>>>(Z, Y, X, up, gch, ksz, g, wt, gin);              \
    return true;
  switch (cin_t) {
    TFL_UDG(1) TFL_UDG(2) TFL_UDG(4) TFL_UDG(8) TFL_UDG(16) TFL_UDG(32) TFL_UDG(64)
    default: return false;
  }
#undef TFL_UDG
}

}  // namespace tfl
