// divnorm.hip -- the L2 norm of velocityDivergence(U, flags) per batch item without the divergence field (gfx950): the figure
// lib/calc_stats.lua:98-118 records after every step of a rollout (div[i]:norm()).
//
// Stage 1 (k_divnorm_planes): one streaming pass over U and flags. Per cell the arithmetic of k_divergence (stencil.hip;
// third_party/tfluids.cc:1008-1066) operation for operation in fp32, so the value is the bits tfl_velocityDivergenceForward
// writes; its square is formed and accumulated in fp64 (the square of an fp32 value is exact there). One block per
// (batch item, z-plane) writes ONE double: the plane's sum. Nothing is written per cell: 16 B/cell in 3-D against the 20 of
// k_divergence. The order of the additions inside a plane is fixed by (Y, X) and by which of the two kernel forms runs --
// per thread its tiles in ascending order (a sum of four cells, left to right, per tile), then a shuffle tree over the wave, then
// the waves in ascending order -- and never by which planes the launch covers: a z-slab rank gets the un-cut grid's plane sums.
// Stage 2 (k_divnorm_finish): one block per batch item adds that item's plane sums in ascending z and takes the root.
// No atomics anywhere, so a call gives the same bits every time.
//
// The fast form follows the streaming stencils (tfl_vec4.hpp): four x-cells per thread, 16-byte loads, the x+1 tap of U_x
// out of the neighbouring lane by DPP, narrower lane segments for short rows. Every load is unconditional (a lane that must
// not read takes the field's first vector and drops it: DESIGN.md 3.6) and a thread fetches its next tile before it sums the
// current one, so a wave never waits with an empty load queue.
#include "tfl_device.hpp"
#include "tfl_host.hpp"
#include "tfl_vec4.hpp"

namespace tfl {

namespace {

constexpr int kDivnormThreads = 1024;      // one block per plane: 16 waves keep ~100 KB of loads in flight on its CU

// the block's sum of `acc` in a fixed order; valid in thread 0
__device__ __forceinline__ double block_sum_fixed(double acc, double* wsum) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
  const int t = threadIdx.y * blockDim.x + threadIdx.x;
  if ((t & 63) == 0) wsum[t >> 6] = acc;
  __syncthreads();
  double s = 0.0;
  if (t == 0)
    for (int w = 0; w < kDivnormThreads / 64; w++) s += wsum[w];
  return s;
}

// is plane k of the array a border plane of the whole grid (Dom::zg / Zg: the array's place in it), or the array's own last
// plane (no k + 1 to read: an array end is a domain end or lies beyond every plane a caller asks for)
template <bool IS3D>
__device__ __forceinline__ bool z_border(const Dom& d, int k) {
  if (!IS3D) return false;
  const int kg = k + d.zg;
  return kg < 1 || kg > d.Zg - 2 || k > d.Z - 2;
}

// What a thread holds of one tile: the vectors as they were loaded (a tile that is not `live` holds the fields' first vectors
// and is never looked at: no select sits between a load and its use, so a tile can stay in flight while the one before it is summed)
template <bool IS3D>
struct DivTile {
  float4 f, ux, uy, uyp, uz, uzp;
  float uxr;                 // U_x(i0 + 4) for the last lane of a row segment
  int i0;
  bool live;
};

// tile t of the block (x fastest): row (t / nti) * blockDim.y + threadIdx.y, float4 column (t % nti) * blockDim.x + threadIdx.x
template <bool IS3D>
__device__ __forceinline__ void divnorm_load(const Dom& d, const float* __restrict__ U, const float* __restrict__ flags, int k,
                                             bool zb, int t, int nt, int nti, DivTile<IS3D>& q) {
  const int tj = t / nti, ti = t - tj * nti;
  const int j = tj * (int)blockDim.y + (int)threadIdx.y;
  q.i0 = (ti * (int)blockDim.x + (int)threadIdx.x) * 4;
  // rows 0 and Y - 1 and border planes hold zeros only: nothing is read there
  q.live = t < nt && q.i0 < d.X && j >= 1 && j <= d.Y - 2 && !zb;
  const int o = q.live ? TFL_AT(d, q.i0, j, k) : 0;
  const int oy = q.live ? d.sy : 0, oz = q.live ? d.sz : 0;
  q.f = *reinterpret_cast<const float4*>(flags + o);
  q.ux = *reinterpret_cast<const float4*>(U + o);
  q.uy = *reinterpret_cast<const float4*>(U + d.sc + o);
  q.uyp = *reinterpret_cast<const float4*>(U + d.sc + o + oy);
  if (IS3D) {
    q.uz = *reinterpret_cast<const float4*>(U + 2 * d.sc + o);
    q.uzp = *reinterpret_cast<const float4*>(U + 2 * d.sc + o + oz);
  }
  // the x+1 tap of the segment's last lane (cell X - 1 is a border cell: a row's last float4 needs none)
  const bool need = q.live && threadIdx.x == blockDim.x - 1 && q.i0 + 4 < d.X;
  q.uxr = U[need ? o + 4 : 0];
}

// EVERY lane of the wave must call this (DPP)
template <bool IS3D>
__device__ __forceinline__ double divnorm_sum(const Dom& d, const DivTile<IS3D>& t) {
  const float f[4] = {t.f.x, t.f.y, t.f.z, t.f.w}, ux[4] = {t.ux.x, t.ux.y, t.ux.z, t.ux.w};
  const float uy[4] = {t.uy.x, t.uy.y, t.uy.z, t.uy.w}, uyp[4] = {t.uyp.x, t.uyp.y, t.uyp.z, t.uyp.w};
  float uxp[4] = {ux[1], ux[2], ux[3], from_lane_above(ux[0])};
  if (threadIdx.x == blockDim.x - 1) uxp[3] = t.uxr;
  float uz[4] = {0.0f, 0.0f, 0.0f, 0.0f}, uzp[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  if (IS3D) {
    uz[0] = t.uz.x; uz[1] = t.uz.y; uz[2] = t.uz.z; uz[3] = t.uz.w;
    uzp[0] = t.uzp.x; uzp[1] = t.uzp.y; uzp[2] = t.uzp.z; uzp[3] = t.uzp.w;
  }
  double s = 0.0;
#pragma unroll
  for (int q = 0; q < 4; q++) {
    const int i = t.i0 + q;
    float v = 0.0f;
    if (t.live && i >= 1 && i <= d.X - 2 && (((int)f[q]) & kFluid)) {
      v = ux[q] - uxp[q] + uy[q] - uyp[q];
      if (IS3D) v += (uz[q] - uzp[q]);
    }
    const double dv = (double)v;
    s += dv * dv;
  }
  return s;
}

// blockDim = (BX, 1024 / BX, 1), BX a power of two <= 32 (a row segment = BX consecutive lanes of one wave); X % 4 == 0, U and
// flags 16-byte aligned. sums[b * zstride + zoff + k] = the sum over plane k of batch item b.
template <bool IS3D>
__global__ __launch_bounds__(kDivnormThreads) void k_divnorm_planes_v4(Dom d, const float* __restrict__ U, const float* __restrict__ flags,
                                                                       double* __restrict__ sums, int zstride, int zoff) {
  __shared__ double wsum[kDivnormThreads / 64];
  int b, k; dom_bk(d, b, k);
  const long long cells = (long long)d.sc;
  U += b * cells * (IS3D ? 3 : 2); flags += b * cells;
  const bool zb = z_border<IS3D>(d, k);
  const int nti = (d.X / 4 + (int)blockDim.x - 1) / (int)blockDim.x, ntj = (d.Y + (int)blockDim.y - 1) / (int)blockDim.y;
  const int nt = nti * ntj;
  double acc = 0.0;
  // two tiles in turn, each fetched while the other is summed (a tile past the last one is not live and adds +0)
  DivTile<IS3D> ta, tb;
  divnorm_load<IS3D>(d, U, flags, k, zb, 0, nt, nti, ta);
  for (int t = 0; t < nt; t += 2) {
    divnorm_load<IS3D>(d, U, flags, k, zb, t + 1, nt, nti, tb);
    acc += divnorm_sum<IS3D>(d, ta);
    divnorm_load<IS3D>(d, U, flags, k, zb, t + 2, nt, nti, ta);
    acc += divnorm_sum<IS3D>(d, tb);
  }
  const double s = block_sum_fixed(acc, wsum);
  if (threadIdx.x == 0 && threadIdx.y == 0) sums[(long long)b * zstride + zoff + k] = s;
}

// The one-cell-per-thread form (X % 4 != 0 or a misaligned view): blockDim = (64, 16, 1), the arithmetic of k_divergence.
template <bool IS3D>
__global__ __launch_bounds__(kDivnormThreads) void k_divnorm_planes_c1(Dom d, const float* __restrict__ U, const float* __restrict__ flags,
                                                                       double* __restrict__ sums, int zstride, int zoff) {
  __shared__ double wsum[kDivnormThreads / 64];
  int b, k; dom_bk(d, b, k);
  const long long cells = (long long)d.sc;
  U += b * cells * (IS3D ? 3 : 2); flags += b * cells;
  const bool zb = z_border<IS3D>(d, k);
  double acc = 0.0;
  for (int j = threadIdx.y; j < d.Y; j += blockDim.y)
    for (int i = threadIdx.x; i < d.X; i += blockDim.x) {
      const int o = TFL_AT(d, i, j, k);
      float v = 0.0f;
      if (!(zb || i < 1 || i > d.X - 2 || j < 1 || j > d.Y - 2) && (((int)flags[o]) & kFluid)) {
        v = U[o] - U[o + 1] + U[o + d.sc] - U[o + d.sc + d.sy];
        if (IS3D) v += (U[o + 2 * d.sc] - U[o + 2 * d.sc + d.sz]);
      }
      const double dv = (double)v;
      acc += dv * dv;
    }
  const double s = block_sum_fixed(acc, wsum);
  if (threadIdx.x == 0 && threadIdx.y == 0) sums[(long long)b * zstride + zoff + k] = s;
}

// norm[b] = sqrt(sums[b][0] + sums[b][1] + ... + sums[b][nz - 1]), the additions in exactly this order
__global__ __launch_bounds__(256) void k_divnorm_finish(const double* __restrict__ sums, int nz, double* __restrict__ norm) {
  __shared__ double part[1024];
  const double* s = sums + (long long)blockIdx.x * nz;
  double acc = 0.0;
  for (int base = 0; base < nz; base += 1024) {
    const int n = nz - base < 1024 ? nz - base : 1024;
    for (int t = threadIdx.x; t < n; t += blockDim.x) part[t] = s[base + t];
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll 16
      for (int t = 0; t < n; t++) acc += part[t];       // (unrolled: the LDS reads of 16 planes travel together, the additions stay in order)
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) norm[blockIdx.x] = sqrt(acc);
}

}  // namespace

void divergence_norm_planes(hipStream_t st, const Scope& sc, bool is3d, int B, int Z, int Y, int X, const float* U, const float* flags,
                            double* sums, int zstride, int zoff) {
  const Dom d = make_dom(sc, Z, Y, X);
  if (d.nw < 1 || B < 1) return;
  const dim3 grd(1, 1, (unsigned)(d.nw * B));
  const Vec4Launch v = vec4_launch(B, d, {U, flags});       // (its row-segment width and its refusals; the block is ours)
  TFL_TIMED_EXT("k_divnorm_planes", st);
  if (v.ok) {
    const dim3 blk(v.blk.x, kDivnormThreads / v.blk.x, 1);
    if (is3d) TFL_LAUNCH_EXT((k_divnorm_planes_v4<true>), grd, blk, 0, st, d, U, flags, sums, zstride, zoff);
    else TFL_LAUNCH_EXT((k_divnorm_planes_v4<false>), grd, blk, 0, st, d, U, flags, sums, zstride, zoff);
    return;
  }
  const dim3 blk(64, kDivnormThreads / 64, 1);
  if (is3d) TFL_LAUNCH_EXT((k_divnorm_planes_c1<true>), grd, blk, 0, st, d, U, flags, sums, zstride, zoff);
  else TFL_LAUNCH_EXT((k_divnorm_planes_c1<false>), grd, blk, 0, st, d, U, flags, sums, zstride, zoff);
}

void divergence_norm_finish(hipStream_t st, int B, int nz, const double* sums, double* norm) {
  if (B < 1) return;
  TFL_TIMED_EXT("k_divnorm_finish", st);
  TFL_LAUNCH_EXT(k_divnorm_finish, (unsigned)B, 256, 0, st, sums, nz, norm);
}

}  // namespace tfl
