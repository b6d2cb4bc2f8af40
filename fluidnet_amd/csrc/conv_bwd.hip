// conv_bwd.hip -- parameter gradients of the projection ConvNet's convolution layers (gfx950): what
// cudnn.{Spatial,Volumetric}Convolution:accGradParameters computes for the reference's model:backward
// (torch/lib/run_epoch.lua:207-235), for the stride-1, zero-padded cross-correlation of conv.hip.
//
//   gradWeight[co][ci][tap] = sum over (b, pos) of x[ci][pos + tap] * g_pre[co][pos],   gradBias[co] = sum of g_pre[co][pos]
//   g_pre = g_out (.) act'(y), y the layer's saved post-activation output
//
// i.e. a GEMM with M = cin * taps rows (plus one row of ones: the bias rides in the same launch), N = cout columns and the
// reduction over every voxel of every batch item. gfx950's fp32 MFMA runs at the fp32 vector rate, so this is an LDS-tiled
// vector-ALU kernel: k_conv_wgrad stages a 32 x 8 tile of x with its halo and the tile's (masked) g once per chunk, every
// thread owns one row and a register block of output channels and runs an fp32 fmaf chain over the tile's voxels; after each
// tile the chain goes into the thread's fp64 sums. A block walks its tiles in a fixed order, adds the threads that shared a
// row in a fixed order and leaves its sums at a fixed place; k_conv_wgrad_finish adds the blocks' partials in a fixed order in
// fp64, rounds once to fp32, accumulates (one fp32 add) or overwrites, and writes the cudnn layout. No atomics: the same
// inputs give the same bits on every call.
//
// The activation mask is applied where g is read; with `wb` the masked value is also written back over g, so that the data
// gradient that follows (conv_direct on the transposed, mirrored weights) reads g_pre without a launch of its own.
#include "tfl_device.hpp"
#include "tfl_host.hpp"
#include "tfl_train.hpp"

namespace tfl {

struct WgArgs {
  const float* x;       // the layer's input [B][cin][Z][Y][X]
  float* g;             // the gradient at the layer's output [B][cout][Z][Y][X]
  const float* y;       // the saved post-activation output [B][ych][Z][Y][X] (act != 0)
  double* partials;     // [block][cin * taps + 1][cout]
  int Z, Y, X, cin, cout, k, taps, ych, act, wb, is3d;
  int ch, tt, S, ntx, nty;
  long long tiles;
  int dil;              // tap spacing (a dilated bank's module; read by the DIL instantiations only)
  int up, gch;          // (the UP instantiations only) an upsample layer's inner convolution: g and y have gch planes at up times
                        // the resolution, column cv = sub * gch + co reads plane co at up_fine_cell(sub, z, y, x); cout = subs * gch
};

// act'(y) from the saved output: ReLU y > 0, ReLU6 0 < y < 6, sigmoid y (1 - y)
__device__ __forceinline__ float act_grad(float g, float y, int act) {
  if (act == 1) return y > 0.0f ? g : 0.0f;
  if (act == 2) return (y > 0.0f && y < 6.0f) ? g : 0.0f;
  return g * (y * (1.0f - y));
}

// DIL = false: tap spacing 1 as a constant -- the kernel of the linear models, unchanged by the dilated form
// UP = true: the strided read of g and y of an upsample layer: the mask is taken behind the shuffle, the masked
// value written back to the fine cell it was read from (every fine cell belongs to one (cell, sub-position): written once)
template <int CB, bool DIL, bool UP = false>
__global__ __launch_bounds__(kWgThreads) void k_conv_wgrad(WgArgs a) {
  extern __shared__ float lds[];
  const int tid = threadIdx.x;
  const int dil = DIL ? a.dil : 1;
  const WgHalo h = wg_halo(a.is3d != 0, a.k, dil);
  float* xs = lds;                        // [ch][HZ][HY][HX]
  float* gs = lds + a.ch * h.floats;      // [voxel][CB]
  const long long cells = (long long)a.Z * a.Y * a.X;
  const int M = a.cin * a.taps;
  const int vx = tid % kWgTX, vy = tid / kWgTX;      // the voxel this thread stages g for
  for (int co0 = 0; co0 < a.cout; co0 += CB) {
    const int sub = UP ? co0 / a.gch : 0, cp0 = UP ? co0 - sub * a.gch : co0;      // (sub-position, first plane of g)
    const int gch = UP ? a.gch : a.cout;
    const long long gcells = UP ? cells * (a.cout / a.gch) : cells;
    for (int ci0 = 0; ci0 < a.cin; ci0 += a.ch)
      for (int t0 = 0; t0 < a.taps; t0 += a.tt) {
        const WgChunk ck = wg_chunk(a.ch, a.tt, a.cin, a.taps, ci0, t0);      // (its first chunk carries the bias row and masks g)
        const WgThread t = wg_thread(tid, ck, h, a.S, ci0, t0, a.k, a.taps, a.is3d != 0, M, dil);
        const bool mask_now = a.act != 0 && (!a.wb || ck.first);
        double acc64[CB];
#pragma unroll
        for (int c = 0; c < CB; c++) acc64[c] = 0.0;
        for (long long tile = blockIdx.x; tile < a.tiles; tile += gridDim.x) {
          const int tx = (int)(tile % a.ntx);
          long long q = tile / a.ntx;
          const int ty = (int)(q % a.nty); q /= a.nty;
          const int z = (int)(q % a.Z), b = (int)(q / a.Z);
          const int x0 = tx * kWgTX, y0 = ty * kWgTY;
          for (int e = tid; e < ck.nch * h.floats; e += kWgThreads) {
            const int c = e / h.floats, hh = e - c * h.floats;
            const int hx = hh % h.HX, hy = (hh / h.HX) % h.HY, hz = hh / (h.HX * h.HY);
            const int gx = x0 + hx - h.r, gy = y0 + hy - h.r, gz = z + hz - h.rz;
            const bool ok = gx >= 0 && gx < a.X && gy >= 0 && gy < a.Y && gz >= 0 && gz < a.Z;
            xs[e] = ok ? a.x[((long long)b * a.cin + ci0 + c) * cells + ((long long)gz * a.Y + gy) * a.X + gx] : 0.0f;
          }
          {
            const int gx = x0 + vx, gy = y0 + vy;
            const bool ok = gx < a.X && gy < a.Y;
            const long long o = UP ? (ok ? up_fine_cell(a.is3d != 0, a.up, sub, z, gy, gx, a.Y, a.X) : 0) : ((long long)z * a.Y + gy) * a.X + gx;
#pragma unroll
            for (int c = 0; c < CB; c++) {
              float v = 0.0f;
              if (ok) {
                float* gp = a.g + ((long long)b * gch + cp0 + c) * gcells + o;
                v = *gp;
                if (mask_now) {
                  v = act_grad(v, a.y[((long long)b * a.ych + cp0 + c) * gcells + o], a.act);
                  if (a.wb) *gp = v;
                }
              }
              gs[wg_g_slot(tid, CB, c)] = v;
            }
          }
          __syncthreads();
          if (t.active) {
            float acc[CB];
#pragma unroll
            for (int c = 0; c < CB; c++) acc[c] = 0.0f;
            for (int v = t.s; v < kWgThreads; v += a.S) {
              const float xv = t.is_bias ? 1.0f : xs[wg_x_slot(t, h, v)];
#pragma unroll
              for (int c = 0; c < CB; c++) acc[c] = fmaf(xv, gs[wg_g_slot(v, CB, c)], acc[c]);
            }
#pragma unroll
            for (int c = 0; c < CB; c++) acc64[c] += (double)acc[c];
          }
          __syncthreads();
        }
        // the slices of a row, added in slice order (the tile loop ended on a barrier: the LDS is free)
        if (a.S > 1) {
          double* red = reinterpret_cast<double*>(lds);      // [slice][row of the chunk][CB]
          if (t.active) {
#pragma unroll
            for (int c = 0; c < CB; c++) red[wg_red_slot(t, ck, t.s, CB, c)] = acc64[c];
          }
          __syncthreads();
          if (t.active && t.s == 0) {
            for (int q = 1; q < a.S; q++) {
#pragma unroll
              for (int c = 0; c < CB; c++) acc64[c] += red[wg_red_slot(t, ck, q, CB, c)];
            }
          }
          __syncthreads();
        }
        if (t.active && t.s == 0) {
#pragma unroll
          for (int c = 0; c < CB; c++) a.partials[wg_partial_slot((int)blockIdx.x, M, t.row, a.cout, co0 + c)] = acc64[c];
        }
      }
  }
}

// The blocks' partials of 32 (row, co) results per block of 32 x 8 threads, in fp64 and in a fixed order: lane y adds the
// partials y, y + 8, ... in ascending order, lane 0 then adds the eight lanes in order; then the cudnn layout.
__global__ __launch_bounds__(256) void k_conv_wgrad_finish(const double* __restrict__ partials, int P, int M, int cout, int taps, int cin,
                                                           int cin_ref, int cout_ref, int skip_in, float* __restrict__ gw,
                                                           float* __restrict__ gb, int accumulate, int join_c, int join_p, int subs) {
  __shared__ double sh[8][33];
  const int total = (M + 1) * cout;
  const int o = blockIdx.x * 32 + threadIdx.x;
  double s = 0.0;
  if (o < total)
    for (int p = threadIdx.y; p < P; p += 8) s += partials[wg_partial_slot(p, M, 0, cout, o)];      // (row * cout + co = o)
  sh[threadIdx.y][threadIdx.x] = s;
  __syncthreads();
  if (threadIdx.y != 0 || o >= total) return;
  for (int q = 1; q < 8; q++) s += sh[q][threadIdx.x];
  const int row = o / cout, co = o - row * cout;
  const float f = (float)s;
  float* dst;
  if (subs > 1) {      // an upsample layer's inner convolution: cout = subs * its padded output channels
    const long long i = wg_cudnn_index_up(row == M ? -1 : row, co, cout / subs, subs, taps, cin, cin_ref, cout_ref);
    if (i < 0) return;
    dst = (row == M ? gb : gw) + i;
  } else if (row == M) {
    if (co >= cout_ref) return;
    dst = gb + co;
  } else {
    const long long i = wg_cudnn_index(row, co, taps, cin, cin_ref, cout_ref, skip_in, join_c, join_p);
    if (i < 0) return;
    dst = gw + i;
  }
  *dst = accumulate ? *dst + f : f;
}

// (model.hip scale_from_stats, restated: the input scale of batch item b from its (sum, sum of squares) pair)
__device__ __forceinline__ float tape_scale(const double* __restrict__ stats, int b, double n) {
  const double s1 = stats[b * 2], s2 = stats[b * 2 + 1];
  return (float)sqrt(fmax(n * s2 - s1 * s1, 0.0) / (n * (n - 1.0)));
}

// dst[b][t] = scale_b * src[b][t] (+ add[b][t]); dst may be add
__global__ __launch_bounds__(256) void k_scale_add(long long per, const double* __restrict__ stats, double count, const float* __restrict__ src,
                                                   const float* add, float* dst) {
  const int b = blockIdx.y;
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t >= per) return;
  const long long o = (long long)b * per + t;
  const float v = tape_scale(stats, b, count) * src[o];
  dst[o] = add ? v + add[o] : v;
}

void scale_add(hipStream_t st, int B, long long per, const double* stats, double count, const float* src, const float* add, float* dst) {
  TFL_TIMED("k_scale_add", st);
  k_scale_add<<<dim3((unsigned)((per + 255) / 256), (unsigned)B), 256, 0, st>>>(per, stats, count, src, add, dst);
}

// the masking of k_conv_wgrad's write-back without the sums: g *= act'(y), plane by plane
__global__ __launch_bounds__(256) void k_act_mask(long long cells, int cout, int ych, float* __restrict__ g, const float* __restrict__ y, int act) {
  const int b = blockIdx.z, c = blockIdx.y;
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t >= cells) return;
  const long long o = ((long long)b * cout + c) * cells + t;
  g[o] = act_grad(g[o], y[((long long)b * ych + c) * cells + t], act);
}

void act_mask(hipStream_t st, int B, int cout, int ych, long long cells, float* g, const float* y, int act) {
  TFL_TIMED("k_act_mask", st);
  k_act_mask<<<dim3((unsigned)((cells + 255) / 256), (unsigned)cout, (unsigned)B), 256, 0, st>>>(cells, cout, ych, g, y, act);
}

bool conv_wgrad_fits(const WgPlan& p) { return p.lds_floats <= 16384; }

bool conv_wgrad(hipStream_t st, bool is3d, const WgPlan& p, int B, int Z, int Y, int X, int cin, int cout, int k, const float* x,
                float* g, const float* y, int ych, int act, bool wb, double* partials) {
  if (!conv_wgrad_fits(p)) return false;
  (void)B;
  WgArgs a;
  a.x = x; a.g = g; a.y = y; a.partials = partials;
  a.Z = Z; a.Y = Y; a.X = X; a.cin = cin; a.cout = cout; a.k = k; a.taps = p.taps; a.ych = ych; a.act = y ? act : 0; a.wb = wb ? 1 : 0;
  a.is3d = is3d ? 1 : 0;
  a.dil = p.dil;
  a.up = p.up; a.gch = cout;
  if (p.up > 1) {
    if (p.dil > 1 || p.vcout != cout * p.subs || cout % p.cb) return false;
    a.cout = p.vcout;
  }
  a.ch = p.ch; a.tt = p.tt; a.S = p.S; a.ntx = (X + kWgTX - 1) / kWgTX; a.nty = (Y + kWgTY - 1) / kWgTY; a.tiles = p.tiles;
  const size_t shmem = sizeof(float) * (size_t)p.lds_floats;
  TFL_TIMED("k_conv_wgrad", st);
#define TFL_WG(N)                                                                                  \
  case N:                                                                                          \
    if (p.up > 1) k_conv_wgrad<N, false, true><<<p.nblocks, kWgThreads, shmem, st>>>(a);           \
    else if (p.dil > 1) k_conv_wgrad<N, true><<<p.nblocks, kWgThreads, shmem, st>>>(a);            \
    else k_conv_wgrad<N, false><<<p.nblocks, kWgThreads, shmem, st>>>(a);                          \
    return true;
  switch (p.cb) {
    TFL_WG(1) TFL_WG(2) TFL_WG(4) TFL_WG(8) TFL_WG(16)
    default: return false;
  }
#undef TFL_WG
}

void conv_wgrad_finish(hipStream_t st, const WgPlan& p, int cin, int cout, int cin_ref, int cout_ref, int skip_in, const double* partials,
                       float* gw, float* gb, int accumulate, int join_c, int join_p) {
  const int M = cin * p.taps;
  if (p.up > 1) cout = p.vcout;
  TFL_TIMED("k_conv_wgrad_finish", st);
  k_conv_wgrad_finish<<<((M + 1) * cout + 31) / 32, dim3(32, 8), 0, st>>>(partials, p.nblocks, M, cout, p.taps, cin, cin_ref, cout_ref,
                                                                        skip_in, gw, gb, accumulate, join_c, join_p, p.up > 1 ? p.subs : 1);
}

// ---- the fixed linear maps of a banked model, backwards: streaming kernels, every output element written once
// by one thread from sums in a fixed order, no atomics ------------------------------------------------------------------------
struct JoinBwdDst { int n; int sh[kTrainMaxBanks]; float* dst[kTrainMaxBanks]; };

// W consecutive floats of a row, added left to right onto s: one 64- or 128-bit load where the row start is aligned for it
template <int W>
__device__ __forceinline__ float row_sum(const float* __restrict__ p, float s) {
  if (W == 2 && ((uintptr_t)p & 7) == 0) { const float2 v = *reinterpret_cast<const float2*>(p); return (s + v.x) + v.y; }
  if (W == 4 && ((uintptr_t)p & 15) == 0) { const float4 v = *reinterpret_cast<const float4*>(p); return (((s + v.x) + v.y) + v.z) + v.w; }
#pragma unroll
  for (int i = 0; i < W; i++) s += p[i];
  return s;
}

// The join's backward, one launch per join: blockIdx.z = bank i, blockIdx.y = (b, c), the block's threads = cells of the bank's
// own grid. From g [B][och] at the join's resolution [Z][Y][X], bank i gets [B][C] at (grid >> sh_i): its channel slice (concat) or
// every channel (add); sh = 0 a copy, else the sum over the (2^sh)^dim cells the nearest up-sample replicated the cell over, in
// fp32, z then y then x (join_bwd_child's order).
template <bool IS3D>
__global__ __launch_bounds__(256) void k_join_bwd(int C, int och, int concat, int Z, int Y, int X, JoinBwdDst jd, const float* __restrict__ g) {
  const int i = blockIdx.z, sh = jd.sh[i];
  const int Zs = IS3D ? Z >> sh : Z, Ys = Y >> sh, Xs = X >> sh;
  const long long cs = (long long)Zs * Ys * Xs, t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t >= cs) return;
  const int b = blockIdx.y / C, c = blockIdx.y - b * C;
  const float* __restrict__ gp = g + ((long long)b * och + join_bwd_plane(concat != 0, i, C, c)) * ((long long)Z * Y * X);
  float* __restrict__ out = jd.dst[i] + (long long)blockIdx.y * cs;
  if (sh == 0) { out[t] = gp[t]; return; }
  const int x = (int)(t % Xs), y = (int)((t / Xs) % Ys), z = (int)(t / ((long long)Xs * Ys));
  const int w = 1 << sh, wz = IS3D ? w : 1;
  float s = 0.0f;
  for (int dz = 0; dz < wz; dz++)
    for (int dy = 0; dy < w; dy++) {
      const float* __restrict__ row = gp + join_bwd_child(IS3D, sh, z, y, x, (dz * w + dy) * w, Y, X);
      if (sh == 1) s = row_sum<2>(row, s);
      else if (sh == 2) s = row_sum<4>(row, s);
      else for (int dx = 0; dx < w; dx++) s += row[dx];
    }
  out[t] = s;
}

bool join_bwd(hipStream_t st, bool is3d, bool concat, int B, int C, int och, int Z, int Y, int X, int n, const int* sh, float* const* dst,
              const float* g) {
  if (n < 1 || n > kTrainMaxBanks) return false;
  JoinBwdDst jd;
  jd.n = n;
  for (int i = 0; i < n; i++) { jd.sh[i] = sh[i]; jd.dst[i] = dst[i]; }
  const long long cells = train_cells(is3d, sh[0], Z, Y, X);      // (bank 0 is the finest)
  const dim3 grd((unsigned)((cells + 255) / 256), (unsigned)(B * C), (unsigned)n);
  TFL_TIMED("k_join_bwd", st);
  if (is3d) k_join_bwd<true><<<grd, 256, 0, st>>>(C, och, concat ? 1 : 0, Z, Y, X, jd, g);
  else k_join_bwd<false><<<grd, 256, 0, st>>>(C, och, concat ? 1 : 0, Z, Y, X, jd, g);
  return true;
}

// The average-pooling pyramid's backward with accumulate, one launch per level: dst = a + P^T c, P^T = every coarse cell of
// c [rows][Z/2][Y/2][X/2] over its 2^dim children times 1/2^dim. A thread owns the two x-children of one coarse cell in one fine row
// (X is even: one 64-bit load and store; the buffers are 8-byte aligned). dst may be a.
template <bool IS3D>
__global__ __launch_bounds__(256) void k_pyr_pool_bwd(int Z, int Y, int X, const float* a, const float* __restrict__ c, float* dst) {
  const int Xh = X >> 1;
  const long long pairs = (long long)Z * Y * Xh, t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t >= pairs) return;
  const int xc = (int)(t % Xh), y = (int)((t / Xh) % Y), z = (int)(t / ((long long)Xh * Y));
  const long long cells = (long long)Z * Y * X;
  const float v = c[(long long)blockIdx.y * (cells >> (IS3D ? 3 : 2)) + pyr_bwd_parent(IS3D, z, y, 2 * xc, Y, X)] * (IS3D ? 0.125f : 0.25f);
  const long long o = (long long)blockIdx.y * cells + ((long long)z * Y + y) * X + 2 * xc;
  float2 f = *reinterpret_cast<const float2*>(a + o);
  f.x += v; f.y += v;
  *reinterpret_cast<float2*>(dst + o) = f;
}

void pyr_pool_bwd(hipStream_t st, bool is3d, int rows, int Z, int Y, int X, const float* a, const float* c, float* dst) {
  const long long pairs = (long long)Z * Y * (X / 2);
  const dim3 grd((unsigned)((pairs + 255) / 256), (unsigned)rows);
  TFL_TIMED("k_pyr_pool_bwd", st);
  if (is3d) k_pyr_pool_bwd<true><<<grd, 256, 0, st>>>(Z, Y, X, a, c, dst);
  else k_pyr_pool_bwd<false><<<grd, 256, 0, st>>>(Z, Y, X, a, c, dst);
}

// The dilate split's backward: dst = ((src0 + src1) + src2) ... in bank order, fp32; 128-bit where every buffer is aligned for it
struct BankSumSrc { int n; const float* src[kTrainMaxBanks]; };
__global__ __launch_bounds__(256) void k_bank_sum(long long count, int vec, BankSumSrc bs, float* __restrict__ dst) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (vec) {
    if (4 * t + 3 < count) {
      float4 s = reinterpret_cast<const float4*>(bs.src[0])[t];
      for (int q = 1; q < bs.n; q++) {
        const float4 v = reinterpret_cast<const float4*>(bs.src[q])[t];
        s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
      }
      reinterpret_cast<float4*>(dst)[t] = s;
      return;
    }
    for (long long e = 4 * t; e < count; e++) {      // (the ragged end: at most three elements, one thread)
      float s = bs.src[0][e];
      for (int q = 1; q < bs.n; q++) s += bs.src[q][e];
      dst[e] = s;
    }
    return;
  }
  if (t >= count) return;
  float s = bs.src[0][t];
  for (int q = 1; q < bs.n; q++) s += bs.src[q][t];
  dst[t] = s;
}

bool bank_sum(hipStream_t st, long long count, int n, const float* const* src, float* dst) {
  if (n < 1 || n > kTrainMaxBanks) return false;
  BankSumSrc bs;
  bs.n = n;
  bool vec = ((uintptr_t)dst & 15) == 0;
  for (int q = 0; q < n; q++) { bs.src[q] = src[q]; vec = vec && ((uintptr_t)src[q] & 15) == 0; }
  const long long threads = vec ? (count + 3) / 4 : count;
  TFL_TIMED("k_bank_sum", st);
  k_bank_sum<<<(unsigned)((threads + 255) / 256), 256, 0, st>>>(count, vec ? 1 : 0, bs, dst);
  return true;
}

}  // namespace tfl
