// criterion.hip -- nn.FluidCriterion (lib/modules/fluid_criterion.lua with lib/modules/weighted_flat_mse_criterion.lua) on the
// device (gfx950): the three loss terms and the gradients to the model's outputs in ONE streaming pass, plus the border weight.
//
//   k_criterion_weight   fluid_criterion.lua:145-158: signedDistanceField (the arithmetic of k_signed_distance, shared through
//                        signed_distance_at) followed by the clamp / ramp / rescale, one rounding per Lua call, in one launch.
//   k_criterion_planes   one block per (batch item, z-plane) reads pPred, pTarget, UPred, UTarget, flags and the weight once,
//                        forms per element in fp32  z = w x - w t  (z = x - t unweighted) and  zd = w dv  with dv the bits
//                        tfl_velocityDivergenceForward writes (k_divergence's arithmetic), squares in fp64 and writes THREE
//                        doubles: the plane's sums of the p, U and divergence terms. With gradients (GRAD) the same launch
//                        writes gradP and gradU: g = ((norm z) w) lambda per term, and for U the gather of k_divergence_bwd
//                        (backward.hip) over go = g_div, which is recomputed at the three -c neighbours from U and flags --
//                        no divergence field and no go field exist in memory.
//   k_criterion_finish   one block adds the plane sums in ascending (b, z) and writes {pLoss, uLoss, divLoss, total}.
//
// The reduction discipline is divnorm.hip's: fp64, a fixed order inside a plane (per thread its tiles in ascending order, a
// shuffle tree over the wave, the waves in ascending order), planes in ascending order, no atomics: the same bits every call,
// and batch item b's plane sums do not depend on B. The streaming form is tfl_vec4.hpp's: four x-cells per thread, 16-byte
// unconditional loads (a lane that must not read takes the field's first vector and drops it), the x neighbours out of the
// neighbouring lane by DPP; X % 4 != 0 or a misaligned view runs one cell per thread.
#include "tfl_device.hpp"
#include "tfl_host.hpp"
#include "tfl_vec4.hpp"

namespace tfl {

namespace {

constexpr int kCritThreads = 1024;

// the block's sums of three accumulators in a fixed order; valid in thread 0
__device__ __forceinline__ void block_sum3_fixed(double& a0, double& a1, double& a2, double (*wsum)[kCritThreads / 64]) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    a0 += __shfl_down(a0, off, 64); a1 += __shfl_down(a1, off, 64); a2 += __shfl_down(a2, off, 64);
  }
  const int t = threadIdx.y * blockDim.x + threadIdx.x;
  if ((t & 63) == 0) { wsum[0][t >> 6] = a0; wsum[1][t >> 6] = a1; wsum[2][t >> 6] = a2; }
  __syncthreads();
  if (t == 0) {
    a0 = a1 = a2 = 0.0;
    for (int w = 0; w < kCritThreads / 64; w++) { a0 += wsum[0][w]; a1 += wsum[1][w]; a2 += wsum[2][w]; }
  }
}

// weighted_flat_mse_criterion.lua's gradient of one element: 2/n (w x - w t) w, then FluidCriterion's :mul(lambda)
__device__ __forceinline__ float grad_of(float norm, float z, float w, float lambda) { return ((norm * z) * w) * lambda; }

// dv of cell (i, j, k): k_divergence (stencil.hip) operation for operation; ct = the cell contributes (interior fluid)
template <bool IS3D>
__device__ __forceinline__ float div_cell(const Dom& d, const float* __restrict__ U, const float* __restrict__ flags, int i, int j, int k,
                                          bool& ct) {
  const int o = TFL_AT(d, i, j, k);
  ct = !on_border<IS3D>(d, i, j, k) && (((int)flags[o]) & kFluid);
  float v = 0.0f;
  if (ct) {
    v = U[o] - U[o + 1] + U[o + d.sc] - U[o + d.sc + d.sy];
    if (IS3D) v += (U[o + 2 * d.sc] - U[o + 2 * d.sc + d.sz]);
  }
  return v;
}
// go = g_div of cell (i, j, k), recomputed from U, flags and the weight
template <bool IS3D, bool HASW>
__device__ __forceinline__ float go_cell(const Dom& d, const CriterionArgs& a, const float* __restrict__ U, const float* __restrict__ flags,
                                         const float* __restrict__ w, int i, int j, int k, bool& ct) {
  const float dv = div_cell<IS3D>(d, U, flags, i, j, k, ct);
  const float wv = HASW ? w[TFL_AT(d, i, j, k)] : 1.0f;
  return grad_of(a.normP, wv * dv, wv, a.lamD);
}

// ---- one cell per thread: blockDim = (64, 16, 1) ------------------------------------------------------------------------
template <bool IS3D, bool GRAD, bool HASW>
__global__ __launch_bounds__(kCritThreads) void k_criterion_planes_c1(Dom d, CriterionArgs a) {
  __shared__ double wsum[3][kCritThreads / 64];
  constexpr int C = IS3D ? 3 : 2;
  int b, k; dom_bk(d, b, k);
  const long long cells = (long long)d.sc;
  const float* __restrict__ p = a.p + b * cells; const float* __restrict__ pt = a.pt + b * cells;
  const float* __restrict__ U = a.U + b * cells * C; const float* __restrict__ Ut = a.Ut + b * cells * C;
  const float* __restrict__ flags = a.flags + b * cells;
  const float* __restrict__ w = HASW ? a.w + b * cells : nullptr;
  float* __restrict__ gP = GRAD ? a.gP + b * cells : nullptr;
  float* __restrict__ gU = GRAD ? a.gU + b * cells * C : nullptr;
  double sp = 0.0, su = 0.0, sd = 0.0;
  for (int j = threadIdx.y; j < d.Y; j += blockDim.y)
    for (int i = threadIdx.x; i < d.X; i += blockDim.x) {
      const int o = TFL_AT(d, i, j, k);
      const float wv = HASW ? w[o] : 1.0f;
      if (a.pOn) {
        const float x = wv * p[o], t = wv * pt[o], z = x - t;
        sp += (double)z * (double)z;
        if (GRAD) gP[o] = grad_of(a.normP, z, wv, a.lamP);
      } else if (GRAD) {
        gP[o] = 0.0f;
      }
      bool self = false;
      float go0 = 0.0f;
      if (a.dOn) {
        const float zd = wv * div_cell<IS3D>(d, U, flags, i, j, k, self);
        sd += (double)zd * (double)zd;
        go0 = grad_of(a.normP, zd, wv, a.lamD);
      }
#pragma unroll
      for (int c = 0; c < C; c++) {
        float r = 0.0f;
        if (a.uOn) {
          const float x = wv * U[o + c * d.sc], t = wv * Ut[o + c * d.sc], z = x - t;
          su += (double)z * (double)z;
          r = r + grad_of(a.normU, z, wv, a.lamU);
        }
        if (GRAD) {
          if (a.dOn) {
            // k_divergence_bwd's gather: the -= of cell n - 1_c arrives before the += of cell n itself
            const int in = i - (c == 0), jn = j - (c == 1), kn = k - (c == 2);
            float dc = 0.0f;
            bool ctn = false;
            if (in >= 0 && jn >= 0 && kn >= 0) {
              const float gn = go_cell<IS3D, HASW>(d, a, U, flags, w, in, jn, kn, ctn);
              if (ctn) dc -= gn;
            }
            if (self) dc += go0;
            r = r + dc;
          }
          gU[o + c * d.sc] = r;
        }
      }
    }
  block_sum3_fixed(sp, su, sd, wsum);
  if (threadIdx.x == 0 && threadIdx.y == 0) {
    const long long n = (long long)b * d.Z + k;
    a.sums[n] = sp; a.sums[a.BZ + n] = su; a.sums[2 * a.BZ + n] = sd;
  }
}

// ---- four x-cells per thread ---------------------------------------------------------------------------------------------
// What a thread holds of four cells of one row: the vectors it loaded, the divergence, go = g_div and who contributes
struct Row4 {
  float w[4], ux[4], uy[4], uz[4], dv[4], go[4];
  unsigned ct;     // bit q: cell q contributes (one register: twelve lane masks held across the tile would spill SGPRs)
  int o;           // the row's offset of cell i0 (0 when the row is not read)
};
__device__ __forceinline__ void unpack4(const float4& v, float* r) { r[0] = v.x; r[1] = v.y; r[2] = v.z; r[3] = v.w; }

// cells i0 .. i0 + 3 of row (j, k); in_array: the row exists and the thread's tile is live. EVERY lane of the wave must call
// this (DPP). Every load is unconditional: a row that is not read takes the fields' first vectors.
template <bool IS3D, bool HASW, bool DIV>
__device__ __forceinline__ void crit_row4(const Dom& d, const CriterionArgs& a, const float* __restrict__ U, const float* __restrict__ flags,
                                          const float* __restrict__ w, int i0, int j, int k, bool in_array, Row4& r) {
  const bool inner = in_array && j >= 1 && j <= d.Y - 2 && (!IS3D || (k >= 1 && k <= d.Z - 2));    // rows that hold contributing cells
  r.o = in_array ? TFL_AT(d, i0, j, k) : 0;
  const int o = r.o, oy = inner ? d.sy : 0, oz = inner ? d.sz : 0;
  unpack4(*reinterpret_cast<const float4*>(U + o), r.ux);
  unpack4(*reinterpret_cast<const float4*>(U + (o + d.sc)), r.uy);
  if (IS3D) unpack4(*reinterpret_cast<const float4*>(U + (o + 2 * d.sc)), r.uz);
  if (HASW) unpack4(*reinterpret_cast<const float4*>(w + o), r.w);
  else r.w[0] = r.w[1] = r.w[2] = r.w[3] = 1.0f;
  if (!DIV) return;
  float f[4], uyp[4], uzp[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  unpack4(*reinterpret_cast<const float4*>(flags + o), f);
  unpack4(*reinterpret_cast<const float4*>(U + (o + d.sc + oy)), uyp);
  if (IS3D) unpack4(*reinterpret_cast<const float4*>(U + (o + 2 * d.sc + oz)), uzp);
  r.ct = 0u;
  // the x+1 tap of the segment's last lane (cell X - 1 is a border cell: a row's last float4 needs none)
  const bool seg_last = threadIdx.x == blockDim.x - 1;
  const bool need = inner && seg_last && i0 + 4 < d.X;
  const float uxr = U[need ? o + 4 : 0];
  float uxp[4] = {r.ux[1], r.ux[2], r.ux[3], from_lane_above(r.ux[0])};
  if (seg_last) uxp[3] = uxr;
#pragma unroll
  for (int q = 0; q < 4; q++) {
    const int i = i0 + q;
    const bool ct = inner && i >= 1 && i <= d.X - 2 && (((int)f[q]) & kFluid);
    r.ct |= ct ? 1u << q : 0u;
    float v = 0.0f;
    if (ct) {
      v = r.ux[q] - uxp[q] + r.uy[q] - uyp[q];
      if (IS3D) v += (r.uz[q] - uzp[q]);
    }
    r.dv[q] = v;
    r.go[q] = grad_of(a.normP, r.w[q] * v, r.w[q], a.lamD);
  }
}

// blockDim = (BX, 1024 / BX, 1), BX a power of two <= 32 (a row segment = BX consecutive lanes of one wave); X % 4 == 0 and
// every pointer 16-byte aligned.
template <bool IS3D, bool GRAD, bool HASW>
__global__ __launch_bounds__(kCritThreads) void k_criterion_planes_v4(Dom d, CriterionArgs a) {
  __shared__ double wsum[3][kCritThreads / 64];
  constexpr int C = IS3D ? 3 : 2;
  int b, k; dom_bk(d, b, k);
  const long long cells = (long long)d.sc;
  const float* __restrict__ p = a.p + b * cells; const float* __restrict__ pt = a.pt + b * cells;
  const float* __restrict__ U = a.U + b * cells * C; const float* __restrict__ Ut = a.Ut + b * cells * C;
  const float* __restrict__ flags = a.flags + b * cells;
  const float* __restrict__ w = HASW ? a.w + b * cells : nullptr;
  float* __restrict__ gP = GRAD ? a.gP + b * cells : nullptr;
  float* __restrict__ gU = GRAD ? a.gU + b * cells * C : nullptr;
  const int nti = (d.X / 4 + (int)blockDim.x - 1) / (int)blockDim.x, ntj = (d.Y + (int)blockDim.y - 1) / (int)blockDim.y;
  const int nt = nti * ntj;
  double sp = 0.0, su = 0.0, sd = 0.0;
  for (int t = 0; t < nt; t++) {
    const int tj = t / nti, ti = t - tj * nti;
    const int j = tj * (int)blockDim.y + (int)threadIdx.y;
    const int i0 = (ti * (int)blockDim.x + (int)threadIdx.x) * 4;
    const bool live = i0 < d.X && j < d.Y;
    Row4 s;
    if (a.dOn) crit_row4<IS3D, HASW, true>(d, a, U, flags, w, i0, j, k, live, s);      // (block-uniform)
    else crit_row4<IS3D, HASW, false>(d, a, U, flags, w, i0, j, k, live, s);
    const int o = s.o;
    float pv[4], ptv[4], ut[3][4];
    unpack4(*reinterpret_cast<const float4*>(p + o), pv);
    unpack4(*reinterpret_cast<const float4*>(pt + o), ptv);
#pragma unroll
    for (int c = 0; c < C; c++) unpack4(*reinterpret_cast<const float4*>(Ut + (o + c * d.sc)), ut[c]);
    float gp[4] = {0.0f, 0.0f, 0.0f, 0.0f}, gu[3][4];
#pragma unroll
    for (int q = 0; q < 4; q++) {
      const float wv = s.w[q];
      if (a.pOn) {
        const float x = wv * pv[q], tt = wv * ptv[q], z = x - tt;
        sp += live ? (double)z * (double)z : 0.0;
        gp[q] = grad_of(a.normP, z, wv, a.lamP);
      }
      if (a.dOn) {
        const float zd = wv * s.dv[q];
        sd += live ? (double)zd * (double)zd : 0.0;
      }
#pragma unroll
      for (int c = 0; c < C; c++) {
        float r = 0.0f;
        if (a.uOn) {
          const float uc = c == 0 ? s.ux[q] : (c == 1 ? s.uy[q] : s.uz[q]);
          const float x = wv * uc, tt = wv * ut[c][q], z = x - tt;
          su += live ? (double)z * (double)z : 0.0;
          r = r + grad_of(a.normU, z, wv, a.lamU);
        }
        gu[c][q] = r;
      }
    }
    if (GRAD) {
      if (a.dOn) {
        // go of the -y and -z neighbours: their rows, recomputed (a row below the array is not read and contributes nothing)
        Row4 ry, rz;
        crit_row4<IS3D, HASW, true>(d, a, U, flags, w, i0, j - 1, k, live && j >= 1, ry);
        if (IS3D) crit_row4<IS3D, HASW, true>(d, a, U, flags, w, i0, j, k - 1, live && k >= 1, rz);
        // go of the -x neighbour: the lane below holds it; the first lane of a row segment past column 0 recomputes it
        float gl = from_lane_below(s.go[3]);
        unsigned cl = __builtin_bit_cast(unsigned, from_lane_below(__builtin_bit_cast(float, s.ct))) >> 3;
        if (threadIdx.x == 0) {
          gl = 0.0f; cl = 0u;
          if (live && i0 > 0) {
            bool c1 = false;
            gl = go_cell<IS3D, HASW>(d, a, U, flags, w, i0 - 1, j, k, c1);
            cl = c1 ? 1u : 0u;
          }
        }
#pragma unroll
        for (int q = 0; q < 4; q++) {
          // k_divergence_bwd's gather: the -= of cell n - 1_c arrives before the += of cell n itself
          const float gxl = q == 0 ? gl : s.go[q - 1];
          const bool cxl = ((q == 0 ? cl : s.ct >> (q - 1)) & 1u) != 0u;
          const bool cs = ((s.ct >> q) & 1u) != 0u;
          float dx = 0.0f, dy = 0.0f, dz = 0.0f;
          if (cxl) dx -= gxl;
          if (cs) dx += s.go[q];
          if ((ry.ct >> q) & 1u) dy -= ry.go[q];
          if (cs) dy += s.go[q];
          gu[0][q] = gu[0][q] + dx;
          gu[1][q] = gu[1][q] + dy;
          if (IS3D) {
            if ((rz.ct >> q) & 1u) dz -= rz.go[q];
            if (cs) dz += s.go[q];
            gu[2][q] = gu[2][q] + dz;
          }
        }
      }
      if (live) {
        v4_store(gP, o, gp);
#pragma unroll
        for (int c = 0; c < C; c++) v4_store(gU, o + c * d.sc, gu[c]);
      }
    }
  }
  block_sum3_fixed(sp, su, sd, wsum);
  if (threadIdx.x == 0 && threadIdx.y == 0) {
    const long long n = (long long)b * d.Z + k;
    a.sums[n] = sp; a.sums[a.BZ + n] = su; a.sums[2 * a.BZ + n] = sd;
  }
}

// loss = {pLoss, uLoss, divLoss, (pLoss + uLoss) + divLoss}; term t = lambda_t * (S_t / n_t), S_t = sums[t][0] + ... + sums[t][n - 1]
// in exactly this order (ascending (b, z)); n_t = 1 without sizeAverage; 0 for a term that is off
__global__ __launch_bounds__(256) void k_criterion_finish(const double* __restrict__ sums, long long n, CriterionFinish f,
                                                          double* __restrict__ loss) {
  __shared__ double part[3][256];
  double acc = 0.0;
  for (long long base = 0; base < n; base += 256) {
    const int m = n - base < 256 ? (int)(n - base) : 256;
    if ((int)threadIdx.x < m) {
#pragma unroll
      for (int t = 0; t < 3; t++) part[t][threadIdx.x] = sums[t * n + base + threadIdx.x];
    }
    __syncthreads();
    if (threadIdx.x < 3) {
#pragma unroll 16
      for (int t = 0; t < m; t++) acc += part[threadIdx.x][t];      // (lanes 0..2 run the three sums side by side, each in order)
    }
    __syncthreads();
  }
  if (threadIdx.x < 3) part[threadIdx.x][0] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    const double pl = f.on[0] ? f.lambda[0] * (part[0][0] / f.n[0]) : 0.0;
    const double ul = f.on[1] ? f.lambda[1] * (part[1][0] / f.n[1]) : 0.0;
    const double dl = f.on[2] ? f.lambda[2] * (part[2][0] / f.n[2]) : 0.0;
    loss[0] = pl; loss[1] = ul; loss[2] = dl; loss[3] = (pl + ul) + dl;
  }
}

// run_epoch.lua:216-229, 287-291 without the host read: the epoch's running sums {p, u, div, total, long-term total} take one
// criterion result, and the guard word is set (and stays set) when the total is NaN or above errLimit. One thread, plain
// fp64 adds in the order written here.
__global__ void k_closure_fold(const double* __restrict__ loss4, double* __restrict__ sums5, int* __restrict__ guard, int longTerm,
                               double errLimit) {
  const double total = loss4[3];
  if (longTerm) {
    sums5[3] = sums5[3] + total;
    sums5[4] = sums5[4] + total;
  } else {
    sums5[0] = sums5[0] + loss4[0];
    sums5[1] = sums5[1] + loss4[1];
    sums5[2] = sums5[2] + loss4[2];
    sums5[3] = sums5[3] + total;
  }
  if (total != total || total > errLimit) *guard = 1;
}

// fluid_criterion.lua:149-157 per cell, one fp32 rounding per Lua call
__global__ __launch_bounds__(256) void k_criterion_weight(int rad, float bw, float m, float s, int Z, int Y, int X,
                                                          const float* __restrict__ flags, float* __restrict__ w) {
  const int x = blockIdx.x * blockDim.x + threadIdx.x;
  const int y = blockIdx.y * blockDim.y + threadIdx.y;
  const int b = blockIdx.z / Z, z = blockIdx.z - b * Z;
  if (x >= X || y >= Y) return;
  const long long N = (long long)Z * Y * X;
  float c = signed_distance_at(rad, Z, Y, X, flags + b * N, x, y, z);
  c = stdmin(stdmax(c, 1.0f), bw);      // :clamp(1, borderWidth)
  c = c + (-1.0f);                      // :add(-1)
  c = c * m;                            // :mul(-1 / (borderWidth - 1))
  c = c + 1.0f;                         // :add(1)
  c = c * s;                            // :mul(borderWeight - 1)
  w[b * N + (long long)z * Y * X + (long long)y * X + x] = c + 1.0f;      // :add(1)
}

template <bool IS3D, bool GRAD>
void launch_planes(hipStream_t st, int B, const Dom& d, const CriterionArgs& a) {
  const dim3 grd(1, 1, (unsigned)(d.nw * B));
  const Vec4Launch v = vec4_launch(B, d, {a.p, a.pt, a.U, a.Ut, a.flags, a.w, a.gP, a.gU});      // (its row-segment width and its refusals; the block is ours)
  TFL_TIMED_EXT("k_criterion_planes", st);
  if (v.ok) {
    const dim3 blk(v.blk.x, kCritThreads / v.blk.x, 1);
    if (a.w) TFL_LAUNCH_EXT((k_criterion_planes_v4<IS3D, GRAD, true>), grd, blk, 0, st, d, a);
    else TFL_LAUNCH_EXT((k_criterion_planes_v4<IS3D, GRAD, false>), grd, blk, 0, st, d, a);
    return;
  }
  const dim3 blk(64, kCritThreads / 64, 1);
  if (a.w) TFL_LAUNCH_EXT((k_criterion_planes_c1<IS3D, GRAD, true>), grd, blk, 0, st, d, a);
  else TFL_LAUNCH_EXT((k_criterion_planes_c1<IS3D, GRAD, false>), grd, blk, 0, st, d, a);
}

}  // namespace

void criterion_weight(hipStream_t st, int B, int Z, int Y, int X, int rad, float bw, float m, float s, const float* flags, float* w) {
  const dim3 blk(64, 4, 1), grd((X + 63) / 64, (Y + 3) / 4, (unsigned)(Z * B));
  TFL_TIMED("k_criterion_weight", st);
  k_criterion_weight<<<grd, blk, 0, st>>>(rad, bw, m, s, Z, Y, X, flags, w);
}

void criterion_planes(hipStream_t st, bool is3d, int B, int Z, int Y, int X, const CriterionArgs& a) {
  const Dom d = whole_dom(Z, Y, X);
  const bool grad = a.gP != nullptr;
  if (is3d) { if (grad) launch_planes<true, true>(st, B, d, a); else launch_planes<true, false>(st, B, d, a); }
  else { if (grad) launch_planes<false, true>(st, B, d, a); else launch_planes<false, false>(st, B, d, a); }
}

void criterion_finish(hipStream_t st, long long n, const double* sums, const CriterionFinish& f, double* loss) {
  TFL_TIMED_EXT("k_criterion_finish", st);
  TFL_LAUNCH_EXT(k_criterion_finish, 1, 256, 0, st, sums, n, f, loss);
}

void closure_fold(hipStream_t st, const double* loss4, double* sums5, int* guard, int longTerm, double errLimit) {
  TFL_TIMED("k_closure_fold", st);
  hipLaunchKernelGGL(k_closure_fold, dim3(1), dim3(1), 0, st, loss4, sums5, guard, longTerm, errLimit);
}

}  // namespace tfl
