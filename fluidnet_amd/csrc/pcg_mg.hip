// pcg_mg.hip -- the multigrid preconditioner of solveLinearSystemPCG (precondType = "mg", gfx950): one symmetric V-cycle of
// aggregation multigrid per CG iteration, matrix-free from the flag grid. The scheme, its parameters, the level geometry and the
// child / parent maps: tfl_pcg_mg.hpp. The CG around it and the workspace: pcg.hip (Solve::build_levels / Solve::vcycle).
//
// Every operation on a level is ONE device function over the level's cells, thread t of nt taking the cells t, t + nt, ...:
//   mg_first     z = omega r / diag                                      (the first sweep of a level, from z = 0)
//   mg_sweep     z' = z + omega (r - A z) / diag                         (damped Jacobi, ping-pong between za and zb)
//                with PROLONG the sweep reads z + alpha P z_c in place of z: the prolongation costs no pass of its own
//   mg_restrict  r_c = P^T (r - A z): a coarse thread forms the residual of its 2^dim children and sums them in the order of
//                mg_child; no residual array is written
//   mg_galerkin  diag, 1 / diag and the plus-face couplings of a coarse level from the finer one (set-up)
// A CLOSED component (no cell of it has an empty neighbour) has a singular matrix with the constants as its null space, and CG keeps
// r orthogonal to them only up to rounding. Any good approximation of A^-1 amplifies that residue far more than the rest of r --
// the better the preconditioner, the more -- and in fp32 the residue then sets the residual CG can reach (measured on the
// restatement: about 1e-5 at |b| = 100 and drifting upwards afterwards, against 1e-6 and stable without it;
// profiles/pcg_mg.md). So for a closed component the cycle's right-hand side is r minus its mean over the component: the
// identity in exact arithmetic, one fixed-order fp64 reduction (k_mg_rsum) folded by the first sweep of level 0 (k_mg_first0),
// which writes that right-hand side to the idle w. An open component (some cell next to an empty one) is cycled as it stands,
// straight from r, without either: the host reads the set-up's "open" word once per component.
// A cell's value never depends on which thread computes it, so a level gives the same bits whether a chip-wide launch or the
// single-block kernel runs it. No block waits for another one: levels of more than kMgBlockCells cells run one launch per
// operation (k_mg_first / k_mg_sweep / k_mg_restrict), and ALL smaller levels run inside ONE launch of one block (k_mg_coarse),
// which walks down and up the hierarchy with __syncthreads() between operations (the expectation: below that size a launch
// costs more than the work it starts; the threshold kMgBlockCells has not been varied, profiles/pcg_mg.md). Neighbours are loaded unconditionally from a clamped index and dropped by a select. No atomics,
// fixed summation orders: bit-reproducible. Every per-application kernel returns at once when the CG state says `done`.
#include "tfl_device.hpp"
#include "tfl_host.hpp"
#include "tfl_pcg_mg.hpp"
#include "tfl_pcg_ws.hpp"

namespace tfl {

namespace {

static_assert(kMgNu % 2 == 0, "pre- and post-smoothing end in zb: an even number of sweeps");
constexpr int kMgBlockThreads = 1024;

// fixed-order reductions, as pcg.hip's: per block, then the kRedBlocks partial sums by every block that needs the total
__device__ __forceinline__ void mg_block_partial(double v, double* __restrict__ partials) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  __shared__ double part[4];
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0) partials[blockIdx.x] = (part[0] + part[1]) + (part[2] + part[3]);
}
__device__ __forceinline__ double mg_reduce_partials(const double* __restrict__ partials) {   // one block of 256
  double v = 0.0;
  for (int t = threadIdx.x; t < kRedBlocks; t += 256) v += partials[t];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  __shared__ double part[4];
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
  __syncthreads();
  return (part[0] + part[1]) + (part[2] + part[3]);
}

__device__ __forceinline__ void mg_cell(const MgLv& L, int o, int& k, int& j, int& i) {
  i = o % L.g.X; j = (o / L.g.X) % L.g.Y; k = o / (L.g.X * L.g.Y);
}

// r - A z at cell o = (k, j, i) of level L, z from `zin`; with PROLONG z is zin + alpha * zc[parent] on the cells with diag != 0.
// Returns z(o) in `z0`. Subtraction order: x plus, x minus, y plus, y minus, z plus, z minus (tests/pcg_mg_ref64.py _apply).
template <bool IS3D, bool PROLONG>
__device__ __forceinline__ float mg_residual(const MgLv& L, const float* __restrict__ zin, const float* __restrict__ zc,
                                             const MgLevelGeom& cg, int o, int k, int j, int i, float& z0) {
  const int sy = L.g.X, sz = L.g.X * L.g.Y;
  const bool xm = i > 0, xp = i < L.g.X - 1, ym = j > 0, yp = j < L.g.Y - 1, zm = IS3D && k > 0, zp = IS3D && k < L.g.Z - 1;
  // neighbour q: 0 x+, 1 x-, 2 y+, 3 y-, 4 z+, 5 z-; a missing one reads the cell itself with coupling 0
  const int nb[6] = {xp ? o + 1 : o, xm ? o - 1 : o, yp ? o + sy : o, ym ? o - sy : o, zp ? o + sz : o, zm ? o - sz : o};
  const int dk[6] = {0, 0, 0, 0, 1, -1}, dj[6] = {0, 0, 1, -1, 0, 0}, di[6] = {1, -1, 0, 0, 0, 0};
  const bool has[6] = {xp, xm, yp, ym, zp, zm};
  float c[6], zn[6];
  c[0] = L.cx[o]; c[1] = L.cx[nb[1]]; c[2] = L.cy[o]; c[3] = L.cy[nb[3]];
  c[4] = IS3D ? L.cz[o] : 0.0f; c[5] = IS3D ? L.cz[nb[5]] : 0.0f;
#pragma unroll
  for (int q = 0; q < 6; q++) {
    if (!IS3D && q >= 4) { zn[q] = 0.0f; continue; }
    float v = zin[nb[q]];
    if (PROLONG) {
      const int kk = has[q] ? k + dk[q] : k, jj = has[q] ? j + dj[q] : j, ii = has[q] ? i + di[q] : i;
      const float up = zc[mg_parent(cg, IS3D, kk, jj, ii)], m = L.invd[nb[q]] != 0.0f ? 1.0f : 0.0f;
      v = v + (kMgAlpha * up) * m;
    }
    zn[q] = v;
    if (!has[q]) c[q] = 0.0f;
  }
  float zv = zin[o];
  if (PROLONG) {
    const float up = zc[mg_parent(cg, IS3D, k, j, i)], m = L.invd[o] != 0.0f ? 1.0f : 0.0f;
    zv = zv + (kMgAlpha * up) * m;
  }
  float az = L.diag[o] * zv;
#pragma unroll
  for (int q = 0; q < 6; q++) {
    if (!IS3D && q >= 4) continue;
    az -= c[q] * zn[q];
  }
  z0 = zv;
  return L.r[o] - az;
}

__device__ __forceinline__ void mg_first(const MgLv& L, float* __restrict__ zout, int t, int nt) {
  for (int o = t; o < L.n; o += nt) zout[o] = (kMgOmega * L.invd[o]) * L.r[o];
}

template <bool IS3D, bool PROLONG>
__device__ __forceinline__ void mg_sweep(const MgLv& L, const float* __restrict__ zin, float* __restrict__ zout,
                                         const float* __restrict__ zc, const MgLevelGeom& cg, int t, int nt) {
  for (int o = t; o < L.n; o += nt) {
    int k, j, i;
    mg_cell(L, o, k, j, i);
    float z0;
    const float res = mg_residual<IS3D, PROLONG>(L, zin, zc, cg, o, k, j, i, z0);
    zout[o] = z0 + (kMgOmega * L.invd[o]) * res;
  }
}

// r of the coarse level C from r and zb of the fine level F
template <bool IS3D>
__device__ __forceinline__ void mg_restrict(const MgLv& F, const MgLv& C, int t, int nt) {
  for (int O = t; O < C.n; O += nt) {
    int K, J, I;
    mg_cell(C, O, K, J, I);
    float acc = 0.0f;
#pragma unroll
    for (int q = 0; q < (IS3D ? 8 : 4); q++) {
      int k, j, i;
      const bool there = mg_child(F.g, IS3D, K, J, I, q, k, j, i);
      k = min(k, F.g.Z - 1); j = min(j, F.g.Y - 1); i = min(i, F.g.X - 1);      // a child outside the grid: a cell inside, dropped
      float z0;
      const float res = mg_residual<IS3D, false>(F, F.zb, nullptr, C.g, (k * F.g.Y + j) * F.g.X + i, k, j, i, z0);
      acc += there ? res : 0.0f;
    }
    C.r[O] = acc;
  }
}

// the Galerkin product P^T A P of piecewise-constant P, coarse cell by coarse cell
template <bool IS3D>
__device__ __forceinline__ void mg_galerkin(const MgLv& F, const MgLv& C, int t, int nt) {
  for (int O = t; O < C.n; O += nt) {
    int K, J, I;
    mg_cell(C, O, K, J, I);
    float diag = 0.0f, inner = 0.0f, cx = 0.0f, cy = 0.0f, cz = 0.0f;
#pragma unroll
    for (int q = 0; q < (IS3D ? 8 : 4); q++) {
      int k, j, i;
      const bool there = mg_child(F.g, IS3D, K, J, I, q, k, j, i);
      k = min(k, F.g.Z - 1); j = min(j, F.g.Y - 1); i = min(i, F.g.X - 1);
      const int o = (k * F.g.Y + j) * F.g.X + i;
      const float m = there ? 1.0f : 0.0f;
      const float fd = F.diag[o] * m, fx = F.cx[o] * m, fy = F.cy[o] * m, fz = IS3D ? F.cz[o] * m : 0.0f;
      diag += fd;
      // a plus face of a lower child lies inside the aggregate, that of an upper child crosses into the next one
      if (q & 1) cx += fx; else inner += fx;
      if (q & 2) cy += fy; else inner += fy;
      if (IS3D) { if (q & 4) cz += fz; else inner += fz; }
    }
    diag = diag - 2.0f * inner;
    C.diag[O] = diag;
    C.invd[O] = diag > 0.0f ? 1.0f / diag : 0.0f;
    C.cx[O] = cx; C.cy[O] = cy; C.cz[O] = cz;
  }
}

// ---- set-up ---------------------------------------------------------------------------------------------------------------
// level 0 from the flags and the component's label: diag as k_pcg_apply forms it (0 off the component)
// *open = 1 when a cell of the component has an empty neighbour (every thread that sees one stores the same word)
template <bool IS3D>
__device__ __forceinline__ void d_mg_level0(Dom d, const float* __restrict__ flags, const int* __restrict__ label, int root, MgLv L,
                                                   int* __restrict__ open) {
  for (long long o = (long long)blockIdx.x * 256 + threadIdx.x; o < d.sc; o += (long long)gridDim.x * 256) {
    const bool in = label[o] == root;       // (a component's cell is never on the border: all six neighbours exist)
    const int nb[6] = {(int)o - d.sz, (int)o - d.sy, (int)o - 1, (int)o + 1, (int)o + d.sy, (int)o + d.sz};
    float diag = 0.0f, coupled = 0.0f, c[6];
#pragma unroll
    for (int q = 0; q < 6; q++) {
      c[q] = 0.0f;
      if (!IS3D && (q == 0 || q == 5)) continue;
      const long long e = in ? (long long)nb[q] : o;
      const int f = (int)flags[e];
      const int l = label[e];
      if (!(f & kObstacle)) diag += 1.0f;
      c[q] = (in && l == root) ? 1.0f : 0.0f;
      coupled += c[q];
    }
    diag = in ? diag : 0.0f;
    if (in && diag != coupled) *open = 1;
    L.diag[o] = diag;
    L.invd[o] = diag > 0.0f ? 1.0f / diag : 0.0f;
    L.cx[o] = c[3]; L.cy[o] = c[4]; L.cz[o] = c[5];
  }
}
template <bool IS3D>
__global__ __launch_bounds__(256) void k_mg_level0(Dom d, const float* __restrict__ flags, const int* __restrict__ label, int root, MgLv L,
                                                   int* __restrict__ open) { d_mg_level0<IS3D>(d, flags, label, root, L, open); }
template <bool IS3D>
__global__ __launch_bounds__(256) void k_mg_galerkin(MgLv F, MgLv C) {
  mg_galerkin<IS3D>(F, C, blockIdx.x * 256 + threadIdx.x, gridDim.x * 256);
}

// ---- the batch view (solveLinearSystemPCGBatched) ---------------------------------------------------------------------------
// The kernels below (k_*_b) run the same device functions with the batch item in blockIdx.y: item b's arrays lie b * stride floats
// behind item 0's, and what the host decides per component above (is there a system, is it preconditioned, is it closed) is
// read from the item's record. Level 0's right-hand side is the idle w (r0) when the component is closed, else the CG's r.
__device__ __forceinline__ MgLv mg_at(const MgLv& L, long long off, float* r0 = nullptr) {
  return MgLv{L.g, L.n, L.diag + off, L.invd + off, L.cx + off, L.cy + off, L.cz + off, r0 ? r0 : L.r + off, L.za + off, L.zb + off};
}
struct MgItem { bool run; long long off; const PcgState* S; int size; bool closed; };
// set-up kernels run for every mg system of the round; per-application kernels only until its CG is done
__device__ __forceinline__ MgItem mg_item(const PcgBatch& bt, bool setup) {
  const int b = blockIdx.y;
  const PcgItemRec& rc = bt.rec[b];
  MgItem it;
  it.off = (long long)b * bt.stride; it.S = pcg_state_of(bt, b); it.size = rc.size; it.closed = rc.open == 0;
  it.run = rc.active && rc.pc == 3 && (setup || !it.S->done);
  return it;
}
// the level-0 right-hand side of item `it`: w0 is item 0's w, null for any other level
__device__ __forceinline__ float* mg_rhs0(const MgItem& it, float* w0) { return (w0 && it.closed) ? w0 + it.off : nullptr; }

template <bool IS3D>
__global__ __launch_bounds__(256) void k_mg_level0_b(PcgBatch bt, Dom d, const float* __restrict__ flags, const int* __restrict__ label, MgLv L) {
  const MgItem it = mg_item(bt, true);
  if (!it.run) return;
  PcgItemRec& rc = bt.rec[blockIdx.y];
  d_mg_level0<IS3D>(d, flags + (long long)blockIdx.y * d.sc, label + it.off, rc.root, mg_at(L, it.off), &rc.open);
}
template <bool IS3D>
__global__ __launch_bounds__(256) void k_mg_galerkin_b(PcgBatch bt, MgLv F, MgLv C) {
  const MgItem it = mg_item(bt, true);
  if (!it.run) return;
  mg_galerkin<IS3D>(mg_at(F, it.off), mg_at(C, it.off), blockIdx.x * 256 + threadIdx.x, gridDim.x * 256);
}

// ---- one application ------------------------------------------------------------------------------------------------------
// the partial sums of r over the grid (r is 0 off the component)
__device__ __forceinline__ void d_mg_rsum(const PcgState* __restrict__ S, int n, const float* __restrict__ r, double* __restrict__ partials) {
  if (S->done) return;
  double acc = 0.0;
  for (int o = blockIdx.x * 256 + threadIdx.x; o < n; o += gridDim.x * 256) acc += (double)r[o];
  mg_block_partial(acc, partials);
}
// the first sweep of level 0 of a closed component: the cycle's right-hand side L.r = r - mean of r, and z = omega L.r / diag
__device__ __forceinline__ void d_mg_first0(const PcgState* __restrict__ S, MgLv L, const float* __restrict__ r,
                                                   const double* __restrict__ partials, int size, float* __restrict__ zout) {
  if (S->done) return;
  const double sum = mg_reduce_partials(partials);
  const float mean = (float)(sum / (double)size);
  for (int o = blockIdx.x * 256 + threadIdx.x; o < L.n; o += gridDim.x * 256) {
    const float invd = L.invd[o];
    const float v = r[o] - (invd != 0.0f ? mean : 0.0f);
    L.r[o] = v;
    zout[o] = (kMgOmega * invd) * v;
  }
}
__global__ __launch_bounds__(256) void k_mg_rsum(const PcgState* __restrict__ S, int n, const float* __restrict__ r, double* __restrict__ partials) {
  d_mg_rsum(S, n, r, partials);
}
__global__ __launch_bounds__(256) void k_mg_first0(const PcgState* __restrict__ S, MgLv L, const float* __restrict__ r,
                                                   const double* __restrict__ partials, int size, float* __restrict__ zout) {
  d_mg_first0(S, L, r, partials, size, zout);
}
__global__ __launch_bounds__(256) void k_mg_first(const PcgState* __restrict__ S, MgLv L, float* __restrict__ zout) {
  if (S->done) return;
  mg_first(L, zout, blockIdx.x * 256 + threadIdx.x, gridDim.x * 256);
}
template <bool IS3D, bool PROLONG>
__global__ __launch_bounds__(256) void k_mg_sweep(const PcgState* __restrict__ S, MgLv L, const float* __restrict__ zin,
                                                  float* __restrict__ zout, const float* __restrict__ zc, MgLevelGeom cg) {
  if (S->done) return;
  mg_sweep<IS3D, PROLONG>(L, zin, zout, zc, cg, blockIdx.x * 256 + threadIdx.x, gridDim.x * 256);
}
template <bool IS3D>
__global__ __launch_bounds__(256) void k_mg_restrict(const PcgState* __restrict__ S, MgLv F, MgLv C) {
  if (S->done) return;
  mg_restrict<IS3D>(F, C, blockIdx.x * 256 + threadIdx.x, gridDim.x * 256);
}

// `sweeps` sweeps of level L from z = 0 that end in L.zb
template <bool IS3D>
__device__ __forceinline__ void mg_block_smooth_from_zero(const MgLv& L, int sweeps) {
  float* a = (sweeps & 1) ? L.zb : L.za;
  float* b = (sweeps & 1) ? L.za : L.zb;
  mg_first(L, a, threadIdx.x, kMgBlockThreads);
  __syncthreads();
  for (int s = 1; s < sweeps; s++) {
    mg_sweep<IS3D, false>(L, a, b, nullptr, L.g, threadIdx.x, kMgBlockThreads);
    __syncthreads();
    float* t = a; a = b; b = t;
  }
}
// the levels first .. count - 1 of the cycle in one block: r of level `first` from level first - 1, down, the coarsest level, up;
// z of level `first` ends in its zb. Every operation reads what the one before wrote to global memory: a barrier between them.
// The hierarchy is h's, `off` floats on (the batch item); r0: level 0's right-hand side when it is not h's (a closed item).
template <bool IS3D>
__device__ __forceinline__ void mg_coarse(const MgDev& h, int first, long long off, float* r0) {
  const int last = h.count - 1;
  auto lv = [&](int l) { return mg_at(h.lv[l], off, l == 0 ? r0 : nullptr); };
  for (int l = first; l <= last; l++) {
    const MgLv L = lv(l);
    mg_restrict<IS3D>(lv(l - 1), L, threadIdx.x, kMgBlockThreads);
    __syncthreads();
    mg_block_smooth_from_zero<IS3D>(L, l == last ? kMgNuCoarse : kMgNu);
  }
  for (int l = last - 1; l >= first; l--) {
    const MgLv L = lv(l);
    mg_sweep<IS3D, true>(L, L.zb, L.za, h.lv[l + 1].zb + off, h.lv[l + 1].g, threadIdx.x, kMgBlockThreads);
    __syncthreads();
    for (int s = 1; s < kMgNu; s++) {
      mg_sweep<IS3D, false>(L, (s & 1) ? L.za : L.zb, (s & 1) ? L.zb : L.za, nullptr, L.g, threadIdx.x, kMgBlockThreads);
      __syncthreads();
    }
  }
}
template <bool IS3D>
__global__ __launch_bounds__(kMgBlockThreads) void k_mg_coarse(const PcgState* __restrict__ S, MgDev h, int first) {
  if (S->done) return;
  mg_coarse<IS3D>(h, first, 0, nullptr);
}

// the batch forms: one item per blockIdx.y. w0: item 0's w on level 0, null on the other levels (mg_rhs0)
__global__ __launch_bounds__(256) void k_mg_rsum_b(PcgBatch bt, int n, const float* __restrict__ r, double* __restrict__ partials) {
  const MgItem it = mg_item(bt, false);
  if (!it.run || !it.closed) return;
  d_mg_rsum(it.S, n, r + it.off, reinterpret_cast<double*>(reinterpret_cast<float*>(partials) + it.off));
}
// the first sweep of a level; on level 0 of a closed item the one that forms the right-hand side
__global__ __launch_bounds__(256) void k_mg_first_b(PcgBatch bt, MgLv L0, float* w0, const float* __restrict__ r,
                                                    const double* __restrict__ partials, float* __restrict__ zout) {
  const MgItem it = mg_item(bt, false);
  if (!it.run) return;
  float* r0 = mg_rhs0(it, w0);
  const MgLv L = mg_at(L0, it.off, r0);
  if (r0) d_mg_first0(it.S, L, r + it.off, reinterpret_cast<const double*>(reinterpret_cast<const float*>(partials) + it.off), it.size, zout + it.off);
  else mg_first(L, zout + it.off, blockIdx.x * 256 + threadIdx.x, gridDim.x * 256);
}
template <bool IS3D, bool PROLONG>
__global__ __launch_bounds__(256) void k_mg_sweep_b(PcgBatch bt, MgLv L, float* w0, const float* __restrict__ zin,
                                                    float* __restrict__ zout, const float* __restrict__ zc, MgLevelGeom cg) {
  const MgItem it = mg_item(bt, false);
  if (!it.run) return;
  mg_sweep<IS3D, PROLONG>(mg_at(L, it.off, mg_rhs0(it, w0)), zin + it.off, zout + it.off, PROLONG ? zc + it.off : nullptr, cg,
                          blockIdx.x * 256 + threadIdx.x, gridDim.x * 256);
}
template <bool IS3D>
__global__ __launch_bounds__(256) void k_mg_restrict_b(PcgBatch bt, MgLv F, float* w0, MgLv C) {
  const MgItem it = mg_item(bt, false);
  if (!it.run) return;
  mg_restrict<IS3D>(mg_at(F, it.off, mg_rhs0(it, w0)), mg_at(C, it.off), blockIdx.x * 256 + threadIdx.x, gridDim.x * 256);
}
template <bool IS3D>
__global__ __launch_bounds__(kMgBlockThreads) void k_mg_coarse_b(PcgBatch bt, MgDev h, float* w0, int first) {
  const MgItem it = mg_item(bt, false);
  if (!it.run) return;
  mg_coarse<IS3D>(h, first, it.off, mg_rhs0(it, w0));
}

inline int mg_grid(long long n) { return (int)((n + 255) / 256); }

template <bool IS3D>
void build_levels(hipStream_t st, const Dom& d, const MgDev& h, const float* flags, const int* label, int root, int* open) {
  (void)hipMemsetAsync(open, 0, sizeof(int), st);
  k_mg_level0<IS3D><<<mg_grid(d.sc), 256, 0, st>>>(d, flags, label, root, h.lv[0], open);
  for (int l = 1; l < h.count; l++) k_mg_galerkin<IS3D><<<mg_grid(h.lv[l].n), 256, 0, st>>>(h.lv[l - 1], h.lv[l]);
}

// what level 0 of a closed component needs besides its arrays: the CG's r, a partial-sum buffer and the component's size
struct MgRhs { const float* r; double* partials; int size; };

// `sweeps` sweeps of a chip-wide level from z = 0 that end in L.zb; rhs: level 0 of a closed component, whose first sweep also
// forms the right-hand side
template <bool IS3D>
void smooth_from_zero(hipStream_t st, const PcgState* S, const MgLv& L, int sweeps, const MgRhs* rhs) {
  float* a = (sweeps & 1) ? L.zb : L.za;
  float* b = (sweeps & 1) ? L.za : L.zb;
  if (rhs) k_mg_first0<<<mg_grid(L.n), 256, 0, st>>>(S, L, rhs->r, rhs->partials, rhs->size, a);
  else k_mg_first<<<mg_grid(L.n), 256, 0, st>>>(S, L, a);
  for (int s = 1; s < sweeps; s++) {
    k_mg_sweep<IS3D, false><<<mg_grid(L.n), 256, 0, st>>>(S, L, a, b, nullptr, L.g);
    std::swap(a, b);
  }
}

template <bool IS3D>
void vcycle(hipStream_t st, const MgDev& h, const PcgState* S, const MgRhs* rhs) {
  if (rhs) k_mg_rsum<<<kRedBlocks, 256, 0, st>>>(S, h.lv[0].n, rhs->r, rhs->partials);
  const int last = h.count - 1, fb = h.first_block_level;      // levels [fb, count) belong to k_mg_coarse
  const int wide = std::min(fb, h.count);                      // levels [0, wide) run one launch per operation
  for (int l = 0; l < wide; l++) {
    if (l > 0) k_mg_restrict<IS3D><<<mg_grid(h.lv[l].n), 256, 0, st>>>(S, h.lv[l - 1], h.lv[l]);
    smooth_from_zero<IS3D>(st, S, h.lv[l], l == last ? kMgNuCoarse : kMgNu, l == 0 ? rhs : nullptr);
  }
  if (fb < h.count) k_mg_coarse<IS3D><<<1, kMgBlockThreads, 0, st>>>(S, h, fb);
  for (int l = std::min(wide, last) - 1; l >= 0; l--) {
    const MgLv& L = h.lv[l];
    k_mg_sweep<IS3D, true><<<mg_grid(L.n), 256, 0, st>>>(S, L, L.zb, L.za, h.lv[l + 1].zb, h.lv[l + 1].g);
    for (int s = 1; s < kMgNu; s++)
      k_mg_sweep<IS3D, false><<<mg_grid(L.n), 256, 0, st>>>(S, L, (s & 1) ? L.za : L.zb, (s & 1) ? L.zb : L.za, nullptr, L.g);
  }
}

// ---- the same schedule for a batch: what the host decides above per component (rhs or not) the kernels read per item ---------
template <bool IS3D>
void build_levels_b(hipStream_t st, int B, const PcgBatch& bt, const Dom& d, const MgDev& h, const float* flags, const int* label) {
  k_mg_level0_b<IS3D><<<dim3(mg_grid(d.sc), B), 256, 0, st>>>(bt, d, flags, label, h.lv[0]);
  for (int l = 1; l < h.count; l++) k_mg_galerkin_b<IS3D><<<dim3(mg_grid(h.lv[l].n), B), 256, 0, st>>>(bt, h.lv[l - 1], h.lv[l]);
}
template <bool IS3D>
void vcycle_b(hipStream_t st, int B, const PcgBatch& bt, const MgDev& h, float* w, const float* r, double* partials) {
  auto grid = [B](const MgLv& L) { return dim3(mg_grid(L.n), B); };
  auto w0 = [w](int l) { return l == 0 ? w : nullptr; };
  k_mg_rsum_b<<<dim3(kRedBlocks, B), 256, 0, st>>>(bt, h.lv[0].n, r, partials);
  const int last = h.count - 1, fb = h.first_block_level;
  const int wide = std::min(fb, h.count);
  for (int l = 0; l < wide; l++) {
    const MgLv& L = h.lv[l];
    if (l > 0) k_mg_restrict_b<IS3D><<<grid(L), 256, 0, st>>>(bt, h.lv[l - 1], w0(l - 1), L);
    const int sweeps = l == last ? kMgNuCoarse : kMgNu;
    float* a = (sweeps & 1) ? L.zb : L.za;
    float* b = (sweeps & 1) ? L.za : L.zb;
    k_mg_first_b<<<grid(L), 256, 0, st>>>(bt, L, w0(l), r, partials, a);
    for (int s = 1; s < sweeps; s++) {
      k_mg_sweep_b<IS3D, false><<<grid(L), 256, 0, st>>>(bt, L, w0(l), a, b, nullptr, L.g);
      std::swap(a, b);
    }
  }
  if (fb < h.count) k_mg_coarse_b<IS3D><<<dim3(1, B), kMgBlockThreads, 0, st>>>(bt, h, w, fb);
  for (int l = std::min(wide, last) - 1; l >= 0; l--) {
    const MgLv& L = h.lv[l];
    k_mg_sweep_b<IS3D, true><<<grid(L), 256, 0, st>>>(bt, L, w0(l), L.zb, L.za, h.lv[l + 1].zb, h.lv[l + 1].g);
    for (int s = 1; s < kMgNu; s++)
      k_mg_sweep_b<IS3D, false><<<grid(L), 256, 0, st>>>(bt, L, w0(l), (s & 1) ? L.za : L.zb, (s & 1) ? L.zb : L.za, nullptr, L.g);
  }
}

}  // namespace

void mg_build_levels_batched(hipStream_t st, bool is3d, int B, const PcgBatch& bt, const Dom& d, const MgDev& h, const float* flags,
                             const int* label) {
  if (is3d) build_levels_b<true>(st, B, bt, d, h, flags, label);
  else build_levels_b<false>(st, B, bt, d, h, flags, label);
}
void mg_vcycle_batched(hipStream_t st, bool is3d, int B, const PcgBatch& bt, const MgDev& h, float* w, const float* r, double* partials) {
  if (is3d) vcycle_b<true>(st, B, bt, h, w, r, partials);
  else vcycle_b<false>(st, B, bt, h, w, r, partials);
}

void mg_build_levels(hipStream_t st, const Dom& d, bool is3d, const MgDev& h, const float* flags, const int* label, int root, int* open) {
  if (is3d) build_levels<true>(st, d, h, flags, label, root, open);
  else build_levels<false>(st, d, h, flags, label, root, open);
}

// z = M^-1 r, left in h.lv[0].zb. Open component: h.lv[0].r is the CG's r. Closed component: r is the CG's r and h.lv[0].r the
// array the cycle's right-hand side (r minus its mean) is written to.
void mg_vcycle(hipStream_t st, bool is3d, const MgDev& h, const PcgState* S, bool closed, const float* r, double* partials, int size) {
  const MgRhs rhs{r, partials, size};
  if (is3d) vcycle<true>(st, h, S, closed ? &rhs : nullptr);
  else vcycle<false>(st, h, S, closed ? &rhs : nullptr);
}

}  // namespace tfl
