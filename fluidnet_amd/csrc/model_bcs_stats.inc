// model_bcs_stats.inc -- the three forms of k_bcs_div_stats (scalar, four cells per thread on flag words, four cells per thread
// on wall codes). model.hip includes this file twice: with TFL_BCS_STORE = 1 it defines k_bcs_div_stats, k_bcs_div_stats_v4 and
// k_bcs_div_stats_code, which write SetWallBcs(U) to Ubc; with TFL_BCS_STORE = 0 the same three kernels under the names
// k_..._nostore, which leave Ubc alone (model.hip's header says who launches which). Same loads, masking, divergence, fp64
// sums and summation order in both. One text for both, and kernels rather than a shared device function: as a body inlined into
// two kernels, each form began with a vector load and a full drain of the load queue that the kernels below do not have
// (tests/test_isa_cpu.py counts them).
#if TFL_BCS_STORE
#define TFL_BCS_KERNEL(name) name
#else
#define TFL_BCS_KERNEL(name) name##_nostore
#endif

// partials[block*2 + {0,1}] = this block's sum u, sum u^2 of U_bc (fp64). A second tiny kernel
// (k_reduce_stats) adds the partials of each sample in a fixed order, so the scale is bit-reproducible
// run to run and independent of how the grid is sharded -- no atomics (8192 same-address fp64 atomics
// cost 0.2 ms at 128^3, 10x the kernel itself).
template <bool IS3D, bool FOLD = false>
__global__ __launch_bounds__(256) void TFL_BCS_KERNEL(k_bcs_div_stats)(Dom d, const float* __restrict__ U, const float* __restrict__ flags,
                                                                       float* __restrict__ Ubc, float* __restrict__ div,
                                                                       double* __restrict__ partials, StatTail tl) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const int j = blockIdx.y * blockDim.y + threadIdx.y;
  int b, k; dom_bk(d, b, k);
  const long long cells = d.sc;
  const int C = IS3D ? 3 : 2;
  double s1 = 0.0, s2 = 0.0;
  if (i < d.X && j < d.Y) {
    U += b * cells * C; flags += b * cells; div += b * cells;
    if (TFL_BCS_STORE) Ubc += b * cells * C;
    const int o = TFL_AT(d, i, j, k);
    bool zx, zy, zz;
    wall_zero_mask<IS3D>(d, flags, i, j, k, o, zx, zy, zz);
    const float ux = zx ? 0.0f : U[o];
    const float uy = zy ? 0.0f : U[o + d.sc];
    const float uz = IS3D ? (zz ? 0.0f : U[o + 2 * d.sc]) : 0.0f;
    if (TFL_BCS_STORE) { Ubc[o] = ux; Ubc[o + d.sc] = uy; if (IS3D) Ubc[o + 2 * d.sc] = uz; }
    s1 = (double)ux + (double)uy + (double)uz;
    s2 = (double)ux * ux + (double)uy * uy + (double)uz * uz;
    float dv = 0.0f;  // velocityDivergenceForward on U_bc, tfluids.cc:1008-1066
    if (!on_border<IS3D>(d, i, j, k) && (((int)flags[o]) & kFluid)) {
      dv = ux - u_bc_at<IS3D, 0>(d, U, flags, i + 1, j, k) + uy - u_bc_at<IS3D, 1>(d, U, flags, i, j + 1, k);
      if (IS3D) dv += (uz - u_bc_at<IS3D, 2>(d, U, flags, i, j, k + 1));
    }
    div[o] = dv;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) { s1 += __shfl_down(s1, off, 64); s2 += __shfl_down(s2, off, 64); }
  __shared__ double part[8];
  const int tid = threadIdx.y * blockDim.x + threadIdx.x;
  if ((tid & 63) == 0) { part[(tid >> 6) * 2] = s1; part[(tid >> 6) * 2 + 1] = s2; }
  __syncthreads();
  const long long blk = blockIdx.x + (long long)gridDim.x * (blockIdx.y + (long long)gridDim.y * ((long long)b * d.Z + k));
  publish_and_maybe_reduce<FOLD>(tl, partials, blk, (part[0] + part[2]) + (part[4] + part[6]), (part[1] + part[3]) + (part[5] + part[7]), tid);
}

// k_bcs_div_stats_v4 on wall codes: the same loads of U, the same arithmetic and summation order, the same stores -- the flag
// rows replaced by the code bytes of the cell's row, the row above (y + 1) and the plane above (z + 1)
template <bool IS3D>
__global__ __launch_bounds__(256, TFL_LB_BCS) void TFL_BCS_KERNEL(k_bcs_div_stats_code)(Dom d, const float* __restrict__ U, const unsigned short* __restrict__ code,
                                                                                       float* __restrict__ Ubc, float* __restrict__ div,
                                                                                       double* __restrict__ partials, StatTail tl) {
  const V4Ctx c = v4_ctx(d);
  const int j = blockIdx.y * blockDim.y + threadIdx.y;
  int b, k; dom_bk(d, b, k);
  const bool live = c.i0 < d.X && j < d.Y;
  const long long cells = d.sc;
  const int C = IS3D ? 3 : 2;
  U += b * cells * C; code += b * cells; div += b * cells;
  if (TFL_BCS_STORE) Ubc += b * cells * C;
  const int o = TFL_AT(d, c.i0, j, k);
  const bool yp = live && j < d.Y - 1, zp = live && IS3D && k < d.Z - 1;
  // unconditional loads (tfl_vec4.hpp): a lane that must not read takes word 0 and drops it
  const unsigned long long cc_v = *reinterpret_cast<const unsigned long long*>(code + (live ? o : 0));      // four 16-bit codes
  const unsigned long long cy_v = *reinterpret_cast<const unsigned long long*>(code + (yp ? o + d.sy : 0));
  const unsigned long long cz_v = *reinterpret_cast<const unsigned long long*>(code + (zp ? o + d.sz : 0));
  const unsigned long long cc = live ? cc_v : 0ull, cy = yp ? cy_v : 0ull, cz = zp ? cz_v : 0ull;
  float u[3][4], uyp[4], uzp[4];
#pragma unroll
  for (int a = 0; a < 3; a++) v4_load(U, o + a * d.sc, live && a < C, 0.0f, u[a]);
  v4_load(U, o + d.sc + d.sy, yp, 0.0f, uyp);
  v4_load(U, o + 2 * d.sc + d.sz, zp, 0.0f, uzp);
  const bool need = c.last && live && c.has_r;
  const int oo = o + 4;
  const unsigned gcode = code[need ? oo : 0];
  const float gu = U[need ? oo : 0];
  double s1 = 0.0, s2 = 0.0;
  float ubx[5];
#pragma unroll
  for (int q = 0; q < 4; q++) {
    const unsigned m = (unsigned)(cc >> (16 * q));
    if (m & 1u) u[0][q] = 0.0f;
    if (m & 2u) u[1][q] = 0.0f;
    if (!IS3D || (m & 4u)) u[2][q] = 0.0f;
    ubx[q] = u[0][q];
    if (live) {
      s1 += (double)u[0][q] + (double)u[1][q] + (double)u[2][q];
      s2 += (double)u[0][q] * u[0][q] + (double)u[1][q] * u[1][q] + (double)u[2][q] * u[2][q];
    }
  }
  ubx[4] = from_lane_above(ubx[0]);
  if (c.last) ubx[4] = (need && !(gcode & 1u)) ? gu : 0.0f;
  float dv[4];
  const bool row_inner = live && j >= 1 && j <= d.Y - 2 && (!IS3D || (k >= 1 && k <= d.Z - 2));
#pragma unroll
  for (int q = 0; q < 4; q++) {
    const int i = c.i0 + q;
    dv[q] = 0.0f;
    if (row_inner && i >= 1 && i <= d.X - 2 && ((unsigned)(cc >> (16 * q)) & 8u)) {   // tfluids.cc:1008-1066 on U_bc
      const float by = ((unsigned)(cy >> (16 * q)) & 2u) ? 0.0f : uyp[q];
      float t = u[0][q] - ubx[q + 1] + u[1][q] - by;
      if (IS3D) {
        const float bz = ((unsigned)(cz >> (16 * q)) & 4u) ? 0.0f : uzp[q];
        t += (u[2][q] - bz);
      }
      dv[q] = t;
    }
  }
  if (live) {
#pragma unroll
    for (int a = 0; a < 3; a++)
      if (TFL_BCS_STORE && a < C) v4_store(Ubc, o + a * d.sc, u[a]);
    v4_store(div, o, dv);
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) { s1 += __shfl_down(s1, off, 64); s2 += __shfl_down(s2, off, 64); }
  __shared__ double part[8];
  const int tid = threadIdx.y * blockDim.x + threadIdx.x;
  if ((tid & 63) == 0) { part[(tid >> 6) * 2] = s1; part[(tid >> 6) * 2 + 1] = s2; }
  __syncthreads();
  const long long blk = blockIdx.x + (long long)gridDim.x * (blockIdx.y + (long long)gridDim.y * ((long long)b * d.Z + k));
  publish_and_maybe_reduce<false>(tl, partials, blk, (part[0] + part[2]) + (part[4] + part[6]), (part[1] + part[3]) + (part[5] + part[7]), tid);
}
template <bool IS3D, bool FOLD = false>
__global__ __launch_bounds__(256, TFL_LB_BCS) void TFL_BCS_KERNEL(k_bcs_div_stats_v4)(Dom d, const float* __restrict__ U, const float* __restrict__ flags,
                                                                          float* __restrict__ Ubc, float* __restrict__ div,
                                                                          double* __restrict__ partials, StatTail tl) {
  const V4Ctx c = v4_ctx(d);
  const int j = blockIdx.y * blockDim.y + threadIdx.y;
  int b, k; dom_bk(d, b, k);
  const bool live = c.i0 < d.X && j < d.Y;
  const long long cells = d.sc;
  const int C = IS3D ? 3 : 2;
  U += b * cells * C; flags += b * cells; div += b * cells;
  if (TFL_BCS_STORE) Ubc += b * cells * C;
  const int o = TFL_AT(d, c.i0, j, k);
  const bool ym = live && j > 0, yp = live && j < d.Y - 1, yp2 = live && j < d.Y - 2;
  const bool zm = live && IS3D && k > 0, zp = live && IS3D && k < d.Z - 1, zp2 = live && IS3D && k < d.Z - 2;
  // flag rows: own (6 wide), y-1, y+1 (6 wide), z-1, z+1 (6 wide); for the +y / +z neighbours' stick tests:
  // (y+2,z), (y+1,z-1), (y+1,z+1), (y,z+2), (y-1,z+1)
  float fc[6], fym[4], fyp[6], fzm[4], fzp[6], fyp2[4], fypzm[4], fypzp[4], fzp2[4], fymzp[4];
  v4_load6<true, true>(c, flags, o, live, 0.0f, fc);
  v4_load(flags, o - d.sy, ym, 0.0f, fym);
  v4_load6<true, true>(c, flags, o + d.sy, yp, 0.0f, fyp);
  v4_load(flags, o - d.sz, zm, 0.0f, fzm);
  v4_load6<true, true>(c, flags, o + d.sz, zp, 0.0f, fzp);
  v4_load(flags, o + 2 * d.sy, yp2, 0.0f, fyp2);
  v4_load(flags, o + d.sy - d.sz, yp && zm, 0.0f, fypzm);
  v4_load(flags, o + d.sy + d.sz, yp && zp, 0.0f, fypzp);
  v4_load(flags, o + 2 * d.sz, zp2, 0.0f, fzp2);
  v4_load(flags, o - d.sy + d.sz, ym && zp, 0.0f, fymzp);
  float u[3][4], uyp[4], uzp[4];
#pragma unroll
  for (int a = 0; a < 3; a++) v4_load(U, o + a * d.sc, live && a < C, 0.0f, u[a]);
  v4_load(U, o + d.sc + d.sy, yp, 0.0f, uyp);
  v4_load(U, o + 2 * d.sc + d.sz, zp, 0.0f, uzp);
  // what the last lane of a row segment needs of cell i0 + 4 (its wall-BC mask and U.x): issued here, with the row loads
  // (loads unconditional, tfl_vec4.hpp v4_load: every lane reads -- the lanes that need nothing, cell 0 of the field)
  const bool need = c.last && live && c.has_r;
  const int oo = o + 4;
  const float gym = flags[need && ym ? oo - d.sy : 0], gyp = flags[need && yp ? oo + d.sy : 0];
  const float gzm = flags[need && zm ? oo - d.sz : 0], gzp = flags[need && zp ? oo + d.sz : 0];
  const float gu = U[need ? oo : 0];
  // own cells
  double s1 = 0.0, s2 = 0.0;
  float ubx[5];
#pragma unroll
  for (int q = 0; q < 4; q++) {
    bool zx, zy, zz;
    wall_mask_from<IS3D>((int)fc[q + 1], (int)fc[q], (int)fc[q + 2], (int)fym[q], (int)fyp[q + 1], (int)fzm[q], (int)fzp[q + 1],
                         zx, zy, zz);
    if (zx) u[0][q] = 0.0f;
    if (zy) u[1][q] = 0.0f;
    if (!IS3D || zz) u[2][q] = 0.0f;
    ubx[q] = u[0][q];
    if (live) {
      s1 += (double)u[0][q] + (double)u[1][q] + (double)u[2][q];
      s2 += (double)u[0][q] * u[0][q] + (double)u[1][q] * u[1][q] + (double)u[2][q] * u[2][q];
    }
  }
  // U_bc.x of cell i0+4: the next lane's first cell, or (segment end) rebuilt from memory
  ubx[4] = from_lane_above(ubx[0]);
  {
    if (c.last) {
      float v = 0.0f;
      if (need) {
        const int f = (int)fc[5];
        bool zx, zy, zz;
        wall_mask_from<IS3D>(f, (int)fc[4], 0, ym ? (int)gym : 0, yp ? (int)gyp : 0, zm ? (int)gzm : 0, zp ? (int)gzp : 0, zx, zy, zz);
        v = zx ? 0.0f : gu;
      }
      ubx[4] = v;
    }
  }
  float dv[4];
  const bool row_inner = live && j >= 1 && j <= d.Y - 2 && (!IS3D || (k >= 1 && k <= d.Z - 2));
#pragma unroll
  for (int q = 0; q < 4; q++) {
    const int i = c.i0 + q;
    dv[q] = 0.0f;
    if (row_inner && i >= 1 && i <= d.X - 2 && (((int)fc[q + 1]) & kFluid)) {   // tfluids.cc:1008-1066 on U_bc
      bool zx, zy, zz;
      // +y neighbour (i, j+1, k): its -y neighbour is this cell
      wall_mask_from<IS3D>((int)fyp[q + 1], (int)fyp[q], (int)fyp[q + 2], (int)fc[q + 1], (int)fyp2[q], (int)fypzm[q],
                           (int)fypzp[q], zx, zy, zz);
      const float by = zy ? 0.0f : uyp[q];
      float t = u[0][q] - ubx[q + 1] + u[1][q] - by;
      if (IS3D) {
        // +z neighbour (i, j, k+1): its -z neighbour is this cell
        wall_mask_from<IS3D>((int)fzp[q + 1], (int)fzp[q], (int)fzp[q + 2], (int)fymzp[q], (int)fypzp[q], (int)fc[q + 1],
                             (int)fzp2[q], zx, zy, zz);
        const float bz = zz ? 0.0f : uzp[q];
        t += (u[2][q] - bz);
      }
      dv[q] = t;
    }
  }
  if (live) {
#pragma unroll
    for (int a = 0; a < 3; a++)
      if (TFL_BCS_STORE && a < C) v4_store(Ubc, o + a * d.sc, u[a]);
    v4_store(div, o, dv);
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) { s1 += __shfl_down(s1, off, 64); s2 += __shfl_down(s2, off, 64); }
  __shared__ double part[8];
  const int tid = threadIdx.y * blockDim.x + threadIdx.x;
  if ((tid & 63) == 0) { part[(tid >> 6) * 2] = s1; part[(tid >> 6) * 2 + 1] = s2; }
  __syncthreads();
  const long long blk = blockIdx.x + (long long)gridDim.x * (blockIdx.y + (long long)gridDim.y * ((long long)b * d.Z + k));
  publish_and_maybe_reduce<FOLD>(tl, partials, blk, (part[0] + part[2]) + (part[4] + part[6]), (part[1] + part[3]) + (part[5] + part[7]), tid);
}
#undef TFL_BCS_KERNEL
