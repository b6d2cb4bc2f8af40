// advect_scalar3_sparse.hip -- the in-place maccormackOurs advectScalar of tfl_simulate_step over a DEVICE-BUILT LIST OF THE BRICKS
// AROUND THE SMOKE. After the short path of advect_scalar3.hip a block whose tile holds nothing but
// +0.0 has no arithmetic left, but it still loads 32 / 36 B per cell, waits at its barrier and stores +0.0 over +0.0 -- 96-97 % of
// the blocks of the flagship scene. Here those blocks are never started:
//
//   the scan        per BRICK of 64 x 4 x 4 cells, aligned to the array origin (it holds whole tiles of every block shape the passes
//                   use: PZ = 2 or 4 planes), one tag nz: some word of s in the brick is not the bit pattern +0 -- EVERY cell, fluid,
//                   obstacle or border; -0.0, denormals, NaN and inf set it. Per batch item one tag `fast`: set unless every
//                   velocity word u of the item satisfies fabsf(u * dt) <= 0.9f, an ordered compare (a NaN or inf sets it).
//                   Two forms write the same tags:
//     k_vel3_fwd_scan   PASS A OF advectVel with the scan as a by-product (the step runs it first: simulate.cpp). That pass stages
//                   every word of the same pre-advection U in LDS anyway, and its block (64 x 4 cells x 1 or 2 planes) lies inside
//                   one brick: per cell it tests the three own-cell velocity words from the tile and the own-cell word of s (one
//                   more 4-byte load, asked for with the tile's loads), and after its stores a wave takes two ballots and its first
//                   lane stores at most two tags. The 16 B/cell pass of its own is gone from every step on the lists.
//     k_scal3_scan  one streaming launch over s and U (16 B/cell), a block per brick: where pass A did not take the request (a
//                   gather path) and for every density channel after the first.
//   THE TAGS        are 32-bit words, [B][1 + bricks]: per item `fast`, then one per brick. "Set" means "equals this scan's number":
//                   the stores are plain and idempotent (every wave of a brick may store the same word), nothing is cleared between
//                   scans and no atomic is needed. Why a stale tag never equals the current number: the words are zeroed at
//                   allocation and a scan's number is never 0; a field's scans are numbered 1, 2, 3 ... by the host
//                   (simulate.cpp scal3_sparse_ask / _done: the number advances whenever a scan was launched with it), so every tag
//                   in memory is 0 or the number of an EARLIER scan, smaller than the current one. Before the 32-bit number would
//                   wrap to 0 the host zeroes the words on the stream, ahead of the scan, and starts again from 1: the same
//                   state as after allocation. (A tag that did compare equal by mistake would list a brick too many: time, not bits.)
//   k_scal3_lists   one block per batch item, the brick map as one 32-bit word per (y, z) row of bricks in LDS.
//                   L_B = the bricks within Chebyshev distance 1 of an nz brick, plus the bricks that intersect the box of the
//                   setConstVals pair pass B folds (the first step of a plume has an all-zero density and a non-empty box);
//                   L_A = the bricks within distance 1 of L_B; with `fast` set both are every brick. It writes the two lists in
//                   ascending order and their counts. |L_B|, the brick count, fast, |L_A| and the scan's
//                   number go to a mapped pinned mirror for the host's policy (simulate.cpp), as k_project publishes the reach word:
//                   no copy on the stream. One extra block of pass A writes them, beside the blocks that advect; this kernel itself
//                   only when no pass over the lists follows (a probe).
//   the passes      fixed grids sized from the occupancy query; a block strides over (list entry x tiles per brick) and calls
//                   scal3_fwd_body / scal3_bwd_body of advect_scalar3.hip for each tile (SBlock{-1, x, y, z, true}: the tile itself), with a
//                   barrier between iterations because the LDS tile and the wave verdict words are reused. Same bodies, same
//                   arithmetic, the short path of 3.12 included: most listed tiles are the empty ring around the smoke. Pass A
//                   touches no brick outside L_A, pass B none outside L_B: dst is s, so their words stay the +0.0 they are.
//
// WHY THE SKIPPED BRICKS ARE EXACT. The condition is that every velocity word satisfies |u dt| <= 0.9 as the scan forms it.
//   (1) The displacement of a cell is scale3(centred, -+dt), centred = 0.5 (u + u') of two faces: rounding is monotone, so
//       |fl(0.5 (u + u'))| <= max(|u|, |u'|) and |fl(centred * dt)| <= 0.9f on every axis, for the fast path (trace_fast) and for
//       the generic trace (sl_euler_ours) alike. The generic trace moves at most the displacement's length along its direction and
//       only ever stops short (line_trace), so the end point lies strictly within 1 cell of the centre on every axis: the end cell
//       is within +-1 of the cell.
//   (2) Pass A at cell c: the lerp corners are int(p - 0.5) and the next, within +-1 of c; the 27-tap bounds search (tile or
//       clamp_bounds_global) reaches +-1 around the end cell: pass A reads s within +-2 of c. Pass B at c reads s at c only, fwd
//       within +-1 (tile, halo 1, or the generic sampler) and fwd / bounds at c: within +-2 is a safe bound.
//   (3) So dst(c) depends on the words of s within Chebyshev distance 4 of c, counting every cell, not only fluid ones. A brick is 4
//       cells thick in y and z and 64 in x: "all words of s within +-4 of a cell of the brick" lies inside the brick's 1-ring.
//   (4) If all those words are +0, every branch of the two bodies gives +0 for the cell. Border cell: pass A writes fwd = 0, pass B
//       f + hs (+0 - 0) (hs finite: tfl_simulate_step asks for the lists only with a finite strength). Non-fluid cell: fwd = s = +0,
//       pass B keeps f, clamped to bounds found over +0 taps or kept when there is none. Fluid cell: lerps with weights in [0, 1]
//       and min / max over +0 and masked taps, then 0 + hs (0 - 0) clamped to [0, 0]. The result is +0, which s already holds.
//   (5) Density hidden in an obstacle cell sets nz: the test is on every word (DESIGN.md 3.14 found the case: pass B clamps an
//       obstacle cell to the bounds of the fluid cells around it).
//   (6) A listed pass-B tile reads fwd and bounds of its own cells and fwd within +-1 of them: bricks of the 1-ring of L_B, all in
//       L_A, which pass A has written THIS step. A skipped brick's stale words -- conv activations, the workspace is shared -- are
//       never read. With pass A of advectVel in front, bounds live on the planes pass B of advectVel writes afterwards and fwd
//       behind them (bounds ws[6N, 9N), a three-channel layout per batch item; fwd ws[9N, 10N): simulate.cpp), disjoint from
//       each other and from that pass A's live temporary ws[0, 3N): the same argument there, and the velocity's temporary is
//       not written by the scalar passes.
//   With `fast` set (some |u dt| > 0.9, a NaN, an inf) nothing is skipped.
// TRACE ERRORS. calcLineTrace's invariant paths (tfl_trace_errors) depend on geometry and velocity only, and a cell of a skipped brick
// runs no trace, so it counts none here. In the two full launches such a cell traces only when it is fluid with a component of
// |u dt| in (0.45, 0.9] (below that the short path of 3.12 skips the trace there as well), and the generic trace runs only when its
// end cell is not fluid. That such a sub-cell trace cannot raise an invariant is not proved here: every test and the benchmark hold
// the two counts equal (both 0), and a scene that made the full path count one inside an empty brick would count fewer here.
//
// What is NOT here: the operator entry tfl_advectScalar, the z-slab step, the single-pass method and every other caller of
// advect_scalar3 never ask for the lists. tests/test_scal3_sparse_cpu.py holds the distance-4 bound against the C oracle and pins
// 0.9f and the brick to this file; tests/test_hip_scal3_sparse.py holds the bits.
#include "tfl_advect.hpp"
#include "tfl_fastmath.hpp"

#include <cstdlib>
#include <mutex>

#define TFL_SCAL3_NO_ENTRY
#include "advect_scalar3.hip"      // namespace tfl { namespace { scal3_fwd_body, scal3_bwd_body, Tile, SBlock ... } }
#include "advect_vel3_kernels.hpp" // namespace tfl { namespace { namespace vel3 { vel3_fwd_body, VTile, VBlock ... } } }

namespace tfl {
namespace {

constexpr int kBrickX = 64, kBrickY = 4, kBrickZ = 4;      // = TX x TY x (a multiple of every PZ)
constexpr float kSparseDisp = 0.9f;                         // the bound on |u dt| of the proof above
constexpr int kMaxBrickRows = 4096, kMaxBricksX = 32;       // the lists kernel's LDS map: rows of bricks in (y, z), bricks per row
static_assert(kBrickX == TX && kBrickY == TY, "a brick is whole tiles");

struct Bricks { int nx, ny, nz, rows, n; };
inline Bricks bricks_of(int Z, int Y, int X) {
  Bricks k;
  k.nx = (X + kBrickX - 1) / kBrickX; k.ny = (Y + kBrickY - 1) / kBrickY; k.nz = (Z + kBrickZ - 1) / kBrickZ;
  k.rows = k.ny * k.nz; k.n = k.rows * k.nx;
  return k;
}

__device__ __forceinline__ unsigned too_fast(float u, float dt) { return __builtin_fabsf(u * dt) <= kSparseDisp ? 0u : 1u; }

// V4: X % 4 == 0 and 16-byte aligned arrays -- a thread takes four consecutive x cells of one row of the brick (16 rows of 16
// float4); else one cell of each of the brick's four planes
template <bool V4>
__global__ __launch_bounds__(256) void k_scal3_scan(Dom d, Bricks bk, float dt, unsigned seq, const float* __restrict__ s, const float* __restrict__ U,
                                                    unsigned* __restrict__ nz) {
  __shared__ unsigned wave_flags[4];
  const int b = (int)blockIdx.z / bk.nz, iz = (int)blockIdx.z - b * bk.nz, iy = (int)blockIdx.y, ix = (int)blockIdx.x;
  const long long cells = (long long)d.sc;
  s += b * cells; U += b * cells * 3;
  const int t = (int)threadIdx.x;
  unsigned bits = 0u;
  unsigned over = 0u;
  if (V4) {
    const int r = t >> 4, x = ix * kBrickX + (t & 15) * 4, y = iy * kBrickY + (r & 3), z = iz * kBrickZ + (r >> 2);
    if (x < d.X && y < d.Y && z < d.Z) {      // (X % 4 == 0: the four cells are inside with the first)
      const long long o = x + (long long)y * d.sy + (long long)z * d.sz;
      const uint4 w = *reinterpret_cast<const uint4*>(s + o);
      const float4 u0 = *reinterpret_cast<const float4*>(U + o), u1 = *reinterpret_cast<const float4*>(U + o + cells),
                   u2 = *reinterpret_cast<const float4*>(U + o + 2 * cells);
      bits = w.x | w.y | w.z | w.w;
      over = too_fast(u0.x, dt) | too_fast(u0.y, dt) | too_fast(u0.z, dt) | too_fast(u0.w, dt) |
             too_fast(u1.x, dt) | too_fast(u1.y, dt) | too_fast(u1.z, dt) | too_fast(u1.w, dt) |
             too_fast(u2.x, dt) | too_fast(u2.y, dt) | too_fast(u2.z, dt) | too_fast(u2.w, dt);
    }
  } else {
    const int x = ix * kBrickX + (t & 63), y = iy * kBrickY + (t >> 6);
    if (x < d.X && y < d.Y) {
#pragma unroll
      for (int q = 0; q < kBrickZ; q++) {
        const int z = iz * kBrickZ + q;
        if (z < d.Z) {
          const long long o = x + (long long)y * d.sy + (long long)z * d.sz;
          bits |= __builtin_bit_cast(unsigned, s[o]);
          over |= too_fast(U[o], dt) | too_fast(U[o + cells], dt) | too_fast(U[o + 2 * cells], dt);
        }
      }
    }
  }
  const unsigned f = (__builtin_amdgcn_ballot_w64(bits != 0u) != 0ull ? 1u : 0u) | (__builtin_amdgcn_ballot_w64(over != 0u) != 0ull ? 2u : 0u);
  if ((t & 63) == 0) wave_flags[t >> 6] = f;
  __syncthreads();
  if (t == 0) {
    const unsigned all = wave_flags[0] | wave_flags[1] | wave_flags[2] | wave_flags[3];
    unsigned* tags = nz + (long long)b * (bk.n + 1);
    if (all & 1u) tags[1 + (iz * bk.ny + iy) * bk.nx + ix] = seq;
    if (all & 2u) tags[0] = seq;
  }
}

// ---- the scan as a by-product of pass A of advectVel (advect_vel3_kernels.hpp) ------------------------------------------------------
// The hook of vel3_fwd_body: a block of that pass (64 x 4 cells x KZ planes from an even plane) lies inside ONE brick -- (vb.x, vb.y,
// k / 4) -- and its tile holds the own-cell velocity words of every cell it covers. The lane's words of s (one per plane of the
// block, from a clamped cell: a lane outside the array leaves the body before it looks at them) are asked for before the tile is
// staged. Per cell the lane's two verdicts are folded into two registers; after the block's last store a wave takes one ballot of
// each and its first lane stores at most two tags: x0 + lane grows with the lane and the row is the wave's, so lane 0 is inside
// the array whenever any lane of the wave is. (With the ballots, branches and stores at the top of every plane's iteration the
// two-plane kernel was 10 us slower at 256^3: profiles/scal3_scan_fold.md.)
struct ScanHook {
  static constexpr bool on = true;
  const float* s;
  unsigned* nz;
  unsigned seq;
  int nx, ny;                                 // bricks per row and rows per plane of bricks: the launch's own gridDim.x, gridDim.y
  unsigned w0, w1;
  unsigned long long tags;                    // the item's tags: [0] fast, [1 + brick] nz
  unsigned brick;
  unsigned over;                              // the lane's cells so far: some velocity word too fast
  // (the wave-uniform address, index and number are put into VECTOR registers here, where the stores need them in the end: the
  // body is short of scalar registers -- see the kernels below -- and has vector registers to spare; timed, it makes no difference)
  template <int KZ>
  __device__ __forceinline__ void ask(const Dom& d, int b, int x, int y, int k0, int ix, int iy) {
    static_assert(KZ == 1 || KZ == 2, "one word of s per plane of the block, both planes in one brick");
    // (the row is the wave's: a uniform row pointer and the lane's 32-bit offset, as the tile's own row loads)
    const float* row = s + ((long long)b * d.sc + (long long)y * d.sy);
    w0 = __builtin_bit_cast(unsigned, vel3::ldg(row + (long long)k0 * d.sz, (unsigned)x * 4u));
    w1 = KZ == 2 ? __builtin_bit_cast(unsigned, vel3::ldg(row + (long long)min(k0 + 1, d.Z - 1) * d.sz, (unsigned)x * 4u)) : 0u;
    const int n = nx * ny * ((d.Z + kBrickZ - 1) / kBrickZ);
    tags = (unsigned long long)(nz + (long long)b * (n + 1));
    brick = 1u + (unsigned)(((k0 / kBrickZ) * ny + iy) * nx + ix);
    asm volatile("" : "+v"(tags), "+v"(brick), "+v"(seq));
  }
  // per cell: the lane's verdicts only, a few vector instructions beside the body's own; the ballots, branches and stores wait
  // until the block's results are on their way (finish): nothing of the body waits for them
  __device__ __forceinline__ void cell(int tz, float u0, float u1, float u2, float dt) {
    if (tz != 0) w0 |= w1;
    over |= too_fast(u0, dt) | too_fast(u1, dt) | too_fast(u2, dt);
  }
  __device__ __forceinline__ void finish(int lane) const {
    unsigned* t = reinterpret_cast<unsigned*>(tags);
    if (__builtin_amdgcn_ballot_w64(w0 != 0u) != 0ull) {
      if (lane == 0) t[brick] = seq;
    }
    if (__builtin_amdgcn_ballot_w64(over != 0u) != 0ull) {
      if (lane == 0) t[0] = seq;
    }
  }
};

// (depth 1: the plain kernel takes 100 scalar registers, the most that eight waves per SIMD leave a wave, and with the hook the
// allocator, left alone, takes 102 in the generic trace of the rare slow lanes: seven waves. Capped at 100 it fits in 98 with no
// spill: 63 VGPRs, 8 waves (the plain kernel: 54, 8). The cap must be a literal, so the four instances are written out)
template <int KZ, bool FAST>
__global__ void k_vel3_fwd_scan(AdvArgs a, const float* __restrict__ U, const float* __restrict__ flags, float* __restrict__ out,
                                const float* __restrict__ s, unsigned* __restrict__ nz, unsigned seq);
#define TFL_VEL3_FWD_SCAN(KZ, FAST, CAP)                                                                                                  \
  template <>                                                                                                                              \
  __global__ __launch_bounds__(256) CAP void k_vel3_fwd_scan<KZ, FAST>(AdvArgs a, const float* __restrict__ U, const float* __restrict__ flags, \
                                                                       float* __restrict__ out, const float* __restrict__ s,              \
                                                                       unsigned* __restrict__ nz, unsigned seq) {                          \
    __shared__ float tile[4 * vel3::VTile<KZ>::LN];                                                                                        \
    vel3::vel3_fwd_body<KZ, FAST, ScanHook>(vel3::own_block(), tile, a, U, flags, out,                                                     \
                                            ScanHook{s, nz, seq, (int)gridDim.x, (int)gridDim.y, 0u, 0u, 0ull, 0u, 0u});                       \
  }
TFL_VEL3_FWD_SCAN(1, true, __attribute__((amdgpu_num_sgpr(100))))
TFL_VEL3_FWD_SCAN(1, false, __attribute__((amdgpu_num_sgpr(100))))
TFL_VEL3_FWD_SCAN(2, true, )
TFL_VEL3_FWD_SCAN(2, false, )
#undef TFL_VEL3_FWD_SCAN

constexpr int kListThreads = 1024;

// dst[r] = the row's bricks within Chebyshev distance 1 of a brick of src (rows are (iy, iz) = (r % ny, r / ny)), plus `extra` on
// the rows [ey0, ey1] x [ez0, ez1]; every brick when all is set
__device__ __forceinline__ void dilate_rows(const unsigned* __restrict__ src, unsigned* __restrict__ dst, const Bricks& bk, unsigned full,
                                            bool all, unsigned extra, int ey0, int ey1, int ez0, int ez1, int t) {
  for (int r = t; r < bk.rows; r += kListThreads) {
    const int iz = r / bk.ny, iy = r - iz * bk.ny;
    unsigned acc = 0u;
#pragma unroll
    for (int dz = -1; dz <= 1; dz++)
#pragma unroll
      for (int dy = -1; dy <= 1; dy++) {
        const int zz = iz + dz, yy = iy + dy;
        if (zz >= 0 && zz < bk.nz && yy >= 0 && yy < bk.ny) acc |= src[zz * bk.ny + yy];
      }
    unsigned w = (acc | (acc << 1) | (acc >> 1)) & full;
    if (iy >= ey0 && iy <= ey1 && iz >= ez0 && iz <= ez1) w |= extra;
    dst[r] = all ? full : w;
  }
}

// the set bricks of rows[] in ascending order into out[]; returns their number (every thread). A thread takes a contiguous run of
// rows; the runs' counts are summed in order by a wave scan and the waves' totals.
__device__ __forceinline__ int compact_rows(const unsigned* __restrict__ rows, const Bricks& bk, int* __restrict__ out, int* wave_total, int t) {
  const int per = (bk.rows + kListThreads - 1) / kListThreads;
  const int r0 = min(t * per, bk.rows), r1 = min(r0 + per, bk.rows);
  int cnt = 0;
  for (int r = r0; r < r1; r++) cnt += __popc(rows[r]);
  const int lane = t & 63, wv = t >> 6;
  int incl = cnt;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const int v = __shfl_up(incl, off, 64);
    if (lane >= off) incl += v;
  }
  if (lane == 63) wave_total[wv] = incl;
  __syncthreads();
  int base = 0, total = 0;
#pragma unroll
  for (int q = 0; q < kListThreads / 64; q++) {
    const int v = wave_total[q];
    base += q < wv ? v : 0;
    total += v;
  }
  int pos = base + incl - cnt;
  for (int r = r0; r < r1; r++) {
    unsigned m = rows[r];
    while (m) {
      const int ix = __ffs((int)m) - 1;
      m &= m - 1u;
      out[pos++] = r * bk.nx + ix;
    }
  }
  __syncthreads();      // wave_total is reused by the next call
  return total;
}

// the counts of item b (|L_B|, the brick count, fast, |L_A|) and, behind a system-scope fence, the scan's number into the pinned mirror
__device__ __forceinline__ void publish_counts(unsigned* mirror, int b, unsigned seq, unsigned nb, unsigned bricks, unsigned fast, unsigned na) {
  volatile unsigned* m = mirror + 8 * b;
  m[0] = nb; m[1] = bricks; m[2] = fast; m[3] = na;
  __threadfence_system();                     // the counts are visible to the host before the number that announces them
  m[4] = seq;
}

// publish: no pass over the lists follows (a probe), so this kernel writes the mirror itself; else the first list pass does, off the
// path every later kernel waits on (two round trips to host memory: measured 3-4 us at the end of this one-block kernel)
__global__ __launch_bounds__(kListThreads) void k_scal3_lists(Bricks bk, int B, BcFoldArg box, unsigned seq, int publish,
                                                              const unsigned* __restrict__ nz,
                                                              int* __restrict__ lists, int* __restrict__ counts, unsigned* mirror) {
  __shared__ unsigned rows_a[kMaxBrickRows], rows_b[kMaxBrickRows];
  __shared__ int wave_total[kListThreads / 64];
  const int b = (int)blockIdx.x, t = (int)threadIdx.x;
  const unsigned full = bk.nx >= 32 ? ~0u : (1u << bk.nx) - 1u;
  nz += (long long)b * (bk.n + 1);            // the item's tags: its `fast` tag, then one per brick
  const bool all = nz[0] == seq;
  nz++;
  // the bricks of the pair's box (inclusive cell indices, clipped to the array)
  unsigned boxmask = 0u;
  int ey0 = 1, ey1 = 0, ez0 = 1, ez1 = 0;
  if (box.dev) {
    const BcFold f = *box.dev;
    const int bx0 = max(f.x0, 0) / kBrickX, bx1 = min(f.x1 / kBrickX, bk.nx - 1);
    if (f.x1 >= 0 && f.y1 >= 0 && f.z1 >= 0 && bx0 <= bx1) {
      boxmask = ((bx1 >= 31 ? ~0u : (1u << (bx1 + 1)) - 1u) & ~((1u << bx0) - 1u)) & full;
      ey0 = max(f.y0, 0) / kBrickY; ey1 = min(f.y1 / kBrickY, bk.ny - 1);
      ez0 = max(f.z0, 0) / kBrickZ; ez1 = min(f.z1 / kBrickZ, bk.nz - 1);
    }
  }
  for (int r = t; r < bk.rows; r += kListThreads) {
    const unsigned* p = nz + (long long)r * bk.nx;
    unsigned w = 0u;
    for (int ix = 0; ix < bk.nx; ix++) w |= p[ix] == seq ? 1u << ix : 0u;
    rows_a[r] = w;
  }
  __syncthreads();
  dilate_rows(rows_a, rows_b, bk, full, all, boxmask, ey0, ey1, ez0, ez1, t);      // L_B
  __syncthreads();
  dilate_rows(rows_b, rows_a, bk, full, all, 0u, 1, 0, 1, 0, t);                   // L_A
  __syncthreads();
  const int na = compact_rows(rows_a, bk, lists + (long long)b * bk.n, wave_total, t);
  const int nb = compact_rows(rows_b, bk, lists + ((long long)B + b) * bk.n, wave_total, t);
  if (t == 0) {
    counts[4 * b] = na; counts[4 * b + 1] = nb; counts[4 * b + 2] = all ? 1 : 0;
    if (publish) publish_counts(mirror, b, seq, (unsigned)nb, (unsigned)bk.n, all ? 1u : 0u, (unsigned)na);
  }
}

// ---- the passes over the lists -----------------------------------------------------------------------------------------------
// Work item w of batch item b = (list entry w / TPB, tile w % TPB of the brick's TPB = 4 / PZ plane groups); the blocks of the
// fixed grid take the items of all batch items round robin.
#define TFL_SCAL3_LIST_LOOP(PZ_, LIST, COUNT_SLOT, NBLK, CALL)                                                   \
  constexpr int TPB = kBrickZ / (PZ_);                                                                           \
  const int G = (a.d.Z + (PZ_) - 1) / (PZ_);                                                                     \
  int first = (int)blockIdx.x;                                                                                   \
  for (int b = 0; b < B; b++) {                                                                                  \
    const int n = counts[4 * b + (COUNT_SLOT)] * TPB;                                                            \
    const int* list = (LIST) + (long long)b * bk.n;                                                              \
    int w = first;                                                                                               \
    for (; w < n; w += (NBLK)) {                                                                                 \
      const int e = list[w / TPB], tq = w % TPB;                                                                 \
      const int row = e / bk.nx, ix = e - row * bk.nx, iz = row / bk.ny, iy = row - iz * bk.ny;                  \
      const int g = iz * TPB + tq;                                                                               \
      if (g < G) {                           /* (the last brick of a Z that is no multiple of 4) */             \
        const SBlock sb = SBlock{-1, ix, iy, b * G + g, true};                                                  \
        CALL;                                                                                                    \
        __syncthreads();                     /* the tile and the wave verdict words are reused */                \
      }                                                                                                          \
    }                                                                                                            \
    first = w - n;                           /* where this block's stride lands in the next item */              \
  }

// (the LAST block of pass A advects nothing: it publishes the counts of k_scal3_lists to the pinned mirror)
template <int TZ, int KZ, bool FAST>
__global__ __launch_bounds__(256 * TZ) void k_scal3_fwd_list(AdvArgs a, Bricks bk, int B, const int* __restrict__ lists, const int* __restrict__ counts,
                                                             unsigned* mirror, unsigned seq, const float* __restrict__ s,
                                                             const float* __restrict__ U, const float* __restrict__ flags,
                                                             float* __restrict__ out, float* __restrict__ bounds) {
  __shared__ float tile[Tile<TZ * KZ, 2>::N];
  const int nblk = (int)gridDim.x - 1;
  if ((int)blockIdx.x == nblk) {
    for (int b = (int)threadIdx.x + TX * ((int)threadIdx.y + TY * (int)threadIdx.z); b < B; b += 256 * TZ)
      publish_counts(mirror, b, seq, (unsigned)counts[4 * b + 1], (unsigned)bk.n, (unsigned)counts[4 * b + 2], (unsigned)counts[4 * b]);
    return;
  }
  TFL_SCAL3_LIST_LOOP(TZ * KZ, lists, 0, nblk, (scal3_fwd_body<TZ, KZ, true, FAST>(sb, tile, a, s, U, flags, out, bounds)))
}
// (s is read and written in place: neither pointer is __restrict__; a thread reads the word of its own cell before it writes it)
template <int TZ, int KZ, bool FAST>
__global__ __launch_bounds__(256 * TZ) void k_scal3_bwd_list(AdvArgs a, Bricks bk, int B, const int* __restrict__ lists, const int* __restrict__ counts,
                                                             double half_strength, const float* s, const float* __restrict__ U,
                                                             const float* __restrict__ flags, const float* __restrict__ fwd,
                                                             const float* __restrict__ bounds, float* dst, BcFoldArg folda) {
  __shared__ float tile[Tile<TZ * KZ, 1>::N];
  TFL_SCAL3_LIST_LOOP(TZ * KZ, lists + (long long)B * bk.n, 1, (int)gridDim.x,
                      (scal3_bwd_body<TZ, KZ, FAST>(sb, tile, a, half_strength, s, U, flags, fwd, bounds, dst, folda)))
}
#undef TFL_SCAL3_LIST_LOOP

// resident blocks of a kernel on the whole device (the occupancy query, once per kernel and device)
int device_slots(const void* fn, int threads) {
  struct Rec { const void* fn; int dev, n; };
  static Rec recs[16];
  static int nrec = 0;
  static std::mutex mu;                       // virtual ranks launch from several host threads
  int dev = 0; (void)hipGetDevice(&dev);
  std::lock_guard<std::mutex> lock(mu);
  for (int q = 0; q < nrec; q++) if (recs[q].fn == fn && recs[q].dev == dev) return recs[q].n;
  int per = 0, cus = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per, fn, threads, 0) != hipSuccess || per <= 0) { (void)hipGetLastError(); per = 2; }
  if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0) { (void)hipGetLastError(); cus = 256; }
  if (nrec < 16) { recs[nrec].fn = fn; recs[nrec].dev = dev; recs[nrec].n = per * cus; nrec++; }
  return per * cus;
}
unsigned list_grid(const void* fn, int threads, const Bricks& bk, int B, int pz) {
  const long long work = (long long)B * bk.n * (kBrickZ / pz);
  const long long slots = device_slots(fn, threads);
  return (unsigned)(work < slots ? work : slots);
}

template <int TZ, int KZ, bool FAST>
void launch_list_a(hipStream_t st, const AdvArgs& a, const Bricks& bk, int B, const Scal3SparseAsk& sp, const float* s, const float* U,
                   const float* flags, float* out, float* bounds) {
  const void* fn = (const void*)k_scal3_fwd_list<TZ, KZ, FAST>;
  TFL_TIMED_EXT("k_scalar_fwd", st);
  TFL_LAUNCH_EXT((k_scal3_fwd_list<TZ, KZ, FAST>), list_grid(fn, 256 * TZ, bk, B, TZ * KZ) + 1u, dim3(TX, TY, TZ), 0, st, a, bk, B, (const int*)sp.lists,
                 (const int*)sp.counts, sp.mirror, sp.seq, s, U, flags, out, bounds);
}
template <int TZ, int KZ, bool FAST>
void launch_list_b(hipStream_t st, const AdvArgs& a, const Bricks& bk, int B, const Scal3SparseAsk& sp, const float* s, const float* U,
                   const float* flags, const float* fwd, const float* bounds, float* dst, const BcFoldArg& fold) {
  const void* fn = (const void*)k_scal3_bwd_list<TZ, KZ, FAST>;
  TFL_TIMED_EXT("k_scalar_bwd", st);
  TFL_LAUNCH_EXT((k_scal3_bwd_list<TZ, KZ, FAST>), list_grid(fn, 256 * TZ, bk, B, TZ * KZ), dim3(TX, TY, TZ), 0, st, a, bk, B, (const int*)sp.lists,
                 (const int*)sp.counts, (double)a.strength * 0.5, s, U, flags, fwd, bounds, dst, fold);
}

template <bool FAST>
void launch_lists(hipStream_t st, const AdvArgs& a, const Bricks& bk, int B, const Scal3SparseAsk& sp, float* s, const float* U, const float* flags,
                  float* fwd, float* bounds, const BcFoldArg& fold) {
  // the block shapes launch() of advect_scalar3.hip picks: pass A 2 x 1 below 6 M cells per item and 1 x 4 above, pass B 1 x 2
  if ((long long)a.d.sc >= 6000000ll) launch_list_a<1, 4, FAST>(st, a, bk, B, sp, s, U, flags, fwd, bounds);
  else launch_list_a<2, 1, FAST>(st, a, bk, B, sp, s, U, flags, fwd, bounds);
  launch_list_b<1, 2, FAST>(st, a, bk, B, sp, s, U, flags, fwd, bounds, s, fold);
}

}  // namespace

int scal3_sparse_bricks(int Z, int Y, int X) {
  const Bricks bk = bricks_of(Z, Y, X);
  return (bk.rows <= kMaxBrickRows && bk.nx <= kMaxBricksX) ? bk.n : 0;
}

bool scal3_sparse_fits(const Dom& d) {
  // a forced block shape or kernel form (TFL_SCAL3_TZ, the marched and the gather kernels) means the caller wants THOSE kernels
  const bool forced = sw::present(Sw::SCAL3_TZ) || sw::num(Sw::SCAL3_MARCH, 0) == 1 || sw::present(Sw::ADVECT_GATHER) || sw::present(Sw::SCALAR_GATHER);
  const bool whole = d.w0 == 0 && d.n0 == d.Z && d.nw == d.Z && d.zg == 0 && d.Zg == d.Z;
  return !forced && whole && scal3_shape_ok(d) && scal3_sparse_bricks(d.Z, d.Y, d.X) > 0;
}

// (sp.scanned: pass A of advectVel has left this scan's tags already -- vel3_fwd_scan below -- and the lists kernel starts the operator)
void scal3_sparse_scan(hipStream_t st, const AdvArgs& a, int B, const float* s, const float* U, const BcFoldArg& box, const Scal3SparseAsk& sp) {
  const Dom& d = a.d;
  const Bricks bk = bricks_of(d.Z, d.Y, d.X);
  const dim3 grd((unsigned)bk.nx, (unsigned)bk.ny, (unsigned)(bk.nz * B));
  if (!sp.scanned) {
    TFL_TIMED_EXT("k_scal3_scan", st);
    if (d.X % 4 == 0 && (((uintptr_t)s | (uintptr_t)U) & 15) == 0) TFL_LAUNCH_EXT((k_scal3_scan<true>), grd, 256, 0, st, d, bk, a.dt, sp.seq, s, U, sp.nz);
    else TFL_LAUNCH_EXT((k_scal3_scan<false>), grd, 256, 0, st, d, bk, a.dt, sp.seq, s, U, sp.nz);
  }
  TFL_TIMED_EXT("k_scal3_lists", st);
  TFL_LAUNCH_EXT(k_scal3_lists, (unsigned)B, kListThreads, 0, st, bk, B, box, sp.seq, sp.run == 2 ? 0 : 1, (const unsigned*)sp.nz,
                 sp.lists, sp.counts, sp.mirror);
}

// Pass A of advectVel in its scanning form (launched by advect_vel3.hip, which has checked the grid and picked the depth): the
// launch geometry of the plain k_vel3_fwd<KZ> over the whole array, the same timer name.
void vel3_fwd_scan(hipStream_t st, int kz, const AdvArgs& a, int B, const float* U, const float* flags, float* out, const Vel3ScanAsk& sc) {
  const Dom& d = a.d;
  static_assert(vel3::TX == kBrickX && vel3::TY == kBrickY && kBrickZ % 2 == 0, "a block of either depth lies inside one brick");
  const int groups = (d.Z + kz - 1) / kz;
  // (the grid's x and y extents ARE the brick counts the hook indexes the tags with)
  const dim3 blk(vel3::TX, vel3::TY, 1), grd((d.X + vel3::TX - 1) / vel3::TX, (d.Y + vel3::TY - 1) / vel3::TY, (unsigned)(groups * B));
  TFL_TIMED_EXT("k_vel_fwd", st);
#define TFL_VEL3_SCAN(KZ, FAST) \
  TFL_LAUNCH_EXT((k_vel3_fwd_scan<KZ, FAST>), grd, blk, 0, st, a, U, flags, out, sc.s, sc.nz, sc.seq)
  if (kz == 1) { if (a.fast) TFL_VEL3_SCAN(1, true); else TFL_VEL3_SCAN(1, false); }
  else { if (a.fast) TFL_VEL3_SCAN(2, true); else TFL_VEL3_SCAN(2, false); }
#undef TFL_VEL3_SCAN
}

void scal3_sparse_passes(hipStream_t st, const AdvArgs& a, int B, float* s, const float* U, const float* flags, float* fwd, float* bounds,
                         const BcFoldArg& fold, const Scal3SparseAsk& sp) {
  const Bricks bk = bricks_of(a.d.Z, a.d.Y, a.d.X);
  if (a.fast) launch_lists<true>(st, a, bk, B, sp, s, U, flags, fwd, bounds, fold);
  else launch_lists<false>(st, a, bk, B, sp, s, U, flags, fwd, bounds, fold);
}

}  // namespace tfl
