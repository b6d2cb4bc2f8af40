// tfl_host.hpp -- host-side launcher prototypes shared by the .hip translation units and the .cpp files.
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <cstdlib>

#include "tfl_device.hpp"
#include "tfl_pack.hpp"
#include "tfl_switches.hpp"

struct tfl_model;

namespace tfl {

// Where an operator computes and which of its passes run: a value that every windowed operator receives as an argument and
// hands to its launchers. A public tfl_* operator that honours the tfl_set_* calls forms one from its context at entry
// (context.cpp scope_of); the z-slab step builds its own per call. All zero = the whole array, every pass, exact advection, dx of
// the array itself.
struct ZWin { int a0, a1, b0, b1; };       // planes [a0, a1) and [b0, b1) in array indices; all zero = the whole array
struct ZOrigin { int first, total; };      // the array inside the whole grid: {first global plane, planes of the whole grid}; {0, 0} = none
struct Scope {
  ZWin win = {0, 0, 0, 0};                 // tfl_set_z_window
  ZOrigin origin = {0, 0};                 // tfl_set_z_origin
  int stages = 0;                          // tfl_set_stages: which passes of a multi-pass operator run (0 = all)
  int advect_fast = 0;                     // tfl_set_advect_mode: 1 = tolerance mode of the LDS-tiled 3-D advection kernels
  int dx_cells = 0;                        // > 0: dx = 1 / dx_cells, formed exactly like getDx does (a z-slab rank: the whole grid's)
  bool windowed() const { return win.a1 > win.a0 || win.b1 > win.b0; }
  int passes() const { return stages ? stages : 0xff; }
};
// A setConstVals pair (lib/simulate.lua:130-160: x = x * invMask + bc) that an operator MAY apply
// to the field it writes (round 4): the pair is the identity outside the box [x0, x1] x [y0, y1] x [z0, z1] (inclusive, array
// indices; the plume's pair covers four y rows), so a producing kernel compares its rows against the box and only the
// threads inside it load bc / invMask ([B][C][Z][Y][X] like the field) -- nothing per cell elsewhere. The descriptor lives in
// DEVICE memory (the plan owns it) and a kernel gets its address: one pointer argument, read with scalar loads at the store
// -- ten scalars by value stayed live through the whole kernel and cost the advection kernels 30 SGPR spills each. A launcher
// that hands the pointer to its kernel says so (Fold below); tfl_simulate_step launches the sparse kernel
// (k_apply_bcs_indexed) when none did.
struct BcFold { const float* bc; const float* inv; int x0, x1, y0, y1, z0, z1; };
// What a kernel is handed: the descriptor's device address and, by value, the box's y / z range packed into two words
// (lo = y0 | z0 << 16, hi = y1 | z1 << 16): the block-uniform gate at the top of the kernel needs no memory access.
struct BcFoldArg { const BcFold* dev; unsigned lo, hi; };     // dev == nullptr: no request
inline BcFoldArg no_fold() { return BcFoldArg{nullptr, 0u, 0u}; }

// addBuoyancy (third_party/tfluids.cc:1162-1233) folded into the kernel that writes the advected velocity (round 5). In
// simulate() the buoyancy force follows advectVel and the first setConstVals directly (lib/simulate.lua:196-226), it is
// pointwise in U and needs the ADVECTED density -- which advectScalar has delivered (pair applied) before advectVel runs. So
// tfl_simulate_step hands pass B of advectVel a request {rho, (sx, sy, sz) = -gravity dt / dx}; the kernel that takes it
// adds 0.5 s_c (rho(i) + rho(i - e_c)) on the faces between two fluid cells behind the folded pair, from two to four more
// loads per cell, and the 32 B/cell launch of k_add_buoyancy disappears. Asked for only together with the U pair (or when
// there is none): the force must see the boundary values.
struct BuoyFold { const float* rho; float sx, sy, sz; };      // rho == nullptr: no request

// What a native step asks of the kernel that writes an operator's result -- the pair and the force above, each may be empty --
// and what the operator's launchers took of it. A request counts as taken only where a launcher hands it to a kernel (take_*);
// the step launches whatever was not taken itself.
struct Fold {
  BcFoldArg bc = {nullptr, 0u, 0u};
  BuoyFold buoy = {nullptr, 0.0f, 0.0f, 0.0f};
  bool bc_took = false, buoy_took = false;
  BcFoldArg hand_bc() { bc_took = bc_took || bc.dev; return bc; }
  BuoyFold hand_buoy() { buoy_took = buoy_took || buoy.rho; return buoy; }
};

// The forces of the `Items` operators (tfl_addBuoyancyItems, tfl_addGravityItems, tfl_vorticityConfinementItems):
// every batch item has its own strengths. The table travels BY VALUE in the kernel arguments and is indexed by the block's item,
// which is block-uniform: the reads are scalar loads from the argument segment. Bit b of `on`: item b has the force; a block of
// an item without it returns (in place) or copies (source != destination) and never reads the item's entries.
constexpr int kMaxItems = 32;
struct ItemVec { float x[kMaxItems], y[kMaxItems], z[kMaxItems]; unsigned on; };
struct ItemAmp { float s[kMaxItems]; unsigned on; };
// The force kernels are written once, template <bool IS3D, class... Tab>, with the table as a trailing argument PACK: empty for the
// operators of the reference, whose instantiations so keep their argument segment and their instruction streams (an empty struct
// would take a byte of it and move the hidden arguments; profiles/datagen_batched.md holds the disassembly diff), one ItemVec /
// ItemAmp for the `Items` operators. items_of(tab...) is that one table.
template <class T> __host__ __device__ inline const T& items_of(const T& t) { return t; }

// What tfl_simulate_step asks of the in-place maccormackOurs advectScalar of a 3-D density (advect_scalar3_sparse.hip, DESIGN.md
// 3.17): find the bricks of 64 x 4 x 4 cells that hold a word other than +0.0, and run the two passes over the bricks around
// them only. The buffers belong to the context (tfl_ctx.hpp Scal3SparseState: one set per density field, allocated once).
struct Scal3SparseAsk {
  int run = 0;                     // 0 = nothing | 1 = scan + lists, then the two full launches (a probe) | 2 = scan + lists + list-driven passes
  int took = 0;                    // out: what the operator did of it (0: it ran the two full launches and nothing else)
  int scanned = 0;                 // pass A of advectVel has run this scan already (Vel3ScanAsk::took): the operator starts at the lists kernel
  unsigned seq = 0;                // the scan's number (> 0), published behind its counts
  unsigned* nz = nullptr;          // [B][1 + bricks] tags, "set" = equals seq (never cleared between scans). Per item: [0] `fast`, some
                                   // velocity face has !(|U dt| <= 0.9); [1 + brick] the brick holds a word of s that is not +0.0
  int* lists = nullptr;            // [2][B][bricks]: the compacted lists L_A, L_B (brick indices, ascending)
  int* counts = nullptr;           // [B][4]: |L_A|, |L_B|, fast as the lists kernel read it
  unsigned* mirror = nullptr;      // device address of the pinned mirror, 8 words per item: |L_B|, bricks, fast, |L_A|, seq
};

// What tfl_simulate_step asks of pass A of advectVel when the advectScalar of density field s follows on the lists: leave that
// scan's tags (the arrays and the number of the Scal3SparseAsk) as a by-product of the words of U the pass stages anyway. Taken
// only by the tile kernels on the whole array (advect_vel3.hip); else advectScalar runs its own k_scal3_scan.
struct Vel3ScanAsk {
  const float* s = nullptr;        // the density field, [B][1][Z][Y][X]; nullptr: no request
  unsigned* nz = nullptr;          // Scal3SparseAsk::nz, ::seq
  unsigned seq = 0;
  bool took = false;               // out: the scanning form of pass A ran
};

// does row (j, k) / cell i of the field lie inside the pair's box
__device__ __forceinline__ bool fold_row(const BcFold& f, int j, int k) {
  return j >= f.y0 && j <= f.y1 && k >= f.z0 && k <= f.z1;
}
__device__ __forceinline__ bool fold_col(const BcFold& f, int i) { return i >= f.x0 && i <= f.x1; }
// Block-uniform gate, evaluated once at the top of a kernel (two argument words, dead right after): can any cell of rows
// [ya, yb] x planes [za, zb] lie in the pair's box?
// Only the blocks that answer yes read the descriptor again at their stores -- for the plume's pair 1 block in 16-32.
__device__ __forceinline__ bool fold_block(const BcFoldArg& a, int ya, int yb, int za, int zb) {
  return (a.dev != nullptr) & (ya <= (int)(a.hi & 0xffffu)) & (yb >= (int)(a.lo & 0xffffu)) & (za <= (int)(a.hi >> 16)) &
         (zb >= (int)(a.lo >> 16));
}

// The launch domain of a launcher that covers the whole array whatever window a host has set (Jacobi, PCG, the public stencil
// operators, the wall plan ...): it takes no scope.
inline Dom whole_dom(int Z, int Y, int X) {
  Dom d; d.X = X; d.Y = Y; d.Z = Z; d.sy = X; d.sz = X * Y; d.sc = X * Y * Z; d.one = 1;
  d.w0 = 0; d.n0 = Z; d.w1 = 0; d.nw = Z;
  d.zg = 0; d.Zg = Z;
  return d;
}
// The launch domain of a windowed launcher: the planes of the scope's window, the array placed at the scope's origin.
inline Dom make_dom(const Scope& sc, int Z, int Y, int X) {
  Dom d = whole_dom(Z, Y, X);
  if (sc.origin.total > 0) { d.zg = sc.origin.first; d.Zg = sc.origin.total; }
  const ZWin w = sc.win;
  if (sc.windowed()) {
    auto clip = [Z](int v) { return v < 0 ? 0 : (v > Z ? Z : v); };
    const int a0 = clip(w.a0), a1 = clip(w.a1) > a0 ? clip(w.a1) : a0;
    const int b0 = clip(w.b0), b1 = clip(w.b1) > b0 ? clip(w.b1) : b0;
    d.w0 = a0; d.n0 = a1 - a0; d.w1 = b0; d.nw = d.n0 + (b1 - b0);
  }
  return d;
}

// Built-in per-kernel timing (the reference only has host timers around the projection,
// lib/simulate.lua:254-260,306-318). When a profile is active on this thread every kernel launch is
// bracketed by hipEvents on the launch stream; tfl_profile_end() sums them per kernel name.
struct KernelTimer {
  // ext = false: the events are recorded on the stream around whatever the scope launches (adds the command
  // processor's event handling to the reading: +2..7 us per kernel). ext = true: nothing is recorded here; the
  // scope passes start()/stop() to hipExtLaunchKernelGGL, which stamps them with the dispatch's own begin / end
  // (the numbers rocprofv3 reports). Both are null when no profile is active.
  KernelTimer(const char* name, hipStream_t st, bool ext = false);
  ~KernelTimer();
  hipEvent_t start() const;
  hipEvent_t stop() const;
  int slot_;
  hipStream_t st_;
  bool ext_;
};
#define TFL_TIMED(name, st) ::tfl::KernelTimer tfl_timer_(name, st)
#define TFL_TIMED_EXT(name, st) ::tfl::KernelTimer tfl_timer_(name, st, true)
// one launch inside a TFL_TIMED_EXT scope; `kernel` in parentheses when it is a template-id with commas
// (the plain launch when no profile is active: hipExtLaunchKernelGGL costs a few us more on the host)
#define TFL_LAUNCH_EXT(kernel, grid, block, shmem, st, ...)                                                        \
  do {                                                                                                             \
    if (tfl_timer_.start())                                                                                        \
      hipExtLaunchKernelGGL(kernel, dim3(grid), dim3(block), (uint32_t)(shmem), st, tfl_timer_.start(),            \
                            tfl_timer_.stop(), 0, __VA_ARGS__);                                                    \
    else                                                                                                           \
      hipLaunchKernelGGL(kernel, dim3(grid), dim3(block), (uint32_t)(shmem), st, __VA_ARGS__);                      \
  } while (0)

// advect.hip
void advect_scalar(hipStream_t st, const Scope& sc, bool is3d, int method, int B, int Z, int Y, int X, float dt, float strength,
                   int outside, unsigned long long* err, const float* s, const float* U, const float* flags,
                   float* fwd, float* bounds, float* mm, float* dst, Fold& f, Scal3SparseAsk* sparse = nullptr);
// advect_scalar3_sparse.hip
int scal3_sparse_bricks(int Z, int Y, int X);      // bricks per batch item; 0 = the grid is outside what the brick map holds
bool scal3_sparse_fits(const Dom& d);              // the whole array, a shape the tile kernels and the brick map take, no forced kernel form
void advect_vel(hipStream_t st, const Scope& sc, bool is3d, int method, int B, int Z, int Y, int X, float dt, float strength,
                unsigned long long* err, const float* U, const float* flags, float* fwd, float* dst, Fold& f, Vel3ScanAsk* scan = nullptr);

void minmax3(hipStream_t st, bool is3d, int B, const Dom& d, int outside, const float* s, const float* flags, float* lo3,
             float* hi3);

// stencil.hip
void set_wall_bcs(hipStream_t st, bool is3d, int B, int Z, int Y, int X, float* U, const float* flags);
void velocity_divergence(hipStream_t st, bool is3d, int B, int Z, int Y, int X, const float* U, const float* flags,
                         float* div);
void velocity_update(hipStream_t st, bool is3d, int B, int Z, int Y, int X, float* U, const float* flags,
                     const float* p);
// the same three on the 3-D planes [k0, k1) of the local array only (the z-slab step's Jacobi projection)
void set_wall_bcs_planes(hipStream_t st, int B, int Z, int Y, int X, int k0, int k1, float* U, const float* flags);
void velocity_divergence_planes(hipStream_t st, int B, int Z, int Y, int X, int k0, int k1, const float* U, const float* flags,
                                float* div);
void velocity_update_planes(hipStream_t st, int B, int Z, int Y, int X, int k0, int k1, float* U, const float* flags,
                            const float* p);
void add_buoyancy(hipStream_t st, const Scope& sc, bool is3d, int B, int Z, int Y, int X, const float* Usrc, float* U, const float* flags,
                  const float* density, float sx, float sy, float sz, Fold& f);
void add_gravity(hipStream_t st, const Scope& sc, bool is3d, int B, int Z, int Y, int X, float* U, const float* flags, float fx,
                 float fy, float fz);
// the same two with per-item strengths (no pair is folded; Usrc != U: the items without the force are copied)
void add_buoyancy_items(hipStream_t st, const Scope& sc, bool is3d, int B, int Z, int Y, int X, const float* Usrc, float* U, const float* flags,
                        const float* density, const ItemVec& t);
void add_gravity_items(hipStream_t st, const Scope& sc, bool is3d, int B, int Z, int Y, int X, float* U, const float* flags, const ItemVec& t);
void empty_domain(hipStream_t st, bool is3d, int bnd, int B, int Z, int Y, int X, float* flags);
void flags_to_occupancy(hipStream_t st, long long numel, const float* flags, float* occ);
void rectangular_blur(hipStream_t st, bool is3d, int B, int C, int Z, int Y, int X, int rad, const float* src, float* dst,
                      float* tmp);
void signed_distance_field(hipStream_t st, int B, int Z, int Y, int X, int rad, const float* flags, float* dst);
void stream_copy(hipStream_t st, long long n4, const float* src, float* dst);   // n4 float4s, 16-byte aligned
void absmax(hipStream_t st, long long n, const float* x, float* out, bool reset);   // *out = max(*out, max |x|)
void reach_flags(hipStream_t st, const float* maxu, float dt, int n, double* flags, const unsigned long long* range_count = nullptr);   // flags[r-1] = (*maxu * dt >= r), r = 1..n (n <= 62); flags[n] = (*range_count != 0) when given
void reach_publish(hipStream_t st, const float* src, float* dst, unsigned* tick);   // dst[0] = *src, dst[1] = ++*tick (mapped pinned mirror)

// divnorm.hip: ||velocityDivergence(U, flags)[b]||_2 in two launches, no divergence field, no atomics.
// Stage 1: sums[b * zstride + zoff + k] = the fp64 sum of the squared fp32 divergence over plane k, for the planes k of the
// scope's window (the scope's origin decides which planes are the domain's border). Stage 2: norm[b] = sqrt of the sum of
// sums[b * nz + 0 .. nz - 1] in ascending order.
void divergence_norm_planes(hipStream_t st, const Scope& sc, bool is3d, int B, int Z, int Y, int X, const float* U, const float* flags,
                            double* sums, int zstride, int zoff);
void divergence_norm_finish(hipStream_t st, int B, int nz, const double* sums, double* norm);

// criterion.hip: nn.FluidCriterion (lib/modules/fluid_criterion.lua) in two launches, plus its border weight.
// What k_criterion_planes is handed by value. w == nullptr: unweighted; gP == gU == nullptr: no gradients. norm* = 2 / n of the
// term's tensor (2 without sizeAverage), lam* = (float)lambda, *On = lambda > 0. sums: [3][BZ] doubles (p, U, div plane sums).
struct CriterionArgs {
  const float *p, *pt, *U, *Ut, *flags, *w;
  float *gP, *gU;
  double* sums;
  long long BZ;
  float normP, normU, lamP, lamU, lamD;
  int pOn, uOn, dOn;
};
struct CriterionFinish { double lambda[3], n[3]; int on[3]; };      // term t = on ? lambda * (S / n) : 0 (n = 1 without sizeAverage)
// w = ((clamp(sdf(flags, rad), 1, bw) - 1) * m + 1) * s + 1, one fp32 rounding per operation (fluid_criterion.lua:149-157)
void criterion_weight(hipStream_t st, int B, int Z, int Y, int X, int rad, float bw, float m, float s, const float* flags, float* w);
void criterion_planes(hipStream_t st, bool is3d, int B, int Z, int Y, int X, const CriterionArgs& a);
void criterion_finish(hipStream_t st, long long n, const double* sums, const CriterionFinish& f, double* loss);
// the training closure's loss fold and guard (tfl_closure_fold): one launch of one thread
void closure_fold(hipStream_t st, const double* loss4, double* sums5, int* guard, int longTerm, double errLimit);

// vorticity.hip
// stages: bit 0 = pass A (U -> curl, |curl|), bit 1 = pass B (curl, |curl|, flags, U -> U); a z-slab rank runs the two
// passes under different z-windows (sc: the window and origin only -- the caller has mapped sc.stages into `stages`)
// Usrc (round 5): U = Usrc + force with every cell of the window written (the four-cells-per-thread kernels only: false =
// not possible here, nothing launched, the caller copies Usrc into U and calls again without it)
bool vorticity_confinement(hipStream_t st, const Scope& sc, bool is3d, int B, int Z, int Y, int X, float* U, const float* flags,
                           float strength, float* curl, float* curl_norm, int stages, const float* Usrc, Fold& f);

// the two launches in place with per-item strengths: k_curl and k_confine skip the items without the force (their words of U are
// not touched, their curl / |curl| planes not written)
void vorticity_confinement_items(hipStream_t st, const Scope& sc, bool is3d, int B, int Z, int Y, int X, float* U, const float* flags,
                                 const ItemAmp& t, float* curl, float* curl_norm);

// U_out = U_in + confinement(U_in), 3-D, one fused launch without curl arrays (U_out != U_in); false = not supported here
bool vorticity_confinement_fused_ok(bool is3d, int Z, int Y, int X);   // does the native step use the fused kernel for this grid
bool vorticity_confinement_fused(hipStream_t st, const Scope& sc, int B, int Z, int Y, int X, const float* Uin, float* Uout, const float* flags,
                                 float strength, Fold& f);

// jacobi.hip
void jacobi_iteration(hipStream_t st, bool is3d, int B, int Z, int Y, int X, const float* p_prev, const float* flags,
                      const float* div, float* p, double* resid_sq /* [B] or nullptr */);

// one 3-D sweep on the planes [k0, k1) of a z-slab's local array (global planes [zg, zg + Z) of a Zg-deep grid; walls in global z)
void jacobi_sweep_slab(hipStream_t st, int B, int Z, int Y, int X, int zg, int Zg, int k0, int k1, const float* p_prev,
                       const float* flags, const float* div, float* p);

// a 2-D grid of up to 16 K cells: the whole Jacobi solve in one launch, p ping-pongs in LDS (false = not taken)
bool jacobi_solve_lds(hipStream_t st, int B, int Y, int X, const float* flags, const float* div, float* p, float* p_prev,
                      int iters, double* resid_sq);

// pcg.hip
// bad_flags: fluid on the domain's border; wavefront_timeout: the pipelined triangular solves never saw a predecessor (only
// with allow_wavefronts: the caller repeats the solve without)
enum class PcgResult { ok, bad_flags, nan_residual, too_many_components, hip_error, wavefront_timeout };
struct PcgProblem {
  bool is3d;
  int B, Z, Y, X;
  float* p;
  const float *flags, *div;
  int precond;      // 0 none, 1 ilu0, 2 ic0, 3 mg
  float tol;
  int max_iter, verbose;
};
long long pcg_workspace_floats(int Z, int Y, int X);     // the total of pcg_ws (tfl_pcg_ws.hpp) for none / ilu0 / ic0
long long pcg_workspace_floats_for(int Z, int Y, int X, int precond);     // ... for PcgProblem::precond; -1: no such preconditioner
// iterations: the sum over the component solves of the iteration counter at exit (may be null)
PcgResult pcg_solve(hipStream_t st, const PcgProblem& q, float* workspace, float* residual, char* msg, size_t msg_len,
                    bool allow_wavefronts, long long* iterations = nullptr);

// pcg_mg.hip: the multigrid preconditioner (tfl_pcg_mg.hpp). Set-up once per component (*open = 1: a cell of the component has an
// empty neighbour, the matrix is regular); one V-cycle per application, r -> zb of level 0, every kernel of it returning at once
// when S->done. closed: the cycle runs on r minus its mean, written to the r array of level 0; else r of level 0 is r itself.
// partials: kRedBlocks doubles.
struct MgDev;
struct PcgState;
void mg_build_levels(hipStream_t st, const Dom& d, bool is3d, const MgDev& h, const float* flags, const int* label, int root, int* open);
void mg_vcycle(hipStream_t st, bool is3d, const MgDev& h, const PcgState* S, bool closed, const float* r, double* partials, int size);
// The same for a batch (pcg_batched.inc): h, label, w, r and partials are item 0's, item b's lie b * bt.stride floats on; flags is
// the caller's tensor. Root, size, "is there an mg system" and "closed" come from the items' records (tfl_pcg_ws.hpp), on the device.
struct PcgBatch;
void mg_build_levels_batched(hipStream_t st, bool is3d, int B, const PcgBatch& bt, const Dom& d, const MgDev& h, const float* flags,
                             const int* label);
void mg_vcycle_batched(hipStream_t st, bool is3d, int B, const PcgBatch& bt, const MgDev& h, float* w, const float* r, double* partials);
// solveLinearSystemPCGBatched: every item's systems advance in the same launches; item b gets the bits pcg_solve gives it alone.
// q.precond is 0 or 3, q.verbose is not read. residuals / iterations: B entries each, may be null. total: the sum of iterations.
long long pcg_batched_workspace_floats(int B, int Z, int Y, int X, int precond);     // -1: not 0 / 3
PcgResult pcg_solve_batched(hipStream_t st, const PcgProblem& q, float* workspace, float* residuals, long long* iterations,
                            long long* total, char* msg, size_t msg_len);

long long npm_workspace_floats(int Z, int Y, int X);     // the total of npm_ws
PcgResult normalize_pressure_mean(hipStream_t st, bool is3d, int B, int Z, int Y, int X, float* p, const float* flags,
                                  float* workspace, char* msg, size_t msg_len);

// model.hip
long long model_stat_blocks(int B, int Z, int Y, int X);
bool model_stats_fold_requested();
long long model_stat_pairs_per_plane(int B, int Z, int Y, int X, const float* U, const float* flags, const float* Ubc, const float* div);   // as model_pre lays them out
void model_pre(hipStream_t st, const Scope& sc, bool is3d, int B, int Z, int Y, int X, const float* U, const float* flags, float* Ubc,
               float* div, double* partials, double* stats, int zlo, int zhi, int stages = 3, unsigned* ticket = nullptr,
               const unsigned short* wall_code = nullptr,       // wall_code: the flags' tfl_wall_plan (round 6), or null
               bool store_ubc = true);      // false: SetWallBcs(U) is not written to Ubc (div and the sums are the same; model.hip header)
void wall_code(hipStream_t st, bool is3d, int B, int Z, int Y, int X, const float* flags, unsigned short* code);
// (z0 / nz, here and in the two below: the planes [z0, z0 + nz) only; nz < 0 = every plane)
void model_net_input(hipStream_t st, bool is3d, int B, int Z, int Y, int X, const float* pDiv, const float* div,
                     const float* flags, const double* stats, double count, float* x3, int z0 = 0, int nz = -1);
// the general net input of lib/model.lua:130-148: channels {pDiv/scale?, SetWallBcs(U)/scale (C)?, div/scale?, occupancy} in
// this order into x [B][in_c][Z][Y][X]; Ubc = the wall-BC'd velocity tfl_model_begin left in UOut
void model_net_input_gen(hipStream_t st, bool is3d, int B, int Z, int Y, int X, int in_pDiv, int in_UDiv, int in_div,
                         const float* pDiv, const float* Ubc, const float* div, const float* flags, const double* stats,
                         double count, float* x, int z0 = 0, int nz = -1);
// stats[b] = {mode 0: sum x, sum x^2 | mode 1: 0, sum x^2 | mode 2: 0, 1} over the n floats of sample b of `field`
// (the three ways tfl_model_opts sets the input scale through scale_from_stats: std, l2 norm with count = 2, none)
void model_field_stats(hipStream_t st, int B, long long n, const float* field, int mode, double* stats);
// the same over the planes [zlo, zhi) of every channel of a [B][C][Z][yx] field only (a z-slab rank's owned planes)
void model_field_stats_planes(hipStream_t st, int B, int C, int Z, long long yx, int zlo, int zhi, const float* field, int mode,
                              double* stats);
// dst[b][ch][cell] = pDiv[b][cell] / scale_b: the joined pressure-skip channel (model.lua:356-360); dst has `och` planes per item
void model_skip_channel(hipStream_t st, int B, long long cells, const float* pDiv, const double* stats, double count,
                        float* dst, int och, int ch, long long t0 = 0, long long nt = -1);     // cells [t0, t0 + nt) only
// returns true when the launch also folded max |u_z| of what it wrote into *reach_acc (round 6: k_project_v4 on full blocks)
// Uin: the velocity it reads -- Uio itself where model_pre stored SetWallBcs(U) there, or the un-masked U model_pre read (the
// same result, model.hip header); Uio: the velocity it writes
bool model_project(hipStream_t st, const Scope& sc, bool is3d, int B, int Z, int Y, int X, const float* pPred, const float* flags,
                   const double* stats, double count, const float* Uin, float* Uio, float* pOut, const float* UBC, const float* UInvMask,
                   int do_clamp, float lo, float hi, const unsigned long long* range_src, unsigned long long* range_dst,
                   const float* reach_src, float* reach_dst, float* reach_acc, const unsigned short* wall_code, unsigned* reach_tick,
                   Fold& f);
void apply_bcs(hipStream_t st, long long n, float* x, const float* bcv, const float* inv, int do_clamp, float lo,
               float hi);

void bc_scan(hipStream_t st, long long n, const float* bcv, const float* inv, int* counters, int* idx);
void apply_bcs_indexed_multi(hipStream_t st, int count, const long long* n, const int* const* idx, float* const* x,
                             const float* const* bcv, const float* const* inv);
void apply_bcs_indexed(hipStream_t st, long long n, const int* idx, float* x, const float* bcv, const float* inv);

// planes [zlo[i], zlo[i] + nplanes[i]) of field i (rows[i] = B*C rows of zstride floats each) <-> buf; returns the
// number of floats moved
long long pack_planes(hipStream_t st, int n, float* const* ptrs, const int* rows, const int* zlo, const int* nplanes,
                      long long zstride, long long yx, float* buf, int unpack, float* const* bufs = nullptr);

// model_host.cpp: a model built by tfl_model_create_graph with banks, batch norm or max pooling (runs un-sharded only)
bool model_is_graph(const tfl_model* m);
// the factor its grid must be divisible by (the mres pyramid times the pooling; 1 = any grid)
int model_grid_factor(const tfl_model* m);
// The z-slab cone of a 3-D model that is not a graph model, walked backwards from what the velocity update reads
// (pPred on the owned planes widened by (1, 0)). Extents are planes below / above the owned range in the resolution named.
struct LayerCone {
  int conv_lo, conv_hi, conv_d;   // the planes each conv launch computes, at its own resolution grid / conv_d (the coarse grid
                                  // of a ConvolutionUpsample)
  int pool_lo, pool_hi;           // the pooled planes (pool > 1), at grid / (2 * conv_d)
  int in_lo, in_hi;               // the planes of the layer's input it reads, at grid / conv_d
};
struct ModelCone {
  bool fused;                     // the 3-D default topology on its fused kernels: staged launches of their own, halo (4, 3)
  bool windowed;                  // the shape-generic forward under per-layer windows (everything else the slab step takes)
  int F;                          // downsampling factor (the pooling product): cuts, owned ranges and local depths align to it
  int in_lo, in_hi;               // planes of net input (pDiv, div, flags, UDiv) the owned planes need below / above
  int depth;                      // the stored halo the cone needs (max over the layers of resolution x extent), before rounding
  bool reads_U;                   // the net input holds UDiv: the divergence message also carries SetWallBcs(U)
  int norm;                       // what sets the input scale on a slab: 0 = UDiv std (tfl_model_begin's sums), 1 = the
                                  // owned planes of another field / function (model_slab_stats), 2 = none (no all-reduce)
  int nlayers;
  LayerCone layer[32];
};
// false (and why in `why`) for graph models, 2-D models and null
bool model_cone(const tfl_model* m, ModelCone* out, const char** why = nullptr);
// A windowed model's input scale over the owned planes [zlo, zhi) of a slab (norm = 1 / 2), into stats[2 * B]; *count = what
// tfl_model_finish then takes with them (z_total: planes of the whole grid)
void model_slab_stats(hipStream_t st, const tfl_model* m, int B, int Z, long long yx, int zlo, int zhi, int z_total,
                      const float* pDiv, const float* U, const float* div, double* stats, double* count);

// conv.hip
// upf > 1: the result goes to sub-position `sub` (= (c*upf + b)*upf + a) of an upf-times finer output grid (pixel shuffle)
// act: 0 none | 1 ReLU | 2 ReLU6 | 3 sigmoid; out_ch: channel planes per batch item of `out` (0 = cout)
// z0 / nz: compute the conv-grid planes [z0, z0 + nz) only (nz < 0: all Z)
bool conv_direct(hipStream_t st, bool is3d, int B, int Z, int Y, int X, int cin, int cout, int ksz, int act,
                 const float* in, const float* w, const float* bias, float* out, int upf = 1, int sub = 0, int out_ch = 0,
                 int z0 = 0, int nz = -1);
// 2x average pooling of `rows` = B*C planes-stacks [Z][Y][X] -> [Z/2 (3-D)][Y/2][X/2]; output planes [k0, k0 + nk) (nk < 0: all)
void avg_pool2(hipStream_t st, bool is3d, int rows, int Z, int Y, int X, const float* in, float* out, int k0 = 0, int nk = -1);
// the model-graph form (tfl_model_create_graph): the same conv with tap spacing `dil`, the output at channel planes
// [c0, c0 + cout) of `out`, and the folded batch norm y = fmaf(act(x), bn_s[c], bn_t[c]) when bn_s is non-null
bool conv_direct_graph(hipStream_t st, bool is3d, int B, int Z, int Y, int X, int cin, int cout, int ksz, int act,
                       const float* in, const float* w, const float* bias, float* out, int upf, int sub, int out_ch, int c0,
                       int dil, const float* bn_s, const float* bn_t);
// 2x average (max = false) or max pooling of [B][C][Z][Y][X] into planes [c0, c0 + C) of an och-plane output, with the
// folded batch norm applied to the result when bn_s is non-null
void pool2_graph(hipStream_t st, bool is3d, bool max, int B, int C, int Z, int Y, int X, const float* in, float* out, int och,
                 int c0, const float* bn_s, const float* bn_t);
// the join of a banked model in one launch (conv.hip k_bank_join): n banks src[q] (C channels, upsampled nearest by
// 2^sh[q]) go into channel slice slot[q] of the och-plane output (concat), or are added onto it in order (add)
constexpr int kMaxJoinBanks = 8;
bool bank_join(hipStream_t st, bool is3d, bool add, int B, int C, int Z, int Y, int X, int n, const int* slot, const int* sh,
               const float* const* src, float* out, int och);

// conv_mfma.hip (3-D default topology: k=3, 8 output channels; x-phase-packed fp32 MFMA)
void conv3_mfma_first(hipStream_t st, const Scope& sc, int B, int Z, int Y, int X, const float* in_planar3, const float* bfrag,
                      const float* bias, float* out_cl8);
void conv3_mfma_first_fused(hipStream_t st, const Scope& sc, int B, int Z, int Y, int X, const float* pDiv, const float* div,
                            const float* flags, const double* stats, double count, const float* bfrag,
                            const float* bias, float* out_cl8);
void conv3_mfma_mid(hipStream_t st, const Scope& sc, int B, int Z, int Y, int X, const float* in_cl8, const float* bfrag,
                    const float* bias, float* out_cl8);
void conv3_mfma_tail(hipStream_t st, const Scope& sc, int B, int Z, int Y, int X, const float* in_cl8, const float* bfrag,
                     const float* bias, const float* w4, const float* b4, const float* w5, const float* b5,
                     float* p_out);

// conv_valu.hip: the same three layers on the vector ALUs, x-taps as Winograd F(2,3) (wq = tfl_model::wino,
// [dz][dy][cin][4][8]); activations between the layers are channel-planar [B][8][Z][Y][X]
void conv3_valu_first_fused(hipStream_t st, const Scope& sc, int B, int Z, int Y, int X, const float* pDiv, const float* div, const float* flags,
                            const double* stats, double count, const float* wq, const float* bias, float* out_p8);
void conv3_valu_mid(hipStream_t st, const Scope& sc, int B, int Z, int Y, int X, const float* in_p8, const float* wq, const float* bias,
                    float* out_p8);
// tail_pack: {bias of the k3 layer [8], w4 [8][8] (out, in), b4 [8], w5 [8], b5 [1]} (tfl_model::tail_pack)
void conv3_valu_tail(hipStream_t st, const Scope& sc, int B, int Z, int Y, int X, const float* in_p8, const float* wq, const float* tail_pack,
                     float* p_out);

// conv_mfma16.hip: the same three layers as a split-operand fp16 MFMA implicit GEMM; activations between the layers are
// "h2": per (b, z, y) two rows [x][8] of fp16 (hi, lo): 32 B per voxel. wfrag / post from conv3_m16_pack_weights.
void conv3_m16_first_fused(hipStream_t st, const Scope& sc, int B, int Z, int Y, int X, const float* pDiv, const float* div, const float* flags,
                           const double* stats, double count, const void* wfrag, const float* bias, float post, void* out_h2,
                           unsigned long long* range_err, const double* partials = nullptr, long long per_sample = 0,
                           double* stats_out = nullptr);
// round 6: can the first layer sum k_bcs_div_stats' partial pairs itself (partials / per_sample / stats_out above)? Then
// tfl_model_forward skips the launch of k_reduce_stats between the two kernels.
bool conv3_m16_first_sums_partials();
void conv3_m16_mid(hipStream_t st, const Scope& sc, int B, int Z, int Y, int X, const void* in_h2, const void* wfrag, const float* bias, float post,
                   void* out_h2, unsigned long long* range_err);
void conv3_m16_tail(hipStream_t st, const Scope& sc, int B, int Z, int Y, int X, const void* in_h2, const void* wfrag, const float* tail_pack,
                    float post, float* p_out, unsigned long long* range_err);
// layers 1 + 2 in ONE launch (round 5: the 64 B/voxel between them stay in LDS); false = not taken (z-window set, or switched
// off): the caller runs conv3_m16_first_fused + conv3_m16_mid
bool conv3_m16_first2_fused(hipStream_t st, const Scope& sc, int B, int Z, int Y, int X, const float* pDiv, const float* div, const float* flags,
                            const double* stats, double count, const void* wfrag1, const float* bias1, float post1,
                            const void* wfrag2, const float* bias2, float post2, void* out_h2, unsigned long long* range_err);
bool conv3_m16_fuse12_requested();      // EXPERIMENTS flavour + TFL_M16_FUSE12=1 (the default library: always false)
// (conv3_m16_frag_halves / conv3_m16_pack_tail / conv3_m16_pack_weights, the host packers of wfrag: tfl_pack.hpp)

// backward.hip
void velocity_divergence_bwd(hipStream_t st, bool is3d, int B, int Z, int Y, int X, const float* flags,
                             const float* grad_out, float* grad_U);
void velocity_update_bwd(hipStream_t st, bool is3d, int B, int Z, int Y, int X, const float* flags,
                         const float* grad_out, float* grad_p);
void upsample_nearest_fwd(hipStream_t st, int ratio, long long rows, int Zo, int Yo, int Xo, const float* in, float* out);
void upsample_nearest_bwd(hipStream_t st, int ratio, long long rows, int Zi, int Yi, int Xi, const float* go, float* gi);

// conv_bwd.hip: the parameter gradients of one convolution layer (tfl_model_backward), deterministic. `p`: the layer's chunking
// (tfl_train.hpp wg_plan). conv_wgrad leaves fp64 partials of gradWeight and gradBias per block; g is masked by act'(y) where it
// is read (y = null: no activation) and, with wb, rewritten masked for the data gradient that follows. conv_wgrad_finish adds
// the partials in a fixed order and writes (accumulate = 0) or adds onto (1) the cudnn-layout gw [cout_ref][cin_ref][taps] and
// gb [cout_ref] (join_c, join_p: the plane map of the stage behind a concat join, tfl_train.hpp wg_cudnn_index). false = the layer
// does not fit the kernel (nothing launched).
struct WgPlan;
bool conv_wgrad_fits(const WgPlan& p);
bool conv_wgrad(hipStream_t st, bool is3d, const WgPlan& p, int B, int Z, int Y, int X, int cin, int cout, int k, const float* x,
                float* g, const float* y, int ych, int act, bool wb, double* partials);
void conv_wgrad_finish(hipStream_t st, const WgPlan& p, int cin, int cout, int cin_ref, int cout_ref, int skip_in, const double* partials,
                       float* gw, float* gb, int accumulate, int join_c = 0, int join_p = 0);
// dst[b][t] = scale_b * src[b][t] (+ add[b][t]) over `per` floats per batch item; scale_b from the (sum, sum of squares) pairs
void scale_add(hipStream_t st, int B, long long per, const double* stats, double count, const float* src, const float* add, float* dst);

// g[b][c][t] *= act'(y[b][c][t]) over the `cout` planes of g (y has `ych` planes per item): conv_wgrad's write-back alone, for a
// backward pass that asks for no parameter gradients (tfl_model_backward_input with NULL gradient tables)
void act_mask(hipStream_t st, int B, int cout, int ych, long long cells, float* g, const float* y, int act);

// multires_bwd.hip: the backward of pooling and of the pixel shuffle in a linear model; no atomics.
// pool_bwd_mask: dst[row][fine] = act'(y[row][fine]) gc[row][fine >> 1] / 2^dim over `rows` = B * C planes [Z][Y][X] (gc at half
// the resolution; Y, X and in 3-D Z even). act as conv_wgrad's.
void pool_bwd_mask(hipStream_t st, bool is3d, int rows, int Z, int Y, int X, const float* y, const float* gc, float* dst, int act);
// up_dgrad: the data gradient of an upsample layer, gin [B][cin_t] on the layer's input grid [Z][Y][X] from g [B][gch] at `up`
// times the resolution and wt [sub][tap][gch][cin_t]; false = no kernel for cin_t planes (nothing launched)
bool up_dgrad(hipStream_t st, bool is3d, int B, int Z, int Y, int X, int up, int gch, int cin_t, int ksz, const float* g, const float* wt,
              float* gin);

// conv_bwd.hip: the fixed linear maps of a banked model, backwards; fixed-order fp32 sums, no atomics.
// join_bwd: from g [B][och] at the join's output [Z][Y][X], bank i's gradient dst[i] [B][C] at (grid >> sh[i]) -- its channel slice
// (concat) or all channels (add); sh = 0 a copy, else the sum over the block of cells the nearest up-sample replicated.
bool join_bwd(hipStream_t st, bool is3d, bool concat, int B, int C, int och, int Z, int Y, int X, int n, const int* sh, float* const* dst,
              const float* g);
// dst = a + P^T c over `rows` planes, [Z][Y][X] fine (all even in the pooled axes), c at half of it; P = the 2x average pooling.
// dst may be a; a, c, dst 8-byte aligned.
void pyr_pool_bwd(hipStream_t st, bool is3d, int rows, int Z, int Y, int X, const float* a, const float* c, float* dst);
// dst = ((src[0] + src[1]) + src[2]) ... over count floats
bool bank_sum(hipStream_t st, long long count, int n, const float* const* src, float* dst);

// input_grad.hip: what tfl_model_backward_input adds behind the first layer's data gradient. Null pointers: gradP /
// gradU / h (no gradient given), gskip (no joined skip channel), gradPDiv / gradUDiv (not asked for), dsrc (the scale is not
// taken from the divergence).
struct IgArgs {
  const float *flags, *pDiv, *UDiv, *UOut, *gradP, *gradU;
  const float* h;           // scale keep (.) gradU, [B][C] (tfl_model_backward's velocity-gradient scratch)
  const float* gx;          // the first layer's data gradient, [B][gxc]
  const float* gskip;       // the joined skip channel's gradient, [B][1]
  const float *x, *pPred;   // the tape's net input [B][in_c] and last-layer output
  const float* dsrc;        // the divergence of U_bc, `dstride` floats per item; dscaled: divided by the scale (the tape's channel)
  const double* stats; double count;      // the tape's input-scale pair and the count that goes with it
  double* partials;         // [B][blocks][5]
  double* gs;               // [B]: the scale's gradient
  float *gradPDiv, *gradUDiv;
  long long dstride;
  int dscaled, gxc, in_c;
  int pch, uch, dch;        // the first plane of pDiv / U_bc / div in x and gx, -1 = the channel is off
  int nmode, nchan;         // normaliser: 0 none | 1 std | 2 l2 norm, of 0 UDiv | 1 pDiv | 2 div
  int blocks;               // blocks per item of the sums launch (tfl_input_grad.hpp ig_sum_blocks)
};
// the five dot products of g_s per item into a.partials, then g_s into a.gs: two launches, no atomics
void input_grad_sums(hipStream_t st, bool is3d, int B, int Z, int Y, int X, const IgArgs& a);
// gradPDiv / gradUDiv from g_x, g_skip, h and g_s: one gather launch
void input_grad_head(hipStream_t st, bool is3d, int B, int Z, int Y, int X, const IgArgs& a);

// weights_refresh.hip: the device-side weight refresh (tfl_model_set_weights_device), one launch each. d_table / d_jobs: the model's
// device tables (tfl_refresh.hpp); max_elems: the most destination elements of one entry (sizes the grid's x).
struct RefreshSrc; struct RefreshLayer; struct PackJob; struct OptimPtrs; struct OptimArgs;
void refresh_layers(hipStream_t st, const RefreshSrc& src, const RefreshLayer* d_table, int nlayers, int max_elems);
void refresh_pack(hipStream_t st, const RefreshSrc& src, const PackJob* d_jobs, int njobs, int max_elems);
// the split-fp16 fragments of the 3-D default topology's three k = 3 layers and tail; d_post[4] = their post-scales
void refresh_pack16(hipStream_t st, const RefreshSrc& src, void* const* wfrag16, float* d_post, float* tail_pack);
// optim.hip: clip + weight decay + Adam / RMSprop over the flat parameter space (tfl_optim_step): at most three launches
void optim_step(hipStream_t st, const OptimPtrs& p, const long long* d_off, int ntens, long long total, double* d_partials, float* m,
                float* v, long long* d_t, const OptimArgs& c, const int* d_guard,       // d_guard: NULL, or a device word read at run time (set: nothing is written)
                bool norm_done = false);      // the partials are already in place (optim_unpack left them): no norm launch
// the data-parallel step's two launches around the all-reduce (tfl_optim_step_reduced). pack: slot i of d_reduce [total +
// kOptimReduceTail] = flat element i (what: 0 the gradients, 1 the parameters, 2 zeros), slot total = (*d_guard != 0).
// unpack: flat element i = (float)(d_reduce[i] / world) into the gradients (to_params: the parameters), *d_rguard (may be NULL:
// nothing skips) = d_reduce[total] != 0, which where set leaves the arrays alone; d_partials non-NULL: also k_optim_norm's partials
void optim_pack(hipStream_t st, const OptimPtrs& p, const long long* d_off, int ntens, long long total, const int* d_guard,
                double* d_reduce, int what);
void optim_unpack(hipStream_t st, const OptimPtrs& p, const long long* d_off, int ntens, long long total, const double* d_reduce,
                  int world, double* d_partials, int* d_rguard, bool to_params);
void optim_fill(hipStream_t st, float* p, long long n, float val);
void optim_set_steps(hipStream_t st, long long* d_t, long long steps);      // *d_t = steps, by a launch (tfl_optim_set_state)

// conv2d_mfma.hip (2-D default topology: 16 channels, k = 3; one MFMA = one tap x four input channels)
void conv2_mfma_first_fused(hipStream_t st, int B, int Y, int X, const float* pDiv, const float* div, const float* flags,
                            const double* stats, double count, const float* bfrag, const float* bias, float* out16);
void conv2_mfma_mid(hipStream_t st, int B, int Y, int X, const float* in16, const float* bfrag, const float* bias,
                    float* out16);
void conv2_mfma_tail(hipStream_t st, int B, int Y, int X, const float* in16, const float* bfrag, const float* bias,
                     const float* w5, const float* b5, float* p_out);

}  // namespace tfl
