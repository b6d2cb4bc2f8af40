// advect_vel3.hip -- advectVel on a 3-D MAC grid, trace-based methods (eulerOurs, maccormackOurs): the
// north-star's "advection kernel" (third_party/tfluids.cc:594-632 SemiLagrangeEulerOursMAC, :660-699
// MacCormackCorrectMAC, :748-774 MacCormackClampMAC; generic/calc_line_trace.cc:313-503).
//
// The gather kernels of advect.hip spend their time in two places (profiles/r02_pmc_sq.txt): the
// vector ALU (650 instructions per wave: three IEEE divisions and a full-range sqrt per trace, branchy
// out-of-domain / obstacle handling whose phi copies are 17 % of the stream, clamped index arithmetic, 64-bit
// addresses) and the texture addresser (123 gather instructions per wave). Here:
//
//  * FAST PATH / SLOW PATH. A cell whose three back-traces are "ordinary" -- fluid cell that is not a border cell, displacement shorter than 0.99 cell, end point in a fluid cell -- needs none of the reference's
//    special cases: ONE trace step, no wall clipping, no ray/box test, no index clamps, every tap inside the 3^3
//    neighbourhood of the cell. That path is straight-line code with the reference's operation order; the
//    division by the trace length uses one refined reciprocal for the three components and the norm a one-step
//    corrected v_sqrt: the root checked exhaustively, the quotient SAMPLE-verified bit-equal to sqrtf() / `/` on the operand range (tfl_fastmath.hpp,
//    tools/ubench/exact_math.hip). Every other lane (walls, obstacles' neighbours, fast flow) runs the generic
//    functions of tfl_device.hpp / tfl_advect.hpp afterwards, from scratch: same result as before by construction.
//  * LDS TILE. Per 64x4x1-cell block the 66x6x3 halo tile of U (3 components) and flags is staged once with
//    coalesced row loads (one field per wave; scalar row pointers, no per-lane address arithmetic); the 18 MAC taps,
//    the trace's flag look-ups, the forward pass's 24 interpolation taps and the backward pass's 48 clamp corners
//    are ds_reads with immediate offsets from one address VGPR. Only the backward pass's 24 interpolation taps of
//    the forward field remain global gathers, issued for the three components together (one L2 round trip).
//  * What bounds these kernels now (profiles/r03_pmc_adv.txt, profiles/r01_r04_where_the_time_went.md): instruction ISSUE -- a SIMD retires one
//    instruction of any kind (VALU, SALU, LDS, VMEM) per ~2.7 clocks here, so the count of ALL instructions per
//    wave is the budget; packed fp32 (v_pk_mul/add) issues at half rate and buys nothing (SLP vectorisation is off
//    for this file). A z-marched variant (4-slot plane ring, 1.55x instead of 4.6x staging) issued 24 % fewer
//    instructions per cell but lost more to block-count quantisation at 128^3 (2048 long blocks on 256 CUs).
//
// Algorithmic HBM bytes per cell are unchanged: pass A 28 B (U3, flags -> fwd3), pass B 40 B (fwd3, U3, flags -> dst3).
//
// The kernels themselves are in advect_vel3_kernels.hpp, one source templated on the block depth (planes per block); this file
// picks the depth and launches them.
#include "advect_vel3_kernels.hpp"

#include <cstdlib>

namespace tfl {
namespace {
using namespace vel3;

// launches of block depth KZ (advect_vel3 picks the depth by grid size): 1 = a block is 64 x 4 cells of one plane (the round-3
// kernels: 54 / 72 VGPRs, no SGPR spills in pass A), 2 = two planes per block on one staged tile (3.1 instead of 4.6 staged words
// per cell and field, at the price of registers -- 63 / 94 VGPRs, SGPR spills): the better one once the staging traffic leaves
// the caches. Only the one-plane pass B takes the folds' requests `f` (k_vel3_bwd_fold); a deeper launch leaves them untaken.
// scan (not null: the caller has checked that pass A covers the whole array): pass A in its scanning form, advect_scalar3_sparse.hip.
template <int KZ>
void launch(hipStream_t st, bool two_pass, const AdvArgs& a, int B, const float* U, const float* flags, float* fwd, float* dst,
            int stages, Fold& f, Vel3ScanAsk* scan = nullptr) {
  const Dom& d = a.d;
  const int groups = (d.n0 + KZ - 1) / KZ + (d.nw - d.n0 + KZ - 1) / KZ;      // (KZ = 1: the window's planes, d.nw)
  const dim3 blk(TX, TY, 1), grd((d.X + TX - 1) / TX, (d.Y + TY - 1) / TY, (unsigned)(groups * B));
  const bool pa = stages & 2, pb = stages & 4;
  float* outA = two_pass ? fwd : dst;
  const double hs = (double)a.strength * 0.5;
  if (pa && scan) {
    vel3_fwd_scan(st, KZ, a, B, U, flags, outA, *scan);
    scan->took = true;
  } else if (pa) {
    TFL_TIMED_EXT("k_vel_fwd", st);
    if (a.fast) TFL_LAUNCH_EXT((k_vel3_fwd<KZ, true>), grd, blk, 0, st, a, U, flags, outA);
    else TFL_LAUNCH_EXT((k_vel3_fwd<KZ, false>), grd, blk, 0, st, a, U, flags, outA);
  }
  if (two_pass && pb) {
    TFL_TIMED_EXT("k_vel_bwd", st);
    if constexpr (KZ == 1) {
      const BcFoldArg fold = f.hand_bc();    // pass B writes the operator's result
      const BuoyFold by = f.hand_buoy();     // ... and may add the buoyancy force that follows it in simulate()
      const bool y_only = by.rho && by.sx == 0.0f && by.sz == 0.0f && by.sy != 0.0f;
      if (y_only) {
        if (a.fast) TFL_LAUNCH_EXT((k_vel3_bwd_fold<true, 2>), grd, blk, 0, st, a, hs, U, flags, (const float*)fwd, dst, fold, by);
        else TFL_LAUNCH_EXT((k_vel3_bwd_fold<false, 2>), grd, blk, 0, st, a, hs, U, flags, (const float*)fwd, dst, fold, by);
      } else if (by.rho) {
        if (a.fast) TFL_LAUNCH_EXT((k_vel3_bwd_fold<true, 7>), grd, blk, 0, st, a, hs, U, flags, (const float*)fwd, dst, fold, by);
        else TFL_LAUNCH_EXT((k_vel3_bwd_fold<false, 7>), grd, blk, 0, st, a, hs, U, flags, (const float*)fwd, dst, fold, by);
      } else {
        if (a.fast) TFL_LAUNCH_EXT((k_vel3_bwd_fold<true, 0>), grd, blk, 0, st, a, hs, U, flags, (const float*)fwd, dst, fold, by);
        else TFL_LAUNCH_EXT((k_vel3_bwd_fold<false, 0>), grd, blk, 0, st, a, hs, U, flags, (const float*)fwd, dst, fold, by);
      }
    } else {
      if (a.fast) TFL_LAUNCH_EXT((k_vel3_bwd<KZ, true>), grd, blk, 0, st, a, hs, U, flags, (const float*)fwd, dst);
      else TFL_LAUNCH_EXT((k_vel3_bwd<KZ, false>), grd, blk, 0, st, a, hs, U, flags, (const float*)fwd, dst);
    }
  }
}
}  // namespace

bool advect_vel3(hipStream_t st, bool two_pass, const AdvArgs& a, int B, const float* U, const float* flags, float* fwd,
                 float* dst, int stages, Fold& f, Vel3ScanAsk* scan) {
  const bool off = sw::present(Sw::ADVECT_GATHER);   // A/B switch: the round-2 gather kernels
  const int kz_env = sw::num(Sw::VEL3_KZ, 0);
  const Dom& d = a.d;
  // 24-bit multiplies address the planes (4*X*Y < 2^24); 32-bit BYTE offsets address the cells of all three channels
  // (o4 + 2*sc4 in the loads / stores of U, fwd, dst): 12*Z*Y*X < 2^32. Larger grids take the gather kernels.
  if (off || d.Z < 3 || (long long)d.X * d.Y * 4 >= (1 << 24) || 12ll * d.sc >= (1ll << 32)) return false;
  // block depth: at 128^3 the four fields' staging stays in the caches and the leaner one-plane kernels win (k_vel_bwd
  // 37.5 vs 42 us); from ~6 M cells per batch item on the two-plane kernels do (256^3: 285 vs 316 us, pass A 144 vs 175)
  const bool deep = kz_env ? kz_env >= 2 : (long long)d.sc >= 6000000ll;
  // ... unless pass B has been asked to add the buoyancy force (tfl_host.hpp BuoyFold): only the one-plane pass B carries that
  // fold (and the sparse setConstVals pair's) -- in the two-plane kernel it costs the fifth wave per SIMD -- and at 256^3 the
  // one-plane pass B with the force (~320 us) beats the two-plane one plus k_add_buoyancy and two k_apply_bcs_indexed
  // (291 + 94 + 11 us). Pass A stays two-plane. TFL_VEL3_KZ_B=2 keeps the old split.
  const bool b_shallow = deep && two_pass && (stages & 4) && f.buoy.rho && sw::num(Sw::VEL3_KZ_B, 0) != 2;
  // the scan request of tfl_simulate_step (tfl_host.hpp Vel3ScanAsk): only a pass A over the whole un-cut array at the array's
  // own origin sees every word once, in blocks that lie inside one brick each; a forced depth still gets THAT depth's kernel
  const bool whole = d.w0 == 0 && d.n0 == d.Z && d.nw == d.Z && d.zg == 0 && d.Zg == d.Z;
  Vel3ScanAsk* sc = scan && scan->s && two_pass && (stages & 2) && whole ? scan : nullptr;
  if (deep && b_shallow) {
    if (stages & 2) launch<2>(st, two_pass, a, B, U, flags, fwd, dst, stages & ~4, f, sc);
    launch<1>(st, two_pass, a, B, U, flags, fwd, dst, stages & ~2, f);
  } else if (deep) launch<2>(st, two_pass, a, B, U, flags, fwd, dst, stages, f, sc);
  else launch<1>(st, two_pass, a, B, U, flags, fwd, dst, stages, f, sc);
  return true;
}

}  // namespace tfl
