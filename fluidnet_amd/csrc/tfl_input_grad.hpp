// tfl_input_grad.hpp -- the host arithmetic of tfl_model_backward_input: where the net input's fields sit among
// its channel planes, the width of the first layer's data gradient, and the workspace layout behind tfl_model_backward's own.
// Plain C++ without a HIP call, so that a stand-alone host program can walk all of it under a sanitizer
// (tests/input_grad_layout_host.cpp); model_build.cpp, model_train.cpp and input_grad.hip include it.
#pragma once
#include <cstdint>
#include <vector>

#include "tfl_train.hpp"

namespace tfl {

// The channel planes of the net input x = {pDiv/s?, U_bc/s (C)?, div/s?, occupancy}: the first plane of each field, or -1 where
// the field is switched off; nx = the planes in front of the occupancy channel (the ones that get a gradient).
struct IgChans { int p, u, d, nx; };
inline IgChans ig_chans(bool is3d, int in_pDiv, int in_UDiv, int in_div) {
  IgChans c;
  int ch = 0;
  c.p = in_pDiv ? ch : -1; ch += in_pDiv ? 1 : 0;
  c.u = in_UDiv ? ch : -1; ch += in_UDiv ? (is3d ? 3 : 2) : 0;
  c.d = in_div ? ch : -1; ch += in_div ? 1 : 0;
  c.nx = ch;
  return c;
}
// nx padded to an output width the shape-generic convolution has (1, 2, 4, 8: nx is at most 5)
inline int ig_width(int nx) {
  int w = 1;
  while (w < nx) w *= 2;
  return w;
}

// the five dot products of the scale's gradient, per batch item
enum { kIgP = 0, kIgU = 1, kIgQp = 2, kIgQu = 3, kIgQd = 4, kIgTerms = 5 };
constexpr int kIgSumThreads = 256, kIgSumMaxBlocks = 1024, kIgCellsPerBlock = 1024, kIgFinishLanes = 64;
// blocks per batch item of k_input_grad_sums: one per 1024 cells, 1024 at the most (a block strides over the item's cells). The pass
// is a stream of some 25 floats per cell: with fewer blocks than these it is bound by latency, not by bandwidth (128 blocks of
// 2048+ cells took 452 us at 128^3: profiles/model_input_grad.md)
inline int ig_sum_blocks(int64_t cells) {
  const int64_t nb = (cells + kIgCellsPerBlock - 1) / kIgCellsPerBlock;
  return (int)(nb < 1 ? 1 : (nb > kIgSumMaxBlocks ? kIgSumMaxBlocks : nb));
}
// the fp64 partial of (item b, block blk, term t)
TFL_HD inline long long ig_partial_slot(int b, int nblocks, int blk, int t) { return ((long long)b * nblocks + blk) * kIgTerms + t; }

// The workspace of tfl_model_backward_input, in floats from its 8-byte aligned start: tfl_model_backward's layout unchanged in
// front (`bwd`), then
//   gx       the first layer's data gradient, [B][gxc] planes
//   gskip    the joined skip channel's gradient, [B][1] (skip models only)
//   ubc, div SetWallBcs(UDiv) [B][C] and its divergence [B][1]: only where the scale is taken from the divergence and the net
//            input has no div channel to read it back from (recompute_div)
//   partials [B][blocks][5] doubles, gs [B] doubles (8-byte aligned)
struct IgLayout { BwdLayout bwd; int64_t gx, gskip, ubc, div, partials, gs, total; int gxc, blocks; bool recompute_div; };
inline IgLayout ig_layout(bool is3d, const std::vector<TrainLayer>& L, const IgChans& ch, bool skip, bool norm_from_div, int B, int Z,
                          int Y, int X, const TrainBanks* bk = nullptr) {
  IgLayout w;
  w.bwd = bwd_layout(is3d, L, B, Z, Y, X, bk);
  const int64_t cells = (int64_t)Z * Y * X, n = (int64_t)B * cells;
  w.gxc = ig_width(ch.nx);
  w.blocks = ig_sum_blocks(cells);
  w.recompute_div = norm_from_div && ch.d < 0;
  int64_t off = w.bwd.total;
  w.gx = off; off += n * w.gxc;
  w.gskip = off; off += skip ? n : 0;
  w.ubc = off; off += w.recompute_div ? n * (is3d ? 3 : 2) : 0;
  w.div = off; off += w.recompute_div ? n : 0;
  off += off & 1;
  w.partials = off; off += 2 * (int64_t)B * w.blocks * kIgTerms;
  w.gs = off; off += 2 * (int64_t)B;
  w.total = off;
  return w;
}

}  // namespace tfl
