// tfl_train.hpp -- the host arithmetic of the training side of the projection ConvNet (tfl_model_set_weights, _forward_train,
// _backward): weight re-layouts, the tape and workspace layouts with their size checks, the chunking of the weight-gradient
// kernel and the map from its (row, co) results back to the cudnn layout. Plain C++ without a HIP call, so that a stand-alone
// host program can run all of it under a sanitizer (tests/train_layout_host.cpp); model_host.cpp and conv_bwd.hip include it.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#if defined(__HIPCC__)
#define TFL_HD __host__ __device__
#else
#define TFL_HD
#endif

namespace tfl {

// A module's cudnn weight [cout*S][cin][taps] (output channel index = o*S + sub) -> [sub][tap][cin_p][cout_p], reference input
// channel ci on plane cmap(ci), and its bias [cout*S] -> [sub][cout_p] (the padding holds zeros)
template <class Map>
void relay_layer(int S, int taps, int cin_p, int cout_p, int ci_n, int co_n, const float* w, const float* b, Map cmap,
                 std::vector<float>& relaid, std::vector<float>& bias_p) {
  relaid.assign((size_t)S * taps * cin_p * cout_p, 0.0f);
  for (int sub = 0; sub < S; sub++)
    for (int co = 0; co < co_n; co++)
      for (int ci = 0; ci < ci_n; ci++)
        for (int t = 0; t < taps; t++)
          relaid[(((size_t)sub * taps + t) * cin_p + cmap(ci)) * cout_p + co] = w[(((size_t)co * S + sub) * ci_n + ci) * taps + t];
  bias_p.assign((size_t)S * cout_p, 0.0f);
  for (int sub = 0; sub < S; sub++)
    for (int co = 0; co < co_n; co++) bias_p[(size_t)sub * cout_p + co] = b[(size_t)co * S + sub];
}

// The data-gradient form of a [tap][cin_p][cout_p] weight: the forward convolution with cin / cout swapped and the taps
// mirrored, wT[tap][co][ci] = w[taps - 1 - tap][ci][co] for the first `cin_t` input planes (a joined skip channel, which sits
// last, gets no data gradient and is left out).
inline void relay_transposed(int taps, int cin_p, int cout_p, int cin_t, const float* relaid, std::vector<float>& wt) {
  wt.assign((size_t)taps * cout_p * cin_t, 0.0f);
  for (int t = 0; t < taps; t++)
    for (int co = 0; co < cout_p; co++)
      for (int ci = 0; ci < cin_t; ci++)
        wt[((size_t)t * cout_p + co) * cin_t + ci] = relaid[((size_t)(taps - 1 - t) * cin_p + ci) * cout_p + co];
}

// The first layer's data-gradient form (tfl_model_backward_input): the same map for the first `nx` input planes -- the net input
// without its occupancy channel, which sits last and needs no gradient -- in a [tap][cout_p][gxc] array, gxc >= nx a width the
// convolution kernels have; the planes [nx, gxc) hold zeros.
inline void relay_first_transposed(int taps, int cin_p, int cout_p, int nx, int gxc, const float* relaid, std::vector<float>& wt) {
  wt.assign((size_t)taps * cout_p * gxc, 0.0f);
  for (int t = 0; t < taps; t++)
    for (int co = 0; co < cout_p; co++)
      for (int ci = 0; ci < nx; ci++)
        wt[((size_t)t * cout_p + co) * gxc + ci] = relaid[((size_t)(taps - 1 - t) * cin_p + ci) * cout_p + co];
}
// The joined skip channel's data-gradient form: the last layer's one output channel against its last input plane, mirrored,
// ws[tap] = w[taps - 1 - tap][cin_p - 1][0] -- a 1 -> 1 channel convolution of the gradient at pPred.
inline void relay_skip(int taps, int cin_p, int cout_p, const float* relaid, std::vector<float>& ws) {
  ws.assign((size_t)taps, 0.0f);
  for (int t = 0; t < taps; t++) ws[t] = relaid[((size_t)(taps - 1 - t) * cin_p + (cin_p - 1)) * cout_p];
}

// One layer as the training side sees it: padded and reference channel counts, kernel size, whether its last input plane is
// the joined pressure-skip channel.
struct TrainLayer { int cin, cout, cin_ref, cout_ref, k, skip_in; };

inline int train_taps(bool is3d, int k) { return is3d ? k * k * k : k * k; }
// channel planes of the saved output of layer l (the layer in front of the last also holds the skip channel)
inline int train_och(const std::vector<TrainLayer>& L, size_t l) { return L[l].cout + ((l + 2 == L.size() && L.back().skip_in) ? 1 : 0); }

// The tape of tfl_model_forward_train, in floats from its 8-byte aligned start:
//   [0, 4 B)   the input-scale pair (two doubles per item: what scale_from_stats reads)
//   x          the net input, [B][in_c] planes
//   out[l]     the post-activation output of every layer but the last, [B][och_l] planes (och: train_och)
//   pPred      the last layer's output, [B][1]
struct TapeLayout { int64_t stats, x, pPred, total; std::vector<int64_t> out; };
inline TapeLayout tape_layout(const std::vector<TrainLayer>& L, int B, int Z, int Y, int X) {
  TapeLayout t;
  const int64_t n = (int64_t)B * Z * Y * X;
  int64_t off = 0;
  t.stats = off; off += 4 * (int64_t)B;
  t.x = off; off += n * L[0].cin;
  for (size_t l = 0; l + 1 < L.size(); l++) { t.out.push_back(off); off += n * train_och(L, l); }
  t.pPred = off; off += n;
  t.total = off;
  return t;
}

// The weight-gradient kernel (conv_bwd.hip) sees a layer as rows (ci, tap) -- plus one row of ones, the bias -- times cout
// columns, and walks them in chunks: `cb` output channels held in registers, `ch` input channels staged in LDS with their halo,
// `tt` taps; a chunk's rows (at most 255, + the bias row in the first chunk) spread over the block's 256 threads, `S` threads
// (voxel slices) per row, added up in slice order inside the block. Every block leaves one fp64 partial per (row, co).
constexpr int kWgTX = 32, kWgTY = 8, kWgThreads = 256;
constexpr int kWgLdsFloats = 12 * 1024;             // x tile with halo: 48 KB
// The index arithmetic of k_conv_wgrad, shared with the host program that walks it under a sanitizer.
// A chunk: input channels [ci0, ci0 + nch) x taps [t0, t0 + ntt); the first chunk also carries the bias row. R = its rows.
struct WgChunk { int nch, ntt, R; bool first; };
TFL_HD inline WgChunk wg_chunk(int ch, int tt, int cin, int taps, int ci0, int t0) {
  WgChunk c;
  c.nch = ch < cin - ci0 ? ch : cin - ci0;
  c.ntt = tt < taps - t0 ? tt : taps - t0;
  c.first = ci0 == 0 && t0 == 0;
  c.R = c.nch * c.ntt + (c.first ? 1 : 0);
  return c;
}
// The LDS tile of x: [channel of the chunk][HZ][HY][HX]
struct WgHalo { int r, rz, HX, HY, HZ, floats; };
TFL_HD inline WgHalo wg_halo(bool is3d, int k) {
  WgHalo h;
  h.r = k / 2; h.rz = is3d ? h.r : 0;
  h.HX = kWgTX + 2 * h.r; h.HY = kWgTY + 2 * h.r; h.HZ = 2 * h.rz + 1;
  h.floats = h.HX * h.HY * h.HZ;
  return h;
}
// What thread `tid` of the block does in a chunk: its voxel slice s (active while s < S), its row rr of the chunk -- the bias
// row or (channel cl of the chunk, tap) --, where its tap starts in the x tile (xoff) and its row of the whole layer (M = the bias)
struct WgThread { int s, rr, cl, tap, xoff, row; bool active, is_bias; };
TFL_HD inline WgThread wg_thread(int tid, const WgChunk& c, const WgHalo& h, int S, int ci0, int t0, int k, int taps, bool is3d, int M) {
  WgThread t;
  t.s = tid / c.R; t.rr = tid - t.s * c.R;
  t.active = t.s < S;
  t.is_bias = c.first && t.rr == c.nch * c.ntt;
  t.cl = t.is_bias ? 0 : t.rr / c.ntt;
  t.tap = t.is_bias ? 0 : t0 + (t.rr - t.cl * c.ntt);
  const int dx = t.tap % k, dy = (t.tap / k) % k, dz = is3d ? t.tap / (k * k) : 0;
  t.xoff = t.cl * h.floats + (dz * h.HY + dy) * h.HX + dx;
  t.row = t.is_bias ? M : (ci0 + t.cl) * taps + t.tap;
  return t;
}
TFL_HD inline int wg_x_slot(const WgThread& t, const WgHalo& h, int v) { return t.xoff + (v / kWgTX) * h.HX + (v % kWgTX); }   // voxel v of the tile
TFL_HD inline int wg_g_slot(int v, int cb, int c) { return v * cb + c; }
TFL_HD inline int wg_red_slot(const WgThread& t, const WgChunk& c, int s, int cb, int ch) { return (s * c.R + t.rr) * cb + ch; }   // fp64 words
TFL_HD inline long long wg_partial_slot(int blk, int M, int row, int cout, int co) { return ((long long)blk * (M + 1) + row) * cout + co; }

struct WgPlan { int taps, cb, ch, tt, S, nblocks, halo_floats, lds_floats; int64_t tiles, partial_doubles; };
inline WgPlan wg_plan(bool is3d, const TrainLayer& L, int B, int Z, int Y, int X) {
  WgPlan p;
  p.taps = train_taps(is3d, L.k);
  p.cb = L.cout < 16 ? L.cout : 16;
  p.halo_floats = wg_halo(is3d, L.k).floats;
  p.tt = p.taps < 255 ? p.taps : 255;
  int ch = 255 / p.tt, fit = kWgLdsFloats / p.halo_floats;
  if (ch > fit) ch = fit;
  if (ch > L.cin) ch = L.cin;
  p.ch = ch < 1 ? 1 : ch;
  const int rows = p.ch * p.tt + 1;
  p.S = kWgThreads / rows < 1 ? 1 : kWgThreads / rows;
  // LDS: the x tile with its halo and the tile's g [voxel][cb]; the slices' fp64 sums [thread][cb] reuse it (S > 1)
  p.lds_floats = p.ch * p.halo_floats + kWgThreads * p.cb;
  if (p.S > 1 && p.lds_floats < 2 * kWgThreads * p.cb) p.lds_floats = 2 * kWgThreads * p.cb;
  p.tiles = (int64_t)B * Z * ((Y + kWgTY - 1) / kWgTY) * ((X + kWgTX - 1) / kWgTX);
  // blocks: one per tile up to the count that keeps the partials of this layer near 16 MB
  const int64_t per_block = (L.cin * (int64_t)p.taps + 1) * L.cout;
  int64_t nb = (16ll << 20) / (8 * per_block);
  if (nb > 1024) nb = 1024;
  if (nb < 8) nb = 8;
  if (nb > p.tiles) nb = p.tiles;
  p.nblocks = (int)nb;
  p.partial_doubles = nb * per_block;
  return p;
}

// (row, co) of a layer's weight gradient -> its place in the cudnn layout [cout_ref][cin_ref][taps], or -1 for a padded plane.
// row = ci * taps + tap over the padded input planes; a joined skip channel sits on the last padded plane and is the last
// reference channel.
TFL_HD inline long long wg_cudnn_index(int row, int co, int taps, int cin, int cin_ref, int cout_ref, int skip_in) {
  const int ci = row / taps, tap = row - ci * taps;
  if (co >= cout_ref) return -1;
  int cr;
  if (skip_in && ci == cin - 1) cr = cin_ref - 1;
  else if (ci < cin_ref - (skip_in ? 1 : 0)) cr = ci;
  else return -1;
  return ((long long)co * cin_ref + cr) * taps + tap;
}

// The workspace of tfl_model_backward, in floats from its 8-byte aligned start: the fp64 partials of the widest layer, two
// gradient buffers of `gc` planes (g_out of a layer and its g_in), and the velocity-gradient scratch [B][C].
struct BwdLayout { int64_t partials, g0, g1, gu, total; int gc; };
inline BwdLayout bwd_layout(bool is3d, const std::vector<TrainLayer>& L, int B, int Z, int Y, int X) {
  BwdLayout w;
  const int64_t n = (int64_t)B * Z * Y * X;
  int64_t pd = 0;
  int gc = 1;
  for (const TrainLayer& l : L) {
    const WgPlan p = wg_plan(is3d, l, B, Z, Y, X);
    if (p.partial_doubles > pd) pd = p.partial_doubles;
    if (l.cout > gc) gc = l.cout;
  }
  w.gc = gc;
  w.partials = 0;
  w.g0 = 2 * pd;
  w.g1 = w.g0 + n * gc;
  w.gu = w.g1 + n * gc;
  w.total = w.gu + n * (is3d ? 3 : 2);
  return w;
}

}  // namespace tfl
