// tfl_train.hpp -- the host arithmetic of the training side of the projection ConvNet (tfl_model_set_weights, _forward_train,
// _backward): weight re-layouts, the tape and workspace layouts with their size checks, the chunking of the weight-gradient
// kernel and the map from its (row, co) results back to the cudnn layout. Plain C++ without a HIP call, so that a stand-alone
// host program can run all of it under a sanitizer (tests/train_layout_host.cpp); tfl_model.hpp (for model_build.cpp and model_train.cpp) and conv_bwd.hip include it.
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
// A module of a banked model also has its tap spacing `dil` (dilate banks: 2^bank) and the resolution it runs at,
// grid >> sh per pooled axis (mres banks: sh = bank).
// A layer of a linear model that changes the resolution has `pool` = 2 (2x average pooling behind its
// activation) or `up` = 2 (ConvolutionUpsample: up^dim sub-position convolutions whose outputs are pixel-shuffled); its
// convolution runs at grid >> sh, its output out[l] lies at grid >> train_out_sh, and what the next layer reads at one more
// shift where it pools.
struct TrainLayer { int cin, cout, cin_ref, cout_ref, k, skip_in; int dil = 1, sh = 0; int pool = 1, up = 1; };
inline int train_subs(bool is3d, const TrainLayer& L) { return is3d ? L.up * L.up * L.up : L.up * L.up; }
inline int train_out_sh(const TrainLayer& L) { return L.sh - (L.up > 1 ? 1 : 0); }
inline bool train_multires(const std::vector<TrainLayer>& L) {
  for (const TrainLayer& l : L) if (l.pool > 1 || l.up > 1) return true;
  return false;
}

// The banks of a graph model as the training side sees them: modules [l0, l0 + nst * n) of the layer table are banked, module
// l0 + s * n + i = stage s of bank i. n = 1: a linear model. gxc: the width of the first layer's data gradient (ig_width), which
// the banks' gradient buffers must hold where the split is the first stage.
constexpr int kTrainMaxBanks = 8;
struct TrainBanks {
  int n = 1;
  bool is3d = false, mres = false, concat = false;
  int l0 = 0, nst = 0, gxc = 0;
  bool any() const { return n > 1; }
  int mod(int s, int i) const { return l0 + s * n + i; }
  int end() const { return l0 + nst * n; }
  bool banked(int l) const { return n > 1 && l >= l0 && l < end(); }
};
// cells of one plane at resolution grid >> sh (2-D: z is not pooled); the grid is divisible by 2^sh (graph_gate)
inline int64_t train_cells(bool is3d, int sh, int Z, int Y, int X) { return (int64_t)(is3d ? Z >> sh : Z) * (Y >> sh) * (X >> sh); }

// the widths the shape-generic convolution kernels write (1, 2, 4 ... 64): c rounded up to one (above 64: none, c itself)
inline int train_width(int c) {
  for (int w = 1; w <= 64; w *= 2) if (c <= w) return w;
  return c;
}
inline int train_taps(bool is3d, int k) { return is3d ? k * k * k : k * k; }
// channel planes of the saved output of layer l (the layer in front of the last also holds the skip channel)
inline int train_och(const std::vector<TrainLayer>& L, size_t l) { return L[l].cout + ((l + 2 == L.size() && L.back().skip_in) ? 1 : 0); }

// The tape of tfl_model_forward_train, in floats from its 8-byte aligned start:
//   [0, 4 B)   the input-scale pair (two doubles per item: what scale_from_stats reads)
//   x          the net input, [B][in_c] planes
//   out[l]     the post-activation output of every layer but the last, [B][och_l] planes (och: train_och)
//   pPred      the last layer's output, [B][1]
// A banked model (bk): out[l] of a banked module has its cout planes at the module's own resolution (planes[l], sh[l]), and
// behind the layers' outputs sit
//   pyr[i]     mres, bank i >= 1: level i of the average-pooling pyramid, [B][cin of the split stage] planes at grid >> i -- bank
//              i's first input, the x of its first weight gradient. Kept rather than pooled again in the backward: at 1/2^dim of
//              the level above it costs an eighth (a quarter) of one activation, against one more launch per level and pass.
//   join       the join's output, [B][join_c] planes at the grid's resolution: the x of the first stage behind the join
// A linear model with pooling / upsampling layers: out[l] is the post-activation output at the convolution's output resolution
// (an upsample layer's: behind the shuffle) -- what the activation mask reads --, and a pooling layer also keeps
//   pooled[l]  its pooled output, [B][cout] planes at half that resolution: the x of the next layer's weight gradient. Kept
//              rather than pooled again in the backward, for the reason the pyramid is kept: 1/2^dim of one activation against
//              one more launch per pooling layer and pass.
struct TapeLayout {
  int64_t stats, x, pPred, total;
  std::vector<int64_t> out;
  std::vector<int64_t> pooled;       // (0: the layer does not pool)
  std::vector<int> planes, sh;       // of out[l]
  int64_t pyr[kTrainMaxBanks] = {0, 0, 0, 0, 0, 0, 0, 0}, join = 0;
  int pyr_c = 0, join_c = 0;
};
inline TapeLayout tape_layout(const std::vector<TrainLayer>& L, int B, int Z, int Y, int X, const TrainBanks* bk = nullptr) {
  TapeLayout t;
  const bool is3d = bk && bk->is3d;
  int64_t off = 0;
  t.stats = off; off += 4 * (int64_t)B;
  t.x = off; off += (int64_t)B * Z * Y * X * L[0].cin;
  for (size_t l = 0; l + 1 < L.size(); l++) {
    const int osh = train_out_sh(L[l]);
    t.out.push_back(off); t.planes.push_back(train_och(L, l)); t.sh.push_back(osh);
    off += (int64_t)B * train_cells(is3d, osh, Z, Y, X) * train_och(L, l);
    t.pooled.push_back(L[l].pool > 1 ? off : 0);
    if (L[l].pool > 1) off += (int64_t)B * train_cells(is3d, osh + 1, Z, Y, X) * L[l].cout;
  }
  if (bk && bk->any()) {
    t.pyr_c = L[bk->l0].cin;
    for (int i = 1; i < bk->n && bk->mres; i++) { t.pyr[i] = off; off += (int64_t)B * train_cells(is3d, i, Z, Y, X) * t.pyr_c; }
    t.join_c = L[bk->mod(bk->nst - 1, 0)].cout * (bk->concat ? bk->n : 1);
    t.join = off; off += (int64_t)B * Z * Y * X * t.join_c;
  }
  t.pPred = off; off += (int64_t)B * Z * Y * X;
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
// (d: the tap spacing of a dilated bank's module, 1 | 2 | 4 ...: the halo radius is d (k / 2) and tap offsets are scaled by d)
struct WgHalo { int r, rz, HX, HY, HZ, floats; };
TFL_HD inline WgHalo wg_halo(bool is3d, int k, int d = 1) {
  WgHalo h;
  h.r = d * (k / 2); h.rz = is3d ? h.r : 0;
  h.HX = kWgTX + 2 * h.r; h.HY = kWgTY + 2 * h.r; h.HZ = 2 * h.rz + 1;
  h.floats = h.HX * h.HY * h.HZ;
  return h;
}
// What thread `tid` of the block does in a chunk: its voxel slice s (active while s < S), its row rr of the chunk -- the bias
// row or (channel cl of the chunk, tap) --, where its tap starts in the x tile (xoff) and its row of the whole layer (M = the bias)
struct WgThread { int s, rr, cl, tap, xoff, row; bool active, is_bias; };
TFL_HD inline WgThread wg_thread(int tid, const WgChunk& c, const WgHalo& h, int S, int ci0, int t0, int k, int taps, bool is3d, int M,
                                   int d = 1) {
  WgThread t;
  t.s = tid / c.R; t.rr = tid - t.s * c.R;
  t.active = t.s < S;
  t.is_bias = c.first && t.rr == c.nch * c.ntt;
  t.cl = t.is_bias ? 0 : t.rr / c.ntt;
  t.tap = t.is_bias ? 0 : t0 + (t.rr - t.cl * c.ntt);
  const int dx = t.tap % k, dy = (t.tap / k) % k, dz = is3d ? t.tap / (k * k) : 0;
  t.xoff = t.cl * h.floats + (dz * d * h.HY + dy * d) * h.HX + dx * d;
  t.row = t.is_bias ? M : (ci0 + t.cl) * taps + t.tap;
  return t;
}
TFL_HD inline int wg_x_slot(const WgThread& t, const WgHalo& h, int v) { return t.xoff + (v / kWgTX) * h.HX + (v % kWgTX); }   // voxel v of the tile
TFL_HD inline int wg_g_slot(int v, int cb, int c) { return v * cb + c; }
TFL_HD inline int wg_red_slot(const WgThread& t, const WgChunk& c, int s, int cb, int ch) { return (s * c.R + t.rr) * cb + ch; }   // fp64 words
TFL_HD inline long long wg_partial_slot(int blk, int M, int row, int cout, int co) { return ((long long)blk * (M + 1) + row) * cout + co; }

// (Z, Y, X: the grid; the plan is that of the module's own resolution, grid >> L.sh)
// An upsample layer is its inner convolution: subs * cout output channels on the layer's input grid, channel sub * cout + co
// = output channel co at sub-position sub (vcout of them; cb divides cout, so a register block never straddles two sub-positions)
struct WgPlan { int taps, cb, ch, tt, S, nblocks, halo_floats, lds_floats; int64_t tiles, partial_doubles; int dil; int up, subs, vcout; };
inline WgPlan wg_plan(bool is3d, const TrainLayer& L, int B, int Z, int Y, int X) {
  WgPlan p;
  if (is3d) Z >>= L.sh;
  Y >>= L.sh; X >>= L.sh;
  p.dil = L.dil;
  p.up = L.up; p.subs = train_subs(is3d, L); p.vcout = L.cout * p.subs;
  p.taps = train_taps(is3d, L.k);
  p.cb = L.cout < 16 ? L.cout : 16;
  p.halo_floats = wg_halo(is3d, L.k, L.dil).floats;
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
  const int64_t per_block = (L.cin * (int64_t)p.taps + 1) * p.vcout;
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
// reference channel. join_c > 0 (the stage behind a concat join): the banks' slices lie join_p planes apart and hold join_c real
// channels each, plane ci = reference channel (ci / join_p) * join_c + ci % join_p.
TFL_HD inline long long wg_cudnn_index(int row, int co, int taps, int cin, int cin_ref, int cout_ref, int skip_in, int join_c = 0,
                                       int join_p = 0) {
  const int ci = row / taps, tap = row - ci * taps;
  if (co >= cout_ref) return -1;
  int cr;
  if (skip_in && ci == cin - 1) cr = cin_ref - 1;
  else if (join_c > 0) {
    const int bank = ci / join_p, c = ci - bank * join_p;
    if (c >= join_c || bank * join_c + c >= cin_ref - (skip_in ? 1 : 0)) return -1;
    cr = bank * join_c + c;
  }
  else if (ci < cin_ref - (skip_in ? 1 : 0)) cr = ci;
  else return -1;
  return ((long long)co * cin_ref + cr) * taps + tap;
}

// The same for an upsample layer's inner convolution: column cv = sub * cout + co of the kernel -> output channel co * subs + sub of
// the cudnn layout [cout_ref * subs][cin_ref][taps] (tfl_refresh.hpp refresh_w_src, the other way round), or -1 for a padded
// plane; row < 0: the bias, [cout_ref * subs].
TFL_HD inline long long wg_cudnn_index_up(int row, int cv, int cout, int subs, int taps, int cin, int cin_ref, int cout_ref) {
  const int sub = cv / cout, co = cv - sub * cout;
  if (co >= cout_ref) return -1;
  if (row < 0) return (long long)co * subs + sub;
  return wg_cudnn_index(row, co * subs + sub, taps, cin, cin_ref, cout_ref * subs, 0);
}
// The fine cell that sub-position `sub` of conv-grid cell (z, y, x) is shuffled to, as an offset into a plane at up times the
// resolution [uz Z][up Y][up X] (uz = up in 3-D, 1 in 2-D): the forward's ConvUp (conv.hip), sub = (sz * up + sy) * up + sx.
TFL_HD inline long long up_fine_cell(bool is3d, int up, int sub, int z, int y, int x, int Y, int X) {
  const int sx = sub % up, sy = (sub / up) % up, sz = is3d ? sub / (up * up) : 0;
  return ((long long)((is3d ? z * up : z) + sz) * (Y * up) + (y * up + sy)) * ((long long)X * up) + (x * up + sx);
}

// The workspace of tfl_model_backward, in floats from its 8-byte aligned start: the fp64 partials of the widest layer, two
// gradient buffers of `gc` planes (g_out of a layer and its g_in), and the velocity-gradient scratch [B][C].
// A linear model with pooling / upsampling layers walks grids of several resolutions: its two buffers hold the
// largest gradient any layer has at its own resolution, which is less than gc planes of the full grid.
// A banked model (bk) has behind them two gradient buffers per bank, gb[i][0 | 1], of `gbc` planes at the bank's resolution: the
// join's backward fills one, the bank's layers walk the pair, and the split's backward reads the banks' last.
struct BwdLayout { int64_t partials, g0, g1, gu, total; int gc; int64_t gb[kTrainMaxBanks][2]; int gbc; };
inline BwdLayout bwd_layout(bool is3d, const std::vector<TrainLayer>& L, int B, int Z, int Y, int X, const TrainBanks* bk = nullptr) {
  BwdLayout w{};
  const int64_t n = (int64_t)B * Z * Y * X;
  int64_t pd = 0;
  int gc = 1;
  for (const TrainLayer& l : L) {
    const WgPlan p = wg_plan(is3d, l, B, Z, Y, X);
    if (p.partial_doubles > pd) pd = p.partial_doubles;
    if (l.cout > gc) gc = l.cout;
    // (the stage behind a concat join reads all the banks' planes: its data gradient is that wide)
    // (padded to a width the data-gradient convolution has: 3 x 8 planes come as 32)
    if (&l != &L[0] && train_width(l.cin - l.skip_in) > gc) gc = train_width(l.cin - l.skip_in);
  }
  w.gc = gc;
  // (a linear model with pooling / upsampling layers: the widest layer at its own resolution -- its gradient at the convolution's
  // output and its data gradient at the convolution's input --, rounded to 16 bytes for k_pool_bwd_mask's stores)
  int64_t gn = n * gc;
  if (train_multires(L)) {
    gn = n;
    for (const TrainLayer& l : L) {
      const int64_t go = (int64_t)B * train_cells(is3d, train_out_sh(l), Z, Y, X) * l.cout;
      const int64_t gi = &l != &L[0] ? (int64_t)B * train_cells(is3d, l.sh, Z, Y, X) * train_width(l.cin - l.skip_in) : 0;
      if (go > gn) gn = go;
      if (gi > gn) gn = gi;
    }
    gn = (gn + 3) & ~(int64_t)3;
  }
  w.partials = 0;
  w.g0 = 2 * pd;
  w.g1 = w.g0 + gn;
  w.gu = w.g1 + gn;
  w.total = w.gu + n * (is3d ? 3 : 2);
  if (bk && bk->any()) {
    int gbc = bk->l0 == 0 ? (bk->gxc > L[0].cin ? bk->gxc : L[0].cin) : L[bk->l0].cin;
    for (int l = bk->l0; l < bk->end(); l++) if (L[l].cout > gbc) gbc = L[l].cout;
    w.gbc = gbc;
    for (int i = 0; i < bk->n; i++) {
      int64_t nb = (int64_t)B * train_cells(is3d, L[bk->mod(0, i)].sh, Z, Y, X) * gbc;
      nb += nb & 1;      // (every buffer stays 8-byte aligned: k_pyr_pool_bwd moves pairs)
      w.gb[i][0] = w.total; w.gb[i][1] = w.total + nb;
      w.total += 2 * nb;
    }
  }
  return w;
}

// ---- the index maps of the three bank kernels of conv_bwd.hip (k_join_bwd, k_pyr_pool_bwd, k_bank_sum) -------------------------
// The join's backward: the gradient of bank i (C planes at grid >> sh) from g at the join's output (och planes at the grid's
// resolution). concat: the bank's channel slice; add: every bank reads all C channels.
TFL_HD inline int join_bwd_plane(bool concat, int i, int C, int c) { return concat ? i * C + c : c; }
// The nearest up-sample by 2^sh replicated coarse cell (z, y, x) over a block of children; child q of its (1 << sh)^dim, in the fixed
// order the sum takes them (x fastest), as an offset into the fine plane [Z][Y][X].
TFL_HD inline long long join_bwd_child(bool is3d, int sh, int z, int y, int x, int q, int Y, int X) {
  const int w = 1 << sh;
  const int dx = q % w, dy = (q / w) % w, dz = is3d ? q / (w * w) : 0;
  return ((long long)((is3d ? z * w : z) + dz) * Y + (y * w + dy)) * X + (x * w + dx);
}
TFL_HD inline int join_bwd_children(bool is3d, int sh) { return is3d ? 1 << (3 * sh) : 1 << (2 * sh); }
// The pyramid pool's backward: fine cell (z, y, x) of a [Z][Y][X] plane reads coarse cell (z/2, y/2, x/2) of [Z/2][Y/2][X/2]
TFL_HD inline long long pyr_bwd_parent(bool is3d, int z, int y, int x, int Y, int X) {
  return ((long long)(is3d ? z >> 1 : z) * (Y >> 1) + (y >> 1)) * (X >> 1) + (x >> 1);
}

}  // namespace tfl
