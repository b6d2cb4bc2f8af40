// A stand-alone host program over the host arithmetic of the banked models' training pass (fluidnet_amd/csrc/tfl_train.hpp,
// tfl_input_grad.hpp): the extended tape and workspace layouts, the weight-gradient plan and chunk walk at tap
// spacing 1 / 2 / 4 with the dilated halo and tap offsets, and the index maps of the join's and the pyramid pool's backward --
// on host buffers sized exactly, so that AddressSanitizer / UBSan see any index that leaves them, with coverage counted: in
// bounds, disjoint, complete. No GPU, no HIP call.
// Built and run by tests/test_bank_layout_cpu.py:  g++ -std=c++17 -fsanitize=address,undefined bank_layout_host.cpp
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <utility>
#include <vector>

#include "../fluidnet_amd/csrc/tfl_input_grad.hpp"
#include "../fluidnet_amd/csrc/tfl_train.hpp"

#define CHECK(c) do { if (!(c)) { std::fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #c); std::exit(1); } } while (0)

using namespace tfl;

// a banked model as model_train.cpp's train_layers / train_banks describe it: `pre` trunk stages, `nst` banked stages of n banks,
// `post` trunk stages (the last one the 1-channel output); c channels, kernel size k in the banked stages
struct Model { std::vector<TrainLayer> L; TrainBanks bk; };
static Model make(bool is3d, int n, bool mres, bool concat, int pre, int nst, int post, int in_c, int c, int k, bool skip) {
  Model m;
  m.bk.n = n; m.bk.is3d = is3d; m.bk.mres = mres; m.bk.concat = concat; m.bk.l0 = pre; m.bk.nst = nst; m.bk.gxc = ig_width(in_c - 1);
  int cin = in_c;
  for (int s = 0; s < pre; s++) { m.L.push_back(TrainLayer{cin, c, cin, c, 3, 0}); cin = c; }
  for (int s = 0; s < nst; s++) {
    for (int i = 0; i < n; i++) {
      TrainLayer t{cin, c, cin, c, k, 0};
      t.dil = mres ? 1 : 1 << i;
      t.sh = mres ? i : 0;
      m.L.push_back(t);
    }
    cin = c;
  }
  cin = concat ? c * n : c;
  for (int s = 0; s < post; s++) {
    const bool last = s + 1 == post;
    const int ci = cin + (last && skip ? 1 : 0);
    m.L.push_back(TrainLayer{ci, last ? 1 : c, ci, last ? 1 : c, 1, last && skip ? 1 : 0});
    cin = c;
  }
  return m;
}

// [offset, offset + size) of every entry of a layout: inside [0, total), pairwise disjoint, and together all of it
static void check_partition(std::vector<std::pair<int64_t, int64_t>> e, int64_t total, int64_t slack) {
  std::sort(e.begin(), e.end());
  int64_t end = 0, gaps = 0;
  for (const auto& p : e) {
    CHECK(p.first >= end && p.second >= 0);
    gaps += p.first - end;
    end = p.first + p.second;
  }
  CHECK(end <= total && gaps + (total - end) <= slack);
}

static void check_layouts(const Model& m, int B, int Z, int Y, int X) {
  const bool is3d = m.bk.is3d;
  const int nl = (int)m.L.size();
  const int64_t n = (int64_t)B * Z * Y * X;
  const TapeLayout t = tape_layout(m.L, B, Z, Y, X, &m.bk);
  std::vector<std::pair<int64_t, int64_t>> e;
  e.push_back({t.stats, 4 * (int64_t)B});
  e.push_back({t.x, n * m.L[0].cin});
  CHECK((int)t.out.size() == nl - 1 && t.planes.size() == t.out.size() && t.sh.size() == t.out.size());
  for (int l = 0; l + 1 < nl; l++) {
    CHECK(t.planes[l] == train_och(m.L, l) && t.sh[l] == m.L[l].sh);
    e.push_back({t.out[l], (int64_t)B * train_cells(is3d, t.sh[l], Z, Y, X) * t.planes[l]});
  }
  CHECK(t.pyr_c == m.L[m.bk.l0].cin && t.join_c == m.L[m.bk.end()].cin - m.L[m.bk.end()].skip_in);
  for (int i = 1; i < m.bk.n && m.bk.mres; i++) e.push_back({t.pyr[i], (int64_t)B * train_cells(is3d, i, Z, Y, X) * t.pyr_c});
  e.push_back({t.join, n * t.join_c});
  e.push_back({t.pPred, n});
  check_partition(e, t.total, 0);

  const IgChans ch = ig_chans(is3d, 1, m.L[0].cin > 3 ? 1 : 0, 1);
  const IgLayout ig = ig_layout(is3d, m.L, ch, m.L.back().skip_in != 0, false, B, Z, Y, X, &m.bk);
  const BwdLayout w = bwd_layout(is3d, m.L, B, Z, Y, X, &m.bk);
  CHECK(ig.bwd.total == w.total && ig.gx == w.total);
  e.clear();
  int64_t pd = 0;
  for (const TrainLayer& l : m.L) pd = std::max(pd, wg_plan(is3d, l, B, Z, Y, X).partial_doubles);
  e.push_back({w.partials, 2 * pd});
  e.push_back({w.g0, n * w.gc});
  e.push_back({w.g1, n * w.gc});
  e.push_back({w.gu, n * (is3d ? 3 : 2)});
  int64_t slack = 0;
  for (int i = 0; i < m.bk.n; i++) {
    const int64_t nb = (int64_t)B * train_cells(is3d, m.L[m.bk.mod(0, i)].sh, Z, Y, X) * w.gbc;
    e.push_back({w.gb[i][0], nb});
    e.push_back({w.gb[i][1], nb});
    slack += 2 * (nb & 1);
    if (m.bk.mres) CHECK(w.gb[i][0] % 2 == 0 && w.gb[i][1] % 2 == 0);      // k_pyr_pool_bwd moves 8-byte pairs
    // every gradient a bank's buffers hold fits: the join's slice, every module's data gradient, the net input's
    for (int s = 0; s < m.bk.nst; s++) CHECK(m.L[m.bk.mod(s, i)].cout <= w.gbc && m.L[m.bk.mod(s, i)].cin <= w.gbc);
    if (m.bk.l0 == 0) CHECK(m.bk.gxc <= w.gbc && ig.gxc == m.bk.gxc);
  }
  check_partition(e, w.total, slack);
  CHECK(t.join_c <= w.gc);                      // the data gradient of the stage behind the join
  if (m.bk.mres) CHECK(w.g1 % 2 == 0 && ig.gx % 2 == 0);
}

// the chunk walk of k_conv_wgrad at the module's tap spacing, through the index helpers the kernel calls: every x-tile slot a tap
// reads lies inside the dilated halo tile, distinct taps of a channel read distinct slots, the halo is what the taps reach
static void check_walk(bool is3d, const TrainLayer& L, int B, int Z, int Y, int X) {
  const WgPlan p = wg_plan(is3d, L, B, Z, Y, X);
  if (p.lds_floats > 16384) return;      // (conv_wgrad_fits: such a model is not trainable)
  CHECK(p.dil == L.dil && p.ch >= 1 && p.S >= 1 && p.nblocks >= 1 && p.nblocks <= p.tiles);
  const int M = L.cin * p.taps, r = L.dil * (L.k / 2);
  const WgHalo h = wg_halo(is3d, L.k, L.dil);
  CHECK(h.r == r && h.HX == kWgTX + 2 * r && h.HY == kWgTY + 2 * r && h.HZ == (is3d ? 2 * r + 1 : 1) && h.floats == p.halo_floats);
  CHECK(p.ch * h.floats + kWgThreads * p.cb <= p.lds_floats);
  std::vector<int> xs((size_t)p.ch * h.floats, -1);
  std::vector<double> partials((size_t)p.partial_doubles, -1.0);
  for (int co0 = 0; co0 < L.cout; co0 += p.cb)
    for (int ci0 = 0; ci0 < L.cin; ci0 += p.ch)
      for (int t0 = 0; t0 < p.taps; t0 += p.tt) {
        const WgChunk ck = wg_chunk(p.ch, p.tt, L.cin, p.taps, ci0, t0);
        CHECK(ck.R * p.S <= kWgThreads);
        for (int tid = 0; tid < kWgThreads; tid++) {
          const WgThread t = wg_thread(tid, ck, h, p.S, ci0, t0, L.k, p.taps, is3d, M, L.dil);
          if (!t.active) continue;
          if (!t.is_bias) {
            // voxel v = (vx, vy) of the tile reads x at tile offset + dil (tap - k/2) + halo radius, per axis
            const int dx = t.tap % L.k, dy = (t.tap / L.k) % L.k, dz = is3d ? t.tap / (L.k * L.k) : 0;
            for (int v = t.s; v < kWgThreads; v += p.S) {
              const int slot = wg_x_slot(t, h, v);
              CHECK(slot >= t.cl * h.floats && slot < (t.cl + 1) * h.floats);
              const int vx = v % kWgTX, vy = v / kWgTX;
              const int want = t.cl * h.floats + ((dz * L.dil) * h.HY + (vy + dy * L.dil)) * h.HX + (vx + dx * L.dil);
              CHECK(slot == want);
              xs[(size_t)slot] = 1;
            }
          }
          if (t.s != 0 || co0 != 0) continue;
          double& slot = partials[(size_t)wg_partial_slot(0, M, t.row, L.cout, 0)];
          CHECK(slot == -1.0);        // every row of the layer once
          slot = 1.0;
        }
      }
  for (int row = 0; row <= M; row++) CHECK(partials[(size_t)wg_partial_slot(0, M, row, L.cout, 0)] == 1.0);
  // the extreme taps reach the halo's faces: the halo is no wider than the taps need
  if (L.k > 1) CHECK(xs[0] == 1 && xs[(size_t)h.floats - 1] == 1);
}

// the join's backward: over all banks and their cells, the children of the coarse cells tile every fine plane exactly once per
// bank (add), the channel slices tile the join's planes exactly once (concat)
static void check_join(bool is3d, bool concat, int n, bool mres, int C, int Z, int Y, int X) {
  const int och = concat ? n * C : C;
  const int64_t cells = (int64_t)Z * Y * X;
  std::vector<int> hit((size_t)och * cells, 0);
  for (int i = 0; i < n; i++) {
    const int sh = mres ? i : 0;
    const int Zs = is3d ? Z >> sh : Z, Ys = Y >> sh, Xs = X >> sh;
    CHECK(train_cells(is3d, sh, Z, Y, X) == (int64_t)Zs * Ys * Xs);
    const int kids = join_bwd_children(is3d, sh);
    for (int c = 0; c < C; c++) {
      const int plane = join_bwd_plane(concat, i, C, c);
      CHECK(plane >= 0 && plane < och);
      for (int z = 0; z < Zs; z++)
        for (int y = 0; y < Ys; y++)
          for (int x = 0; x < Xs; x++)
            for (int q = 0; q < kids; q++) {
              const long long o = join_bwd_child(is3d, sh, z, y, x, q, Y, X);
              CHECK(o >= 0 && o < cells);
              // the child is a cell the nearest up-sample filled from (z, y, x)
              const int fx = (int)(o % X), fy = (int)((o / X) % Y), fz = (int)(o / ((long long)X * Y));
              CHECK((fx >> sh) == x && (fy >> sh) == y && (is3d ? fz >> sh : fz) == z);
              hit[(size_t)plane * cells + o]++;
            }
    }
  }
  for (int v : hit) CHECK(v == (concat ? 1 : n));
}

// the pyramid pool's backward: every fine cell reads one coarse cell inside the coarse plane, and every coarse cell is read by
// exactly 2^dim fine cells (its children under the 2x average pooling); the kernel's pairs (two x-children) tile the fine plane
static void check_pyramid(bool is3d, int Z, int Y, int X) {
  const int Zc = is3d ? Z / 2 : Z, Yc = Y / 2, Xc = X / 2;
  std::vector<int> reads((size_t)Zc * Yc * Xc, 0), fine((size_t)Z * Y * X, 0);
  const long long pairs = (long long)Z * Y * (X / 2);
  for (long long t = 0; t < pairs; t++) {
    const int Xh = X >> 1;
    const int xc = (int)(t % Xh), y = (int)((t / Xh) % Y), z = (int)(t / ((long long)Xh * Y));
    const long long par = pyr_bwd_parent(is3d, z, y, 2 * xc, Y, X);
    CHECK(par == pyr_bwd_parent(is3d, z, y, 2 * xc + 1, Y, X));
    CHECK(par >= 0 && par < (long long)reads.size());
    CHECK(par == ((long long)(is3d ? z / 2 : z) * Yc + y / 2) * Xc + xc);
    reads[(size_t)par] += 2;
    const long long o = ((long long)z * Y + y) * X + 2 * xc;
    fine[(size_t)o]++; fine[(size_t)o + 1]++;
  }
  for (int v : reads) CHECK(v == (is3d ? 8 : 4));
  for (int v : fine) CHECK(v == 1);
}

// the stage behind a concat join of padded banks (yang: 6 real channels on 8 planes per bank): every cudnn weight element is the
// image of exactly one (row, co) of the padded gradient, through the inverse of the forward's plane map
static void check_join_weight_map(int n, int join_c, int join_p, int cout_ref, int cout_p, int taps) {
  const int cin = n * join_p, cin_ref = n * join_c;
  std::vector<int> hit((size_t)cout_ref * cin_ref * taps, 0);
  for (int row = 0; row < cin * taps; row++)
    for (int co = 0; co < cout_p; co++) {
      const long long i = wg_cudnn_index(row, co, taps, cin, cin_ref, cout_ref, 0, join_c, join_p);
      if (i < 0) continue;
      CHECK(i < (long long)hit.size());
      hit[(size_t)i]++;
      const int cr = (int)((i / taps) % cin_ref), plane = row / taps;
      CHECK(i / ((long long)taps * cin_ref) == co && i % taps == row % taps);
      CHECK(plane == (cr / join_c) * join_p + cr % join_c);        // (model_build.cpp upload_layer's cmap)
    }
  for (int h : hit) CHECK(h == 1);
}

int main() {
  for (int n = 2; n <= 3; n++) {
    check_join_weight_map(n, 6, 8, 6, 8, 1);
    check_join_weight_map(n, 6, 8, 6, 8, 27);
    check_join_weight_map(n, 8, 8, 8, 8, 9);
    check_join_weight_map(n, 16, 16, 16, 16, 9);
  }
  // the grids of tests/model_bank_grad_ref.py, the loop's, and the benchmark's
  const int grids[][4] = {{2, 1, 24, 40}, {2, 8, 12, 36}, {2, 1, 32, 32}, {1, 128, 128, 128}, {16, 1, 128, 128}};
  for (const auto& g : grids) {
    const bool is3d = g[1] > 1;
    for (int n = 2; n <= 3; n++)
      for (int mres = 0; mres < 2; mres++)
        for (int concat = 0; concat < 2; concat++) {
          // the default split (the first stage) and a split behind a trunk stage; 8 (3-D) / 16 (2-D) channels; with and without UDiv
          const Model models[] = {make(is3d, n, mres, concat, 0, 2, 3, 3, is3d ? 8 : 16, 3, false),
                                  make(is3d, n, mres, concat, 1, 2, 2, 3, is3d ? 8 : 16, 3, false),
                                  make(is3d, n, mres, concat, 0, 1, 3, is3d ? 6 : 5, 6, 3, false),
                                  make(is3d, n, mres, concat, 0, 2, 3, 3, 8, 3, !mres)};
          for (const Model& m : models) {
            check_layouts(m, g[0], g[1], g[2], g[3]);
            if (g[0] * g[1] * g[2] * g[3] > 100000) continue;      // (the walks do not depend on the grid beyond the tile count)
            for (const TrainLayer& l : m.L) check_walk(is3d, l, g[0], g[1], g[2], g[3]);
          }
          if (g[0] * g[1] * g[2] * g[3] > 100000) continue;
          check_join(is3d, concat != 0, n, mres != 0, is3d ? 8 : 16, g[1], g[2], g[3]);
        }
    if (g[0] * g[1] * g[2] * g[3] > 100000) continue;
    check_pyramid(is3d, g[1], g[2], g[3]);
    check_pyramid(is3d, is3d ? g[1] / 2 : g[1], g[2] / 2, g[3] / 2);
  }
  // tap spacings 1, 2, 4 at k = 1, 3, 5, 2-D and 3-D: the plan is legal or the model is refused (3-D, k = 3, d = 4: two channels)
  for (int is3d = 0; is3d < 2; is3d++)
    for (int k : {1, 3, 5})
      for (int d : {1, 2, 4})
        for (int c : {1, 6, 8, 16}) {
          TrainLayer t{c, c, c, c, k, 0};
          t.dil = d;
          check_walk(is3d != 0, t, 2, is3d ? 8 : 1, 12, 36);
        }
  {
    TrainLayer t{8, 8, 8, 8, 3, 0};
    t.dil = 4;
    const WgPlan p = wg_plan(true, t, 2, 8, 12, 36);
    CHECK(p.halo_floats == 5760 && p.ch == 2 && p.lds_floats <= 16384);
    // tap spacing 1: the plan of the linear models, unchanged
    t.dil = 1;
    const WgPlan q = wg_plan(true, t, 2, 8, 12, 36);
    CHECK(q.halo_floats == 34 * 10 * 3 && q.ch == 8 && q.tt == 27 && q.S == 1);
  }
  std::puts("bank layout OK");
  return 0;
}
