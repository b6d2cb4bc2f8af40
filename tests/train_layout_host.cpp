// A stand-alone host program over fluidnet_amd/csrc/tfl_train.hpp -- the re-layouts of tfl_model_set_weights, the tape and
// workspace layouts with their sizes, the chunk walk of the weight-gradient kernel and its map back to the cudnn layout --
// on host buffers sized exactly, so that AddressSanitizer / UBSan see any index that leaves them. No GPU, no HIP call.
// Built and run by tests/test_train_layout_cpu.py:  g++ -std=c++17 -fsanitize=address,undefined train_layout_host.cpp
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../fluidnet_amd/csrc/tfl_train.hpp"

#define CHECK(c) do { if (!(c)) { std::fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #c); std::exit(1); } } while (0)

using namespace tfl;

static int taps_of(bool is3d, int k) { return train_taps(is3d, k); }

// the re-layouts: every cudnn element lands where conv_direct / the data-gradient convolution read it
static void check_relayout(bool is3d, int cin_ref, int cout_ref, int cin_p, int cout_p, int k, bool skip_in) {
  const int taps = taps_of(is3d, k);
  std::vector<float> w((size_t)cout_ref * cin_ref * taps), b(cout_ref);
  for (size_t i = 0; i < w.size(); i++) w[i] = 1.0f + (float)i;
  for (size_t i = 0; i < b.size(); i++) b[i] = -1.0f - (float)i;
  auto cmap = [&](int ci) { return (skip_in && ci == cin_ref - 1) ? cin_p - 1 : ci; };
  std::vector<float> relaid, bias_p, wt;
  relay_layer(1, taps, cin_p, cout_p, cin_ref, cout_ref, w.data(), b.data(), cmap, relaid, bias_p);
  CHECK(relaid.size() == (size_t)taps * cin_p * cout_p && bias_p.size() == (size_t)cout_p);
  size_t nonzero = 0;
  for (float v : relaid) nonzero += v != 0.0f;
  CHECK(nonzero == w.size());
  for (int co = 0; co < cout_ref; co++)
    for (int ci = 0; ci < cin_ref; ci++)
      for (int t = 0; t < taps; t++)
        CHECK(relaid[((size_t)t * cin_p + cmap(ci)) * cout_p + co] == w[((size_t)co * cin_ref + ci) * taps + t]);
  const int cin_t = cin_p - (skip_in ? 1 : 0);
  relay_transposed(taps, cin_p, cout_p, cin_t, relaid.data(), wt);
  CHECK(wt.size() == (size_t)taps * cout_p * cin_t);
  for (int t = 0; t < taps; t++)
    for (int co = 0; co < cout_p; co++)
      for (int ci = 0; ci < cin_t; ci++)
        CHECK(wt[((size_t)t * cout_p + co) * cin_t + ci] == relaid[((size_t)(taps - 1 - t) * cin_p + ci) * cout_p + co]);
  // the way back: every (row, co) of the padded gradient maps to its own cudnn element or to none
  std::vector<int> hit(w.size(), 0);
  for (int row = 0; row < cin_p * taps; row++)
    for (int co = 0; co < cout_p; co++) {
      const long long i = wg_cudnn_index(row, co, taps, cin_p, cin_ref, cout_ref, skip_in ? 1 : 0);
      if (i < 0) continue;
      CHECK(i < (long long)w.size());
      hit[(size_t)i]++;
      const int ci = row / taps, t = row % taps;
      CHECK(relaid[((size_t)t * cin_p + ci) * cout_p + co] == w[(size_t)i]);      // the same element the forward laid there
    }
  for (int h : hit) CHECK(h == 1);
}

// the chunk walk of k_conv_wgrad on the host, through the index helpers the kernel itself calls (wg_chunk, wg_thread, wg_x_slot,
// wg_g_slot, wg_red_slot, wg_partial_slot): every row exactly once per output-channel block, every LDS and partial index
// inside its buffer
static void check_walk(bool is3d, const TrainLayer& L, int B, int Z, int Y, int X) {
  const WgPlan p = wg_plan(is3d, L, B, Z, Y, X);
  CHECK(p.ch >= 1 && p.tt >= 1 && p.tt <= 255 && p.S >= 1 && p.nblocks >= 1 && p.nblocks <= p.tiles);
  const int M = L.cin * p.taps;
  const WgHalo h = wg_halo(is3d, L.k);
  CHECK(h.floats == p.halo_floats);
  std::vector<char> xs((size_t)p.ch * h.floats), gs((size_t)kWgThreads * p.cb);
  CHECK(p.lds_floats >= (int)(xs.size() + gs.size()));
  std::vector<double> red((size_t)p.lds_floats / 2);          // the slices' sums reuse the LDS
  std::vector<double> partials((size_t)p.partial_doubles, -1.0);
  for (int blk = 0; blk < p.nblocks; blk += (p.nblocks > 3 ? p.nblocks - 1 : 1)) {      // the first and the last block
    for (int co0 = 0; co0 < L.cout; co0 += p.cb)
      for (int ci0 = 0; ci0 < L.cin; ci0 += p.ch)
        for (int t0 = 0; t0 < p.taps; t0 += p.tt) {
          const WgChunk ck = wg_chunk(p.ch, p.tt, L.cin, p.taps, ci0, t0);
          CHECK(ck.R * p.S <= kWgThreads);
          for (int tid = 0; tid < kWgThreads; tid++) {
            const WgThread t = wg_thread(tid, ck, h, p.S, ci0, t0, L.k, p.taps, is3d, M);
            gs[(size_t)wg_g_slot(tid, p.cb, p.cb - 1)] = 1;        // (every thread stages its voxel's g)
            if (!t.active) continue;
            for (int v = t.s; v < kWgThreads; v += p.S) {
              if (!t.is_bias) xs[(size_t)wg_x_slot(t, h, v)] = 1;
              gs[(size_t)wg_g_slot(v, p.cb, p.cb - 1)] = 1;
            }
            if (p.S > 1) red[(size_t)wg_red_slot(t, ck, t.s, p.cb, p.cb - 1)] = 1.0;
            if (t.s != 0) continue;
            for (int c = 0; c < p.cb; c++) {
              double& slot = partials[(size_t)wg_partial_slot(blk, M, t.row, L.cout, co0 + c)];
              CHECK(slot == -1.0);        // written once
              slot = 1.0;
            }
          }
        }
    for (int row = 0; row <= M; row++)
      for (int co = 0; co < L.cout; co++) CHECK(partials[(size_t)wg_partial_slot(blk, M, row, L.cout, co)] == 1.0);
  }
}

int main() {
  // re-layouts: plain, padded (yang's 6 -> 8), with the joined skip channel, 2-D and 3-D, k = 1 / 3 / 5
  check_relayout(true, 3, 8, 3, 8, 3, false);
  check_relayout(true, 6, 6, 8, 8, 1, false);
  check_relayout(false, 6, 1, 8, 1, 1, false);
  check_relayout(false, 17, 1, 17, 1, 1, true);
  check_relayout(true, 9, 1, 9, 1, 1, true);
  check_relayout(false, 7, 1, 9, 1, 3, true);       // padded planes between the real channels and the skip channel
  check_relayout(false, 3, 8, 3, 8, 5, false);
  check_relayout(true, 16, 16, 16, 16, 3, false);
  // layouts and the chunk walk over the test grids and a 128^3 / 128^2 one
  const int grids[][4] = {{2, 5, 7, 19}, {1, 8, 12, 36}, {1, 3, 4, 66}, {2, 1, 9, 33}, {1, 1, 16, 64}, {3, 1, 5, 130}, {1, 128, 128, 128},
                          {16, 1, 128, 128}};
  const TrainLayer tables[][5] = {
      {{3, 8, 3, 8, 3, 0}, {8, 8, 8, 8, 3, 0}, {8, 8, 8, 8, 3, 0}, {8, 8, 8, 8, 1, 0}, {8, 1, 8, 1, 1, 0}},
      {{3, 16, 3, 16, 3, 0}, {16, 16, 16, 16, 3, 0}, {16, 16, 16, 16, 3, 0}, {16, 16, 16, 16, 3, 0}, {17, 1, 17, 1, 1, 1}},
      {{3, 8, 3, 6, 3, 0}, {8, 8, 6, 6, 1, 0}, {8, 8, 6, 6, 1, 0}, {8, 1, 6, 1, 1, 0}, {0, 0, 0, 0, 0, 0}},
      {{3, 8, 3, 8, 5, 0}, {8, 8, 8, 8, 3, 0}, {9, 1, 9, 1, 1, 1}, {0, 0, 0, 0, 0, 0}, {0, 0, 0, 0, 0, 0}},
      {{5, 64, 5, 64, 7, 0}, {64, 32, 64, 32, 5, 0}, {32, 1, 32, 1, 9, 0}, {0, 0, 0, 0, 0, 0}, {0, 0, 0, 0, 0, 0}},
  };
  for (const auto& g : grids)
    for (const auto& tab : tables) {
      const bool is3d = g[1] > 1;
      std::vector<TrainLayer> L;
      for (const TrainLayer& l : tab) if (l.cin) L.push_back(l);
      const TapeLayout t = tape_layout(L, g[0], g[1], g[2], g[3]);
      const int64_t n = (int64_t)g[0] * g[1] * g[2] * g[3];
      CHECK(t.stats == 0 && t.x == 4 * g[0] && t.out.size() + 1 == L.size());
      int64_t end = t.x + n * L[0].cin;
      for (size_t l = 0; l + 1 < L.size(); l++) { CHECK(t.out[l] == end); end += n * train_och(L, l); CHECK(train_och(L, l) == L[l + 1].cin); }
      CHECK(t.pPred == end && t.total == end + n);
      const BwdLayout w = bwd_layout(is3d, L, g[0], g[1], g[2], g[3]);
      CHECK(w.partials == 0 && (w.g0 % 2) == 0 && w.g1 == w.g0 + n * w.gc && w.gu == w.g1 + n * w.gc && w.total == w.gu + n * (is3d ? 3 : 2));
      for (const TrainLayer& l : L) {
        const WgPlan p = wg_plan(is3d, l, g[0], g[1], g[2], g[3]);
        CHECK(2 * p.partial_doubles <= w.g0 && l.cout <= w.gc);
        if (p.lds_floats <= 16384) check_walk(is3d, l, g[0], g[1], g[2], g[3]);
      }
    }
  std::puts("train layout OK");
  return 0;
}
