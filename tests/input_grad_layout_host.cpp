// A stand-alone host program over the host arithmetic of tfl_model_backward_input -- fluidnet_amd/csrc/tfl_input_grad.hpp (the
// net input's channel map, the workspace layout behind tfl_model_backward's, the partial-sum slots), the two new weight forms of
// tfl_train.hpp (relay_first_transposed, relay_skip) and their device-refresh maps of tfl_refresh.hpp (refresh_wt_src with
// wt_first, refresh_ws_src) -- on host buffers sized exactly, so that AddressSanitizer / UBSan see any index that leaves them,
// and the gathers are held to the host packers byte for byte. No GPU, no HIP call.
// Built and run by tests/test_input_grad_layout_cpu.py:  g++ -std=c++17 -fsanitize=address,undefined input_grad_layout_host.cpp
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../fluidnet_amd/csrc/tfl_input_grad.hpp"
#include "../fluidnet_amd/csrc/tfl_refresh.hpp"

#define CHECK(c) do { if (!(c)) { std::fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #c); std::exit(1); } } while (0)

using namespace tfl;

// the channel map: the fields in model.lua's order, the occupancy channel behind them, a width the convolutions have
static void check_chans() {
  for (int is3d = 0; is3d < 2; is3d++)
    for (int m = 1; m < 8; m++) {
      const int ip = m & 1, iu = (m >> 1) & 1, id = (m >> 2) & 1, C = is3d ? 3 : 2;
      const IgChans c = ig_chans(is3d != 0, ip, iu, id);
      CHECK(c.nx == ip + iu * C + id && c.nx >= 1 && c.nx <= 5);
      CHECK((c.p >= 0) == (ip != 0) && (c.u >= 0) == (iu != 0) && (c.d >= 0) == (id != 0));
      std::vector<int> owner(c.nx, 0);
      if (ip) owner[c.p]++;
      if (iu) for (int k = 0; k < C; k++) owner[c.u + k]++;
      if (id) owner[c.d]++;
      for (int o : owner) CHECK(o == 1);
      if (ip && iu) CHECK(c.p < c.u);
      if (iu && id) CHECK(c.u < c.d);
      if (ip && id) CHECK(c.p < c.d);
      const int w = ig_width(c.nx);
      CHECK(w >= c.nx && w < 2 * c.nx + 1 && (w == 1 || w == 2 || w == 4 || w == 8));
    }
}

// the two weight forms: the host packers against their definition, and the device gathers against the host packers
static void check_forms(bool is3d, int in_c, int cout_ref, int cout_p, int k, int last_cin_ref, int last_cin_p, int last_k) {
  const int taps = train_taps(is3d, k), nx = in_c - 1, gxc = ig_width(nx);
  std::vector<float> w((size_t)cout_ref * in_c * taps), b(cout_ref, 0.5f);
  for (size_t i = 0; i < w.size(); i++) w[i] = 1.0f + (float)i;
  std::vector<float> relaid, bias_p, wt;
  relay_layer(1, taps, in_c, cout_p, in_c, cout_ref, w.data(), b.data(), [](int ci) { return ci; }, relaid, bias_p);
  relay_first_transposed(taps, in_c, cout_p, nx, gxc, relaid.data(), wt);
  CHECK(wt.size() == (size_t)taps * cout_p * gxc);
  for (int t = 0; t < taps; t++)
    for (int co = 0; co < cout_p; co++)
      for (int ci = 0; ci < gxc; ci++) {
        const float want = (ci < nx && co < cout_ref) ? w[((size_t)co * in_c + ci) * taps + (taps - 1 - t)] : 0.0f;
        CHECK(wt[((size_t)t * cout_p + co) * gxc + ci] == want);
      }
  RefreshLayer L{};
  L.S = 1; L.taps = taps; L.cin = in_c; L.cout = cout_p; L.cin_ref = in_c; L.cout_ref = cout_ref;
  L.cin_t = gxc; L.wt_first = nx; L.n_wt = taps * cout_p * gxc;
  std::vector<float> dev((size_t)L.n_wt, -7.0f);
  for (int d = 0; d < L.n_wt; d++) {
    const long long s = refresh_wt_src(L, d);
    CHECK(s < (long long)w.size());
    dev[(size_t)d] = s >= 0 ? w[(size_t)s] : 0.0f;
  }
  CHECK(std::memcmp(dev.data(), wt.data(), wt.size() * sizeof(float)) == 0);
  // the last layer with the joined skip channel on its last padded plane
  const int lt = train_taps(is3d, last_k);
  std::vector<float> lw((size_t)last_cin_ref * lt), lb(1, 0.25f), ws;
  for (size_t i = 0; i < lw.size(); i++) lw[i] = 100.0f + (float)i;
  auto cmap = [&](int ci) { return ci == last_cin_ref - 1 ? last_cin_p - 1 : ci; };
  relay_layer(1, lt, last_cin_p, 1, last_cin_ref, 1, lw.data(), lb.data(), cmap, relaid, bias_p);
  relay_skip(lt, last_cin_p, 1, relaid.data(), ws);
  CHECK(ws.size() == (size_t)lt);
  for (int t = 0; t < lt; t++) CHECK(ws[(size_t)t] == lw[(size_t)(last_cin_ref - 1) * lt + (lt - 1 - t)]);
  RefreshLayer K{};
  K.S = 1; K.taps = lt; K.cin = last_cin_p; K.cout = 1; K.cin_ref = last_cin_ref; K.cout_ref = 1; K.skip_in = 1;
  K.cin_t = last_cin_p - 1; K.n_ws = lt;
  std::vector<float> dws((size_t)K.n_ws, -7.0f);
  for (int d = 0; d < K.n_ws; d++) {
    const long long s = refresh_ws_src(K, d);
    CHECK(s >= 0 && s < (long long)lw.size());
    dws[(size_t)d] = lw[(size_t)s];
  }
  CHECK(std::memcmp(dws.data(), ws.data(), ws.size() * sizeof(float)) == 0);
  // (and the existing form of the same layer is untouched by wt_first = 0: its first plane still maps to a real channel)
  CHECK(refresh_wt_src(K, 0) >= 0);
}

// the workspace: tfl_model_backward's part unchanged in front, the new regions behind it in order, disjoint, the fp64 ones aligned;
// every partial slot of every (item, block, term) inside its region and owned once
static void check_layout(bool is3d, const std::vector<TrainLayer>& L, int ip, int iu, int id, bool skip, bool from_div, int B, int Z, int Y, int X) {
  const IgChans ch = ig_chans(is3d, ip, iu, id);
  const IgLayout w = ig_layout(is3d, L, ch, skip, from_div, B, Z, Y, X);
  const BwdLayout b = bwd_layout(is3d, L, B, Z, Y, X);
  const int64_t cells = (int64_t)Z * Y * X, n = B * cells;
  CHECK(w.bwd.total == b.total && w.bwd.g0 == b.g0 && w.bwd.g1 == b.g1 && w.bwd.gu == b.gu && w.bwd.partials == b.partials);
  CHECK(w.gx == b.total && w.gxc == ig_width(ch.nx));
  CHECK(w.gskip == w.gx + n * w.gxc);
  CHECK(w.ubc == w.gskip + (skip ? n : 0));
  CHECK(w.recompute_div == (from_div && !id));
  CHECK(w.div == w.ubc + (w.recompute_div ? n * (is3d ? 3 : 2) : 0));
  CHECK(w.partials >= w.div + (w.recompute_div ? n : 0) && w.partials - (w.div + (w.recompute_div ? n : 0)) <= 1);
  CHECK(w.partials % 2 == 0 && w.gs % 2 == 0);
  CHECK(w.blocks == ig_sum_blocks(cells) && w.blocks >= 1 && w.blocks <= kIgSumMaxBlocks);
  CHECK((int64_t)w.blocks * kIgSumThreads <= cells + (int64_t)kIgCellsPerBlock || w.blocks == 1);
  CHECK(w.gs == w.partials + 2 * (int64_t)B * w.blocks * kIgTerms);
  CHECK(w.total == w.gs + 2 * (int64_t)B);
  std::vector<double> partials((size_t)B * w.blocks * kIgTerms, 0.0);
  for (int bi = 0; bi < B; bi++)
    for (int blk = 0; blk < w.blocks; blk++)
      for (int t = 0; t < kIgTerms; t++) partials[(size_t)ig_partial_slot(bi, w.blocks, blk, t)] += 1.0;
  for (double v : partials) CHECK(v == 1.0);
}

int main() {
  check_chans();
  check_forms(false, 3, 16, 16, 3, 17, 17, 1);      // 2-D default with the skip
  check_forms(true, 3, 8, 8, 3, 9, 9, 1);           // 3-D default with the skip
  check_forms(true, 3, 8, 8, 5, 9, 9, 1);           // k5-skip
  check_forms(true, 3, 6, 8, 3, 7, 9, 3);           // yang: 6 channels padded to 8, the skip plane behind the padding
  check_forms(true, 6, 8, 8, 3, 9, 9, 1);           // every input channel, 3-D: nx = 5 -> 8 planes
  check_forms(false, 4, 16, 16, 3, 17, 17, 3);      // UDiv + div, 2-D: nx = 3 -> 4 planes
  check_forms(false, 2, 16, 16, 1, 17, 17, 1);      // one field: nx = 1
  const std::vector<TrainLayer> d2 = {{3, 16, 3, 16, 3, 0}, {16, 16, 16, 16, 3, 0}, {16, 1, 16, 1, 1, 0}};
  const std::vector<TrainLayer> s3 = {{6, 8, 6, 8, 5, 0}, {8, 8, 8, 8, 3, 0}, {9, 1, 9, 1, 1, 1}};
  const int shapes[][4] = {{2, 1, 9, 33}, {3, 1, 5, 130}, {1, 8, 12, 36}, {1, 3, 4, 66}, {1, 1, 1, 2}, {1, 64, 64, 64}, {2, 128, 128, 128}};
  for (const auto& s : shapes) {
    const bool is3d = s[1] > 1;
    for (int m = 1; m < 8; m++)
      for (int skip = 0; skip < 2; skip++)
        for (int fd = 0; fd < 2; fd++)
          check_layout(is3d, is3d ? s3 : d2, m & 1, (m >> 1) & 1, (m >> 2) & 1, skip != 0, fd != 0, s[0], s[1], s[2], s[3]);
  }
  std::printf("input grad layout OK\n");
  return 0;
}
