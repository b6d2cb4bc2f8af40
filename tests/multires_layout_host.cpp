// A stand-alone host program over the host arithmetic of the training pass of linear models with pooling / upsampling layers
// (fluidnet_amd/csrc/tfl_train.hpp, tfl_refresh.hpp, tfl_input_grad.hpp): the tape with the pooled outputs, the
// workspace whose gradient buffers follow the layers' own resolutions, the weight-gradient plan of an upsample layer's inner
// convolution with its strided read (up_fine_cell) and its way back to the cudnn layout (wg_cudnn_index_up), the data-gradient
// weights of every sub-position as the device refresh gathers them (refresh_wt_src), and the cell arithmetic of the fused pool
// backward -- on host buffers sized exactly, so that AddressSanitizer / UBSan see any index that leaves them, with coverage
// counted: in bounds, disjoint, complete. No GPU, no HIP call.
// Built and run by tests/test_model_multires_grad_cpu.py:  g++ -std=c++17 -fsanitize=address,undefined multires_layout_host.cpp
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <utility>
#include <vector>

#include "../fluidnet_amd/csrc/tfl_input_grad.hpp"
#include "../fluidnet_amd/csrc/tfl_refresh.hpp"
#include "../fluidnet_amd/csrc/tfl_train.hpp"

#define CHECK(c) do { if (!(c)) { std::fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #c); std::exit(1); } } while (0)

using namespace tfl;

// a layer table as model_train.cpp's train_layers describes it: the shift walks down with every pool and up with every upsample
struct Spec { int cout, k, pool, up; };
static std::vector<TrainLayer> make(const std::vector<Spec>& s, int in_c) {
  std::vector<TrainLayer> L;
  int cin = in_c, sh = 0;
  for (const Spec& q : s) {
    TrainLayer t{cin, q.cout, cin, q.cout, q.k, 0};
    t.pool = q.pool; t.up = q.up; t.sh = sh;
    sh += (q.pool > 1 ? 1 : 0) - (q.up > 1 ? 1 : 0);
    L.push_back(t);
    cin = q.cout;
  }
  CHECK(sh == 0);
  return L;
}
static const std::vector<Spec> kTog2 = {{16, 5, 2, 1}, {32, 5, 1, 1}, {32, 5, 1, 1}, {64, 5, 1, 1}, {64, 1, 1, 1}, {32, 1, 1, 1}, {1, 3, 1, 2}};
static const std::vector<Spec> kTog3 = {{16, 3, 2, 1}, {16, 3, 2, 1}, {16, 3, 1, 1}, {16, 3, 1, 1}, {32, 1, 1, 1}, {32, 1, 1, 2}, {1, 3, 1, 2}};
static const std::vector<Spec> kCustom = {{8, 3, 2, 1}, {8, 3, 1, 1}, {8, 1, 1, 2}, {1, 3, 1, 1}};

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

// the tape and the workspace, and the host walk of Backward::trunk_multires over them: every buffer it hands a kernel holds what
// the kernel writes
static void check_layouts(bool is3d, const std::vector<TrainLayer>& L, int B, int Z, int Y, int X) {
  TrainBanks bk;
  bk.is3d = is3d;
  const int nl = (int)L.size();
  const int64_t n = (int64_t)B * Z * Y * X;
  CHECK(train_multires(L));
  const TapeLayout t = tape_layout(L, B, Z, Y, X, &bk);
  std::vector<std::pair<int64_t, int64_t>> e;
  e.push_back({t.stats, 4 * (int64_t)B});
  e.push_back({t.x, n * L[0].cin});
  CHECK((int)t.out.size() == nl - 1 && (int)t.pooled.size() == nl - 1);
  for (int l = 0; l + 1 < nl; l++) {
    CHECK(t.sh[l] == train_out_sh(L[l]) && t.sh[l] >= 0 && t.planes[l] == L[l].cout);
    e.push_back({t.out[l], (int64_t)B * train_cells(is3d, t.sh[l], Z, Y, X) * L[l].cout});
    CHECK((t.pooled[l] > 0) == (L[l].pool > 1));
    if (L[l].pool > 1) e.push_back({t.pooled[l], (int64_t)B * train_cells(is3d, t.sh[l] + 1, Z, Y, X) * L[l].cout});
    // what the next layer reads lies at the next layer's resolution
    CHECK(L[l + 1].sh == t.sh[l] + (L[l].pool > 1 ? 1 : 0));
  }
  e.push_back({t.pPred, n});
  check_partition(e, t.total, 0);
  CHECK(train_out_sh(L.back()) == 0);

  const BwdLayout w = bwd_layout(is3d, L, B, Z, Y, X, &bk);
  const IgChans ch = ig_chans(is3d, 1, 0, 1);
  const IgLayout ig = ig_layout(is3d, L, ch, false, false, B, Z, Y, X, &bk);
  CHECK(ig.bwd.total == w.total && ig.gx == w.total);
  int64_t pd = 0;
  for (const TrainLayer& l : L) pd = std::max(pd, wg_plan(is3d, l, B, Z, Y, X).partial_doubles);
  const int64_t gn = w.g1 - w.g0;
  CHECK(w.partials == 0 && w.g0 == 2 * pd && w.gu - w.g1 == gn && w.total == w.gu + n * (is3d ? 3 : 2));
  CHECK(gn % 4 == 0 && w.g0 % 2 == 0);      // (16-byte rows where the workspace itself is 16-byte aligned)
  // the walk: g at the layer's output (behind the pool), through the pool into the other buffer, the data gradient into the other
  int64_t need = n;      // the gradient at pPred
  for (int l = nl - 1; l >= 0; l--) {
    const int64_t go = (int64_t)B * train_cells(is3d, train_out_sh(L[l]), Z, Y, X) * L[l].cout;
    if (L[l].pool > 1) need = std::max(need, go / (is3d ? 8 : 4));
    need = std::max(need, go);
    if (l > 0) need = std::max(need, (int64_t)B * train_cells(is3d, L[l].sh, Z, Y, X) * L[l].cin);
  }
  CHECK(need <= gn && gn < need + 4);
}

// the strided read of an upsample layer: over the sub-positions and the cells of the convolution's grid, up_fine_cell tiles the
// plane at up times the resolution exactly once, in the forward's order (conv.hip ConvUp: x offset = sub % up)
static void check_fine_cells(bool is3d, int up, int Z, int Y, int X) {
  const int subs = is3d ? up * up * up : up * up, uz = is3d ? up : 1;
  std::vector<int> hit((size_t)Z * uz * Y * up * X * up, 0);
  for (int sub = 0; sub < subs; sub++)
    for (int z = 0; z < Z; z++)
      for (int y = 0; y < Y; y++)
        for (int x = 0; x < X; x++) {
          const long long o = up_fine_cell(is3d, up, sub, z, y, x, Y, X);
          CHECK(o >= 0 && o < (long long)hit.size());
          const int fx = (int)(o % (X * up)), fy = (int)((o / (X * up)) % (Y * up)), fz = (int)(o / ((long long)X * up * Y * up));
          CHECK(fx == x * up + sub % up && fy == y * up + (sub / up) % up && fz == (is3d ? z * up + sub / (up * up) : z));
          hit[(size_t)o]++;
        }
  for (int v : hit) CHECK(v == 1);
}

// the inner convolution's (row, column) results -> the cudnn layout [cout_ref subs][cin_ref][taps] and [cout_ref subs]: every
// element the image of exactly one result, the padded planes of none; and the partials of the kernel's last block fit
static void check_weight_map(bool is3d, const TrainLayer& L, int cin_ref, int cout_ref) {
  const WgPlan p = wg_plan(is3d, L, 2, is3d ? 4 : 1, 8, 36);
  CHECK(p.lds_floats <= 16384);      // conv_wgrad_fits
  CHECK(p.up == L.up && p.subs == train_subs(is3d, L) && p.vcout == L.cout * p.subs && L.cout % p.cb == 0);
  const int M = L.cin * p.taps;
  CHECK(wg_partial_slot(p.nblocks - 1, M, M, p.vcout, p.vcout - 1) == p.partial_doubles - 1);
  std::vector<int> hw((size_t)cout_ref * p.subs * cin_ref * p.taps, 0), hb((size_t)cout_ref * p.subs, 0);
  for (int row = -1; row < M; row++)
    for (int cv = 0; cv < p.vcout; cv++) {
      const long long i = wg_cudnn_index_up(row, cv, L.cout, p.subs, p.taps, L.cin, cin_ref, cout_ref);
      const int sub = cv / L.cout, co = cv % L.cout;
      if (co >= cout_ref || (row >= 0 && row / p.taps >= cin_ref)) { CHECK(i < 0); continue; }
      std::vector<int>& h = row < 0 ? hb : hw;
      CHECK(i >= 0 && i < (long long)h.size());
      h[(size_t)i]++;
      if (row < 0) CHECK(i == co * p.subs + sub);
      else CHECK(i == (((long long)co * p.subs + sub) * cin_ref + row / p.taps) * p.taps + row % p.taps);
    }
  for (int v : hw) CHECK(v == 1);
  for (int v : hb) CHECK(v == 1);
}

// the device refresh of an upsample layer's data-gradient weights: the gather of refresh_wt_src over [sub][tap][cout][cin] against
// the host packers (relay_layer, then relay_transposed per sub-position), byte for byte; sources inside the cudnn weight
static void check_refresh(int S, int taps, int cin_p, int cout_p, int cin_ref, int cout_ref) {
  std::vector<float> w((size_t)cout_ref * S * cin_ref * taps), b((size_t)cout_ref * S, 0.0f);
  for (size_t i = 0; i < w.size(); i++) w[i] = (float)(i + 1);
  std::vector<float> relaid, bias, want, one;
  relay_layer(S, taps, cin_p, cout_p, cin_ref, cout_ref, w.data(), b.data(), [](int ci) { return ci; }, relaid, bias);
  for (int sub = 0; sub < S; sub++) {
    relay_transposed(taps, cin_p, cout_p, cin_p, relaid.data() + (size_t)sub * taps * cin_p * cout_p, one);
    want.insert(want.end(), one.begin(), one.end());
  }
  RefreshLayer r{};
  r.S = S; r.taps = taps; r.cin = cin_p; r.cout = cout_p; r.cin_ref = cin_ref; r.cout_ref = cout_ref; r.cin_t = cin_p;
  r.n_wt = S * taps * cout_p * cin_p;
  CHECK((size_t)r.n_wt == want.size());
  for (int d = 0; d < r.n_wt; d++) {
    const long long s = refresh_wt_src(r, d);
    CHECK(s < (long long)w.size());
    CHECK((s >= 0 ? w[(size_t)s] : 0.0f) == want[(size_t)d]);
  }
}

// k_pool_bwd_mask: a thread owns V consecutive x-cells of a fine row; the V it may be launched with tile the fine plane once, and
// cell i of the thread reads coarse cell parent + (i >> 1), inside the coarse plane, every coarse cell from its 2^dim children
static void check_pool_bwd(bool is3d, int Z, int Y, int X) {
  const int Zc = is3d ? Z / 2 : Z, Yc = Y / 2, Xc = X / 2;
  for (int V : {1, 2, 4}) {
    if (X % V) continue;
    std::vector<int> reads((size_t)Zc * Yc * Xc, 0), fine((size_t)Z * Y * X, 0);
    const int Xv = X / V;
    for (long long t = 0; t < (long long)Z * Y * Xv; t++) {
      const int xv = (int)(t % Xv), y = (int)((t / Xv) % Y), z = (int)(t / ((long long)Xv * Y));
      const long long par = pyr_bwd_parent(is3d, z, y, xv * V, Y, X);
      const long long o = ((long long)z * Y + y) * X + (long long)xv * V;
      for (int i = 0; i < V; i++) {
        const long long c = par + (i >> 1);
        CHECK(c >= 0 && c < (long long)reads.size());
        CHECK(c == pyr_bwd_parent(is3d, z, y, xv * V + i, Y, X));
        reads[(size_t)c]++;
        CHECK(o + i < (long long)fine.size());
        fine[(size_t)(o + i)]++;
      }
    }
    for (int v : reads) CHECK(v == (is3d ? 8 : 4));
    for (int v : fine) CHECK(v == 1);
  }
}

int main() {
  // the grids of tests/model_multires_grad_ref.py, the loop's, fit()'s and the two measured ones
  const int g3[][4] = {{2, 4, 8, 36}, {1, 8, 12, 68}, {4, 64, 64, 64}};
  const int g2[][4] = {{2, 1, 10, 34}, {1, 1, 16, 64}, {3, 1, 6, 132}, {2, 1, 16, 32}, {2, 1, 32, 32}, {16, 1, 128, 128}};
  for (const auto& g : g3) check_layouts(true, make(kTog3, 3), g[0], g[1], g[2], g[3]);
  for (const auto& g : g2) check_layouts(false, make(kTog2, 3), g[0], g[1], g[2], g[3]);
  check_layouts(false, make(kCustom, 3), 2, 1, 10, 68);
  check_layouts(true, make(kCustom, 3), 1, 4, 10, 36);
  check_layouts(true, make(kCustom, 5), 1, 2, 2, 6);      // (odd cell counts on the coarse level)
  // a model without such layers: the layouts of before (tests/train_layout_host.cpp holds them in full)
  {
    const std::vector<TrainLayer> L = make({{8, 3, 1, 1}, {8, 3, 1, 1}, {1, 1, 1, 1}}, 3);
    TrainBanks bk;
    CHECK(!train_multires(L));
    const BwdLayout w = bwd_layout(false, L, 2, 1, 9, 33, &bk);
    CHECK(w.gc == 8 && w.g1 - w.g0 == (int64_t)2 * 9 * 33 * 8 && w.gu - w.g1 == w.g1 - w.g0);
    const TapeLayout t = tape_layout(L, 2, 1, 9, 33, &bk);
    CHECK(t.pooled[0] == 0 && t.pooled[1] == 0 && t.total == 8 + 2 * 9 * 33 * (3 + 8 + 8 + 1));
  }
  for (int up : {2})
    for (int is3d = 0; is3d < 2; is3d++) {
      check_fine_cells(is3d != 0, up, is3d ? 1 : 1, 2, 9);
      check_fine_cells(is3d != 0, up, is3d ? 2 : 1, 3, 17);
    }
  for (int is3d = 0; is3d < 2; is3d++) {
    for (const TrainLayer& l : make(is3d ? kTog3 : kTog2, 3)) check_weight_map(is3d != 0, l, l.cin, l.cout);
    for (const TrainLayer& l : make(kCustom, 3)) check_weight_map(is3d != 0, l, l.cin, l.cout);
    TrainLayer pad{8, 8, 6, 6, 3, 0};      // (padded planes: 6 real channels on 8)
    pad.up = 2;
    check_weight_map(is3d != 0, pad, 6, 6);
    check_refresh(is3d ? 8 : 4, is3d ? 27 : 9, 32, 1, 32, 1);
    check_refresh(is3d ? 8 : 4, 1, 8, 8, 6, 6);
    check_refresh(1, is3d ? 27 : 9, 8, 8, 8, 8);
  }
  check_pool_bwd(true, 4, 8, 36);
  check_pool_bwd(true, 2, 6, 34);
  check_pool_bwd(false, 1, 10, 34);
  check_pool_bwd(false, 1, 6, 132);
  check_pool_bwd(false, 1, 2, 6);
  std::puts("multires layout OK");
  return 0;
}
