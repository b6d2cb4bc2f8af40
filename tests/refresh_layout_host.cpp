// A stand-alone host program over fluidnet_amd/csrc/tfl_refresh.hpp -- the gather maps of the device-side weight refresh
// (tfl_model_set_weights_device) and the flat parameter space of the optimiser step -- walked on the host exactly as the kernels
// of weights_refresh.hip / optim.hip walk them, over buffers sized exactly, so that AddressSanitizer / UBSan see any index that
// leaves them; every result is held to the host packers (tfl_train.hpp relay_layer / relay_transposed, tfl_pack.hpp) byte for
// byte. No GPU, no HIP call. Built and run by tests/test_refresh_layout_cpu.py:
//   g++ -std=c++17 -ffp-contract=off -fsanitize=address,undefined refresh_layout_host.cpp
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../fluidnet_amd/csrc/tfl_pack.hpp"
#include "../fluidnet_amd/csrc/tfl_refresh.hpp"
#include "../fluidnet_amd/csrc/tfl_train.hpp"

#define CHECK(c) do { if (!(c)) { std::fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #c); std::exit(1); } } while (0)

using namespace tfl;

static uint32_t g_seed = 12345u;
static float rnd() {      // in (-1, 1), never zero
  g_seed = g_seed * 1664525u + 1013904223u;
  const float v = ((float)((g_seed >> 8) & 0xffff) + 0.5f) / 65536.0f;
  return (g_seed & 0x80000000u) ? -v : v;
}
template <class T> static bool same_bytes(const std::vector<T>& a, const std::vector<T>& b) {
  return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(T)) == 0);
}

// ---- the generic forms: one layer as model_build.cpp build_layers lays it out -----------------------------------------------
static RefreshLayer layer_of(bool is3d, int k, int up, int cin_ref, int cout_ref, int cin_p, int cout_p, int join_c, int join_p, bool skip_in,
                             bool transposed) {
  RefreshLayer L{};
  L.taps = is3d ? k * k * k : k * k;
  L.S = is3d ? up * up * up : up * up;
  L.cin = cin_p; L.cout = cout_p; L.cin_ref = cin_ref; L.cout_ref = cout_ref;
  L.join_c = join_c; L.join_p = join_p; L.skip_in = skip_in ? 1 : 0;
  L.cin_t = cin_p - (skip_in ? 1 : 0);
  L.n_w = L.S * L.taps * L.cin * L.cout; L.n_b = L.S * L.cout; L.n_wt = transposed ? L.taps * L.cout * L.cin_t : 0;
  return L;
}
static void check_layer(const RefreshLayer& L) {
  std::vector<float> w((size_t)L.cout_ref * L.S * L.cin_ref * L.taps), b((size_t)L.cout_ref * L.S);
  for (float& v : w) v = rnd();
  for (float& v : b) v = rnd();
  auto cmap = [&](int ci) {      // model_build.cpp upload_layer
    return (L.skip_in && ci == L.cin_ref - 1) ? L.cin - 1 : L.join_c > 0 ? (ci / L.join_c) * L.join_p + ci % L.join_c : ci;
  };
  std::vector<float> relaid, bias_p, wt;
  relay_layer(L.S, L.taps, L.cin, L.cout, L.cin_ref, L.cout_ref, w.data(), b.data(), cmap, relaid, bias_p);
  // the walk of k_refresh_layers: d over [0, n_w + n_b + n_wt)
  std::vector<float> gw((size_t)L.n_w), gb((size_t)L.n_b), gwt((size_t)L.n_wt);
  std::vector<int> hit(w.size(), 0);
  for (int d = 0; d < L.n_w + L.n_b + L.n_wt; d++) {
    if (d < L.n_w) {
      const long long s = refresh_w_src(L, d);
      CHECK(s < (long long)w.size());
      gw[(size_t)d] = s >= 0 ? w[(size_t)s] : 0.0f;
      if (s >= 0) hit[(size_t)s]++;
    } else if (d < L.n_w + L.n_b) {
      const int e = d - L.n_w, s = refresh_b_src(L, e);
      gb[(size_t)e] = s >= 0 ? b[(size_t)s] : 0.0f;
    } else {
      const int e = d - L.n_w - L.n_b;
      const long long s = refresh_wt_src(L, e);
      gwt[(size_t)e] = s >= 0 ? w[(size_t)s] : 0.0f;
    }
  }
  CHECK(same_bytes(gw, relaid));
  CHECK(same_bytes(gb, bias_p));
  for (int h : hit) CHECK(h == 1);           // every cudnn element lands exactly once
  if (L.n_wt) {
    relay_transposed(L.taps, L.cin, L.cout, L.cin_t, relaid.data(), wt);
    CHECK(same_bytes(gwt, wt));
  }
}
static int padded(int c) { for (int w : {1, 2, 4, 8, 16, 32, 64}) if (c <= w) return w; return -1; }
// a linear model: layer tables as lib/model.lua gives them; in_c input channels; skip = addPressureSkip
static void check_linear(bool is3d, int in_c, std::vector<int> osize, std::vector<int> ksize, std::vector<int> usize, bool skip, bool trains) {
  const int n = (int)osize.size();
  int prev_ref = in_c, prev_p = in_c;
  for (int l = 0; l < n; l++) {
    const bool last = l + 1 == n, sk = skip && last;
    const int cp = last ? osize[l] : padded(osize[l]);
    check_layer(layer_of(is3d, ksize[l], usize[l], prev_ref + (sk ? 1 : 0), osize[l], prev_p + (sk ? 1 : 0), cp, 0, 0, sk, trains && l > 0));
    prev_ref = osize[l]; prev_p = cp;
  }
}

// ---- the packed forms of the default topologies ----------------------------------------------------------------------------
enum Fill { kRandom, kScaled37, kWideSpan, kAllZero };
// a layer's weights: random; the same scaled by 37; magnitudes spanning 2^-24 .. 1 of the maximum (both fp16 halves of the
// split pass through subnormals); all zero
static std::vector<float> weights_of(size_t n, Fill f) {
  std::vector<float> w(n);
  for (size_t i = 0; i < n; i++) {
    const float r = rnd();
    w[i] = f == kRandom ? 0.3f * r : f == kScaled37 ? 37.0f * 0.3f * r : f == kWideSpan ? std::ldexp(0.5f + 0.5f * r * r, -(int)(i % 25)) * (r < 0 ? -0.7f : 0.7f) : 0.0f;
  }
  return w;
}
static void check_default3(Fill f) {
  const int cin[5] = {3, 8, 8, 8, 8}, cout[5] = {8, 8, 8, 8, 1}, taps[5] = {27, 27, 27, 1, 1};
  std::vector<float> w[5], b[5];
  const float* wp[5]; const float* bp[5];
  for (int l = 0; l < 5; l++) {
    w[l] = weights_of((size_t)cout[l] * cin[l] * taps[l], f); b[l] = weights_of((size_t)cout[l], f == kAllZero ? kAllZero : kRandom);
    wp[l] = w[l].data(); bp[l] = b[l].data();
  }
  for (int l = 0; l < 3; l++) {
    std::vector<float> want, got;
    pack_bfrag3(wp[l], cin[l], want);
    got.resize((size_t)cin[l] * 9 * 64);
    for (int d = 0; d < (int)got.size(); d++) { const int s = pack_bfrag3_src(cin[l], d); CHECK(s < (int)w[l].size()); got[(size_t)d] = s >= 0 ? w[l][(size_t)s] : 0.0f; }
    CHECK(same_bytes(got, want));
    pack_wino3(wp[l], cin[l], want);
    got.assign((size_t)9 * 4 * cin[l] * 8, 0.0f);
    for (int d = 0; d < (int)got.size(); d++) {
      int p; const int s = pack_wino3_src(cin[l], d, &p);
      CHECK(s >= 0 && s + 2 < (int)w[l].size());
      got[(size_t)d] = pack_wino3_val(wp[l] + s, p);
    }
    CHECK(same_bytes(got, want));
    // the split-fp16 fragments: one exponent per layer from max |w|, then every half through the integer conversion
    std::vector<uint16_t> fr(conv3_m16_frag_halves(cin[l]), 0), gfr(fr.size(), 0);
    const float post = conv3_m16_pack_weights(wp[l], cin[l], fr.data());
    float post4 = 0.0f;
    if (l == 2) post4 = conv3_m16_pack_tail(wp[3], fr.data());
    float mx = 0.0f;
    for (float v : w[l]) mx = fmaxf(mx, fabsf(v));
    const int e = m16_exp(mx), n = m16_frag_halves(cin[l]);
    CHECK((size_t)n + (cin[l] == 8 ? kM16TailHalves : 0) == fr.size());
    for (int d = 0; d < n; d++) {
      const M16Src s = m16_frag_src(cin[l], d);
      CHECK(s.idx < (int)w[l].size());
      gfr[(size_t)d] = s.idx >= 0 ? m16_half(w[l][(size_t)s.idx], e, s.lo, s.hi) : (uint16_t)0;
    }
    const float gpost = m16_post(e);
    CHECK(std::memcmp(&gpost, &post, 4) == 0);
    if (l == 2) {
      float mx4 = 0.0f;
      for (float v : w[3]) mx4 = fmaxf(mx4, fabsf(v));
      const int e4 = m16_exp(mx4);
      for (int d = 0; d < kM16TailHalves; d++) {
        const M16Src s = m16_tail_src(d);
        CHECK(s.idx >= 0 && s.idx < 64);
        gfr[(size_t)(n + d)] = m16_half(w[3][(size_t)s.idx], e4, s.lo, s.hi);
      }
      const float gpost4 = m16_post(e4);
      CHECK(std::memcmp(&gpost4, &post4, 4) == 0);
      if (f == kAllZero) CHECK(e4 == 0);
    }
    CHECK(same_bytes(gfr, fr));
    if (f == kAllZero) CHECK(e == 0);
    if (f == kWideSpan) {      // the case is what it claims: subnormal halves of both kinds occur
      int sub = 0;
      for (uint16_t h : fr) sub += (h & 0x7c00u) == 0 && (h & 0x3ffu) != 0;
      CHECK(sub > 16);
    }
  }
  std::vector<float> want, got(kTailPackFloats, 0.0f);
  pack_tail3(wp, bp, 0.0f, want);
  for (int d = 0; d < 89; d++) {
    int l, bias, i;
    pack_tail3_src(d, &l, &bias, &i);
    CHECK(l >= 2 && l <= 4 && i >= 0 && (size_t)i < (bias ? b[l].size() : w[l].size()));
    got[(size_t)d] = bias ? b[l][(size_t)i] : w[l][(size_t)i];
  }
  CHECK(same_bytes(got, want));
}
static void check_default2(Fill f) {
  const int cin[4] = {3, 16, 16, 16};
  for (int l = 0; l < 4; l++) {
    const std::vector<float> w = weights_of((size_t)16 * cin[l] * 9, f);
    std::vector<float> want, got;
    pack_bfrag2(w.data(), cin[l], want);
    got.resize((size_t)9 * ((cin[l] + 3) / 4) * 64);
    CHECK(got.size() == want.size());
    for (int d = 0; d < (int)got.size(); d++) { const int s = pack_bfrag2_src(cin[l], d); CHECK(s < (int)w.size()); got[(size_t)d] = s >= 0 ? w[(size_t)s] : 0.0f; }
    CHECK(same_bytes(got, want));
  }
}

// ---- the conversions: every binary16 pattern back and forth, and the host's f2h on a sweep of floats -------------------------
static void check_conversions() {
  for (uint32_t h = 0; h < 0x10000u; h++) {
    if (((h >> 10) & 31) == 31) continue;
    const float a = refresh_h2f((uint16_t)h), b = h2f((uint16_t)h);
    CHECK(std::memcmp(&a, &b, 4) == 0);
    CHECK(refresh_f2h(a) == (uint16_t)h);
  }
  for (uint32_t u = 0x32000000u; u < 0x47000000u; u += 997u) {      // 2^-27 .. 2^15, through the subnormal halves and the ties
    float x; std::memcpy(&x, &u, 4);
    CHECK(refresh_f2h(x) == f2h(x) && refresh_f2h(-x) == f2h(-x));
  }
  for (int k = -26; k < 15; k++)         // exact ties and their neighbours
    for (int m = 0; m < 2048; m++) {
      const float x = std::ldexp(1.0f + (float)m / 2048.0f, k);
      CHECK(refresh_f2h(x) == f2h(x));
    }
}

// ---- the optimiser's flat space: every element once, in a tensor that holds it ---------------------------------------------
static void check_optim_walk(const std::vector<long long>& sizes) {
  std::vector<long long> off(1, 0);
  for (long long s : sizes) off.push_back(off.back() + s);
  const int n = (int)sizes.size();
  const long long total = off.back();
  std::vector<int> hit((size_t)total, 0);
  long long prev_hi = 0;
  for (int b = 0; b < kOptimNormBlocks; b++) {
    long long lo, hi;
    optim_chunk(total, kOptimNormBlocks, b, &lo, &hi);
    CHECK(lo == prev_hi && hi >= lo && hi <= total);
    prev_hi = hi;
    for (long long i = lo; i < hi; i++) {
      const int t = optim_tensor_of(off.data(), n, i);
      CHECK(t >= 0 && t < n && i >= off[(size_t)t] && i < off[(size_t)t + 1]);
      hit[(size_t)i]++;
    }
  }
  CHECK(prev_hi == total);
  for (int h : hit) CHECK(h == 1);
}

int main() {
  check_conversions();
  // every layer of the test models: 3-D and 2-D default, yang (6 channels padded to 8), k5-skip (skip channel), tog (S = 4 / 8)
  check_linear(true, 3, {8, 8, 8, 8, 1}, {3, 3, 3, 1, 1}, {1, 1, 1, 1, 1}, false, true);
  check_linear(false, 3, {16, 16, 16, 16, 1}, {3, 3, 3, 3, 1}, {1, 1, 1, 1, 1}, false, true);
  check_linear(true, 3, {6, 6, 6, 1}, {3, 1, 1, 1}, {1, 1, 1, 1}, false, true);
  check_linear(false, 3, {6, 6, 6, 1}, {3, 1, 1, 1}, {1, 1, 1, 1}, false, true);
  check_linear(true, 3, {8, 8, 1}, {5, 3, 1}, {1, 1, 1}, true, true);
  check_linear(false, 3, {8, 8, 1}, {5, 3, 1}, {1, 1, 1}, true, true);
  check_linear(false, 3, {16, 32, 32, 64, 64, 32, 1}, {5, 5, 5, 5, 1, 1, 3}, {1, 1, 1, 1, 1, 1, 2}, false, false);
  check_linear(true, 3, {16, 16, 16, 16, 32, 32, 1}, {3, 3, 3, 3, 1, 1, 3}, {1, 1, 1, 1, 1, 2, 2}, false, false);
  check_linear(false, 5, {6, 1}, {3, 3}, {1, 1}, true, true);        // padded planes between the plain channels and the skip plane
  // the layer behind a concat join: two and three banks of 8 channels, and of 6 padded to 8 (the slices lie 8 apart)
  check_layer(layer_of(true, 3, 1, 16, 8, 16, 8, 8, 8, false, false));
  check_layer(layer_of(true, 3, 1, 24, 8, 24, 8, 8, 8, false, false));
  check_layer(layer_of(false, 3, 1, 12, 6, 16, 8, 6, 8, false, false));
  check_layer(layer_of(true, 1, 1, 13, 1, 17, 1, 6, 8, true, false));     // ... with the skip channel behind them
  for (Fill f : {kRandom, kScaled37, kWideSpan, kAllZero}) { check_default3(f); check_default2(f); }
  check_optim_walk({648, 8, 1728, 8, 1728, 8, 64, 8, 8, 1});
  check_optim_walk({3, 1});
  check_optim_walk({162, 6, 36, 6, 36, 6, 6, 1});
  std::printf("refresh layout OK\n");
  return 0;
}
