// model_host.cpp -- the host side of the projection ConvNet behind include/tfluids_hip.h: the tfl_model object (layer table,
// packed weights, conv path), its creation, its workspace layout, the fp16 range gate, the wall plans, and the forward pass
// (tfl_model_begin / _finish / _forward) in its six forms. tfl_model's fields are private to this file: the native steps ask
// through model_is_graph / model_grid_factor / model_cone / model_range_counter (tfl_host.hpp, tfl_ops.hpp).
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "tfl_abi.hpp"
#include "tfl_input_grad.hpp"
#include "tfl_ops.hpp"
#include "tfl_refresh.hpp"
#include "tfl_train.hpp"

using tfl::fail; using tfl::check_flags; using tfl::check_vel; using tfl::check_scalar; using tfl::check_launch;

struct tfl_layer {
  int cin = 0, cout = 0, k = 0;
  int pool = 1;        // 2: 2x average pooling after the non-linearity (model_utils.lua:184-208)
  int up = 1;          // 2: {Spatial,Volumetric}ConvolutionUpsample -- up^dim sub-position convolutions, pixel-shuffled
  float* w = nullptr;  // device, [sub][tap][cin][cout]
  float* b = nullptr;  // device, [sub][cout]
  int stage = 0;       // 1-based stage of lib/model.lua's layer tables
  int bank = 0;        // 0-based bank (0 outside [banksSplitStage, banksJoinStage))
  // graph models only
  int dil = 1;         // dilation (banksType 'dilate': 2^(bank - 1))
  float* bn = nullptr; // device, the folded batch norm after this module: scale[cout] then shift[cout]
  // what the module's cudnn weight looked like (tfl_model_set_weights lays a new one out the same way): its channel counts,
  // whether its last input channel is the joined skip channel, and (join_c > 0) that input channel ci sits on plane
  // (ci / join_c) * join_p + ci % join_c -- the concat of the banks
  int cin_ref = 0, cout_ref = 0, join_c = 0, join_p = 0;
  bool skip_in = false;
  float* wt = nullptr; // device, trainable models: the data-gradient form [tap][cout][cin] (tfl_train.hpp); the first layer's has
                       // gxc input planes of which the first nx are real (relay_first_transposed: tfl_model_backward_input)
  int nx = 0, gxc = 0; // first layer of a trainable model: the net input's planes without the occupancy channel, and padded
  float* ws = nullptr; // device, the last layer of a trainable model with the joined skip channel: its gradient's form [tap]
};
// The forward a model runs (tfl_model_finish dispatches on it), named after its kernel file; TFL_CONV_PATH at creation picks
// it for the 3-D `default` topology (3->8 k3, 8->8 k3, 8->8 k3, 8->8 k1, 8->1 k1), and "direct" = generic for both defaults.
enum class ConvPath {
  conv_mfma16,   // 3-D default: split-operand fp16 MFMA (conv_mfma16.hip), TFL_CONV_PATH unset or "mfma16"
  conv_valu,     // 3-D default: fp32 Winograd on the vector ALUs (conv_valu.hip), "winograd" and any unrecognised value
  conv_mfma,     // 3-D default: fp32-operand MFMA (conv_mfma.hip), "mfma"
  conv2d_mfma,   // 2-D default topology (3->16, 16->16 x3 k3, 16->1 k1): conv2d_mfma.hip
  generic,       // everything else that is not a graph model: the shape-generic kernels (conv.hip), layer by layer
  graph,         // tfl_model_create_graph: banks / batch norm / max pooling (graph_forward)
};
static bool default3(ConvPath p) { return p == ConvPath::conv_mfma16 || p == ConvPath::conv_valu || p == ConvPath::conv_mfma; }
struct tfl_model {
  bool is3d = false;
  int max_c = 0;
  bool multires = false;   // some layer pools / upsamples (the `tog` topologies)
  int max_down = 1;        // coarsest activation resolution = grid / max_down
  std::vector<tfl_layer> layers;
  ConvPath path = ConvPath::generic;
  // 3-D `default` topology: the weights of its three forms (pack_default3)
  float* bfrag[3] = {nullptr, nullptr, nullptr};  // per-lane B fragments of the three k=3 layers
  float* wino[3] = {nullptr, nullptr, nullptr};   // F(2,3)-in-x transformed weights of the same layers, [dz][dy][cin][4][8]
  float* tail_w4 = nullptr;                       // [8][8] (out, in) of the 8->8 k1 layer
  float* tail_w5 = nullptr;                       // [8] of the 8->1 k1 layer
  float* tail_pack = nullptr;                     // conv_valu.hip: {bias3[8], w4[8][8], b4[8], w5[8], b5[1]} in one buffer
  // conv_mfma16.hip
  void* wfrag16[3] = {nullptr, nullptr, nullptr}; // A fragments of the three k=3 layers (conv3_m16_pack_weights)
  float post16[3] = {0.0f, 0.0f, 0.0f};           // 2^-(11 + e) of each layer
  float post16_tail = 0.0f;                       // the same for the tail's 8 -> 8 (k = 1) layer (conv3_m16_pack_tail)
  unsigned long long* d_range_err = nullptr;      // blocks that clamped an activation at the fp16 range
  unsigned long long* h_range = nullptr;          // pinned, device-mapped: the projection kernel copies a non-zero count here, so the
  unsigned long long* d_range_host = nullptr;     // NEXT call sees it without a stream sync (d_range_host = its device address)
  // 2-D `default` topology (conv2d_mfma.hip)
  float* bfrag2[4] = {nullptr, nullptr, nullptr, nullptr};
  double* d_stats = nullptr;  // [2 * kMaxBatch]: sum(u), sum(u^2) per sample
  long long stat_pairs_per_plane = 0;   // partial pairs per z-plane the last tfl_model_begin wrote (model.hip model_pre's layout)
  unsigned* d_ticket = nullptr;   // model.hip publish_and_maybe_reduce: blocks of the current k_bcs_div_stats launch that have published
  // forward-graph switches (tfl_model_opts); `custom` = any of them differs from default_conf.lua -> generic kernels only
  tfl_model_opts opts = {1, 0, 1, 1, TFL_NORM_UDIV, TFL_NORMFUNC_STD, TFL_NONLIN_RELU, 0};
  bool custom = false;
  int in_c = 3;               // net input channels
  float* zero_bias = nullptr; // 64 zeros: the bias of the data-gradient convolutions (tfl_model_backward)
  // graph models: banks / batch norm / max pooling (shape-generic kernels, un-sharded)
  int banks = 1, bank_type = TFL_BANKS_MRES, aggregate = TFL_AGG_CONCAT, split = 0, join = 0, nstages = 0;
  bool pool_max = false;
  int bank_c = 0;             // channel planes of each bank's two scratch buffers
  int bank_down = 1;          // bank 1's finest resolution inside [split, join) = grid / bank_down (bank i: / 2^(i-1) more, mres)
  int split_c = 0;            // channels entering the split (the mres pyramid's planes)
  int split_down = 1;         // resolution at the split = grid / split_down
  // tfl_model_set_weights_device: the device tables of its launches (refresh_tables, at creation; null: more than
  // kRefreshMaxLayers layers) and the words its fp16 launch leaves the post-scales in
  tfl::RefreshLayer* d_refresh = nullptr;
  tfl::PackJob* d_jobs = nullptr;
  int njobs = 0, refresh_elems = 0, job_elems = 0;     // (..._elems: the most destination elements of one table entry)
  float* d_post16 = nullptr;                           // [4]: post16[0..2], post16_tail
};

namespace {
// the tfl_model_opts of a new model (NULL = default_conf.lua's), checked against the layer table; false on error
static bool model_opts_of(tfl_ctx* c, int nlayers, const int32_t* pool, const int32_t* up, const tfl_model_opts* opts,
                          tfl_model_opts* out) {
  auto bad = [&](const char* m) { fail(c, TFL_EINVAL, "model_create: %s", m); return false; };
  tfl_model_opts o = {1, 0, 1, 1, TFL_NORM_UDIV, TFL_NORMFUNC_STD, TFL_NONLIN_RELU, 0};
  if (opts) {
    o = *opts;
    o.in_pDiv = o.in_pDiv != 0; o.in_UDiv = o.in_UDiv != 0; o.in_div = o.in_div != 0; o.normalize = o.normalize != 0;
    o.pressure_skip = o.pressure_skip != 0;
    if (!o.in_pDiv && !o.in_UDiv && !o.in_div) return bad("Are you sure you dont want any (U, div or p) fields?");   // model.lua:50-52
    if (o.norm_chan < TFL_NORM_UDIV || o.norm_chan > TFL_NORM_DIV) return bad("Incorrect normalize input channel.");
    if (o.norm_func != TFL_NORMFUNC_STD && o.norm_func != TFL_NORMFUNC_L2) return bad("Incorrect normalize input function");
    if (o.nonlin < TFL_NONLIN_RELU || o.nonlin > TFL_NONLIN_SIGMOID) return bad("Bad mconf.nonlinType");
    if (o.pressure_skip && nlayers < 2) return bad("addPressureSkip needs a hidden layer to join pDiv to");
    if (o.pressure_skip && (pool || up)) {
      // the skip joins pDiv at full resolution in front of the last layer: with the layer table in hand, refuse the
      // combinations tfl_model_finish cannot run (it used to report them on every forward instead: ADVICE r02)
      bool multires = false;
      for (int l = 0; l < nlayers; l++) multires = multires || (pool && pool[l] > 1) || (up && up[l] > 1);
      const bool tail = (pool && (pool[nlayers - 1] > 1 || pool[nlayers - 2] > 1)) || (up && (up[nlayers - 1] > 1 || up[nlayers - 2] > 1));
      if (tail || (nlayers > 2 && multires)) {
        fail(c, TFL_EUNSUPPORTED, "model_create: addPressureSkip with pooling / upsampling layers");
        return false;
      }
    }
  }
  *out = o;
  return true;
}

// the layer table and weight packing of tfl_model_create_opts / _graph (C++ linkage: templates)
// `bytes` host bytes into the device buffer dst, allocated here when dst is null (creation; tfl_model_set_weights refills it
// in place); false on failure (what was allocated goes with the model)
template <class T> bool upload(T*& dst, const void* src, size_t bytes) {
  if (!dst && hipMalloc((void**)&dst, bytes) != hipSuccess) return false;
  return hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice) == hipSuccess;
}

// Where the conv modules sit in lib/model.lua's stage table: module i is bank bank[i] of stage stage[i] (1-based), and stage s
// starts at module first[s]. Stages [split, join) run `banks` banks side by side; a linear model has one bank per stage.
struct StageTable {
  std::vector<int> stage, bank, first;
  int banks = 1, split = 0, join = 0;
  bool mres = false, concat = false;
  bool banked(int st) const { return banks > 1 && st >= split && st < join; }
};

StageTable stage_table(int nst, int banks = 1, int split = 0, int join = 0) {
  StageTable t;
  t.banks = banks; t.split = split; t.join = join;
  t.first.assign(nst + 2, -1);
  for (int st = 1; st <= nst; st++) {
    t.first[st] = (int)t.stage.size();
    for (int b = 0; b < (t.banked(st) ? banks : 1); b++) { t.stage.push_back(st); t.bank.push_back(b); }
  }
  return t;
}

// A module's cudnn weight [cout*S][cin][taps] (output channel index = o*S + sub) -> [sub][tap][cin_p][cout_p] and its bias
// [cout*S] -> [sub][cout_p] (tfl_train.hpp relay_layer; the padding holds zeros), uploaded into L -- at creation, and again by
// tfl_model_set_weights into the same buffers. transposed: also the data-gradient form L.wt (every layer of a model
// tfl_model_backward takes; the first layer's is read by tfl_model_backward_input alone) and the skip form L.ws.
bool upload_layer(tfl_layer& L, bool is3d, const float* w, const float* b, bool transposed) {
  const int taps = is3d ? L.k * L.k * L.k : L.k * L.k;
  const int S = is3d ? L.up * L.up * L.up : L.up * L.up;
  auto cmap = [&](int ci) {
    return (L.skip_in && ci == L.cin_ref - 1) ? L.cin - 1 : L.join_c > 0 ? (ci / L.join_c) * L.join_p + ci % L.join_c : ci;
  };
  std::vector<float> relaid, bias_p;
  tfl::relay_layer(S, taps, L.cin, L.cout, L.cin_ref, L.cout_ref, w, b, cmap, relaid, bias_p);
  if (!upload(L.w, relaid.data(), relaid.size() * sizeof(float)) || !upload(L.b, bias_p.data(), bias_p.size() * sizeof(float))) return false;
  if (!transposed) return true;
  std::vector<float> wt;
  if (L.nx > 0) tfl::relay_first_transposed(taps, L.cin, L.cout, L.nx, L.gxc, relaid.data(), wt);
  else tfl::relay_transposed(taps, L.cin, L.cout, L.cin - (L.skip_in ? 1 : 0), relaid.data(), wt);
  if (!upload(L.wt, wt.data(), wt.size() * sizeof(float))) return false;
  if (!L.skip_in) return true;
  std::vector<float> ws;
  tfl::relay_skip(taps, L.cin, L.cout, relaid.data(), ws);
  return upload(L.ws, ws.data(), ws.size() * sizeof(float));
}

// batch norm after hidden module i, folded in double: scale = w / sqrt(var + eps), shift = b - mean * scale, each rounded once
// to fp32, as [2][cout_p] (padded channels: 0, 0 -- they stay exact zeros)
std::vector<float> bn_fold(const tfl_model_graph* g, int i, int co_n, int cout_p) {
  std::vector<float> bn((size_t)2 * cout_p, 0.0f);
  for (int co = 0; co < co_n; co++) {
    const double wt = (g->bn_weight && g->bn_weight[i]) ? (double)g->bn_weight[i][co] : 1.0;
    const double bi = (g->bn_bias && g->bn_bias[i]) ? (double)g->bn_bias[i][co] : 0.0;
    const double sc = wt / std::sqrt((double)g->bn_var[i][co] + g->bn_eps[i]);
    bn[co] = (float)sc;
    bn[cout_p + co] = (float)(bi - (double)g->bn_mean[i][co] * sc);
  }
  return bn;
}

// The layer table of a new model, for both create functions: checks every module against the stage table, pads its channel
// counts, lays out and uploads its weights (and, with g->batch_norm, its folded batch norm), and tracks the resolution, the
// widest activation and the bank buffers' shapes. g = null for a linear model. Null on error (c->err says why).
tfl_model* build_layers(tfl_ctx* c, bool is3d, int n, const int32_t* cin, const int32_t* cout, const int32_t* ksize,
                        const int32_t* pool, const int32_t* up, const float* const* weights, const float* const* biases,
                        const tfl_model_opts& o, const StageTable& t, const tfl_model_graph* g) {
  auto bad = [&](const char* msg) -> tfl_model* { fail(c, TFL_EINVAL, "model_create: %s", msg); return nullptr; };
  const int in_c = o.in_pDiv + o.in_UDiv * (is3d ? 3 : 2) + o.in_div + 1;
  if (cin[0] != in_c) {
    fail(c, TFL_EINVAL, "model_create: the first layer must take %d input channels {pDiv, UDiv, div, occupancy as selected}", in_c);
    return nullptr;
  }
  if (cout[n - 1] != 1) return bad("the last layer must output 1 channel (pressure)");
  tfl_model* m = new tfl_model();
  m->is3d = is3d;
  m->opts = o; m->in_c = in_c;
  m->custom = !(o.in_pDiv && !o.in_UDiv && o.in_div && o.normalize && o.norm_chan == TFL_NORM_UDIV &&
                o.norm_func == TFL_NORMFUNC_STD && o.nonlin == TFL_NONLIN_RELU && !o.pressure_skip);
  auto cleanup = [&](const char* msg) -> tfl_model* { tfl_model_destroy(c, m); return bad(msg); };
  if (hipMalloc((void**)&m->d_stats, sizeof(double) * 2 * kMaxBatch) != hipSuccess) return cleanup("hipMalloc failed");
#ifdef TFL_EXPERIMENTS      // the ticket words of the producer-side stats fold (model.hip kStatTickets): EXPERIMENTS flavour and linear models only
  if (!g && (hipMalloc((void**)&m->d_ticket, sizeof(unsigned) * (1 << 16)) != hipSuccess || hipMemset(m->d_ticket, 0, sizeof(unsigned) * (1 << 16)) != hipSuccess))
    return cleanup("hipMalloc failed");
#endif
  // The shape-generic kernels are instantiated for 1, 2, 4, 8, 16, 32, 64 output channels. Any other width (the
  // `yang` topology of model.lua:188-205 has 6) is zero-padded to the next one: the extra channels carry
  // relu(0 + 0) = 0 into zero weights of the next layer, i.e. every sum gains exact `+ 0 * 0` terms only.
  auto padded = [](int cch) { for (int w : {1, 2, 4, 8, 16, 32, 64}) if (cch <= w) return w; return -1; };
  const int N = t.banks;
  std::vector<int> cout_p(t.first.size(), 0);     // padded output channels of each stage
  int down = 1;                                   // resolution of the current activations = grid / down
  for (int i = 0; i < n; i++) {
    const int st = t.stage[i], bk = t.bank[i];
    const bool last = i + 1 == n, skip_in = o.pressure_skip && last;     // skip_in: also reads pDiv/scale (last channel)
    const bool joined = N > 1 && st == t.join && t.concat;          // input = the concat of the banks
    if (cin[i] < 1 || cout[i] < 1 || ksize[i] < 1 || (ksize[i] % 2) != 1) return cleanup("convolution size must be odd and positive");
    if (st > 1 && cin[i] != cout[t.first[st - 1]] * (joined ? N : 1) + (skip_in ? 1 : 0)) return cleanup("layer channel counts do not chain");
    tfl_layer L;
    L.stage = st; L.bank = bk; L.pool = pool ? pool[i] : 1; L.up = up ? up[i] : 1;
    L.dil = (N > 1 && !t.mres && bk > 0) ? (1 << bk) : 1;
    if ((L.pool != 1 && L.pool != 2) || (L.up != 1 && L.up != 2)) return cleanup("pooling / upsampling factors must be 1 or 2");
    if (L.pool > 1 && L.up > 1) return cleanup("Pooling and upsampling in the same layer!");               // model.lua:322-324
    if (L.pool > 1 && last) return cleanup("Pooling is not allowed in the last layer");                    // model.lua:247
    const int cp = last ? cout[i] : padded(cout[i]);
    const int prev_p = st == 1 ? in_c : cout_p[st - 1];
    const int cin_p = st == 1 ? in_c : prev_p * (joined ? N : 1) + (skip_in ? 1 : 0);     // the skip channel sits last
    if (bk == 0) {     // (the banks of a stage have bank 0's shape)
      cout_p[st] = cp;
      if (N > 1 && st == t.split) {
        m->split_c = cin_p; m->split_down = down; m->bank_down = down;
        // the pyramid's coarsest level, whatever the banked stages do after it
        if (t.mres && (down << (N - 1)) > m->max_down) m->max_down = down << (N - 1);
      }
      if (down % L.up) return cleanup("a layer upsamples beyond the grid resolution");
      down /= L.up;
      if (t.banked(st)) {
        if (down < m->bank_down) m->bank_down = down;
        if (cp > m->bank_c) m->bank_c = cp;
      }
      down *= L.pool;
      const int coarsest = (t.mres && t.banked(st)) ? down << (N - 1) : down;
      if (coarsest > m->max_down) m->max_down = coarsest;
      if (L.pool > 1 || L.up > 1 || down != 1) m->multires = true;
    }
    if (cp < 0) return cleanup("unsupported output channel count (at most 64)");
    L.cin = cin_p; L.cout = cp; L.k = ksize[i];
    // reference input channel ci -> its plane in the padded layout (banks' slices prev_p apart; the skip channel last)
    L.cin_ref = cin[i]; L.cout_ref = cout[i]; L.skip_in = skip_in;
    if (joined) { L.join_c = cout[t.first[st - 1]]; L.join_p = prev_p; }
    const bool has_bn = g && g->batch_norm && !last;
    if (has_bn && (!g->bn_mean[i] || !g->bn_var[i])) { m->layers.push_back(L); return cleanup("addBatchNorm: a module lacks running_mean / running_var"); }
    const std::vector<float> bn = has_bn ? bn_fold(g, i, cout[i], cp) : std::vector<float>();
    const bool ok = upload_layer(L, is3d, weights[i], biases[i], false) &&
                    (bn.empty() || upload(L.bn, bn.data(), bn.size() * sizeof(float)));
    m->layers.push_back(L);
    if (!ok) return cleanup("uploading weights failed");
    const int width = (N > 1 && st == t.join - 1 && t.concat) ? cp * N : cp + (o.pressure_skip ? 1 : 0);
    if (!last && width > m->max_c) m->max_c = width;
  }
  if (down != 1) return cleanup("the layers do not return to the grid resolution (pool / up factors)");
  if (N > 1 && t.mres) m->multires = true;
  if (m->max_c < 1) m->max_c = 1;
  // A model tfl_model_backward takes: a linear one without pooling / upsampling, or a graph model without batch norm
  // whose modules neither pool nor upsample and all fit the weight-gradient kernel's tile at their tap spacing. It holds the
  // data-gradient weights and the zero bias of their convolutions.
  bool trainable = !g ? !m->multires : !g->batch_norm;
  for (const tfl_layer& L : m->layers) {
    if (!g) break;
    tfl::TrainLayer tl{L.cin, L.cout, L.cin_ref, L.cout_ref, L.k, L.skip_in ? 1 : 0};
    tl.dil = L.dil;
    trainable = trainable && L.pool == 1 && L.up == 1 && tfl::conv_wgrad_fits(tfl::wg_plan(is3d, tl, 1, 8, 8, 8));
    if (L.join_c > 0 && L.cin > 64) trainable = false;      // (no convolution kernel writes its data gradient's planes)
  }
  if (trainable) {
    const std::vector<float> zeros(64, 0.0f);
    bool ok = upload(m->zero_bias, zeros.data(), zeros.size() * sizeof(float));
    for (tfl_layer& L : m->layers) {
      // the stage behind a concat join reads banks x channels planes, which need not be a width the convolution kernels write
      // (3 x 8): its data gradient is padded like the first layer's, the planes behind the real ones zero
      if (L.join_c > 0) { L.nx = L.cin; L.gxc = tfl::train_width(L.cin); }
      if (L.stage != 1) continue;      // (a split at the first stage: every bank's first module reads the net input)
      L.nx = in_c - 1;                 // (the occupancy channel sits last and gets no gradient)
      L.gxc = tfl::ig_width(in_c - 1);
    }
    for (int i = 0; i < n && ok; i++) ok = upload_layer(m->layers[i], is3d, weights[i], biases[i], true);
    if (!ok) return cleanup("uploading weights failed");
  }
  return m;
}

// The device tables of tfl_model_set_weights_device, once the model's buffers exist: one RefreshLayer per layer (destinations
// and the parameters of upload_layer's map) and one PackJob per fp32 buffer of a default topology. False on a HIP failure.
bool refresh_tables(tfl_model* m) {
  const int n = (int)m->layers.size();
  if (n > tfl::kRefreshMaxLayers) return true;       // (the device refresh refuses such a model; everything else works)
  std::vector<tfl::RefreshLayer> tab;
  for (const tfl_layer& L : m->layers) {
    tfl::RefreshLayer r{};
    r.w = L.w; r.b = L.b; r.wt = L.wt;
    r.taps = m->is3d ? L.k * L.k * L.k : L.k * L.k;
    r.S = m->is3d ? L.up * L.up * L.up : L.up * L.up;
    r.cin = L.cin; r.cout = L.cout; r.cin_ref = L.cin_ref; r.cout_ref = L.cout_ref;
    r.join_c = L.join_c; r.join_p = L.join_p; r.skip_in = L.skip_in ? 1 : 0;
    r.cin_t = L.nx > 0 ? L.gxc : L.cin - (L.skip_in ? 1 : 0);
    r.wt_first = L.nx; r.ws = L.ws;
    r.n_w = r.S * r.taps * r.cin * r.cout; r.n_b = r.S * r.cout; r.n_wt = L.wt ? r.taps * r.cout * r.cin_t : 0;
    r.n_ws = L.ws ? r.taps : 0;
    m->refresh_elems = std::max(m->refresh_elems, r.n_w + r.n_b + r.n_wt + r.n_ws);
    tab.push_back(r);
  }
  if (!upload(m->d_refresh, tab.data(), tab.size() * sizeof(tfl::RefreshLayer))) return false;
  std::vector<tfl::PackJob> jobs;
  auto job = [&](float* dst, int kind, int layer, int ci_n, int cnt) { if (dst) jobs.push_back(tfl::PackJob{dst, kind, layer, ci_n, cnt}); };
  if (default3(m->path)) {
    for (int l = 0; l < 3; l++) job(m->bfrag[l], tfl::kPackBfrag3, l, m->layers[l].cin_ref, m->layers[l].cin_ref * 9 * 64);
    job(m->tail_w4, tfl::kPackCopy, 3, 8, 64);
    job(m->tail_w5, tfl::kPackCopy, 4, 8, 8);
    // (the fp16 launch writes the tail's post-scale behind the 89 floats; the fp32 paths keep a zero there)
    job(m->tail_pack, tfl::kPackTail3, 2, 8, m->path == ConvPath::conv_mfma16 ? tfl::kTailPackFloats - 1 : tfl::kTailPackFloats);
    for (int l = 0; l < 3; l++) job(m->wino[l], tfl::kPackWino3, l, m->layers[l].cin_ref, 9 * 4 * m->layers[l].cin_ref * 8);
    if (m->path == ConvPath::conv_mfma16 && hipMalloc((void**)&m->d_post16, 4 * sizeof(float)) != hipSuccess) return false;
  } else if (m->path == ConvPath::conv2d_mfma) {
    for (int l = 0; l < 4; l++) job(m->bfrag2[l], tfl::kPackBfrag2, l, m->layers[l].cin_ref, 9 * ((m->layers[l].cin_ref + 3) / 4) * 64);
    job(m->tail_w5, tfl::kPackCopy, 4, 16, 16);
  }
  for (const tfl::PackJob& j : jobs) m->job_elems = std::max(m->job_elems, j.n);
  m->njobs = (int)jobs.size();
  return jobs.empty() || upload(m->d_jobs, jobs.data(), jobs.size() * sizeof(tfl::PackJob));
}

// TFL_CONV_PATH -> the form of the 3-D default topology ("direct" never gets here: it keeps the generic kernels)
ConvPath conv3d_path(const char* force) {
  if (!force || !*force || strcmp(force, "mfma16") == 0) return ConvPath::conv_mfma16;
  if (strcmp(force, "mfma") == 0) return ConvPath::conv_mfma;
  return ConvPath::conv_valu;
}

// The 3-D default topology's own weights: the fp32 MFMA B fragments and tail weights (every form), the fp16 A fragments and
// range words (conv_mfma16), the tail pack and the Winograd-transformed weights (conv_mfma16 and conv_valu). Sets the path;
// returns what failed, or null.
const char* pack_default3(tfl_model* m, const int32_t* cin, const float* const* weights, const float* const* biases, ConvPath path) {
  m->path = path;
  for (int l = 0; l < 3; l++) {
    std::vector<float> frag;
    tfl::pack_bfrag3(weights[l], cin[l], frag);
    if (!upload(m->bfrag[l], frag.data(), frag.size() * sizeof(float))) return "uploading MFMA weight fragments failed";
  }
  if (!upload(m->tail_w4, weights[3], 64 * sizeof(float)) || !upload(m->tail_w5, weights[4], 8 * sizeof(float)))
    return "uploading tail weights failed";
  if (path == ConvPath::conv_mfma16) {
    for (int l = 0; l < 3; l++) {
      std::vector<uint16_t> fr(tfl::conv3_m16_frag_halves(cin[l]));
      m->post16[l] = tfl::conv3_m16_pack_weights(weights[l], cin[l], fr.data());
      if (l == 2) m->post16_tail = tfl::conv3_m16_pack_tail(weights[3], fr.data());     // the 8 -> 8 (k = 1) layer's A fragment
      if (!upload(m->wfrag16[l], fr.data(), fr.size() * sizeof(uint16_t))) return "uploading fp16 MFMA weight fragments failed";
    }
    if (!m->d_range_err) {      // (once: tfl_model_set_weights packs again and keeps the words)
      if (hipMalloc((void**)&m->d_range_err, sizeof(unsigned long long)) != hipSuccess ||
          hipMemset(m->d_range_err, 0, sizeof(unsigned long long)) != hipSuccess)
        return "hipMalloc failed";
      // the word a later call reads without a sync; failing to get mapped memory only loses the early warning
      if (hipHostMalloc((void**)&m->h_range, sizeof(unsigned long long), hipHostMallocMapped) == hipSuccess) {
        *m->h_range = 0;
        if (hipHostGetDevicePointer((void**)&m->d_range_host, m->h_range, 0) != hipSuccess) { (void)hipHostFree(m->h_range); m->h_range = nullptr; m->d_range_host = nullptr; }
      } else m->h_range = nullptr;
    }
  }
  if (path == ConvPath::conv_mfma) return nullptr;
  std::vector<float> tp;
  tfl::pack_tail3(weights, biases, m->post16_tail, tp);
  if (!upload(m->tail_pack, tp.data(), tp.size() * sizeof(float))) return "uploading tail weights failed";
  // the three k = 3 layers' weights, Winograd-transformed along x
  for (int l = 0; l < 3; l++) {
    std::vector<float> u;
    tfl::pack_wino3(weights[l], cin[l], u);
    if (!upload(m->wino[l], u.data(), u.size() * sizeof(float))) return "uploading transformed weights failed";
  }
  return nullptr;
}

// The 2-D default topology's own weights (conv2d_mfma.hip); returns what failed, or null
const char* pack_default2(tfl_model* m, const int32_t* cin, const float* const* weights) {
  m->path = ConvPath::conv2d_mfma;
  for (int l = 0; l < 4; l++) {
    std::vector<float> frag;
    tfl::pack_bfrag2(weights[l], cin[l], frag);
    if (!upload(m->bfrag2[l], frag.data(), frag.size() * sizeof(float))) return "uploading 2-D MFMA weight fragments failed";
  }
  if (!upload(m->tail_w5, weights[4], 16 * sizeof(float))) return "uploading tail weights failed";
  return nullptr;
}

// A forward pass after one that clamped activations at the fp16 range would build on wrong values where the reference's
// fp32 cuDNN carries on: refuse it until the host has acknowledged the count (tfl_model_range_errors).
// The word is written by the device whenever the projection of an earlier pass gets there (no synchronisation), so WHICH later
// call sees it first depends on how far the host runs ahead: the gate is best-effort in time, but it is taken at ONE defined
// point per unit of work -- the entry of a forward pass, or the entry of tfl_simulate_step[_slab] (whose model calls then ask
// for no gate: tfl_ops.hpp Ask::gated, so that they do not refuse half-way through the step).
static int range_gate(tfl_ctx* c, tfl_model* m, const char* who) {
  if (m && m->h_range && *(volatile unsigned long long*)m->h_range != 0)
    return fail(c, TFL_ERANGE, "%s: an earlier forward pass of this model clamped activations at the fp16 range (|x| > 65504 after the "
                               "std normalisation: a blown-up simulation); its pressure is not the reference's. Read and reset the count with "
                               "tfl_model_range_errors, or create the model under TFL_CONV_PATH=winograd (strict fp32, no range limit)", who);
  return TFL_OK;
}

// floats of a graph model's bank buffers behind pPred: per bank two scratch buffers of bank_c planes at its finest
// resolution, and (mres) the pyramid level it starts from; with `base`, their addresses (layout in this order)
static int64_t graph_ws_floats(const tfl_model* m, int B, int Z, int Y, int X, float* base, float* (*bank)[2], float** pyr = nullptr) {
  if (m->path != ConvPath::graph || m->banks < 2) return 0;
  auto cells = [&](int f) { return (int64_t)B * (m->is3d ? (Z + f - 1) / f : Z) * ((Y + f - 1) / f) * ((X + f - 1) / f); };
  const bool mres = m->bank_type == TFL_BANKS_MRES;
  int64_t off = 0;
  for (int i = 0; i < m->banks; i++) {
    const int64_t n = (int64_t)m->bank_c * cells(mres ? m->bank_down << i : m->bank_down);
    if (base) { bank[i][0] = base + off; bank[i][1] = base + off + n; }
    off += 2 * n;
    if (mres && i > 0) {
      if (base) pyr[i] = base + off;
      off += (int64_t)m->split_c * cells(m->split_down << i);
    }
  }
  return off;
}

struct ModelWs { double* partials; float* div; float* x3; float* act[2]; float* pPred; float* bank[tfl::kMaxJoinBanks][2]; float* pyr[tfl::kMaxJoinBanks]; };
int model_ws(tfl_ctx* c, const tfl_model* m, const tfl_tensor* flags, float* workspace, int64_t workspace_floats,
             ModelWs* w) {
  const int B = flags->B, Z = flags->Z, Y = flags->Y, X = flags->X;
  if (B > kMaxBatch) return fail(c, TFL_EINVAL, "model: batch size above %d", kMaxBatch);
  const int64_t n = (int64_t)B * Z * Y * X;
  if (!workspace || workspace_floats < tfl_model_workspace_floats(m, B, Z, Y, X))
    return fail(c, TFL_EINVAL, "model: workspace too small (%lld floats needed)",
                (long long)tfl_model_workspace_floats(m, B, Z, Y, X));
  if (((uintptr_t)workspace & 7) != 0) return fail(c, TFL_EINVAL, "model: workspace must be 8-byte aligned");
  w->partials = (double*)workspace;
  w->div = workspace + 4 * tfl::model_stat_blocks(B, Z, Y, X);
  w->x3 = w->div + n;
  w->act[0] = w->x3 + (int64_t)m->in_c * n;
  if (m->path == ConvPath::conv_mfma16) w->act[0] = (float*)(((uintptr_t)w->act[0] + 15) & ~(uintptr_t)15);
  w->act[1] = w->act[0] + (int64_t)m->max_c * n;
  w->pPred = w->act[1] + (int64_t)m->max_c * n;
  graph_ws_floats(m, B, Z, Y, X, w->pPred + n, w->bank, w->pyr);
  return TFL_OK;
}

// the wall codes of THESE flags, if the host registered them with this context (tfl_wall_plan_create), else null
static const unsigned short* wall_code_of(tfl_ctx* c, const tfl_model* m, const tfl_tensor* flags) {
  std::lock_guard<std::mutex> lock(c->wall_mu);
  for (const tfl_wall_plan* wp : c->wall_plans)
    if (wp->flags == flags->data && wp->is3d == m->is3d && wp->B == flags->B && wp->Z == flags->Z && wp->Y == flags->Y && wp->X == flags->X) return wp->code;
  return nullptr;
}

// a graph model's grid must be divisible by its largest downsampling factor (the mres pyramid times the pooling): refused
// before anything is launched (the reference fails at the join)
static int graph_gate(tfl_ctx* c, const tfl_model* m, const tfl_tensor* flags, const char* who) {
  if (m->path != ConvPath::graph) return TFL_OK;
  const int f = m->max_down;
  if ((m->is3d && flags->Z % f) || flags->Y % f || flags->X % f)
    return fail(c, TFL_EINVAL, "%s: grid %dx%dx%d is not divisible by the model's downsampling factor %d (banks x pooling)", who,
                flags->Z, flags->Y, flags->X, f);
  return TFL_OK;
}

// What every forward of tfl_model_finish reads. U: the wall-BC'd velocity tfl_model_begin left in UOut; (st_in, count): the
// input scale; sc: the window and stage mask of the call.
struct Fwd {
  hipStream_t st;
  int B, Z, Y, X;
  const float *pDiv, *U, *flags;
  const double* st_in; double count;
  const tfl::Scope& sc;
  bool conv1_sums_stats;      // tfl_model_forward (whole array, the model's own stats buffer): conv layer 1 sums the partials
};

// the net input {pDiv/scale, div/scale, occupancy}, or the channels tfl_model_opts selects, into w.x3 on the planes
// [z0, z0 + nz) (nz < 0: every plane)
void net_input(const tfl_model* m, const ModelWs& w, const Fwd& a, int z0, int nz) {
  if (m->custom)
    tfl::model_net_input_gen(a.st, m->is3d, a.B, a.Z, a.Y, a.X, m->opts.in_pDiv, m->opts.in_UDiv, m->opts.in_div, a.pDiv,
                             a.U, w.div, a.flags, a.st_in, a.count, w.x3, z0, nz);
  else
    tfl::model_net_input(a.st, m->is3d, a.B, a.Z, a.Y, a.X, a.pDiv, w.div, a.flags, a.st_in, a.count, w.x3, z0, nz);
}

// One conv module of a graph model at [Zc][Yc][Xc] (updated to its output's): its conv(s) -- one per ConvolutionUpsample
// sub-position -- then the pooling; the module's batch norm rides on whichever launch writes last. P / Q are two scratch
// buffers (`in` may be one of them); the result goes to planes [c0, c0 + cout) of the och-plane `dst`, or (dst = null)
// into P or Q. Returns where the result is, null when no kernel exists for the width.
float* graph_layer(hipStream_t st, const tfl_model* m, const tfl_layer& L, int B, int& Zc, int& Yc, int& Xc, const float* in,
                   float* P, float* Q, float* dst, int och, int c0, int act) {
  float* conv_out = in == P ? Q : P;
  const bool pools = L.pool > 1;
  float* cdst = (pools || !dst) ? conv_out : dst;
  const float* bs = L.bn ? L.bn : nullptr;
  const float* bt = L.bn ? L.bn + L.cout : nullptr;
  const int taps = m->is3d ? L.k * L.k * L.k : L.k * L.k;
  const int S = m->is3d ? L.up * L.up * L.up : L.up * L.up;
  for (int sub = 0; sub < S; sub++)
    if (!tfl::conv_direct_graph(st, m->is3d, B, Zc, Yc, Xc, L.cin, L.cout, L.k, act, in, L.w + (size_t)sub * taps * L.cin * L.cout,
                                L.b + (size_t)sub * L.cout, cdst, L.up, sub, cdst == dst ? och : 0, cdst == dst ? c0 : 0, L.dil,
                                pools ? nullptr : bs, pools ? nullptr : bt))
      return nullptr;
  if (m->is3d) Zc *= L.up;
  Yc *= L.up; Xc *= L.up;
  if (!pools) return cdst;
  float* pdst = dst ? dst : (conv_out == P ? Q : P);
  tfl::pool2_graph(st, m->is3d, m->pool_max, B, L.cout, Zc, Yc, Xc, conv_out, pdst, dst ? och : L.cout, dst ? c0 : 0, bs, bt);
  if (m->is3d) Zc /= 2;
  Yc /= 2; Xc /= 2;
  return pdst;
}

// The conv stack of a graph model (lib/model.lua:262-362): trunk stages in the act[] ping-pong, the banks in their own
// buffers, one k_bank_join launch at the join (none when every bank wrote its own concat slice: dilate + concat).
// gt (tfl_model_forward_train): the same launches with the tape as their destinations -- every module's output in its own entry
// (so no bank writes its slice of the join itself: k_bank_join copies or adds every bank, and for 'add' bank 1 is copied into the
// join first), the pyramid levels and the join in theirs. Copies are exact: the bits are those of the inference form.
struct GraphTape { std::vector<float*> out; float* pyr[tfl::kMaxJoinBanks]; float* join; };
int graph_forward(tfl_ctx* c, const tfl_model* m, const ModelWs& w, const Fwd& a, const GraphTape* gt = nullptr) {
  net_input(m, w, a, 0, -1);
  hipStream_t st = a.st;
  const int B = a.B;
  const int act = 1 + m->opts.nonlin;
  const int nl = (int)m->layers.size();
  const bool mres = m->bank_type == TFL_BANKS_MRES, concat = m->aggregate == TFL_AGG_CONCAT;
  const float* in = w.x3;
  int Zc = a.Z, Yc = a.Y, Xc = a.X;
  auto none = [&](const tfl_layer& L) { return fail(c, TFL_EUNSUPPORTED, "model_finish: no kernel for %d output channels", L.cout); };
  for (int l = 0; l < nl;) {
    const tfl_layer& L0 = m->layers[l];
    if (m->banks > 1 && L0.stage == m->split) {
      float* join = gt ? gt->join : in == w.act[0] ? w.act[1] : w.act[0];     // (`in` is read by every bank: the join goes elsewhere)
      const int N = m->banks, Cp = m->layers[l + (m->join - m->split - 1) * N].cout, och = concat ? Cp * N : Cp;
      // mres: the average-pooling pyramid, one launch per level (model.lua:266-276)
      const float* bin[tfl::kMaxJoinBanks];
      int bZ[tfl::kMaxJoinBanks], bY[tfl::kMaxJoinBanks], bX[tfl::kMaxJoinBanks];
      bin[0] = in; bZ[0] = Zc; bY[0] = Yc; bX[0] = Xc;
      for (int i = 1; i < N; i++) {
        bin[i] = in; bZ[i] = bZ[i - 1]; bY[i] = bY[i - 1]; bX[i] = bX[i - 1];
        if (!mres) continue;
        float* level = gt ? gt->pyr[i] : w.pyr[i];
        tfl::avg_pool2(st, m->is3d, B * m->split_c, bZ[i - 1], bY[i - 1], bX[i - 1], bin[i - 1], level);
        bin[i] = level;
        if (m->is3d) bZ[i] /= 2;
        bY[i] /= 2; bX[i] /= 2;
      }
      int slot[tfl::kMaxJoinBanks], sh[tfl::kMaxJoinBanks], n = 0;
      const float* src[tfl::kMaxJoinBanks];
      int jZ = 0, jY = 0, jX = 0;
      for (int i = 0; i < N; i++) {
        const float* x = bin[i];
        int z = bZ[i], y = bY[i], xx = bX[i];
        const bool direct = !gt && (i == 0 || (concat && !mres));            // this bank writes its slice of the join itself
        for (int s = m->split; s < m->join; s++) {
          const int li = l + (s - m->split) * N + i;
          const tfl_layer& L = m->layers[li];
          const bool last = s + 1 == m->join;
          if (gt) x = graph_layer(st, m, L, B, z, y, xx, x, w.bank[i][0], w.bank[i][1], gt->out[li], L.cout, 0, act);
          else x = graph_layer(st, m, L, B, z, y, xx, x, w.bank[i][0], w.bank[i][1], (last && direct) ? join : nullptr, och,
                               concat ? i * Cp : 0, act);
          if (!x) return none(L);
        }
        if (i == 0) { jZ = z; jY = y; jX = xx; }
        if (gt && !concat && i == 0) {      // 'add' starts from bank 1
          HIP_TRY(c, hipMemcpyAsync(join, x, sizeof(float) * (size_t)B * Cp * z * y * xx, hipMemcpyDeviceToDevice, st));
        } else if (!direct) { slot[n] = i; sh[n] = mres ? i : 0; src[n] = x; n++; }
      }
      if (n > 0 && !tfl::bank_join(st, m->is3d, !concat, B, Cp, jZ, jY, jX, n, slot, sh, src, join, och))
        return fail(c, TFL_EINVAL, "model_finish: bad bank join");
      in = join; Zc = jZ; Yc = jY; Xc = jX;
      l += (m->join - m->split) * N;
      continue;
    }
    const bool last = l + 1 == nl;
    const bool joins_skip = m->opts.pressure_skip && l + 2 == nl;
    float* dst = last ? w.pPred : gt ? gt->out[l] : (joins_skip ? (in == w.act[0] ? w.act[1] : w.act[0]) : nullptr);
    float* out = graph_layer(st, m, L0, B, Zc, Yc, Xc, in, w.act[0], w.act[1], dst, joins_skip ? L0.cout + 1 : L0.cout, 0,
                             last ? 0 : act);
    if (!out) return none(L0);
    // addPressureSkip: pDiv/scale becomes the last input channel of the last layer (model.lua:356-360)
    if (joins_skip) tfl::model_skip_channel(st, B, (long long)a.Z * a.Y * a.X, a.pDiv, a.st_in, a.count, out, L0.cout + 1, L0.cout);
    in = out;
    l++;
  }
  return TFL_OK;
}
// tfl_model_opts: the input scale comes from another field / function / not at all. All three reach the kernels through the
// (stats, count) pair scale_from_stats reads -- sqrt((n s2 - s1^2) / (n (n - 1))): the l2 norm is (s1, s2, n) = (0, sum x^2, 2),
// "no scaling" is (0, 1, 2). Forms that pair in the model's stats buffer (a.st_in) and a.count. A caller that passes stats has
// formed it itself (a z-slab rank: over its owned planes, all-reduced -- model_slab_stats).
int opts_stats(tfl_ctx* c, const tfl_model* m, const ModelWs& w, Fwd& a) {
  const tfl_model_opts& o = m->opts;
  const long long cells = (long long)a.Z * a.Y * a.X;
  const float* field = o.norm_chan == TFL_NORM_PDIV ? a.pDiv : (o.norm_chan == TFL_NORM_DIV ? w.div : a.U);
  const long long nf = o.norm_chan == TFL_NORM_UDIV ? cells * (m->is3d ? 3 : 2) : cells;
  if (!o.normalize) { tfl::model_field_stats(a.st, a.B, nf, field, 2, m->d_stats); a.count = 2.0; }
  else if (o.norm_func == TFL_NORMFUNC_L2) { tfl::model_field_stats(a.st, a.B, nf, field, 1, m->d_stats); a.count = 2.0; }
  else if (o.norm_chan != TFL_NORM_UDIV) {
    if (nf < 2) return fail(c, TFL_EINVAL, "model_finish: Sample variance requires more than one sample.");
    tfl::model_field_stats(a.st, a.B, nf, field, 0, m->d_stats); a.count = (double)nf;
  }
  return TFL_OK;
}

// The 3-D default topology's three forms. Stage bits: 1 = first conv layer, 2 = second, 4 = third + the two 1x1x1 layers.
// Split-operand fp16 MFMA (conv_mfma16.hip); the two activation buffers hold the "h2" form (32 B per voxel, as 8 fp32).
// Layers 1 + 2 in one launch where the whole array is computed (round 5); a z-slab rank runs them under separate windows.
void forward_mfma16(const tfl_model* m, const ModelWs& w, const Fwd& a) {
  const bool fused12 = (a.sc.passes() & 3) == 3 &&
                       tfl::conv3_m16_first2_fused(a.st, a.sc, a.B, a.Z, a.Y, a.X, a.pDiv, w.div, a.flags, a.st_in, a.count, m->wfrag16[0],
                                                   m->layers[0].b, m->post16[0], m->wfrag16[1], m->layers[1].b, m->post16[1],
                                                   w.act[1], m->d_range_err);
  if ((a.sc.passes() & 1) && !fused12) {
    if (a.conv1_sums_stats)
      tfl::conv3_m16_first_fused(a.st, a.sc, a.B, a.Z, a.Y, a.X, a.pDiv, w.div, a.flags, a.st_in, a.count, m->wfrag16[0], m->layers[0].b,
                                 m->post16[0], w.act[0], m->d_range_err, w.partials, m->stat_pairs_per_plane * a.Z, m->d_stats);
    else
      tfl::conv3_m16_first_fused(a.st, a.sc, a.B, a.Z, a.Y, a.X, a.pDiv, w.div, a.flags, a.st_in, a.count, m->wfrag16[0], m->layers[0].b,
                                 m->post16[0], w.act[0], m->d_range_err);
  }
  if ((a.sc.passes() & 2) && !fused12)
    tfl::conv3_m16_mid(a.st, a.sc, a.B, a.Z, a.Y, a.X, w.act[0], m->wfrag16[1], m->layers[1].b, m->post16[1], w.act[1], m->d_range_err);
  if (a.sc.passes() & 4)
    tfl::conv3_m16_tail(a.st, a.sc, a.B, a.Z, a.Y, a.X, w.act[1], m->wfrag16[2], m->tail_pack, m->post16[2], w.pPred, m->d_range_err);
}

// fp32 Winograd on the vector ALUs (conv_valu.hip): the first layer builds {pDiv/scale, div/scale, occupancy} while staging
// its LDS tile
void forward_valu(const tfl_model* m, const ModelWs& w, const Fwd& a) {
  if (a.sc.passes() & 1)
    tfl::conv3_valu_first_fused(a.st, a.sc, a.B, a.Z, a.Y, a.X, a.pDiv, w.div, a.flags, a.st_in, a.count, m->wino[0], m->layers[0].b, w.act[0]);
  if (a.sc.passes() & 2) tfl::conv3_valu_mid(a.st, a.sc, a.B, a.Z, a.Y, a.X, w.act[0], m->wino[1], m->layers[1].b, w.act[1]);
  if (a.sc.passes() & 4) tfl::conv3_valu_tail(a.st, a.sc, a.B, a.Z, a.Y, a.X, w.act[1], m->wino[2], m->tail_pack, w.pPred);
}

// fp32-operand MFMA (conv_mfma.hip): the first layer builds {pDiv/scale, div/scale, occupancy} while staging its LDS tile
void forward_mfma(const tfl_model* m, const ModelWs& w, const Fwd& a) {
  if (a.sc.passes() & 1)
    tfl::conv3_mfma_first_fused(a.st, a.sc, a.B, a.Z, a.Y, a.X, a.pDiv, w.div, a.flags, a.st_in, a.count, m->bfrag[0],
                                m->layers[0].b, w.act[0]);
  if (a.sc.passes() & 2) tfl::conv3_mfma_mid(a.st, a.sc, a.B, a.Z, a.Y, a.X, w.act[0], m->bfrag[1], m->layers[1].b, w.act[1]);
  if (a.sc.passes() & 4)
    tfl::conv3_mfma_tail(a.st, a.sc, a.B, a.Z, a.Y, a.X, w.act[1], m->bfrag[2], m->layers[2].b, m->tail_w4, m->layers[3].b,
                         m->tail_w5, m->layers[4].b, w.pPred);
}

// The 2-D default topology (conv2d_mfma.hip), whole grid only
void forward_mfma2d(const tfl_model* m, const ModelWs& w, const Fwd& a) {
  tfl::conv2_mfma_first_fused(a.st, a.B, a.Y, a.X, a.pDiv, w.div, a.flags, a.st_in, a.count, m->bfrag2[0], m->layers[0].b, w.act[0]);
  tfl::conv2_mfma_mid(a.st, a.B, a.Y, a.X, w.act[0], m->bfrag2[1], m->layers[1].b, w.act[1]);
  tfl::conv2_mfma_mid(a.st, a.B, a.Y, a.X, w.act[1], m->bfrag2[2], m->layers[2].b, w.act[0]);
  tfl::conv2_mfma_tail(a.st, a.B, a.Y, a.X, w.act[0], m->bfrag2[3], m->layers[3].b, m->tail_w5, m->layers[4].b, w.pPred);
}

// Every other linear model, layer by layer on the shape-generic kernels. The planes of every launch: the whole grid, or (a
// z-window [za, zb) on a 3-D model: a z-slab rank's owned planes) the cone of the planes the velocity update reads, layer by
// layer (model_cone).
// outs (tfl_model_forward_train): where each layer's output goes instead of the act[] ping-pong -- the tape.
int generic_forward(tfl_ctx* c, const tfl_model* m, const ModelWs& w, const Fwd& a, float* const* outs = nullptr) {
  hipStream_t st = a.st;
  const int B = a.B, Z = a.Z, Y = a.Y, X = a.X;
  const bool windowed = a.sc.windowed();
  const tfl::ZWin& win = a.sc.win;
  if (m->multires && ((m->is3d && Z % m->max_down) || Y % m->max_down || X % m->max_down))
    return fail(c, TFL_EINVAL, "model_finish: grid %dx%dx%d is not divisible by the model's pooling factor %d", Z, Y, X, m->max_down);
  const size_t nl = m->layers.size();
  tfl::ModelCone cone;
  int za = 0, zb = Z;
  if (windowed) {
    const char* why = nullptr;
    if (!tfl::model_cone(m, &cone, &why)) return fail(c, TFL_EUNSUPPORTED, "model_finish: %s", why);
    if (win.b1 > win.b0) return fail(c, TFL_EINVAL, "model_finish: the shape-generic forward takes one z-window run");
    za = std::max(win.a0, 0); zb = std::min(win.a1, Z);
    if (za % cone.F || zb % cone.F)
      return fail(c, TFL_EINVAL, "model_finish: z-window [%d, %d) is not aligned to the model's downsampling factor %d", za, zb, cone.F);
  }
  auto span = [&](int lo, int hi, int dd, int Zd, int& z0, int& nz) {     // planes [za/dd - lo, zb/dd + hi) of a Zd-deep level
    if (!windowed) { z0 = 0; nz = Zd; return; }
    const int a = std::max(za / dd - lo, 0), b = std::min(zb / dd + hi, Zd);
    z0 = a; nz = b > a ? b - a : 0;
  };
  int z0, nz;
  if (windowed) span(cone.in_lo, cone.in_hi, 1, Z, z0, nz); else { z0 = 0; nz = -1; }
  net_input(m, w, a, z0, nz);
  const int act = 1 + m->opts.nonlin;            // conv_direct: 1 ReLU, 2 ReLU6, 3 sigmoid
  const float* in = w.x3;
  int Zc = Z, Yc = Y, Xc = X;     // resolution of `in`
  for (size_t l = 0; l < nl; l++) {
    const tfl_layer& L = m->layers[l];
    const bool last = l + 1 == nl;
    const bool joins_skip = m->opts.pressure_skip && l + 2 == nl;
    float* out = outs ? outs[l] : last ? w.pPred : (in == w.act[0] ? w.act[1] : w.act[0]);
    const int taps = m->is3d ? L.k * L.k * L.k : L.k * L.k;
    const int S = m->is3d ? L.up * L.up * L.up : L.up * L.up;
    if (windowed) span(cone.layer[l].conv_lo, cone.layer[l].conv_hi, cone.layer[l].conv_d, Zc, z0, nz);
    for (int sub = 0; sub < S; sub++)      // ConvolutionUpsample: one strided-store convolution per sub-position
      if (!tfl::conv_direct(st, m->is3d, B, Zc, Yc, Xc, L.cin, L.cout, L.k, last ? 0 : act, in,
                            L.w + (size_t)sub * taps * L.cin * L.cout, L.b + (size_t)sub * L.cout, out, L.up, sub,
                            joins_skip ? L.cout + 1 : 0, z0, nz))
        return fail(c, TFL_EUNSUPPORTED, "model_finish: no kernel for %d output channels", L.cout);
    // addPressureSkip: pDiv/scale becomes the last input channel of the last layer (model.lua:356-360); windowed: on the
    // planes the last layer reads (the skip needs a full-resolution net, so they are at the grid's resolution)
    if (joins_skip) {
      long long t0 = 0, nt = -1;
      if (windowed) { span(cone.layer[nl - 1].in_lo, cone.layer[nl - 1].in_hi, 1, Z, z0, nz); t0 = (long long)z0 * Y * X; nt = (long long)nz * Y * X; }
      tfl::model_skip_channel(st, B, (long long)Z * Y * X, a.pDiv, a.st_in, a.count, out, L.cout + 1, L.cout, t0, nt);
    }
    if (m->is3d) Zc *= L.up;
    Yc *= L.up; Xc *= L.up;
    in = out;
    if (L.pool > 1) {
      float* pooled = in == w.act[0] ? w.act[1] : w.act[0];
      if (windowed) span(cone.layer[l].pool_lo, cone.layer[l].pool_hi, 2 * cone.layer[l].conv_d, Zc / 2, z0, nz);
      else { z0 = 0; nz = -1; }
      tfl::avg_pool2(st, m->is3d, B * L.cout, Zc, Yc, Xc, in, pooled, z0, nz);
      if (m->is3d) Zc /= 2;
      Yc /= 2; Xc /= 2;
      in = pooled;
    }
  }
  return TFL_OK;
}
}  // namespace

namespace tfl {
bool model_is_graph(const tfl_model* m) { return m && m->path == ConvPath::graph; }
int model_grid_factor(const tfl_model* m) { return m ? m->max_down : 1; }

// The z-slab cone of a model: ONE backward walk over the layer table gives both the window of every launch and
// the halo depth, so the two cannot disagree. Start: pPred on the owned planes widened by (1, 0) -- what the velocity update
// reads. Per layer, from its output back to its input:
//   2x pooling       pooled planes (lo, hi) at grid / 2d  <-  pre-pool planes (2 lo, 2 hi) at grid / d (owned ranges are
//                    multiples of F, so a pooling window never straddles the owned boundary: outward alignment is exact)
//   ConvolutionUpsample  fine planes (lo, hi) at grid / d  <-  coarse conv planes (ceil(lo / 2), ceil(hi / 2)) at grid / 2d
//                    (fine plane 2 kc + c comes from coarse plane kc: the floor mapping)
//   conv k           conv planes (lo, hi)  <-  input planes (lo + k/2, hi + k/2) at the same resolution
// The stored halo must hold every plane any level reads: depth = max over the layers of d x (input extent).
bool model_cone(const tfl_model* m, ModelCone* out, const char** why) {
  auto no = [&](const char* w) { if (why) *why = w; return false; };
  if (!m) return no("no model");
  if (m->path == ConvPath::graph) return no("banked, batch-norm and max-pool models run un-sharded only (tfl_simulate_step)");
  if (!m->is3d) return no("2-D grids have no z to cut (run replicas)");
  const int n = (int)m->layers.size();
  if (n > (int)(sizeof(out->layer) / sizeof(out->layer[0]))) return no("more than 32 layers");
  ModelCone c{};
  c.fused = default3(m->path);
  c.windowed = !c.fused;
  c.F = m->max_down;
  c.nlayers = n;
  c.reads_U = m->opts.in_UDiv != 0;
  c.norm = !m->opts.normalize ? 2 : ((m->opts.norm_chan == TFL_NORM_UDIV && m->opts.norm_func == TFL_NORMFUNC_STD) ? 0 : 1);
  int lo = 1, hi = 0, d = 1, depth = 1;
  for (int l = n - 1; l >= 0; l--) {
    const tfl_layer& L = m->layers[l];
    LayerCone& w = c.layer[l];
    w.pool_lo = w.pool_hi = 0;
    if (L.pool > 1) { w.pool_lo = lo; w.pool_hi = hi; lo *= 2; hi *= 2; d /= 2; }
    if (L.up > 1) { lo = (lo + 1) / 2; hi = (hi + 1) / 2; d *= 2; }
    w.conv_lo = lo; w.conv_hi = hi; w.conv_d = d;
    lo += L.k / 2; hi += L.k / 2;
    w.in_lo = lo; w.in_hi = hi;
    depth = std::max(depth, d * std::max(lo, hi));
  }
  c.in_lo = lo; c.in_hi = hi;
  c.depth = depth;
  *out = c;
  return true;
}

void model_slab_stats(hipStream_t st, const tfl_model* m, int B, int Z, long long yx, int zlo, int zhi, int z_total,
                      const float* pDiv, const float* U, const float* div, double* stats, double* count) {
  const tfl_model_opts& o = m->opts;
  const bool udiv = o.norm_chan == TFL_NORM_UDIV;
  const float* field = o.norm_chan == TFL_NORM_PDIV ? pDiv : (o.norm_chan == TFL_NORM_DIV ? div : U);
  const int mode = !o.normalize ? 2 : (o.norm_func == TFL_NORMFUNC_L2 ? 1 : 0);
  model_field_stats_planes(st, B, udiv ? 3 : 1, Z, yx, zlo, zhi, field, mode, stats);
  // as tfl_model_finish's un-cut forms: std over the whole grid's n values, l2 and none through n = 2
  *count = mode == 0 ? (double)z_total * (double)yx * (udiv ? 3.0 : 1.0) : 2.0;
}

// (library-internal, C++ linkage: the device word of a model's fp16 range counter, for the z-slab step's collective gate -- simulate_slab.cpp)
const unsigned long long* model_range_counter(const tfl_model* m) { return m ? m->d_range_err : nullptr; }

int model_begin(tfl_ctx* c, tfl_model* m, const tfl_tensor* UDiv, const tfl_tensor* flags, const tfl_tensor* UOut, float* workspace,
                int64_t workspace_floats, int zlo, int zhi, double* stats, const Scope& sc, Ask& ask) {
  TRY(check_flags(c, "model_begin", flags));
  if (!m) return fail(c, TFL_EINVAL, "model_begin: null model");
  if (ask.gated) TRY(range_gate(c, m, "model_begin"));
  const int is3D = m->is3d ? 1 : 0;
  TRY(check_vel(c, "model_begin", "UDiv", UDiv, flags, is3D));
  TRY(check_vel(c, "model_begin", "UOut", UOut, flags, is3D));
  if (zlo < 0 || zhi > flags->Z || zlo >= zhi) return fail(c, TFL_EINVAL, "model_begin: bad z range [%d, %d)", zlo, zhi);
  TRY(graph_gate(c, m, flags, "model_begin"));
  ModelWs w;
  TRY(model_ws(c, m, flags, workspace, workspace_floats, &w));
  // SetWallBcs(UDiv) lands in UOut. UOut may alias UDiv: a thread rewrites only the cell it read, and
  // neighbour values are re-derived from the flags, so a neighbour already holding the BC-applied
  // value gives the identical result (the BC is idempotent).
  int stg = sc.passes();   // tfl_set_stages: 2 = wall BCs + divergence + partial sums, 4 = reduce [zlo, zhi)
  if (ask.conv1_sums_stats) stg &= ~4;   // tfl_model_forward: the first conv layer reduces the partials itself (round 6)
  m->stat_pairs_per_plane = tfl::model_stat_pairs_per_plane(flags->B, flags->Z, flags->Y, flags->X, UDiv->data, flags->data, UOut->data, w.div);
  const unsigned short* code = wall_code_of(c, m, flags);
  tfl::model_pre(c->stream, sc, m->is3d, flags->B, flags->Z, flags->Y, flags->X, UDiv->data, flags->data, UOut->data,
                 w.div, w.partials, stats ? stats : m->d_stats, zlo, zhi, ((stg & 2) ? 1 : 0) | ((stg & 4) ? 2 : 0), m->d_ticket, code,
                 ask.project_reads == nullptr);
  return check_launch(c, "model_begin");
}

int model_finish(tfl_ctx* c, tfl_model* m, const tfl_tensor* pDiv, const tfl_tensor* flags, const tfl_tensor* pOut,
                 const tfl_tensor* UOut, float* workspace, int64_t workspace_floats, const double* stats, double count,
                 const tfl_tensor* UBC, const tfl_tensor* UBCInvMask, int doClamp, float lo, float hi, const Scope& sc, Ask& ask) {
  TRY(check_flags(c, "model_finish", flags));
  if (!m) return fail(c, TFL_EINVAL, "model_finish: null model");
  const int is3D = m->is3d ? 1 : 0;
  TRY(check_vel(c, "model_finish", "UOut", UOut, flags, is3D));
  TRY(check_scalar(c, "model_finish", "pDiv", pDiv, flags));
  TRY(check_scalar(c, "model_finish", "pOut", pOut, flags));
  if ((UBC == nullptr) != (UBCInvMask == nullptr)) return fail(c, TFL_EINVAL, "model_finish: UBC and UBCInvMask go together");
  if (UBC) {
    TRY(check_vel(c, "model_finish", "UBC", UBC, flags, is3D));
    TRY(check_vel(c, "model_finish", "UBCInvMask", UBCInvMask, flags, is3D));
  }
  if (!(count > 1.0)) return fail(c, TFL_EINVAL, "model_finish: Sample variance requires more than one sample.");
  ModelWs w;
  TRY(model_ws(c, m, flags, workspace, workspace_floats, &w));
  TRY(graph_gate(c, m, flags, "model_finish"));
  const bool windowed = sc.windowed();
  if (m->path == ConvPath::graph && (stats || sc.stages || windowed))
    return fail(c, TFL_EUNSUPPORTED, "model_finish: banked, batch-norm and max-pool models run un-sharded only");
  if (m->custom && !stats && (sc.stages || windowed))
    return fail(c, TFL_EUNSUPPORTED, "model_finish: a windowed forward of a model with non-default tfl_model_opts takes the caller's "
                                     "input-scale stats over the owned planes (tfl_simulate_step_slab forms them)");
  Fwd a{c->stream, flags->B, flags->Z, flags->Y, flags->X, pDiv->data, UOut->data, flags->data, stats ? stats : m->d_stats,
        count, sc, ask.conv1_sums_stats};
  if (m->custom && !stats) TRY(opts_stats(c, m, w, a));
  // tfl_set_stages (z-slab ranks run each layer under its own z-window): the 3-D default topology's forms take stage bits 1,
  // 2 and 4 (see there); the other 3-D linear models take 1 = the whole net, each launch on its layer's cone of the
  // z-window's planes. 8 = velocity update / un-scale / wall BCs on the window.
  const int stg = sc.passes();
  if (sc.stages && !default3(m->path) && !(m->path == ConvPath::generic && m->is3d))
    return fail(c, TFL_EUNSUPPORTED, "model_finish: stage masks need a 3-D model that is not a graph model");
  switch (m->path) {
    case ConvPath::conv_mfma16: forward_mfma16(m, w, a); break;
    case ConvPath::conv_valu: forward_valu(m, w, a); break;
    case ConvPath::conv_mfma: forward_mfma(m, w, a); break;
    case ConvPath::conv2d_mfma: forward_mfma2d(m, w, a); break;
    case ConvPath::generic: if (stg & 1) TRY(generic_forward(c, m, w, a)); break;
    case ConvPath::graph: TRY(graph_forward(c, m, w, a)); break;
  }
  if (stg & 8) {
    const bool pub = ask.reach_via_project;
    ask.reach_folded = tfl::model_project(a.st, sc, m->is3d, a.B, a.Z, a.Y, a.X, w.pPred, flags->data, a.st_in, a.count,
                                          ask.project_reads ? ask.project_reads : UOut->data, UOut->data, pOut->data,
                                          UBC ? UBC->data : nullptr, UBC ? UBCInvMask->data : nullptr, doClamp, lo, hi,
                                          m->d_range_host ? m->d_range_err : nullptr, m->d_range_host, pub ? c->d_reach : nullptr,
                                          pub ? c->d_reach_host : nullptr, pub ? c->d_reach : nullptr, wall_code_of(c, m, flags),
                                          pub ? c->d_reach_tick : nullptr, ask.fold);
    ask.reach_published = pub;
  }
  return check_launch(c, "model_finish");
}

int model_forward(tfl_ctx* c, tfl_model* m, const tfl_tensor* pDiv, const tfl_tensor* UDiv, const tfl_tensor* flags,
                  const tfl_tensor* pOut, const tfl_tensor* UOut, float* workspace, int64_t workspace_floats, const tfl_tensor* UBC,
                  const tfl_tensor* UBCInvMask, int doClamp, float lo, float hi, const Scope& sc, Ask& ask) {
  TRY(check_flags(c, "model_forward", flags));
  if (sc.stages || sc.windowed())
    return fail(c, TFL_EINVAL, "model_forward: clear the z-window / stage mask first (use tfl_model_begin / _finish)");
  // round 6: with the default 3-D conv path the first layer's blocks sum k_bcs_div_stats' partial pairs themselves (the same
  // order, the same bits) -- no k_reduce_stats launch between the two kernels (4.3 us of pure latency at 128^3)
  ask.conv1_sums_stats = m && m->path == ConvPath::conv_mfma16 && conv3_m16_first_sums_partials() && !conv3_m16_fuse12_requested() &&
                         !model_stats_fold_requested();
  // SetWallBcs(UDiv) is an intermediate of this call: where the net's input has no UDiv channel and the input scale is not taken
  // from a pass over it (opts_stats), only the projection would read it back from UOut -- and that kernel zeroes the very
  // components the wall BCs zeroed, so it reads UDiv itself and the store is left out (model.hip header).
  // tfl_model_begin / _finish, the z-slab step and the training forward keep the store: their callers find U_bc in UOut.
  // So does a call whose UDiv lies inside its own workspace (tfl_simulate_step without a confinement force hands over the
  // advection's scratch velocity, which shares the step's workspace with this call): the conv stack overwrites it before the
  // projection runs, and U_bc in UOut is then the only copy.
  bool keep = !m || !UDiv || !UDiv->data || m->opts.in_UDiv || (m->custom && m->opts.norm_chan == TFL_NORM_UDIV);
  if (!keep && workspace) {
    const uintptr_t u0 = (uintptr_t)UDiv->data, u1 = u0 + sizeof(float) * (size_t)UDiv->B * UDiv->C * UDiv->Z * UDiv->Y * UDiv->X;
    const uintptr_t w0 = (uintptr_t)workspace, w1 = w0 + sizeof(float) * (size_t)(workspace_floats > 0 ? workspace_floats : 0);
    keep = u0 < w1 && w0 < u1;
  }
  ask.project_reads = keep ? nullptr : UDiv->data;
  TRY(model_begin(c, m, UDiv, flags, UOut, workspace, workspace_floats, 0, flags->Z, nullptr, sc, ask));
  const double count = (double)flags->Z * flags->Y * flags->X * (m->is3d ? 3 : 2);
  return model_finish(c, m, pDiv, flags, pOut, UOut, workspace, workspace_floats, nullptr, count, UBC, UBCInvMask, doClamp, lo, hi, sc, ask);
}
}  // namespace tfl

extern "C" {

tfl_model* tfl_model_create(tfl_ctx* c, int is3D, int nlayers, const int32_t* cin, const int32_t* cout,
                            const int32_t* ksize, const float* const* weights, const float* const* biases) {
  return tfl_model_create_ex(c, is3D, nlayers, cin, cout, ksize, nullptr, nullptr, weights, biases);
}

tfl_model* tfl_model_create_ex(tfl_ctx* c, int is3D, int nlayers, const int32_t* cin, const int32_t* cout,
                               const int32_t* ksize, const int32_t* pool, const int32_t* up,
                               const float* const* weights, const float* const* biases) {
  return tfl_model_create_opts(c, is3D, nlayers, cin, cout, ksize, pool, up, weights, biases, nullptr);
}

tfl_model* tfl_model_create_opts(tfl_ctx* c, int is3D, int nlayers, const int32_t* cin, const int32_t* cout,
                                 const int32_t* ksize, const int32_t* pool, const int32_t* up,
                                 const float* const* weights, const float* const* biases, const tfl_model_opts* opts) {
  if (!c) return nullptr;
  auto bad = [&](const char* m) -> tfl_model* { fail(c, TFL_EINVAL, "model_create: %s", m); return nullptr; };
  if (nlayers < 1 || !cin || !cout || !ksize || !weights || !biases) return bad("null or empty layer description");
  tfl_model_opts o;
  if (!model_opts_of(c, nlayers, pool, up, opts, &o)) return nullptr;
  tfl_model* m = build_layers(c, is3D != 0, nlayers, cin, cout, ksize, pool, up, weights, biases, o, stage_table(nlayers), nullptr);
  if (!m) return nullptr;
  // the default topologies run on kernels of their own (TFL_CONV_PATH=direct forces the generic ones)
  auto done = [&]() -> tfl_model* {      // the tables of tfl_model_set_weights_device, now that every buffer exists
    if (refresh_tables(m)) return m;
    tfl_model_destroy(c, m);
    return bad("hipMalloc failed");
  };
  const char* force = tfl::sw::text(tfl::Sw::CONV_PATH);
  if ((force && strcmp(force, "direct") == 0) || m->custom || m->multires || nlayers != 5) return done();
  const int dflt3[5][3] = {{3, 8, 3}, {8, 8, 3}, {8, 8, 3}, {8, 8, 1}, {8, 1, 1}};
  const int dflt2[5][3] = {{3, 16, 3}, {16, 16, 3}, {16, 16, 3}, {16, 16, 3}, {16, 1, 1}};
  auto is = [&](const int (&t)[5][3]) {
    for (int l = 0; l < 5; l++) if (cin[l] != t[l][0] || cout[l] != t[l][1] || ksize[l] != t[l][2]) return false;
    return true;
  };
  const char* err = nullptr;
  if (m->is3d && is(dflt3)) err = pack_default3(m, cin, weights, biases, conv3d_path(force));
  if (!m->is3d && is(dflt2)) err = pack_default2(m, cin, weights);
  if (err) { tfl_model_destroy(c, m); return bad(err); }
  return done();
}

// Every defineModelGraph configuration (include/tfluids_hip.h tfl_model_create_graph; lib/model.lua:253-392). The trivial
// graph is tfl_model_create_opts; everything else is laid out here for the shape-generic kernels (graph_forward below).
tfl_model* tfl_model_create_graph(tfl_ctx* c, int is3D, int nconv, const int32_t* cin, const int32_t* cout,
                                  const int32_t* ksize, const int32_t* pool, const int32_t* up,
                                  const float* const* weights, const float* const* biases, const tfl_model_opts* opts,
                                  const tfl_model_graph* g) {
  if (!c) return nullptr;
  auto bad = [&](const char* m) -> tfl_model* { fail(c, TFL_EINVAL, "model_create: %s", m); return nullptr; };
  auto unsupported = [&](const char* m) -> tfl_model* { fail(c, TFL_EUNSUPPORTED, "model_create: %s", m); return nullptr; };
  if (g) {
    if (g->banks_num < 1 || g->banks_num > tfl::kMaxJoinBanks) return bad("banksNum must be 1 .. 8");
    if (g->pool_type != TFL_POOL_AVG && g->pool_type != TFL_POOL_MAX) return bad("Bad pool type.  Must be 'avg' or 'max'");
  }
  if (!g || (g->banks_num == 1 && !g->batch_norm && g->pool_type == TFL_POOL_AVG))
    return tfl_model_create_opts(c, is3D, nconv, cin, cout, ksize, pool, up, weights, biases, opts);
  if (nconv < 2 || !cin || !cout || !ksize || !weights || !biases) return bad("null or empty layer description");
  const int N = g->banks_num;
  int nst = nconv;
  if (N > 1) {
    if (g->bank_type != TFL_BANKS_MRES && g->bank_type != TFL_BANKS_DILATE) return bad("banksType must be 'mres' or 'dilate'");
    if (g->aggregate != TFL_AGG_CONCAT && g->aggregate != TFL_AGG_ADD) return bad("ERROR: unsupported mconf.banksAggregateMethod");
    if (!(g->split_stage < g->join_stage)) return bad("banksSplitStage must come before banksJoinStage");
    nst = nconv - (N - 1) * (g->join_stage - g->split_stage);
    if (g->split_stage < 1 || g->join_stage >= nst) return bad("banksSplitStage / banksJoinStage must lie before the last stage (model.lua:257-258)");
  }
  if (g->batch_norm && (!g->bn_mean || !g->bn_var || !g->bn_eps)) return bad("addBatchNorm needs running_mean, running_var and eps per module");
  StageTable t = N > 1 ? stage_table(nst, N, g->split_stage, g->join_stage) : stage_table(nst);
  t.mres = g->bank_type == TFL_BANKS_MRES; t.concat = g->aggregate == TFL_AGG_CONCAT;
  auto P = [&](const int32_t* a, int i) { return a ? a[i] : 1; };
  for (int i = 0; i < nconv; i++) {
    const int f = t.first[t.stage[i]];
    if (cin[i] != cin[f] || cout[i] != cout[f] || ksize[i] != ksize[f] || P(pool, i) != P(pool, f) || P(up, i) != P(up, f))
      return bad("the banks of a stage must have the same shape");
    if (N > 1 && !t.mres && t.bank[i] > 0 && P(up, i) > 1) return bad("upsampling not supported for dilated convolutions.");
  }
  // the stage table the options are checked against (one entry per stage)
  std::vector<int32_t> spool(nst), sup(nst);
  for (int st = 1; st <= nst; st++) { spool[st - 1] = P(pool, t.first[st]); sup[st - 1] = P(up, t.first[st]); }
  tfl_model_opts o;
  if (!model_opts_of(c, nst, spool.data(), sup.data(), opts, &o)) return nullptr;
  if (o.pressure_skip && N > 1 && t.mres) return unsupported("addPressureSkip with pooling / upsampling layers");
  tfl_model* m = build_layers(c, is3D != 0, nconv, cin, cout, ksize, pool, up, weights, biases, o, t, g);
  if (!m) return nullptr;
  m->path = ConvPath::graph; m->banks = N; m->bank_type = g->bank_type; m->aggregate = g->aggregate;
  m->split = t.split; m->join = t.join; m->nstages = nst;
  m->pool_max = g->pool_type == TFL_POOL_MAX;
  if (!refresh_tables(m)) { tfl_model_destroy(c, m); return bad("hipMalloc failed"); }
  return m;
}

void tfl_model_destroy(tfl_ctx* c, tfl_model* m) {
  (void)c;
  if (!m) return;
  for (auto& L : m->layers) { if (L.w) (void)hipFree(L.w); if (L.b) (void)hipFree(L.b); if (L.bn) (void)hipFree(L.bn); if (L.wt) (void)hipFree(L.wt); if (L.ws) (void)hipFree(L.ws); }
  if (m->zero_bias) (void)hipFree(m->zero_bias);
  for (int l = 0; l < 3; l++) if (m->bfrag[l]) (void)hipFree(m->bfrag[l]);
  for (int l = 0; l < 3; l++) if (m->wino[l]) (void)hipFree(m->wino[l]);
  for (int l = 0; l < 3; l++) if (m->wfrag16[l]) (void)hipFree(m->wfrag16[l]);
  if (m->d_range_err) (void)hipFree(m->d_range_err);
  if (m->h_range) (void)hipHostFree(m->h_range);
  for (int l = 0; l < 4; l++) if (m->bfrag2[l]) (void)hipFree(m->bfrag2[l]);
  if (m->tail_w4) (void)hipFree(m->tail_w4);
  if (m->tail_pack) (void)hipFree(m->tail_pack);
  if (m->tail_w5) (void)hipFree(m->tail_w5);
  if (m->d_stats) (void)hipFree(m->d_stats);
  if (m->d_ticket) (void)hipFree(m->d_ticket);
  if (m->d_refresh) (void)hipFree(m->d_refresh);
  if (m->d_jobs) (void)hipFree(m->d_jobs);
  if (m->d_post16) (void)hipFree(m->d_post16);
  delete m;
}

int64_t tfl_model_range_errors(tfl_ctx* c, tfl_model* m) {
  if (!c || !m) return -1;
  if (!m->d_range_err) return 0;
  unsigned long long v = 0;
  if (hipMemcpyAsync(&v, m->d_range_err, sizeof(v), hipMemcpyDeviceToHost, c->stream) != hipSuccess) return -1;
  if (hipMemsetAsync(m->d_range_err, 0, sizeof(v), c->stream) != hipSuccess) return -1;
  if (hipStreamSynchronize(c->stream) != hipSuccess) return -1;
  if (m->h_range) *(volatile unsigned long long*)m->h_range = 0;      // acknowledged: the next forward runs again
  return (int64_t)v;
}


int64_t tfl_model_range_flag(tfl_ctx* c, tfl_model* m) {
  if (!c || !m) return -1;
  return m->h_range ? (int64_t)*(volatile unsigned long long*)m->h_range : 0;
}

int64_t tfl_model_workspace_floats(const tfl_model* m, int B, int Z, int Y, int X) {
  if (!m) return -1;
  const int64_t n = (int64_t)B * Z * Y * X;
  // per-block fp64 stat partials (2 doubles = 4 floats per block, kept first for 8-byte alignment)
  // + div[1] + net input[in_c] + two ping-pong activation buffers[max_c] + pPred[1]
  // (+4: the fp16 MFMA path aligns its activation buffers to 16 bytes)
  return 4 * tfl::model_stat_blocks(B, Z, Y, X) + n * (1 + (int64_t)m->in_c + 2 * (int64_t)m->max_c + 1) + (m->path == ConvPath::conv_mfma16 ? 4 : 0) +
         graph_ws_floats(m, B, Z, Y, X, nullptr, nullptr);
}

float* tfl_model_div(const tfl_model* m, int B, int Z, int Y, int X, float* workspace) {
  if (!m || !workspace) return nullptr;
  return workspace + 4 * tfl::model_stat_blocks(B, Z, Y, X);
}

int tfl_model_begin(tfl_ctx* c, tfl_model* m, const tfl_tensor* UDiv, const tfl_tensor* flags, const tfl_tensor* UOut,
                    float* workspace, int64_t workspace_floats, int zlo, int zhi, double* stats) {
  tfl::Ask none;
  return tfl::model_begin(c, m, UDiv, flags, UOut, workspace, workspace_floats, zlo, zhi, stats, tfl::scope_of(c), none);
}

tfl_wall_plan* tfl_wall_plan_create(tfl_ctx* c, const tfl_tensor* flags) {
  if (!c || !flags || !flags->data) return nullptr;
  if (check_flags(c, "wall_plan_create", flags) != TFL_OK) return nullptr;
  const long long n = (long long)flags->B * flags->Z * flags->Y * flags->X;
  tfl_wall_plan* p = new tfl_wall_plan();
  p->flags = flags->data; p->B = flags->B; p->Z = flags->Z; p->Y = flags->Y; p->X = flags->X;
  if (hipMalloc((void**)&p->code, (size_t)n * sizeof(unsigned short)) != hipSuccess) { (void)hipGetLastError(); c->err = "wall_plan_create: hipMalloc failed"; delete p; return nullptr; }
  (void)hipDeviceSynchronize();               // one-time set-up: whoever filled the flags (any stream) is done
  p->is3d = flags->Z > 1; p->owner = c;
  tfl::wall_code(c->stream, p->is3d, flags->B, flags->Z, flags->Y, flags->X, flags->data, p->code);
  if (hipStreamSynchronize(c->stream) != hipSuccess) { (void)hipGetLastError(); (void)hipFree(p->code); c->err = "wall_plan_create: the code kernel failed"; delete p; return nullptr; }
  std::lock_guard<std::mutex> lock(c->wall_mu);
  for (tfl_wall_plan*& q : c->wall_plans)     // a new plan for the same array replaces the old registration (its owner still frees it)
    if (q->flags == p->flags) { q->owner = nullptr; q = p; return p; }
  c->wall_plans.push_back(p);
  return p;
}

// Take the plan out of its context's registry WITHOUT freeing it: no HIP call, safe from a finalizer (where the hipFree of
// tfl_wall_plan_destroy could invalidate a graph capture in progress). The step stops finding it at once -- which matters when the
// flags array has died and its address may be handed out again before the host gets round to tfl_wall_plan_destroy.
void tfl_wall_plan_retire(tfl_wall_plan* p) {
  if (!p) return;
  tfl_ctx* o = p->owner;
  if (!o) return;
  std::lock_guard<std::mutex> lock(o->wall_mu);
  for (size_t i = 0; i < o->wall_plans.size(); i++)
    if (o->wall_plans[i] == p) { o->wall_plans.erase(o->wall_plans.begin() + (long)i); break; }
  p->owner = nullptr;
}

void tfl_wall_plan_destroy(tfl_ctx* c, tfl_wall_plan* p) {
  if (!p) return;
  (void)c;                                    // (the plan knows its context, and whether that context still exists)
  tfl_wall_plan_retire(p);
  if (p->code) (void)hipFree(p->code);
  delete p;
}

int tfl_model_finish(tfl_ctx* c, tfl_model* m, const tfl_tensor* pDiv, const tfl_tensor* flags,
                     const tfl_tensor* pOut, const tfl_tensor* UOut, float* workspace, int64_t workspace_floats,
                     const double* stats, double count, const tfl_tensor* UBC, const tfl_tensor* UBCInvMask,
                     int doClamp, float lo, float hi) {
  tfl::Ask none;
  return tfl::model_finish(c, m, pDiv, flags, pOut, UOut, workspace, workspace_floats, stats, count, UBC, UBCInvMask, doClamp, lo, hi, tfl::scope_of(c), none);
}

int tfl_model_forward(tfl_ctx* c, tfl_model* m, const tfl_tensor* pDiv, const tfl_tensor* UDiv,
                      const tfl_tensor* flags, const tfl_tensor* pOut, const tfl_tensor* UOut, float* workspace,
                      int64_t workspace_floats, const tfl_tensor* UBC, const tfl_tensor* UBCInvMask, int doClamp,
                      float lo, float hi) {
  tfl::Ask none;
  return tfl::model_forward(c, m, pDiv, UDiv, flags, pOut, UOut, workspace, workspace_floats, UBC, UBCInvMask, doClamp, lo, hi, tfl::scope_of(c), none);
}

}  // extern "C"

// ---- the training side: new weights in place, the forward that keeps a tape, the parameter gradients ----
namespace {
// Linear models without pooling / upsampling, and graph models whose modules neither pool nor upsample and that hold no batch
// norm (they hold the data-gradient weights: build_layers); the rest is refused by name
int train_gate(tfl_ctx* c, const tfl_model* m, const char* who) {
  if (m->path == ConvPath::graph && !m->zero_bias)
    return fail(c, TFL_EUNSUPPORTED, "%s: graph models (tfl_model_create_graph) with batch norm, with pooling or ConvolutionUpsample stages, or "
                                     "with a module the weight-gradient kernel's tile cannot hold have no training pass", who);
  if (m->path != ConvPath::graph && (m->multires || !m->zero_bias))
    return fail(c, TFL_EUNSUPPORTED, "%s: models with pooling or ConvolutionUpsample layers (`tog`) have no training pass: the "
                                     "backward of pooling and of the pixel shuffle is not built", who);
  return TFL_OK;
}
// what tfl_model_set_weights_device (and so tfl_optim_step) cannot do, said before anything is launched
int refresh_gate(tfl_ctx* c, const tfl_model* m, const char* who) {
  if (!m->d_refresh)
    return fail(c, TFL_EUNSUPPORTED, "%s: models of more than %d layers take their weights from the host (tfl_model_set_weights)", who,
                tfl::kRefreshMaxLayers);
  if (m->path == ConvPath::conv_mfma16) {
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    HIP_TRY(c, hipStreamIsCapturing(c->stream, &cs));
    if (cs != hipStreamCaptureStatusNone)
      return fail(c, TFL_EUNSUPPORTED, "%s: the split-fp16 MFMA path reads its three post-scales back to the host, which a "
                                       "capturing stream cannot do (create the model under another TFL_CONV_PATH to capture)", who);
  }
  return TFL_OK;
}
std::vector<tfl::TrainLayer> train_layers(const tfl_model* m) {
  std::vector<tfl::TrainLayer> v;
  const bool mres = m->banks > 1 && m->bank_type == TFL_BANKS_MRES;
  for (const tfl_layer& L : m->layers) {
    tfl::TrainLayer t{L.cin, L.cout, L.cin_ref, L.cout_ref, L.k, L.skip_in ? 1 : 0};
    t.dil = L.dil;
    t.sh = (mres && L.stage >= m->split && L.stage < m->join) ? L.bank : 0;
    v.push_back(t);
  }
  return v;
}
static_assert(tfl::kTrainMaxBanks == tfl::kMaxJoinBanks, "tfl_train.hpp and tfl_host.hpp disagree on the most banks");
// the banked modules of the layer table (n = 1: none)
tfl::TrainBanks train_banks(const tfl_model* m) {
  tfl::TrainBanks bk;
  bk.is3d = m->is3d;
  if (m->path != ConvPath::graph || m->banks < 2) return bk;
  bk.n = m->banks; bk.mres = m->bank_type == TFL_BANKS_MRES; bk.concat = m->aggregate == TFL_AGG_CONCAT;
  bk.nst = m->join - m->split; bk.gxc = m->layers[0].gxc;
  while (m->layers[bk.l0].stage != m->split) bk.l0++;
  return bk;
}
// the `count` that goes with the model's input-scale pair (opts_stats; tfl_model_forward's own for the default normaliser)
double scale_count(const tfl_model* m, int Z, int Y, int X) {
  const tfl_model_opts& o = m->opts;
  const double cells = (double)Z * Y * X;
  if (!o.normalize || o.norm_func == TFL_NORMFUNC_L2) return 2.0;
  return o.norm_chan == TFL_NORM_UDIV ? cells * (m->is3d ? 3 : 2) : cells;
}
int check_tape(tfl_ctx* c, const char* who, const tfl::TapeLayout& t, const float* tape, int64_t tape_floats) {
  if (!tape || tape_floats < t.total) return fail(c, TFL_EINVAL, "%s: tape too small (%lld floats needed)", who, (long long)t.total);
  if (((uintptr_t)tape & 7) != 0) return fail(c, TFL_EINVAL, "%s: tape must be 8-byte aligned", who);
  return TFL_OK;
}

// what tfl_model_backward_input takes and gives beyond tfl_model_backward: the forward's inputs and its U, and where the two
// input gradients go (either may be null)
struct InputSide { const tfl_tensor *pDiv, *UDiv, *UOut, *gradPDiv, *gradUDiv; };
tfl::IgChans input_chans(const tfl_model* m) { return tfl::ig_chans(m->is3d, m->opts.in_pDiv, m->opts.in_UDiv, m->opts.in_div); }
tfl::IgLayout input_layout(const tfl_model* m, int B, int Z, int Y, int X) {
  const tfl::TrainBanks bk = train_banks(m);
  return tfl::ig_layout(m->is3d, train_layers(m), input_chans(m), m->opts.pressure_skip != 0,
                        m->opts.normalize && m->opts.norm_chan == TFL_NORM_DIV, B, Z, Y, X, &bk);
}

// tfl_model_backward (in = null: its launches exactly) and tfl_model_backward_input
int model_backward(tfl_ctx* c, tfl_model* m, const char* who, const tfl_tensor* flags, const tfl_tensor* gradP, const tfl_tensor* gradU,
                   const float* tape, int64_t tape_floats, float* workspace, int64_t workspace_floats, float* const* gradWeights,
                   float* const* gradBiases, int accumulate, const InputSide* in) {
  TRY(check_flags(c, who, flags));
  if (!m) return fail(c, TFL_EINVAL, "%s: null model", who);
  TRY(train_gate(c, m, who));
  const int is3D = m->is3d ? 1 : 0;
  if (gradP) TRY(check_scalar(c, who, "gradP", gradP, flags));
  if (gradU) TRY(check_vel(c, who, "gradU", gradU, flags, is3D));
  if (!is3D && flags->Z != 1) return fail(c, TFL_EINVAL, "%s: 2D model but zdepth > 1", who);
  if (in) {
    TRY(check_scalar(c, who, "pDiv", in->pDiv, flags));
    TRY(check_vel(c, who, "UDiv", in->UDiv, flags, is3D));
    TRY(check_vel(c, who, "UOut", in->UOut, flags, is3D));
    if (in->gradPDiv) TRY(check_scalar(c, who, "gradPDiv", in->gradPDiv, flags));
    if (in->gradUDiv) TRY(check_vel(c, who, "gradUDiv", in->gradUDiv, flags, is3D));
  }
  const int B = flags->B, Z = flags->Z, Y = flags->Y, X = flags->X;
  if (B > kMaxBatch) return fail(c, TFL_EINVAL, "%s: batch size above %d", who, kMaxBatch);
  const std::vector<tfl::TrainLayer> tl = train_layers(m);
  const int nl = (int)tl.size();
  TRY(graph_gate(c, m, flags, who));
  const tfl::TrainBanks bk = train_banks(m);
  const tfl::TapeLayout t = tfl::tape_layout(tl, B, Z, Y, X, &bk);
  TRY(check_tape(c, who, t, tape, tape_floats));
  const tfl::IgLayout ig = in ? input_layout(m, B, Z, Y, X) : tfl::IgLayout{};
  const tfl::BwdLayout w = in ? ig.bwd : tfl::bwd_layout(m->is3d, tl, B, Z, Y, X, &bk);
  const int64_t need = in ? ig.total : w.total;
  if (!workspace || workspace_floats < need)
    return fail(c, TFL_EINVAL, "%s: workspace too small (%lld floats needed)", who, (long long)need);
  if (((uintptr_t)workspace & 7) != 0) return fail(c, TFL_EINVAL, "%s: workspace must be 8-byte aligned", who);
  // the parameter gradients: both tables, or (input gradients only) neither
  const bool params = gradWeights || gradBiases || !in;
  if (params && (!gradWeights || !gradBiases)) return fail(c, TFL_EINVAL, "%s: null gradient table", who);
  for (int l = 0; l < nl && params; l++) {
    if (!gradWeights[l] || !gradBiases[l]) return fail(c, TFL_EINVAL, "%s: layer %d has no gradient buffer", who, l);
    if (!tfl::conv_wgrad_fits(tfl::wg_plan(m->is3d, tl[l], B, Z, Y, X)))
      return fail(c, TFL_EUNSUPPORTED, "%s: layer %d (k = %d) does not fit the weight-gradient kernel's tile", who, l, tl[l].k);
  }
  hipStream_t st = c->stream;
  const long long cells = (long long)Z * Y * X;
  const int C = m->is3d ? 3 : 2;
  const double* stats = (const double*)(tape + t.stats);
  const double count = scale_count(m, Z, Y, X);
  float* g = workspace + w.g0;
  float* g2 = workspace + w.g1;
  float* gu = workspace + w.gu;
  double* partials = (double*)(workspace + w.partials);
  // g_pPred = scale gradP + velocityUpdateBackward(setWallBcsBackward(scale gradU)): the wall mask only zeroes, so the
  // scale goes in front of it
  if (gradU) {
    tfl::scale_add(st, B, cells * C, stats, count, gradU->data, nullptr, gu);
    tfl::set_wall_bcs(st, m->is3d, B, Z, Y, X, gu, flags->data);
    tfl::velocity_update_bwd(st, m->is3d, B, Z, Y, X, flags->data, gu, g);
    if (gradP) tfl::scale_add(st, B, cells, stats, count, gradP->data, g, g);
  } else if (gradP) {
    tfl::scale_add(st, B, cells, stats, count, gradP->data, nullptr, g);
  } else {
    HIP_TRY(c, hipMemsetAsync(g, 0, sizeof(float) * (size_t)B * cells, st));
  }
  const int act = 1 + m->opts.nonlin;
  const bool graph = m->path == ConvPath::graph;
  const bool want_in = in && (in->gradPDiv || in->gradUDiv);
  // One module's step on its own grid [Zl][Yl][Xl]: the weight and bias gradient (or the activation mask alone), the joined skip
  // channel's gradient, and -- gout != null -- the data gradient g_in = conv(g_pre, W transposed and mirrored, at the module's tap
  // spacing) into gout; the joined skip channel gets none. A first-stage module's is the net input's, gxc wide.
  auto step = [&](int l, int Zl, int Yl, int Xl, const float* x, const float* y, int ych, float* gl, float* gout) -> int {
    const tfl_layer& L = m->layers[l];
    const bool first = L.stage == 1;
    if (params) {
      const tfl::WgPlan p = tfl::wg_plan(m->is3d, tl[l], B, Z, Y, X);
      // (the masked gradient is written back wherever a data gradient follows: the first layer's only for the input gradients)
      if (!tfl::conv_wgrad(st, m->is3d, p, B, Zl, Yl, Xl, L.cin, L.cout, L.k, x, gl, y, y ? ych : 0, act, (!first || in) && y, partials))
        return fail(c, TFL_EUNSUPPORTED, "%s: no weight-gradient kernel for layer %d (%d output channels)", who, l, L.cout);
      tfl::conv_wgrad_finish(st, p, L.cin, L.cout, L.cin_ref, L.cout_ref, L.skip_in ? 1 : 0, partials, gradWeights[l], gradBiases[l],
                             accumulate != 0, L.join_c, L.join_p);
    } else if (y) {
      tfl::act_mask(st, B, L.cout, ych, (long long)Zl * Yl * Xl, gl, y, act);
    }
    // the joined skip channel's gradient: the gradient at pPred against the skip plane's taps, mirrored
    if (in && L.skip_in && !tfl::conv_direct(st, m->is3d, B, Z, Y, X, L.cout, 1, L.k, 0, gl, L.ws, m->zero_bias, workspace + ig.gskip))
      return fail(c, TFL_EUNSUPPORTED, "%s: no kernel for the skip channel's gradient", who);
    if (!gout) return TFL_OK;
    const int gin_c = L.nx > 0 ? L.gxc : L.cin - (L.skip_in ? 1 : 0);      // (nx: the first stage, and the stage behind a concat join)
    const bool ok = graph ? tfl::conv_direct_graph(st, m->is3d, B, Zl, Yl, Xl, L.cout, gin_c, L.k, 0, gl, L.wt, m->zero_bias, gout, 1, 0, 0, 0,
                                                   L.dil, nullptr, nullptr)
                          : tfl::conv_direct(st, m->is3d, B, Zl, Yl, Xl, L.cout, gin_c, L.k, 0, gl, L.wt, m->zero_bias, gout);
    if (!ok) return fail(c, TFL_EUNSUPPORTED, "%s: no kernel for %d channels", who, gin_c);
    return TFL_OK;
  };
  for (int l = nl - 1; l >= 0;) {
    if (bk.banked(l)) {
      // The banks, g = the gradient at the join's output: the join's backward hands every bank its gradient at its
      // own resolution, each bank walks its modules last stage to first, and the split's backward adds the banks' data gradients
      // -- mres: through the pyramid pool's transpose, coarsest level first -- into the trunk's next buffer (or, where the split is
      // the first stage, into the net input's gradient).
      const int N = bk.n, S = bk.nst, Cp = m->layers[bk.mod(S - 1, 0)].cout;
      int shs[tfl::kMaxJoinBanks], bZ[tfl::kMaxJoinBanks], bY[tfl::kMaxJoinBanks], bX[tfl::kMaxJoinBanks];
      float* head[tfl::kMaxJoinBanks];
      for (int i = 0; i < N; i++) {
        shs[i] = tl[bk.mod(0, i)].sh; head[i] = workspace + w.gb[i][0];
        bZ[i] = m->is3d ? Z >> shs[i] : Z; bY[i] = Y >> shs[i]; bX[i] = X >> shs[i];
      }
      // (g = the data gradient of the stage behind the join: behind a concat join its planes are padded to a kernel width)
      const int gch = bk.concat ? m->layers[bk.end()].gxc : Cp;
      if (!tfl::join_bwd(st, m->is3d, bk.concat, B, Cp, gch, Z, Y, X, N, shs, head, g))
        return fail(c, TFL_EINVAL, "%s: bad bank join", who);
      const float* xin = bk.l0 == 0 ? tape + t.x : tape + t.out[bk.l0 - 1];
      const bool need_split = bk.l0 > 0 || want_in;
      const float* tail[tfl::kMaxJoinBanks];
      for (int i = 0; i < N; i++) {
        float* ga = workspace + w.gb[i][0];
        float* gb = workspace + w.gb[i][1];
        for (int s = S - 1; s >= 0; s--) {
          const int li = bk.mod(s, i);
          const float* x = s > 0 ? tape + t.out[bk.mod(s - 1, i)] : (bk.mres && i > 0) ? tape + t.pyr[i] : xin;
          float* gout = (s > 0 || need_split) ? gb : nullptr;
          TRY(step(li, bZ[i], bY[i], bX[i], x, tape + t.out[li], m->layers[li].cout, ga, gout));
          if (gout) std::swap(ga, gb);
        }
        tail[i] = ga;
      }
      if (need_split) {
        const int planes = bk.l0 == 0 ? ig.gxc : m->layers[bk.l0].cin;
        float* dest = bk.l0 == 0 ? workspace + ig.gx : g2;
        if (bk.mres) {
          const float* coarse = tail[N - 1];
          for (int i = N - 2; i >= 0; i--) {
            float* dst = i == 0 ? dest : const_cast<float*>(tail[i]);
            tfl::pyr_pool_bwd(st, m->is3d, B * planes, bZ[i], bY[i], bX[i], tail[i], coarse, dst);
            coarse = dst;
          }
        } else if (!tfl::bank_sum(st, (long long)B * planes * cells, N, tail, dest)) {
          return fail(c, TFL_EINVAL, "%s: bad bank split", who);
        }
      }
      std::swap(g, g2);
      l = bk.l0 - 1;
      continue;
    }
    const float* x = l == 0 ? tape + t.x : (bk.any() && l == bk.end()) ? tape + t.join : tape + t.out[l - 1];
    const float* y = l + 1 < nl ? tape + t.out[l] : nullptr;
    float* gout = l > 0 ? g2 : want_in ? workspace + ig.gx : nullptr;
    TRY(step(l, Z, Y, X, x, y, tfl::train_och(tl, l), g, gout));
    if (l > 0) std::swap(g, g2);
    l--;
  }
  if (!want_in) return check_launch(c, who);
  // behind the first layer's data gradient: the scale's gradient and the head (input_grad.hip)
  const tfl::IgChans ch = input_chans(m);
  const tfl_model_opts& o = m->opts;
  tfl::IgArgs a{};
  a.flags = flags->data; a.pDiv = in->pDiv->data; a.UDiv = in->UDiv->data; a.UOut = in->UOut->data;
  a.gradP = gradP ? gradP->data : nullptr; a.gradU = gradU ? gradU->data : nullptr; a.h = gradU ? gu : nullptr;
  a.gx = workspace + ig.gx; a.gskip = o.pressure_skip ? workspace + ig.gskip : nullptr;
  a.x = tape + t.x; a.pPred = tape + t.pPred;
  a.stats = stats; a.count = count;
  a.partials = (double*)(workspace + ig.partials); a.gs = (double*)(workspace + ig.gs);
  a.gradPDiv = in->gradPDiv ? in->gradPDiv->data : nullptr; a.gradUDiv = in->gradUDiv ? in->gradUDiv->data : nullptr;
  a.gxc = ig.gxc; a.in_c = m->in_c; a.pch = ch.p; a.uch = ch.u; a.dch = ch.d;
  a.nmode = !o.normalize ? 0 : (o.norm_func == TFL_NORMFUNC_STD ? 1 : 2);
  a.nchan = o.norm_chan; a.blocks = ig.blocks;
  if (a.nmode && o.norm_chan == TFL_NORM_DIV) {
    if (ig.recompute_div) {      // no div channel on the tape to read it back from
      float* ubc = workspace + ig.ubc;
      HIP_TRY(c, hipMemcpyAsync(ubc, in->UDiv->data, sizeof(float) * (size_t)B * cells * C, hipMemcpyDeviceToDevice, st));
      tfl::set_wall_bcs(st, m->is3d, B, Z, Y, X, ubc, flags->data);
      tfl::velocity_divergence(st, m->is3d, B, Z, Y, X, ubc, flags->data, workspace + ig.div);
      a.dsrc = workspace + ig.div; a.dstride = cells; a.dscaled = 0;
    } else {
      a.dsrc = tape + t.x + (long long)ch.d * cells; a.dstride = (long long)m->in_c * cells; a.dscaled = 1;
    }
  }
  if (a.nmode) tfl::input_grad_sums(st, m->is3d, B, Z, Y, X, a);
  tfl::input_grad_head(st, m->is3d, B, Z, Y, X, a);
  return check_launch(c, who);
}
}  // namespace

extern "C" {

int tfl_model_set_weights(tfl_ctx* c, tfl_model* m, const float* const* weights, const float* const* biases) {
  if (!c) return TFL_EINVAL;
  if (!m || !weights || !biases) return fail(c, TFL_EINVAL, "model_set_weights: null model or weight table");
  const int n = (int)m->layers.size();
  for (int l = 0; l < n; l++)
    if (!weights[l] || !biases[l]) return fail(c, TFL_EINVAL, "model_set_weights: layer %d has no weight or no bias", l);
  // every launch that reads the old weights is done before they change; the copies below are synchronous
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  for (int l = 0; l < n; l++)
    if (!upload_layer(m->layers[l], m->is3d, weights[l], biases[l], m->layers[l].wt != nullptr))
      return fail(c, TFL_EHIP, "model_set_weights: uploading layer %d failed", l);
  std::vector<int32_t> cin;
  for (const tfl_layer& L : m->layers) cin.push_back(L.cin_ref);
  const char* err = nullptr;
  if (default3(m->path)) err = pack_default3(m, cin.data(), weights, biases, m->path);
  else if (m->path == ConvPath::conv2d_mfma) err = pack_default2(m, cin.data(), weights);
  if (err) return fail(c, TFL_EHIP, "model_set_weights: %s", err);
  return TFL_OK;
}

int tfl_model_set_weights_device(tfl_ctx* c, tfl_model* m, const float* const* d_weights, const float* const* d_biases) {
  if (!c) return TFL_EINVAL;
  const char* who = "model_set_weights_device";
  if (!m || !d_weights || !d_biases) return fail(c, TFL_EINVAL, "%s: null model or weight table", who);
  const int n = (int)m->layers.size();
  for (int l = 0; l < n; l++)
    if (!d_weights[l] || !d_biases[l]) return fail(c, TFL_EINVAL, "%s: layer %d has no weight or no bias", who, l);
  TRY(refresh_gate(c, m, who));
  tfl::RefreshSrc src{};
  for (int l = 0; l < n; l++) { src.w[l] = d_weights[l]; src.b[l] = d_biases[l]; }
  tfl::refresh_layers(c->stream, src, m->d_refresh, n, m->refresh_elems);
  if (m->njobs > 0) tfl::refresh_pack(c->stream, src, m->d_jobs, m->njobs, m->job_elems);
  if (m->path == ConvPath::conv_mfma16) {
    tfl::refresh_pack16(c->stream, src, m->wfrag16, m->d_post16, m->tail_pack);
    TRY(check_launch(c, who));
    // the one host read: the conv kernels of this path take the three post-scales by value. (m->post16_tail is NOT refreshed: the
    // kernels read the tail's post-scale from tail_pack[89], which the launch above wrote; the host field is only the value
    // pack_default3 hands from conv3_m16_pack_tail to pack_tail3 within one host packing, and is recomputed there before use.)
    HIP_TRY(c, hipMemcpyAsync(m->post16, m->d_post16, 3 * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return TFL_OK;
  }
  return check_launch(c, who);
}

int64_t tfl_model_tape_floats(const tfl_model* m, int B, int Z, int Y, int X) {
  if (!m || !m->zero_bias || B < 1 || Z < 1 || Y < 1 || X < 1) return -1;
  const tfl::TrainBanks bk = train_banks(m);
  return tfl::tape_layout(train_layers(m), B, Z, Y, X, &bk).total;
}

int tfl_model_forward_train(tfl_ctx* c, tfl_model* m, const tfl_tensor* pDiv, const tfl_tensor* UDiv, const tfl_tensor* flags,
                            const tfl_tensor* pOut, const tfl_tensor* UOut, float* workspace, int64_t workspace_floats, float* tape,
                            int64_t tape_floats) {
  const char* who = "model_forward_train";
  TRY(check_flags(c, who, flags));
  if (!m) return fail(c, TFL_EINVAL, "%s: null model", who);
  TRY(train_gate(c, m, who));
  const int is3D = m->is3d ? 1 : 0;
  TRY(check_vel(c, who, "UDiv", UDiv, flags, is3D));
  TRY(check_vel(c, who, "UOut", UOut, flags, is3D));
  TRY(check_scalar(c, who, "pDiv", pDiv, flags));
  TRY(check_scalar(c, who, "pOut", pOut, flags));
  const tfl::Scope sc = tfl::scope_of(c);
  if (sc.stages || sc.windowed()) return fail(c, TFL_EINVAL, "%s: clear the z-window / stage mask first", who);
  const int B = flags->B, Z = flags->Z, Y = flags->Y, X = flags->X;
  TRY(graph_gate(c, m, flags, who));
  const tfl::TrainBanks bk = train_banks(m);
  const tfl::TapeLayout t = tfl::tape_layout(train_layers(m), B, Z, Y, X, &bk);
  TRY(check_tape(c, who, t, tape, tape_floats));
  ModelWs w;
  TRY(model_ws(c, m, flags, workspace, workspace_floats, &w));
  // the same calls as tfl_model_forward of a model on the shape-generic path, with the tape in place of the activation buffers
  tfl::Ask ask;
  ask.gated = false;       // (fp32 throughout: no fp16 range to guard)
  TRY(tfl::model_begin(c, m, UDiv, flags, UOut, workspace, workspace_floats, 0, Z, nullptr, sc, ask));
  Fwd a{c->stream, B, Z, Y, X, pDiv->data, UOut->data, flags->data, m->d_stats, (double)Z * Y * X * (m->is3d ? 3 : 2), sc, false};
  if (m->custom) TRY(opts_stats(c, m, w, a));
  w.x3 = tape + t.x; w.pPred = tape + t.pPred;
  std::vector<float*> outs;
  for (size_t l = 0; l < m->layers.size(); l++) outs.push_back(l + 1 < m->layers.size() ? tape + t.out[l] : w.pPred);
  if (m->path == ConvPath::graph) {
    GraphTape gt{};
    gt.out = outs;
    for (int i = 1; i < bk.n && bk.mres; i++) gt.pyr[i] = tape + t.pyr[i];
    gt.join = bk.any() ? tape + t.join : nullptr;
    TRY(graph_forward(c, m, w, a, &gt));
  } else {
    TRY(generic_forward(c, m, w, a, outs.data()));
  }
  tfl::model_project(a.st, sc, m->is3d, B, Z, Y, X, w.pPred, flags->data, a.st_in, a.count, UOut->data, UOut->data, pOut->data, nullptr, nullptr, 0,
                     0.0f, 0.0f, nullptr, nullptr, nullptr, nullptr, nullptr, wall_code_of(c, m, flags), nullptr, ask.fold);
  HIP_TRY(c, hipMemcpyAsync(tape + t.stats, m->d_stats, sizeof(double) * 2 * B, hipMemcpyDeviceToDevice, c->stream));
  return check_launch(c, who);
}

int64_t tfl_model_backward_workspace_floats(const tfl_model* m, int B, int Z, int Y, int X) {
  if (!m || !m->zero_bias || B < 1 || Z < 1 || Y < 1 || X < 1) return -1;
  const tfl::TrainBanks bk = train_banks(m);
  return tfl::bwd_layout(m->is3d, train_layers(m), B, Z, Y, X, &bk).total;
}

int tfl_model_backward(tfl_ctx* c, tfl_model* m, const tfl_tensor* flags, const tfl_tensor* gradP, const tfl_tensor* gradU,
                       const float* tape, int64_t tape_floats, float* workspace, int64_t workspace_floats, float* const* gradWeights,
                       float* const* gradBiases, int accumulate) {
  return model_backward(c, m, "model_backward", flags, gradP, gradU, tape, tape_floats, workspace, workspace_floats, gradWeights,
                        gradBiases, accumulate, nullptr);
}

int64_t tfl_model_backward_input_workspace_floats(const tfl_model* m, int B, int Z, int Y, int X) {
  if (!m || !m->zero_bias || B < 1 || Z < 1 || Y < 1 || X < 1) return -1;
  return input_layout(m, B, Z, Y, X).total;
}

int tfl_model_backward_input(tfl_ctx* c, tfl_model* m, const tfl_tensor* flags, const tfl_tensor* pDiv, const tfl_tensor* UDiv,
                             const tfl_tensor* UOut, const tfl_tensor* gradP, const tfl_tensor* gradU, const float* tape,
                             int64_t tape_floats, float* workspace, int64_t workspace_floats, float* const* gradWeights,
                             float* const* gradBiases, int accumulate, const tfl_tensor* gradPDiv, const tfl_tensor* gradUDiv) {
  const InputSide in{pDiv, UDiv, UOut, gradPDiv, gradUDiv};
  return model_backward(c, m, "model_backward_input", flags, gradP, gradU, tape, tape_floats, workspace, workspace_floats, gradWeights,
                        gradBiases, accumulate, &in);
}

}  // extern "C"

// ---- the optimiser step on the device: state, the hyper-parameters by value, then the refresh above ----------
struct tfl_optim {
  tfl_model* model = nullptr;
  tfl_optim_config cfg{};
  int ntens = 0;                 // 2 per layer: weight, bias
  long long total = 0;           // parameters
  long long* d_off = nullptr;    // [ntens + 1] prefix offsets of the tensors in the flat parameter space
  float* m = nullptr;            // [total] first moment (RMSprop: the mean square)
  float* v = nullptr;            // [total] second moment (Adam)
  long long* d_t = nullptr;      // the step counter
  double* d_partials = nullptr;  // [kOptimNormBlocks] partial sums of g^2
  int32_t* d_rguard = nullptr;   // the reduced guard word of the last tfl_optim_step_reduced (0 before the first)
};

namespace {
int optim_config_ok(tfl_ctx* c, const tfl_optim_config* k, const char* who) {
  if (!k) return fail(c, TFL_EINVAL, "%s: null config", who);
  if (k->method != TFL_OPTIM_ADAM && k->method != TFL_OPTIM_RMSPROP) return fail(c, TFL_EINVAL, "%s: unknown optimisation method", who);
  for (double x : {k->learningRate, k->learningRateDecay, k->beta1, k->beta2, k->epsilon, k->weightDecay, k->alpha, k->initialMean, k->gradNormThreshold})
    if (!std::isfinite(x)) return fail(c, TFL_EINVAL, "%s: a hyper-parameter is not finite", who);
  return TFL_OK;
}
// what a call with a transport needs of it and of the caller's reduce buffer
int optim_reduce_args_ok(tfl_ctx* c, const tfl_optim* o, const char* who, const tfl_comm* comm, const double* d_reduce, int64_t reduce_doubles) {
  if (comm->size < (int32_t)(offsetof(tfl_comm, allreduce_sum) + sizeof(comm->allreduce_sum)) || !comm->allreduce_sum)
    return fail(c, TFL_EINVAL, "%s: tfl_comm has no size or lacks allreduce_sum", who);
  if (!d_reduce || ((uintptr_t)d_reduce & 7) != 0) return fail(c, TFL_EINVAL, "%s: the reduce buffer is null or not 8-byte aligned", who);
  if (reduce_doubles < (int64_t)o->total + tfl::kOptimReduceTail)
    return fail(c, TFL_EINVAL, "%s: the reduce buffer holds %lld doubles, tfl_optim_reduce_doubles asks for %lld", who,
                (long long)reduce_doubles, (long long)(o->total + tfl::kOptimReduceTail));
  return TFL_OK;
}
// tfl_optim_step_guarded (comm == NULL) and tfl_optim_step_reduced: pack, all-reduce and unpack in front of the same update
int optim_step_any(tfl_ctx* c, tfl_optim* o, const char* who, float* const* d_weights, float* const* d_biases, float* const* d_gradWeights,
                   float* const* d_gradBiases, const int32_t* d_guard, const tfl_comm* comm, int32_t world, double* d_reduce,
                   int64_t reduce_doubles) {
  if (!c) return TFL_EINVAL;
  if (((uintptr_t)d_guard & 3) != 0) return fail(c, TFL_EINVAL, "%s: the guard word is not 4-byte aligned", who);
  if (!o || !d_weights || !d_biases || !d_gradWeights || !d_gradBiases) return fail(c, TFL_EINVAL, "%s: null optimiser or parameter table", who);
  const int n = o->ntens / 2;
  tfl::OptimPtrs p{};
  for (int l = 0; l < n; l++) {
    if (!d_weights[l] || !d_biases[l] || !d_gradWeights[l] || !d_gradBiases[l])
      return fail(c, TFL_EINVAL, "%s: layer %d lacks a parameter or a gradient array", who, l);
    p.x[2 * l] = d_weights[l]; p.x[2 * l + 1] = d_biases[l];
    p.g[2 * l] = d_gradWeights[l]; p.g[2 * l + 1] = d_gradBiases[l];
  }
  if (comm) {
    if (world < 1) return fail(c, TFL_EINVAL, "%s: a world of %d ranks", who, (int)world);
    TRY(optim_reduce_args_ok(c, o, who, comm, d_reduce, reduce_doubles));
  }
  TRY(refresh_gate(c, o->model, who));
  const tfl_optim_config& k = o->cfg;
  const bool adam = k.method == TFL_OPTIM_ADAM;
  tfl::OptimArgs a{};
  a.method = adam ? 0 : 1;
  a.b1 = (float)k.beta1; a.omb1 = (float)(1.0 - k.beta1);
  a.b2 = (float)(adam ? k.beta2 : k.alpha); a.omb2 = (float)(1.0 - (adam ? k.beta2 : k.alpha));
  a.eps = (float)k.epsilon; a.wd = (float)k.weightDecay;
  a.lr = k.learningRate; a.lrd = k.learningRateDecay; a.beta1 = k.beta1; a.beta2 = k.beta2;
  a.threshold = k.gradNormThreshold > 0.0 ? k.gradNormThreshold : 0.0;
  if (comm) {
    tfl::optim_pack(c->stream, p, o->d_off, o->ntens, o->total, d_guard, d_reduce, 0);
    TRY(check_launch(c, who));
    if (comm->allreduce_sum(comm->user, d_reduce, (int64_t)o->total + 1) != 0) { c->err = "optim_step_reduced: comm callback failed (allreduce_sum)"; return TFL_EINVAL; }
    tfl::optim_unpack(c->stream, p, o->d_off, o->ntens, o->total, d_reduce, world, a.threshold > 0.0 ? o->d_partials : nullptr, o->d_rguard, false);
    d_guard = o->d_rguard;
  }
  tfl::optim_step(c->stream, p, o->d_off, o->ntens, o->total, o->d_partials, o->m, o->v, o->d_t, a, d_guard, comm != nullptr);
  TRY(check_launch(c, who));
  return tfl_model_set_weights_device(c, o->model, d_weights, d_biases);
}
}  // namespace

extern "C" {

tfl_optim* tfl_optim_create(tfl_ctx* c, tfl_model* m, const tfl_optim_config* config) {
  if (!c) return nullptr;
  const char* who = "optim_create";
  if (!m) { fail(c, TFL_EINVAL, "%s: null model", who); return nullptr; }
  if (optim_config_ok(c, config, who) != TFL_OK) return nullptr;
  if ((int)m->layers.size() > tfl::kRefreshMaxLayers) { fail(c, TFL_EUNSUPPORTED, "%s: more than %d layers", who, tfl::kRefreshMaxLayers); return nullptr; }
  tfl_optim* o = new tfl_optim();
  o->model = m; o->cfg = *config;
  std::vector<long long> off(1, 0);
  for (const tfl_layer& L : m->layers) {
    const long long taps = m->is3d ? L.k * L.k * L.k : L.k * L.k, S = m->is3d ? L.up * L.up * L.up : L.up * L.up;
    off.push_back(off.back() + (long long)L.cout_ref * S * L.cin_ref * taps);
    off.push_back(off.back() + (long long)L.cout_ref * S);
  }
  o->ntens = (int)off.size() - 1; o->total = off.back();
  const size_t bytes = sizeof(float) * (size_t)o->total;
  const bool adam = config->method == TFL_OPTIM_ADAM;
  bool ok = hipMalloc((void**)&o->d_off, off.size() * sizeof(long long)) == hipSuccess &&
            hipMemcpy(o->d_off, off.data(), off.size() * sizeof(long long), hipMemcpyHostToDevice) == hipSuccess &&
            hipMalloc((void**)&o->m, bytes) == hipSuccess && (!adam || hipMalloc((void**)&o->v, bytes) == hipSuccess) &&
            hipMalloc((void**)&o->d_t, sizeof(long long)) == hipSuccess &&
            hipMalloc((void**)&o->d_partials, sizeof(double) * tfl::kOptimNormBlocks) == hipSuccess &&
            hipMalloc((void**)&o->d_rguard, sizeof(int32_t)) == hipSuccess &&
            hipMemsetAsync(o->d_rguard, 0, sizeof(int32_t), c->stream) == hipSuccess &&
            hipMemsetAsync(o->d_t, 0, sizeof(long long), c->stream) == hipSuccess &&
            hipMemsetAsync(o->m, 0, bytes, c->stream) == hipSuccess && (!adam || hipMemsetAsync(o->v, 0, bytes, c->stream) == hipSuccess);
  if (ok && !adam && config->initialMean != 0.0) tfl::optim_fill(c->stream, o->m, o->total, (float)config->initialMean);
  if (!ok || check_launch(c, who) != TFL_OK) { if (!ok) fail(c, TFL_EHIP, "%s: hipMalloc failed", who); tfl_optim_destroy(c, o); return nullptr; }
  return o;
}

int tfl_optim_set_config(tfl_ctx* c, tfl_optim* o, const tfl_optim_config* config) {
  if (!c) return TFL_EINVAL;
  if (!o) return fail(c, TFL_EINVAL, "optim_set_config: null optimiser");
  TRY(optim_config_ok(c, config, "optim_set_config"));
  if (config->method != o->cfg.method) return fail(c, TFL_EINVAL, "optim_set_config: the method is fixed at creation");
  o->cfg = *config;
  return TFL_OK;
}

int tfl_optim_step(tfl_ctx* c, tfl_optim* o, float* const* d_weights, float* const* d_biases, float* const* d_gradWeights,
                   float* const* d_gradBiases) {
  return tfl_optim_step_guarded(c, o, d_weights, d_biases, d_gradWeights, d_gradBiases, nullptr);
}

int tfl_optim_step_guarded(tfl_ctx* c, tfl_optim* o, float* const* d_weights, float* const* d_biases, float* const* d_gradWeights,
                           float* const* d_gradBiases, const int32_t* d_guard) {
  return optim_step_any(c, o, d_guard ? "optim_step_guarded" : "optim_step", d_weights, d_biases, d_gradWeights, d_gradBiases, d_guard,
                        nullptr, 1, nullptr, 0);
}

int64_t tfl_optim_reduce_doubles(tfl_ctx* c, tfl_optim* o) {
  if (!c || !o) return -1;
  return (int64_t)o->total + tfl::kOptimReduceTail;
}

int tfl_optim_step_reduced(tfl_ctx* c, tfl_optim* o, float* const* d_weights, float* const* d_biases, float* const* d_gradWeights,
                           float* const* d_gradBiases, const int32_t* d_guard, const tfl_comm* comm, int32_t world, double* d_reduce,
                           int64_t reduce_doubles) {
  if (!comm) return tfl_optim_step_guarded(c, o, d_weights, d_biases, d_gradWeights, d_gradBiases, d_guard);
  return optim_step_any(c, o, "optim_step_reduced", d_weights, d_biases, d_gradWeights, d_gradBiases, d_guard, comm, world, d_reduce,
                        reduce_doubles);
}

int tfl_optim_reduced_guard(tfl_ctx* c, tfl_optim* o, int32_t* d_out) {
  if (!c) return TFL_EINVAL;
  if (!o || !d_out) return fail(c, TFL_EINVAL, "optim_reduced_guard: null optimiser or output word");
  if (hipMemcpyAsync(d_out, o->d_rguard, sizeof(int32_t), hipMemcpyDeviceToDevice, c->stream) != hipSuccess)
    return fail(c, TFL_EHIP, "optim_reduced_guard: the copy failed");
  return TFL_OK;
}

int tfl_optim_sync_parameters(tfl_ctx* c, tfl_optim* o, float* const* d_weights, float* const* d_biases, const tfl_comm* comm,
                              int32_t rank, double* d_reduce, int64_t reduce_doubles) {
  if (!c) return TFL_EINVAL;
  const char* who = "optim_sync_parameters";
  if (!o || !d_weights || !d_biases) return fail(c, TFL_EINVAL, "%s: null optimiser or parameter table", who);
  const int n = o->ntens / 2;
  tfl::OptimPtrs p{};
  for (int l = 0; l < n; l++) {
    if (!d_weights[l] || !d_biases[l]) return fail(c, TFL_EINVAL, "%s: layer %d lacks a parameter array", who, l);
    p.x[2 * l] = d_weights[l]; p.x[2 * l + 1] = d_biases[l];
  }
  TRY(refresh_gate(c, o->model, who));
  if (comm) {
    if (rank < 0) return fail(c, TFL_EINVAL, "%s: rank %d", who, (int)rank);
    TRY(optim_reduce_args_ok(c, o, who, comm, d_reduce, reduce_doubles));
    tfl::optim_pack(c->stream, p, o->d_off, o->ntens, o->total, nullptr, d_reduce, rank == 0 ? 1 : 2);
    TRY(check_launch(c, who));
    if (comm->allreduce_sum(comm->user, d_reduce, (int64_t)o->total) != 0) { c->err = "optim_sync_parameters: comm callback failed (allreduce_sum)"; return TFL_EINVAL; }
    tfl::optim_unpack(c->stream, p, o->d_off, o->ntens, o->total, d_reduce, 1, nullptr, nullptr, true);
    TRY(check_launch(c, who));
  }
  return tfl_model_set_weights_device(c, o->model, d_weights, d_biases);
}

int64_t tfl_optim_steps(tfl_ctx* c, tfl_optim* o) {
  if (!c || !o) return -1;
  long long t = 0;
  if (hipMemcpyAsync(&t, o->d_t, sizeof(t), hipMemcpyDeviceToHost, c->stream) != hipSuccess) return -1;
  if (hipStreamSynchronize(c->stream) != hipSuccess) return -1;
  return (int64_t)t;
}

int64_t tfl_optim_get_state(tfl_ctx* c, tfl_optim* o, float* d_m, float* d_v) {
  if (!c || !o) return -1;
  const size_t bytes = sizeof(float) * (size_t)o->total;
  if (d_m && hipMemcpyAsync(d_m, o->m, bytes, hipMemcpyDeviceToDevice, c->stream) != hipSuccess) return -1;
  if (d_v && o->v && hipMemcpyAsync(d_v, o->v, bytes, hipMemcpyDeviceToDevice, c->stream) != hipSuccess) return -1;
  return (int64_t)o->total;
}

int tfl_optim_set_state(tfl_ctx* c, tfl_optim* o, const float* d_m, const float* d_v, int64_t steps) {
  if (!c) return TFL_EINVAL;
  const char* who = "optim_set_state";
  if (!o) return fail(c, TFL_EINVAL, "%s: null optimiser", who);
  if (steps < 0) return fail(c, TFL_EINVAL, "%s: a step count of %lld", who, (long long)steps);
  const size_t bytes = sizeof(float) * (size_t)o->total;
  if (d_m) HIP_TRY(c, hipMemcpyAsync(o->m, d_m, bytes, hipMemcpyDeviceToDevice, c->stream));
  if (d_v && o->v) HIP_TRY(c, hipMemcpyAsync(o->v, d_v, bytes, hipMemcpyDeviceToDevice, c->stream));
  tfl::optim_set_steps(c->stream, o->d_t, (long long)steps);
  return check_launch(c, who);
}

void tfl_optim_destroy(tfl_ctx* c, tfl_optim* o) {
  (void)c;
  if (!o) return;
  if (o->d_off) (void)hipFree(o->d_off);
  if (o->m) (void)hipFree(o->m);
  if (o->v) (void)hipFree(o->v);
  if (o->d_t) (void)hipFree(o->d_t);
  if (o->d_partials) (void)hipFree(o->d_partials);
  if (o->d_rguard) (void)hipFree(o->d_rguard);
  delete o;
}

}  // extern "C"
