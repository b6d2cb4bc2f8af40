// model_build.cpp -- everything that makes or refills the buffers of a tfl_model (tfl_model.hpp): the options and the stage table
// of a new model, its layer table with the padded, re-laid weights (build_layers / upload_layer), the default topologies' own
// packings, the device tables of the weight refresh, and the entries tfl_model_create* / _destroy / _set_weights[_device]. The
// forward that reads the buffers is model_host.cpp, the training pass model_train.cpp.
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "tfl_input_grad.hpp"
#include "tfl_model.hpp"

using tfl::fail; using tfl::check_launch;
using tfl::model::layer_taps; using tfl::model::layer_subs;

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
// the data-gradient form of a layer from its re-laid weight [sub][tap][cin][cout]: one slice per sub-position (an upsample layer of a
// model enabled for training has several; the first layer, which has its own form, never upsamples)
bool transposed_form(const tfl_layer& L, bool is3d, const std::vector<float>& relaid, std::vector<float>& wt) {
  const int taps = layer_taps(is3d, L), S = layer_subs(is3d, L);
  if (L.nx > 0) {
    if (S != 1) return false;
    tfl::relay_first_transposed(taps, L.cin, L.cout, L.nx, L.gxc, relaid.data(), wt);
    return true;
  }
  wt.clear();
  std::vector<float> one;
  for (int sub = 0; sub < S; sub++) {
    tfl::relay_transposed(taps, L.cin, L.cout, L.cin - (L.skip_in ? 1 : 0), relaid.data() + (size_t)sub * taps * L.cin * L.cout, one);
    wt.insert(wt.end(), one.begin(), one.end());
  }
  return true;
}

bool upload_layer(tfl_layer& L, bool is3d, const float* w, const float* b, bool transposed) {
  const int taps = layer_taps(is3d, L), S = layer_subs(is3d, L);
  auto cmap = [&](int ci) {
    return (L.skip_in && ci == L.cin_ref - 1) ? L.cin - 1 : L.join_c > 0 ? (ci / L.join_c) * L.join_p + ci % L.join_c : ci;
  };
  std::vector<float> relaid, bias_p;
  tfl::relay_layer(S, taps, L.cin, L.cout, L.cin_ref, L.cout_ref, w, b, cmap, relaid, bias_p);
  if (!upload(L.w, relaid.data(), relaid.size() * sizeof(float)) || !upload(L.b, bias_p.data(), bias_p.size() * sizeof(float))) return false;
  if (!transposed) return true;
  std::vector<float> wt;
  if (!transposed_form(L, is3d, relaid, wt) || !upload(L.wt, wt.data(), wt.size() * sizeof(float))) return false;
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
    trainable = trainable && L.pool == 1 && L.up == 1 && tfl::conv_wgrad_fits(tfl::wg_plan(is3d, tfl::model::train_layer(L), 1, 8, 8, 8));
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
    r.taps = layer_taps(m->is3d, L);
    r.S = layer_subs(m->is3d, L);
    r.cin = L.cin; r.cout = L.cout; r.cin_ref = L.cin_ref; r.cout_ref = L.cout_ref;
    r.join_c = L.join_c; r.join_p = L.join_p; r.skip_in = L.skip_in ? 1 : 0;
    r.cin_t = L.nx > 0 ? L.gxc : L.cin - (L.skip_in ? 1 : 0);
    r.wt_first = L.nx; r.ws = L.ws;
    r.n_w = r.S * r.taps * r.cin * r.cout; r.n_b = r.S * r.cout; r.n_wt = L.wt ? r.S * r.taps * r.cout * r.cin_t : 0;
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
}  // namespace

namespace tfl {
namespace model {
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

std::vector<long long> param_counts(const tfl_model* m) {
  std::vector<long long> n;
  for (const tfl_layer& L : m->layers) {
    const long long outs = (long long)L.cout_ref * layer_subs(m->is3d, L);
    n.push_back(outs * L.cin_ref * layer_taps(m->is3d, L));
    n.push_back(outs);
  }
  return n;
}
}  // namespace model
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
// graph is tfl_model_create_opts; everything else is laid out here for the shape-generic kernels (model_host.cpp graph_forward).
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

// The training-side forms of a linear model with pooling / upsampling layers, built from the weights the model
// holds on the device. Every refusal comes before anything is allocated or written.
int tfl_model_enable_multires_training(tfl_ctx* c, tfl_model* m) {
  if (!c) return TFL_EINVAL;
  const char* who = "model_enable_multires_training";
  if (!m) return fail(c, TFL_EINVAL, "%s: null model", who);
  if (m->zero_bias) return TFL_OK;      // (a model with a training pass already)
  if (m->path == ConvPath::graph)
    return fail(c, TFL_EUNSUPPORTED, "%s: graph models (tfl_model_create_graph: banks, max pooling, batch norm) with pooling or "
                                     "ConvolutionUpsample stages stay without a training pass", who);
  const int n = (int)m->layers.size();
  if (n > tfl::kRefreshMaxLayers)
    return fail(c, TFL_EUNSUPPORTED, "%s: models of more than %d layers have no training pass with pooling or ConvolutionUpsample layers",
                who, tfl::kRefreshMaxLayers);
  for (int l = 0; l < n; l++) {
    const tfl_layer& L = m->layers[l];
    if (!tfl::conv_wgrad_fits(tfl::wg_plan(m->is3d, tfl::model::train_layer(L), 1, 8, 8, 8)))
      return fail(c, TFL_EUNSUPPORTED, "%s: layer %d (k = %d, %d input channels) does not fit the weight-gradient kernel's tile", who, l, L.k, L.cin);
    if (L.up > 1 && (l == 0 || tfl::train_width(L.cin) != L.cin))
      return fail(c, TFL_EUNSUPPORTED, "%s: layer %d: no data-gradient kernel for an upsample layer of %d input channels", who, l, L.cin);
  }
  // every launch that reads or writes the weights is done before they are read back
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  tfl_layer& F = m->layers[0];
  F.nx = m->in_c - 1; F.gxc = tfl::ig_width(m->in_c - 1);      // (build_layers: the first layer's form)
  for (tfl_layer& L : m->layers) {
    std::vector<float> relaid((size_t)layer_subs(m->is3d, L) * layer_taps(m->is3d, L) * L.cin * L.cout), wt;
    HIP_TRY(c, hipMemcpy(relaid.data(), L.w, relaid.size() * sizeof(float), hipMemcpyDeviceToHost));
    if (!transposed_form(L, m->is3d, relaid, wt) || !upload(L.wt, wt.data(), wt.size() * sizeof(float)))
      return fail(c, TFL_EHIP, "%s: uploading the data-gradient weights failed", who);
  }
  if (!refresh_tables(m)) return fail(c, TFL_EHIP, "%s: hipMalloc failed", who);
  // (last: the model counts as trainable only once everything else is in place)
  const std::vector<float> zeros(64, 0.0f);
  if (!upload(m->zero_bias, zeros.data(), zeros.size() * sizeof(float))) return fail(c, TFL_EHIP, "%s: hipMalloc failed", who);
  return TFL_OK;
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

// ---- new weights in place: from the host (synchronous), or from device arrays on the stream ----
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
  TRY(tfl::model::refresh_gate(c, m, who));
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

}  // extern "C"
