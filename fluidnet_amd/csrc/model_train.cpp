// model_train.cpp -- the training pass of the projection ConvNet: which models have one
// (train_gate), the layer table as the layouts of tfl_train.hpp / tfl_input_grad.hpp see it, the forward that keeps a tape
// (tfl_model_forward_train, on model_host.cpp's two shape-generic forwards) and the backward, phase by phase (`Backward`):
// tfl_model_backward's parameter gradients and tfl_model_backward_input's gradients to pDiv and UDiv. The kernels are
// conv_bwd.hip's, backward.hip's and input_grad.hip's; the new weights go back in through model_build.cpp.
#include <algorithm>
#include <cstddef>
#include <vector>

#include "tfl_input_grad.hpp"
#include "tfl_model.hpp"

using tfl::fail; using tfl::check_flags; using tfl::check_vel; using tfl::check_scalar; using tfl::check_launch;
using namespace tfl::model;

namespace {
// Linear models without pooling / upsampling, linear models with them once tfl_model_enable_multires_training has built their
// training-side forms, and graph models whose modules neither pool nor upsample and that hold no batch norm
// (they all hold the data-gradient weights and the zero bias: build_layers); the rest is refused by name
int train_gate(tfl_ctx* c, const tfl_model* m, const char* who) {
  if (m->path == ConvPath::graph && !m->zero_bias)
    return fail(c, TFL_EUNSUPPORTED, "%s: graph models (tfl_model_create_graph) with batch norm, with pooling or ConvolutionUpsample stages, or "
                                     "with a module the weight-gradient kernel's tile cannot hold have no training pass", who);
  if (m->path != ConvPath::graph && !m->zero_bias)
    return fail(c, TFL_EUNSUPPORTED, "%s: models with pooling or ConvolutionUpsample layers (`tog`) have no training pass: the "
                                     "backward of pooling and of the pixel shuffle is not built", who);
  return TFL_OK;
}
// a model with a training pass on a non-empty grid: what the three *_floats entries answer for (else -1)
bool trainable_at(const tfl_model* m, int B, int Z, int Y, int X) { return m && m->zero_bias && B >= 1 && Z >= 1 && Y >= 1 && X >= 1; }
std::vector<tfl::TrainLayer> train_layers(const tfl_model* m) {
  std::vector<tfl::TrainLayer> v;
  const bool mres = m->banks > 1 && m->bank_type == TFL_BANKS_MRES;
  int sh = 0;      // a linear model with pooling / upsampling layers: the shift of the current activations
  for (const tfl_layer& L : m->layers) {
    tfl::TrainLayer t = train_layer(L);
    t.sh = (mres && L.stage >= m->split && L.stage < m->join) ? L.bank : 0;
    if (multires_trainable(m)) {
      t.sh = sh;
      sh += (L.pool > 1 ? 1 : 0) - (L.up > 1 ? 1 : 0);
    }
    v.push_back(t);
  }
  return v;
}
// a linear model with pooling / upsampling layers takes grids its coarsest level divides (generic_forward's own refusal, said
// before anything is enqueued)
int multires_gate(tfl_ctx* c, const tfl_model* m, const tfl_tensor* flags, const char* who) {
  if (!multires_trainable(m)) return TFL_OK;
  const int f = m->max_down;
  if ((m->is3d && flags->Z % f) || flags->Y % f || flags->X % f)
    return fail(c, TFL_EINVAL, "%s: grid %dx%dx%d is not divisible by the model's pooling factor %d", who, flags->Z, flags->Y, flags->X, f);
  return TFL_OK;
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

// what tfl_model_backward_input takes and gives beyond tfl_model_backward: the forward's inputs and its U, and where the two
// input gradients go (either may be null)
struct InputSide { const tfl_tensor *pDiv, *UDiv, *UOut, *gradPDiv, *gradUDiv; };
tfl::IgChans input_chans(const tfl_model* m) { return tfl::ig_chans(m->is3d, m->opts.in_pDiv, m->opts.in_UDiv, m->opts.in_div); }
tfl::IgLayout input_layout(const tfl_model* m, int B, int Z, int Y, int X) {
  const tfl::TrainBanks bk = train_banks(m);
  return tfl::ig_layout(m->is3d, train_layers(m), input_chans(m), m->opts.pressure_skip != 0,
                        m->opts.normalize && m->opts.norm_chan == TFL_NORM_DIV, B, Z, Y, X, &bk);
}

// tfl_model_backward (in = null: its launches exactly) and tfl_model_backward_input, phase by phase. The
// phases share the call's arguments and what validate() resolved of them: the grid, the layer table and the three layouts.
struct Backward {
  tfl_ctx* c; tfl_model* m; const char* who;      // who: the entry's name, in front of every refusal
  const tfl_tensor *flags, *gradP, *gradU;
  const float* tape; int64_t tape_floats; float* ws; int64_t ws_floats;
  float* const* gradWeights; float* const* gradBiases; int accumulate;
  const InputSide* in;
  int B = 0, Z = 0, Y = 0, X = 0;
  std::vector<tfl::TrainLayer> tl;
  tfl::TrainBanks bk;
  tfl::TapeLayout t;                   // the tape
  tfl::BwdLayout w;                    // the workspace of the parameter gradients ...
  tfl::IgLayout ig;                    // ... and (in) of the input gradients around it
  bool params = false;                 // the parameter gradients: both tables, or (input gradients only) neither
  bool want_in = false;                // an input gradient is asked for
  hipStream_t st = nullptr;
  long long cells = 0; int C = 0;      // of the grid; the velocity's channels
  const double* stats = nullptr; double count = 0.0;      // the input-scale pair of the forward (on the tape)
  float* gu = nullptr; double* partials = nullptr;        // workspace: scale gradU (wall BCs applied), the weight gradient's partials
  int act = 0; bool graph = false;

  int validate();          // every refusal, before anything is enqueued; the layouts
  int head_gradient();     // the gradient at pPred from gradP / gradU, into the workspace's g0
  int module(int l, int Zl, int Yl, int Xl, const float* x, const float* y, int ych, float* gl, float* gout);
  int banks(float* g, float* g2);
  int trunk();             // every module from the last to the first, the banks where they sit
  int trunk_multires();    // the same for a linear model whose resolution changes from layer to layer
  int input_head();        // behind the first layer's data gradient: the gradients to pDiv and UDiv
};

int Backward::validate() {
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
  B = flags->B; Z = flags->Z; Y = flags->Y; X = flags->X;
  if (B > kMaxBatch) return fail(c, TFL_EINVAL, "%s: batch size above %d", who, kMaxBatch);
  tl = train_layers(m);
  TRY(graph_gate(c, m, flags, who));
  TRY(multires_gate(c, m, flags, who));
  bk = train_banks(m);
  t = tfl::tape_layout(tl, B, Z, Y, X, &bk);
  TRY(check_buffer(c, who, "tape", tape, tape_floats, t.total));
  ig = in ? input_layout(m, B, Z, Y, X) : tfl::IgLayout{};
  w = in ? ig.bwd : tfl::bwd_layout(m->is3d, tl, B, Z, Y, X, &bk);
  TRY(check_buffer(c, who, "workspace", ws, ws_floats, in ? ig.total : w.total));
  params = gradWeights || gradBiases || !in;
  if (params && (!gradWeights || !gradBiases)) return fail(c, TFL_EINVAL, "%s: null gradient table", who);
  for (int l = 0; l < (int)tl.size() && params; l++) {
    if (!gradWeights[l] || !gradBiases[l]) return fail(c, TFL_EINVAL, "%s: layer %d has no gradient buffer", who, l);
    if (!tfl::conv_wgrad_fits(tfl::wg_plan(m->is3d, tl[l], B, Z, Y, X)))
      return fail(c, TFL_EUNSUPPORTED, "%s: layer %d (k = %d) does not fit the weight-gradient kernel's tile", who, l, tl[l].k);
  }
  want_in = in && (in->gradPDiv || in->gradUDiv);
  st = c->stream;
  cells = (long long)Z * Y * X;
  C = m->is3d ? 3 : 2;
  stats = (const double*)(tape + t.stats);
  count = scale_count(m, Z, Y, X);
  gu = ws + w.gu;
  partials = (double*)(ws + w.partials);
  act = 1 + m->opts.nonlin;
  graph = m->path == ConvPath::graph;
  return TFL_OK;
}

// g_pPred = scale gradP + velocityUpdateBackward(setWallBcsBackward(scale gradU)): the wall mask only zeroes, so the
// scale goes in front of it
int Backward::head_gradient() {
  float* g = ws + w.g0;
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
  return TFL_OK;
}

// One module's step on its own grid [Zl][Yl][Xl]: the weight and bias gradient (or the activation mask alone), the joined skip
// channel's gradient, and -- gout != null -- the data gradient g_in = conv(g_pre, W transposed and mirrored, at the module's tap
// spacing) into gout; the joined skip channel gets none. A first-stage module's is the net input's, gxc wide.
int Backward::module(int l, int Zl, int Yl, int Xl, const float* x, const float* y, int ych, float* gl, float* gout) {
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
  if (in && L.skip_in && !tfl::conv_direct(st, m->is3d, B, Z, Y, X, L.cout, 1, L.k, 0, gl, L.ws, m->zero_bias, ws + ig.gskip))
    return fail(c, TFL_EUNSUPPORTED, "%s: no kernel for the skip channel's gradient", who);
  if (!gout) return TFL_OK;
  const int gin_c = L.nx > 0 ? L.gxc : L.cin - (L.skip_in ? 1 : 0);      // (nx: the first stage, and the stage behind a concat join)
  const bool ok = graph ? tfl::conv_direct_graph(st, m->is3d, B, Zl, Yl, Xl, L.cout, gin_c, L.k, 0, gl, L.wt, m->zero_bias, gout, 1, 0, 0, 0,
                                                 L.dil, nullptr, nullptr)
                        : tfl::conv_direct(st, m->is3d, B, Zl, Yl, Xl, L.cout, gin_c, L.k, 0, gl, L.wt, m->zero_bias, gout);
  if (!ok) return fail(c, TFL_EUNSUPPORTED, "%s: no kernel for %d channels", who, gin_c);
  return TFL_OK;
}

// The banks, g = the gradient at the join's output: the join's backward hands every bank its gradient at its
// own resolution, each bank walks its modules last stage to first, and the split's backward adds the banks' data gradients
// -- mres: through the pyramid pool's transpose, coarsest level first -- into g2, the trunk's next buffer (or, where the split is
// the first stage, into the net input's gradient).
int Backward::banks(float* g, float* g2) {
  const int N = bk.n, S = bk.nst, Cp = m->layers[bk.mod(S - 1, 0)].cout;
  int shs[tfl::kMaxJoinBanks], bZ[tfl::kMaxJoinBanks], bY[tfl::kMaxJoinBanks], bX[tfl::kMaxJoinBanks];
  float* head[tfl::kMaxJoinBanks];
  for (int i = 0; i < N; i++) {
    shs[i] = tl[bk.mod(0, i)].sh; head[i] = ws + w.gb[i][0];
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
    float* ga = ws + w.gb[i][0];
    float* gb = ws + w.gb[i][1];
    for (int s = S - 1; s >= 0; s--) {
      const int li = bk.mod(s, i);
      const float* x = s > 0 ? tape + t.out[bk.mod(s - 1, i)] : (bk.mres && i > 0) ? tape + t.pyr[i] : xin;
      float* gout = (s > 0 || need_split) ? gb : nullptr;
      TRY(module(li, bZ[i], bY[i], bX[i], x, tape + t.out[li], m->layers[li].cout, ga, gout));
      if (gout) std::swap(ga, gb);
    }
    tail[i] = ga;
  }
  if (!need_split) return TFL_OK;
  const int planes = bk.l0 == 0 ? ig.gxc : m->layers[bk.l0].cin;
  float* dest = bk.l0 == 0 ? ws + ig.gx : g2;
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
  return TFL_OK;
}

// g holds the gradient at the current module's output, g2 takes its data gradient: the two swap behind every module that has a
// module in front of it, and behind the banks
int Backward::trunk() {
  float* g = ws + w.g0;
  float* g2 = ws + w.g1;
  const int nl = (int)tl.size();
  for (int l = nl - 1; l >= 0;) {
    if (bk.banked(l)) {
      TRY(banks(g, g2));
      std::swap(g, g2);
      l = bk.l0 - 1;
      continue;
    }
    const float* x = l == 0 ? tape + t.x : (bk.any() && l == bk.end()) ? tape + t.join : tape + t.out[l - 1];
    const float* y = l + 1 < nl ? tape + t.out[l] : nullptr;
    float* gout = l > 0 ? g2 : want_in ? ws + ig.gx : nullptr;
    TRY(module(l, Z, Y, X, x, y, tfl::train_och(tl, l), g, gout));
    if (l > 0) std::swap(g, g2);
    l--;
  }
  return TFL_OK;
}

// A linear model with pooling / upsampling layers. Layer l's convolution runs on grid >> sh_l; g arrives at the
// resolution of what the next layer read. A pooling layer first takes it back through the pool, masked by its own activation in
// the same pass (pool_bwd_mask, into the other buffer); an upsample layer's weight gradient reads g where the shuffle put it and
// its data gradient adds the sub-positions inside one launch (up_dgrad). Neither the skip channel nor banks exist here.
int Backward::trunk_multires() {
  float* g = ws + w.g0;
  float* g2 = ws + w.g1;
  const int nl = (int)tl.size();
  for (int l = nl - 1; l >= 0; l--) {
    const tfl_layer& L = m->layers[l];
    const tfl::TrainLayer& T = tl[l];
    const int Zi = m->is3d ? Z >> T.sh : Z, Yi = Y >> T.sh, Xi = X >> T.sh;                 // the convolution's grid
    const int Zo = m->is3d ? Zi * T.up : Zi, Yo = Yi * T.up, Xo = Xi * T.up;                // its output's, behind the shuffle
    const float* x = l == 0 ? tape + t.x : tl[l - 1].pool > 1 ? tape + t.pooled[l - 1] : tape + t.out[l - 1];
    const float* y = l + 1 < nl ? tape + t.out[l] : nullptr;
    if (T.pool > 1) {
      tfl::pool_bwd_mask(st, m->is3d, B * L.cout, Zo, Yo, Xo, y, g, g2, act);
      std::swap(g, g2);
      y = nullptr;      // (g is masked already)
    }
    const bool dgrad = l > 0 || want_in;
    if (params) {
      const tfl::WgPlan p = tfl::wg_plan(m->is3d, T, B, Z, Y, X);
      if (!tfl::conv_wgrad(st, m->is3d, p, B, Zi, Yi, Xi, L.cin, L.cout, L.k, x, g, y, y ? L.cout : 0, act, dgrad && y, partials))
        return fail(c, TFL_EUNSUPPORTED, "%s: no weight-gradient kernel for layer %d (%d output channels)", who, l, L.cout);
      tfl::conv_wgrad_finish(st, p, L.cin, L.cout, L.cin_ref, L.cout_ref, 0, partials, gradWeights[l], gradBiases[l], accumulate != 0, 0, 0);
    } else if (y) {
      tfl::act_mask(st, B, L.cout, L.cout, (long long)Zo * Yo * Xo, g, y, act);
    }
    if (!dgrad) break;
    float* gout = l > 0 ? g2 : ws + ig.gx;
    const int gin_c = L.nx > 0 ? L.gxc : L.cin;
    const bool ok = T.up > 1 ? tfl::up_dgrad(st, m->is3d, B, Zi, Yi, Xi, T.up, L.cout, gin_c, L.k, g, L.wt, gout)
                             : tfl::conv_direct(st, m->is3d, B, Zi, Yi, Xi, L.cout, gin_c, L.k, 0, g, L.wt, m->zero_bias, gout);
    if (!ok) return fail(c, TFL_EUNSUPPORTED, "%s: no kernel for %d channels", who, gin_c);
    std::swap(g, g2);
  }
  return TFL_OK;
}

// behind the first layer's data gradient: the scale's gradient and the head (input_grad.hip)
int Backward::input_head() {
  const tfl::IgChans ch = input_chans(m);
  const tfl_model_opts& o = m->opts;
  tfl::IgArgs a{};
  a.flags = flags->data; a.pDiv = in->pDiv->data; a.UDiv = in->UDiv->data; a.UOut = in->UOut->data;
  a.gradP = gradP ? gradP->data : nullptr; a.gradU = gradU ? gradU->data : nullptr; a.h = gradU ? gu : nullptr;
  a.gx = ws + ig.gx; a.gskip = o.pressure_skip ? ws + ig.gskip : nullptr;
  a.x = tape + t.x; a.pPred = tape + t.pPred;
  a.stats = stats; a.count = count;
  a.partials = (double*)(ws + ig.partials); a.gs = (double*)(ws + ig.gs);
  a.gradPDiv = in->gradPDiv ? in->gradPDiv->data : nullptr; a.gradUDiv = in->gradUDiv ? in->gradUDiv->data : nullptr;
  a.gxc = ig.gxc; a.in_c = m->in_c; a.pch = ch.p; a.uch = ch.u; a.dch = ch.d;
  a.nmode = !o.normalize ? 0 : (o.norm_func == TFL_NORMFUNC_STD ? 1 : 2);
  a.nchan = o.norm_chan; a.blocks = ig.blocks;
  if (a.nmode && o.norm_chan == TFL_NORM_DIV) {
    if (ig.recompute_div) {      // no div channel on the tape to read it back from
      float* ubc = ws + ig.ubc;
      HIP_TRY(c, hipMemcpyAsync(ubc, in->UDiv->data, sizeof(float) * (size_t)B * cells * C, hipMemcpyDeviceToDevice, st));
      tfl::set_wall_bcs(st, m->is3d, B, Z, Y, X, ubc, flags->data);
      tfl::velocity_divergence(st, m->is3d, B, Z, Y, X, ubc, flags->data, ws + ig.div);
      a.dsrc = ws + ig.div; a.dstride = cells; a.dscaled = 0;
    } else {
      a.dsrc = tape + t.x + (long long)ch.d * cells; a.dstride = (long long)m->in_c * cells; a.dscaled = 1;
    }
  }
  if (a.nmode) tfl::input_grad_sums(st, m->is3d, B, Z, Y, X, a);
  tfl::input_grad_head(st, m->is3d, B, Z, Y, X, a);
  return TFL_OK;
}

int model_backward(tfl_ctx* c, tfl_model* m, const char* who, const tfl_tensor* flags, const tfl_tensor* gradP, const tfl_tensor* gradU,
                   const float* tape, int64_t tape_floats, float* workspace, int64_t workspace_floats, float* const* gradWeights,
                   float* const* gradBiases, int accumulate, const InputSide* in) {
  Backward b{c, m, who, flags, gradP, gradU, tape, tape_floats, workspace, workspace_floats, gradWeights, gradBiases, accumulate, in};
  TRY(b.validate());
  TRY(b.head_gradient());
  TRY(multires_trainable(m) ? b.trunk_multires() : b.trunk());
  if (b.want_in) TRY(b.input_head());
  return check_launch(c, who);
}
}  // namespace

extern "C" {

int64_t tfl_model_tape_floats(const tfl_model* m, int B, int Z, int Y, int X) {
  if (!trainable_at(m, B, Z, Y, X)) return -1;
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
  TRY(multires_gate(c, m, flags, who));
  const tfl::TrainBanks bk = train_banks(m);
  const tfl::TapeLayout t = tfl::tape_layout(train_layers(m), B, Z, Y, X, &bk);
  TRY(check_buffer(c, who, "tape", tape, tape_floats, t.total));
  ModelWs w;
  TRY(model_ws(c, m, flags, workspace, workspace_floats, &w));
  // the same calls as tfl_model_forward of a model on the shape-generic path, with the tape in place of the activation buffers
  tfl::Ask ask;
  ask.gated = false;       // (fp32 throughout: no fp16 range to guard)
  TRY(tfl::model_begin(c, m, UDiv, flags, UOut, workspace, workspace_floats, 0, Z, nullptr, sc, ask));
  Fwd a{c->stream, B, Z, Y, X, pDiv->data, UOut->data, flags->data, m->d_stats, (double)Z * Y * X * (m->is3d ? 3 : 2), sc, false};
  if (m->custom) TRY(opts_stats(c, m, w, a));
  w.x3 = tape + t.x; w.pPred = tape + t.pPred;
  std::vector<float*> outs, pooled;
  for (size_t l = 0; l < m->layers.size(); l++) {
    outs.push_back(l + 1 < m->layers.size() ? tape + t.out[l] : w.pPred);
    pooled.push_back(m->layers[l].pool > 1 && l < t.pooled.size() && t.pooled[l] > 0 ? tape + t.pooled[l] : nullptr);
  }
  if (m->path == ConvPath::graph) {
    GraphTape gt{};
    gt.out = outs;
    for (int i = 1; i < bk.n && bk.mres; i++) gt.pyr[i] = tape + t.pyr[i];
    gt.join = bk.any() ? tape + t.join : nullptr;
    TRY(graph_forward(c, m, w, a, &gt));
  } else {
    TRY(generic_forward(c, m, w, a, outs.data(), pooled.data()));
  }
  tfl::model_project(a.st, sc, m->is3d, B, Z, Y, X, w.pPred, flags->data, a.st_in, a.count, UOut->data, UOut->data, pOut->data, nullptr, nullptr, 0,
                     0.0f, 0.0f, nullptr, nullptr, nullptr, nullptr, nullptr, wall_code_of(c, m, flags), nullptr, ask.fold);
  HIP_TRY(c, hipMemcpyAsync(tape + t.stats, m->d_stats, sizeof(double) * 2 * B, hipMemcpyDeviceToDevice, c->stream));
  return check_launch(c, who);
}

int64_t tfl_model_backward_workspace_floats(const tfl_model* m, int B, int Z, int Y, int X) {
  if (!trainable_at(m, B, Z, Y, X)) return -1;
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
  if (!trainable_at(m, B, Z, Y, X)) return -1;
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
