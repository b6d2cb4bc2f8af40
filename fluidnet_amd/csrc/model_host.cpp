// model_host.cpp -- the inference forward of the projection ConvNet behind include/tfluids_hip.h: the fp16 range gate and its two
// entries, the workspace layout and its entries, the wall plans, and the forward pass (tfl_model_begin / _finish / _forward) in
// its six forms, with the z-slab cone and slab stats the native steps ask for. The tfl_model object is tfl_model.hpp's and is
// made by model_build.cpp; the training pass (model_train.cpp) reuses the workspace layout, the gates and the two shape-generic
// forwards from here (tfl_model.hpp says which). The native steps never see tfl_model's fields: they ask through model_is_graph /
// model_grid_factor / model_cone / model_range_counter (tfl_host.hpp, tfl_ops.hpp).
#include <algorithm>
#include <cstddef>
#include <vector>

#include "tfl_model.hpp"

using tfl::fail; using tfl::check_flags; using tfl::check_vel; using tfl::check_scalar; using tfl::check_launch;
using namespace tfl::model;

namespace {
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
  const int taps = layer_taps(m->is3d, L), S = layer_subs(m->is3d, L);
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
}  // namespace

namespace tfl {
namespace model {
int model_ws(tfl_ctx* c, const tfl_model* m, const tfl_tensor* flags, float* workspace, int64_t workspace_floats,
             ModelWs* w) {
  const int B = flags->B, Z = flags->Z, Y = flags->Y, X = flags->X;
  if (B > kMaxBatch) return fail(c, TFL_EINVAL, "model: batch size above %d", kMaxBatch);
  const int64_t n = (int64_t)B * Z * Y * X;
  TRY(check_buffer(c, "model", "workspace", workspace, workspace_floats, tfl_model_workspace_floats(m, B, Z, Y, X)));
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

const unsigned short* wall_code_of(tfl_ctx* c, const tfl_model* m, const tfl_tensor* flags) {
  std::lock_guard<std::mutex> lock(c->wall_mu);
  for (const tfl_wall_plan* wp : c->wall_plans)
    if (wp->flags == flags->data && wp->is3d == m->is3d && wp->B == flags->B && wp->Z == flags->Z && wp->Y == flags->Y && wp->X == flags->X) return wp->code;
  return nullptr;
}

int graph_gate(tfl_ctx* c, const tfl_model* m, const tfl_tensor* flags, const char* who) {
  if (m->path != ConvPath::graph) return TFL_OK;
  const int f = m->max_down;
  if ((m->is3d && flags->Z % f) || flags->Y % f || flags->X % f)
    return fail(c, TFL_EINVAL, "%s: grid %dx%dx%d is not divisible by the model's downsampling factor %d (banks x pooling)", who,
                flags->Z, flags->Y, flags->X, f);
  return TFL_OK;
}

// The conv stack of a graph model (lib/model.lua:262-362): trunk stages in the act[] ping-pong, the banks in their own
// buffers, one k_bank_join launch at the join (none when every bank wrote its own concat slice: dilate + concat).
// gt (tfl_model_forward_train): the same launches with the tape as their destinations -- every module's output in its own entry
// (so no bank writes its slice of the join itself: k_bank_join copies or adds every bank, and for 'add' bank 1 is copied into the
// join first), the pyramid levels and the join in theirs. Copies are exact: the bits are those of the inference form.
int graph_forward(tfl_ctx* c, const tfl_model* m, const ModelWs& w, const Fwd& a, const GraphTape* gt) {
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
}  // namespace model
}  // namespace tfl

namespace {
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
}  // namespace

// Every other linear model, layer by layer on the shape-generic kernels. The planes of every launch: the whole grid, or (a
// z-window [za, zb) on a 3-D model: a z-slab rank's owned planes) the cone of the planes the velocity update reads, layer by
// layer (model_cone).
// outs (tfl_model_forward_train): where each layer's output goes instead of the act[] ping-pong -- the tape; pooled_to: the same
// for the pooled output of a pooling layer.
int tfl::model::generic_forward(tfl_ctx* c, const tfl_model* m, const ModelWs& w, const Fwd& a, float* const* outs, float* const* pooled_to) {
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
    const int taps = layer_taps(m->is3d, L), S = layer_subs(m->is3d, L);
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
      float* pooled = (pooled_to && pooled_to[l]) ? pooled_to[l] : in == w.act[0] ? w.act[1] : w.act[0];
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
