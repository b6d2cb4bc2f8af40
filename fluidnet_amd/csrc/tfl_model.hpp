// tfl_model.hpp -- the tfl_model object behind the opaque tfl_model* of include/tfluids_hip.h (layer table, packed weights, conv
// path) and what the ConvNet host files share of it. Private to model_build.cpp (makes and refills it), model_host.cpp (the
// inference forward), model_train.cpp (the training pass) and optim_host.cpp (asks through param_counts / refresh_gate alone), as
// tfl_ctx.hpp is to its users: the native steps and abi.cpp never see the fields, they ask through model_is_graph /
// model_grid_factor / model_cone / model_range_counter (tfl_host.hpp, tfl_ops.hpp).
#pragma once
#include <vector>

#include "tfl_abi.hpp"
#include "tfl_ops.hpp"
#include "tfl_refresh.hpp"
#include "tfl_train.hpp"

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
                       // gxc input planes of which the first nx are real (relay_first_transposed: tfl_model_backward_input);
                       // an upsample layer's (tfl_model_enable_multires_training) is [sub][tap][cout][cin], one per sub-position
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

// What crosses a file boundary between the ConvNet host files (C++ linkage, not part of the library's symbol table).
namespace tfl {
namespace model __attribute__((visibility("hidden"))) {

// taps of a layer's kernel and the sub-position convolutions of a ConvolutionUpsample layer (1 otherwise)
inline int layer_taps(bool is3d, const tfl_layer& L) { return is3d ? L.k * L.k * L.k : L.k * L.k; }
inline int layer_subs(bool is3d, const tfl_layer& L) { return is3d ? L.up * L.up * L.up : L.up * L.up; }
// the layer as the training side sees it (tfl_train.hpp), at the grid's resolution (sh = 0: train_layers sets the banks')
inline TrainLayer train_layer(const tfl_layer& L) {
  TrainLayer t{L.cin, L.cout, L.cin_ref, L.cout_ref, L.k, L.skip_in ? 1 : 0};
  t.dil = L.dil;
  t.pool = L.pool; t.up = L.up;
  return t;
}
// a caller's float buffer (`what`: workspace, tape): there, long enough and 8-byte aligned -- or the refusal, under the entry's name
inline int check_buffer(tfl_ctx* c, const char* who, const char* what, const float* p, int64_t have, int64_t need) {
  if (!p || have < need) return fail(c, TFL_EINVAL, "%s: %s too small (%lld floats needed)", who, what, (long long)need);
  if (((uintptr_t)p & 7) != 0) return fail(c, TFL_EINVAL, "%s: %s must be 8-byte aligned", who, what);
  return TFL_OK;
}

// -- model_build.cpp --
// what tfl_model_set_weights_device (and so tfl_optim_step) cannot do, said before anything is launched
int refresh_gate(tfl_ctx* c, const tfl_model* m, const char* who);
// a linear model with pooling / upsampling layers that tfl_model_enable_multires_training has given its training-side forms
inline bool multires_trainable(const tfl_model* m) { return m->path != ConvPath::graph && m->multires && m->zero_bias; }
// the elements of every layer's cudnn weight and bias, {weight, bias} per layer in layer order (the optimiser's flat space)
std::vector<long long> param_counts(const tfl_model* m);

// -- model_host.cpp --
// the model's workspace as tfl_model_workspace_floats lays it out; refuses (`model: ...`) a null, short or misaligned one
struct ModelWs { double* partials; float* div; float* x3; float* act[2]; float* pPred; float* bank[kMaxJoinBanks][2]; float* pyr[kMaxJoinBanks]; };
int model_ws(tfl_ctx* c, const tfl_model* m, const tfl_tensor* flags, float* workspace, int64_t workspace_floats, ModelWs* w);
// the wall codes of THESE flags, if the host registered them with this context (tfl_wall_plan_create), else null
const unsigned short* wall_code_of(tfl_ctx* c, const tfl_model* m, const tfl_tensor* flags);
// a graph model's grid must be divisible by its largest downsampling factor (the mres pyramid times the pooling): refused
// before anything is launched (the reference fails at the join)
int graph_gate(tfl_ctx* c, const tfl_model* m, const tfl_tensor* flags, const char* who);
// What every forward of tfl_model_finish reads. U: the wall-BC'd velocity tfl_model_begin left in UOut; (st_in, count): the
// input scale; sc: the window and stage mask of the call.
struct Fwd {
  hipStream_t st;
  int B, Z, Y, X;
  const float *pDiv, *U, *flags;
  const double* st_in; double count;
  const Scope& sc;
  bool conv1_sums_stats;      // tfl_model_forward (whole array, the model's own stats buffer): conv layer 1 sums the partials
};
// the input scale of a model with non-default tfl_model_opts, into the model's stats buffer and a.count
int opts_stats(tfl_ctx* c, const tfl_model* m, const ModelWs& w, Fwd& a);
// The two shape-generic forwards; tfl_model_forward_train hands them the tape as their destinations (gt / outs).
struct GraphTape { std::vector<float*> out; float* pyr[kMaxJoinBanks]; float* join; };
int graph_forward(tfl_ctx* c, const tfl_model* m, const ModelWs& w, const Fwd& a, const GraphTape* gt = nullptr);
// (pooled: where a pooling layer's pooled output goes, per layer; null entries and a null table: the act[] ping-pong)
int generic_forward(tfl_ctx* c, const tfl_model* m, const ModelWs& w, const Fwd& a, float* const* outs = nullptr,
                    float* const* pooled = nullptr);

}  // namespace model
}  // namespace tfl
