// tfl_refresh.hpp -- the index arithmetic of the device-side weight refresh (tfl_model_set_weights_device, weights_refresh.hip)
// and of the optimiser step's flat parameter space (optim.hip). Every re-layout the model holds is written as a GATHER: one
// thread per destination element asks here which cudnn-layout source element it holds (or none: a padded zero), so the padding
// is rewritten as zeros on every refresh and no two threads share a destination. Plain C++ without a HIP call: the kernels call
// these functions on the device, and a stand-alone host program walks them over exactly sized buffers under a sanitizer and
// holds the result to the host packers byte for byte (tests/refresh_layout_host.cpp; tfl_train.hpp relay_layer /
// relay_transposed, tfl_pack.hpp).
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#ifndef TFL_HD
#define TFL_HD __host__ __device__
#endif
#else
#ifndef TFL_HD
#define TFL_HD
#endif
#endif

namespace tfl {

// the most layers a model may have for the device refresh and the optimiser step: their launches take the caller's device
// pointers by value (one weight and one bias pointer per layer), so that nothing is copied to the device per call
constexpr int kRefreshMaxLayers = 32;
struct RefreshSrc { const float* w[kRefreshMaxLayers]; const float* b[kRefreshMaxLayers]; };

// ---- the generic forms of every layer: w [sub][tap][cin][cout], b [sub][cout], wt [tap][cout][cin_t], ws [tap] ---------------
// One entry per layer of the model's device table (built at creation): destinations and map parameters (tfl_model.hpp tfl_layer)
struct RefreshLayer {
  float *w, *b, *wt;          // wt = null: the layer holds no data-gradient form
  int S, taps, cin, cout;     // sub-positions (ConvolutionUpsample), taps, padded channel counts
  int cin_ref, cout_ref;      // the cudnn weight's channel counts: [cout_ref * S][cin_ref][taps]
  int join_c, join_p;         // > 0: reference input channel ci sits on plane (ci / join_c) * join_p + ci % join_c
  int skip_in;                // the last reference input channel is the joined skip channel, on the last padded plane
  int cin_t;                  // input planes of wt (cin without the skip plane)
  int n_w, n_b, n_wt;         // elements of the three destinations
  // the input-gradient forms (tfl_model_backward_input). The FIRST layer's wt: cin_t is padded to a width conv_direct has, and
  // only its first wt_first planes are real (the net input without the occupancy channel; the rest are zeros). The last layer of
  // a model with the joined skip channel: ws [tap] = the skip plane's taps of output channel 0, mirrored.
  int wt_first;               // > 0: wt is the first layer's form with this many real planes
  float* ws;                  // null: no skip form
  int n_ws;
};
// the reference input channel that sits on padded plane cp, or -1 (the inverse of upload_layer's cmap)
TFL_HD inline int refresh_ci_of_plane(const RefreshLayer& L, int cp) {
  if (L.skip_in && cp == L.cin - 1) return L.cin_ref - 1;
  int ci = cp;
  if (L.join_c > 0) {
    const int bank = cp / L.join_p, r = cp - bank * L.join_p;
    if (r >= L.join_c) return -1;
    ci = bank * L.join_c + r;
  }
  return ci < L.cin_ref - (L.skip_in ? 1 : 0) ? ci : -1;
}
// element d of w -> its element of the cudnn weight, or -1 (padding)
TFL_HD inline long long refresh_w_src(const RefreshLayer& L, int d) {
  const int co = d % L.cout, cp = (d / L.cout) % L.cin, t = (d / (L.cout * L.cin)) % L.taps, sub = d / (L.cout * L.cin * L.taps);
  const int ci = refresh_ci_of_plane(L, cp);
  if (co >= L.cout_ref || ci < 0) return -1;
  return (((long long)co * L.S + sub) * L.cin_ref + ci) * L.taps + t;
}
// element d of b -> its element of the cudnn bias, or -1
TFL_HD inline int refresh_b_src(const RefreshLayer& L, int d) {
  const int co = d % L.cout, sub = d / L.cout;
  return co < L.cout_ref ? co * L.S + sub : -1;
}
// element d of wt -> its element of the cudnn weight, or -1: wt[sub][tap][co][ci] = w[sub][taps - 1 - tap][ci][co] (n_wt covers
// sub-position 0 alone, or -- an upsample layer of a model enabled for training -- all S)
TFL_HD inline long long refresh_wt_src(const RefreshLayer& L, int d) {
  const int cp = d % L.cin_t, co = (d / L.cin_t) % L.cout, t = (d / (L.cin_t * L.cout)) % L.taps, sub = d / (L.cin_t * L.cout * L.taps);
  if (L.wt_first > 0 && cp >= L.wt_first) return -1;
  const int ci = refresh_ci_of_plane(L, cp);
  if (co >= L.cout_ref || ci < 0) return -1;
  return (((long long)co * L.S + sub) * L.cin_ref + ci) * L.taps + (L.taps - 1 - t);
}
// element d of ws -> its element of the cudnn weight: ws[tap] = w[taps - 1 - tap][skip plane][0] (sub-position 0)
TFL_HD inline long long refresh_ws_src(const RefreshLayer& L, int d) {
  return (long long)(L.cin_ref - 1) * L.taps + (L.taps - 1 - d);
}

// ---- the fp32 forms of the two default topologies (tfl_pack.hpp pack_bfrag3 / pack_wino3 / pack_tail3 / pack_bfrag2) ---------
enum { kPackBfrag3 = 0, kPackWino3 = 1, kPackCopy = 2, kPackTail3 = 3, kPackBfrag2 = 4 };
// One entry per packed buffer: n destination floats from layer `layer`'s weight (kPackTail3: from layers 2, 3, 4)
struct PackJob { float* dst; int kind, layer, ci_n, n; };
TFL_HD inline int pack_bfrag3_src(int ci_n, int d) {
  const int lane = d & 63, ky = (d >> 6) % 3, kz = (d / 192) % 3, c = d / 576;
  const int k = lane >> 4, n = lane & 15, ph = n >> 3, co = n & 7, kx = k - ph;
  if (kx < 0 || kx > 2) return -1;
  return (((co * ci_n + c) * 3 + kz) * 3 + ky) * 3 + kx;
}
// element d of wino = [dz dy][cin][4][8]: the first of its three x-taps in the cudnn weight, and which of the four it is
TFL_HD inline int pack_wino3_src(int ci_n, int d, int* p) {
  const int co = d & 7, c = (d >> 5) % ci_n, zy = d / (32 * ci_n);
  *p = (d >> 3) & 3;
  return ((co * ci_n + c) * 9 + zy) * 3;
}
TFL_HD inline float pack_wino3_val(const float* g, int p) {
  return p == 0 ? g[0] : p == 1 ? 0.5f * ((g[0] + g[2]) + g[1]) : p == 2 ? 0.5f * ((g[0] + g[2]) - g[1]) : g[2];
}
// element d < 89 of the tail pack: element *i of layer *layer's bias (*bias = 1) or weight
TFL_HD inline void pack_tail3_src(int d, int* layer, int* bias, int* i) {
  if (d < 8) { *layer = 2; *bias = 1; *i = d; }
  else if (d < 72) { *layer = 3; *bias = 0; *i = d - 8; }
  else if (d < 80) { *layer = 3; *bias = 1; *i = d - 72; }
  else if (d < 88) { *layer = 4; *bias = 0; *i = d - 80; }
  else { *layer = 4; *bias = 1; *i = 0; }
}
TFL_HD inline int pack_bfrag2_src(int ci_n, int d) {
  const int c4n = (ci_n + 3) / 4;
  const int lane = d & 63, c4 = (d >> 6) % c4n, tap = d / (64 * c4n);
  const int k = lane >> 4, n = lane & 15, c = 4 * c4 + k;
  return c < ci_n ? (n * ci_n + c) * 9 + tap : -1;
}

// ---- the split-fp16 A fragments of conv_mfma16.hip (tfl_pack.hpp conv3_m16_pack_weights / _pack_tail) ----------------------
// float -> IEEE binary16 bits, round to nearest even through the subnormals, never flushed: tfl_pack.hpp f2h in the same integer
// arithmetic (a hardware conversion would obey the wave's fp16 denormal mode). Deliberately a second copy, not the host's
// function made TFL_HD: while the host packers are the yardstick of the device ones they stay untouched, and
// tests/refresh_layout_host.cpp holds the two conversions to each other (every binary16 pattern, every tie and its
// neighbours, a sweep through the subnormal range). Once that period ends the two become one TFL_HD function.
TFL_HD inline uint16_t refresh_f2h(float f) {
  uint32_t u; __builtin_memcpy(&u, &f, 4);
  const uint32_t sign = (u >> 16) & 0x8000u;
  u &= 0x7fffffffu;
  if (u >= 0x47800000u) return (uint16_t)(sign | 0x7c00u);
  if (u < 0x38800000u) {
    if (u < 0x33000000u) return (uint16_t)sign;
    const int e = (int)(u >> 23);
    const uint32_t m = (u & 0x7fffffu) | 0x800000u;
    const int shift = 126 - e;
    uint32_t r = m >> shift;
    const uint32_t rem = m & ((1u << shift) - 1), half = 1u << (shift - 1);
    if (rem > half || (rem == half && (r & 1))) r++;
    return (uint16_t)(sign | r);
  }
  uint32_t r = ((u - 0x38000000u) >> 13);
  const uint32_t rem = u & 0x1fffu;
  if (rem > 0x1000u || (rem == 0x1000u && (r & 1))) r++;
  return (uint16_t)(sign | r);
}
// binary16 bits -> float (exact)
TFL_HD inline float refresh_h2f(uint16_t h) {
  const uint32_t sign = (uint32_t)(h & 0x8000u) << 16;
  const uint32_t e = (h >> 10) & 31, m = h & 0x3ffu;
  float v;
  if (e == 0) v = (float)m * 5.9604644775390625e-8f;                 // m 2^-24: exact, and a normal fp32
  else {
    const uint32_t u = e == 31 ? 0x7f800000u : (((e + 112u) << 23) | (m << 13));
    __builtin_memcpy(&v, &u, 4);
  }
  uint32_t u; __builtin_memcpy(&u, &v, 4); u |= sign; __builtin_memcpy(&v, &u, 4);
  return v;
}
// the exponent e with max|w| 2^e in [8, 16); 0 for an all-zero or non-finite layer
TFL_HD inline int m16_exp(float mx) {
  uint32_t u; __builtin_memcpy(&u, &mx, 4);
  if (!(mx > 0.0f) || (u & 0x7f800000u) == 0x7f800000u) return 0;
  int ex; (void)frexpf(mx, &ex);
  return 4 - ex;
}
TFL_HD inline float m16_post(int e) { return ldexpf(1.0f, -(11 + e)); }
// one fragment half from its weight: {w_h, w_l} of w 2^e (lo = 1: the low half), times 2^11 where it multiplies the
// activations' high halves (hi = 1)
TFL_HD inline uint16_t m16_half(float w, int e, int lo, int hi) {
  const float ws = ldexpf(w, e);
  const float wh = refresh_h2f(refresh_f2h(ws));
  const float base = lo ? refresh_h2f(refresh_f2h((ws - wh) * 2048.0f)) : wh;
  return refresh_f2h(hi ? base * 2048.0f : base);
}
struct M16Src { int idx, lo, hi; };      // idx < 0: the half is zero
// halves of a layer's fragment buffer in front of the tail's fragment (cin == 8: conv3_m16_frag_halves minus its last 256)
TFL_HD inline int m16_frag_halves(int cin) { return cin == 3 ? (9 * 64 + 1) * 8 + (7 * 64 + 1) * 8 : (9 * 2 * 64 + 1) * 8 + (14 * 64 + 1) * 8; }
constexpr int kM16TailHalves = 64 * 4;
// half d of that buffer -> its weight of the cudnn layer [8][cin][27]
TFL_HD inline M16Src m16_frag_src(int cin, int d) {
  const int RT = cin == 3 ? 1 : 2, M = 9 * RT * 64 * 8;
  M16Src s = {-1, 0, 0};
  if (d < M) {
    const int j = d & 7, lane = (d >> 3) & 63, r = (d >> 9) % RT, p = d / (512 * RT);
    const int m = lane & 15, g = lane >> 4, co = m >> 1;
    int ci = -1, act_hi = 1;
    if (g < 3) {
      if (cin == 8) { ci = j; act_hi = r == 0; }
      else if (j < 3) { ci = j; act_hi = 1; }
      else if (j < 5) { ci = j - 3; act_hi = 0; }
    }
    if (ci >= 0) { s.idx = ((co * cin + ci) * 9 + p) * 3 + g; s.lo = m & 1; s.hi = act_hi; }
    return s;
  }
  d -= M + 8;
  const int F = cin == 3 ? 7 : 14;
  if (d < 0 || d >= F * 512) return s;         // the two runs of 16 zero bytes
  const int j = d & 7, lane = (d >> 3) & 63, f = d >> 9;
  const int m = lane & 15, g = lane >> 4, co = m >> 1;
  int kind, dy, hi, ci;
  if (cin == 3) { kind = f < 3 ? 0 : (f < 6 ? 1 : 2); dy = kind == 2 ? 0 : f % 3; ci = j < 3 ? j : (j < 5 ? j - 3 : -1); hi = j < 3; }
  else { kind = f < 6 ? 0 : (f < 12 ? 1 : 2); dy = kind == 2 ? 0 : ((f % 6) >> 1); ci = j; hi = (f & 1) == 0; }
  int kz = -1, ky = 0, kx = 0;
  if (kind == 0) { kz = g == 3 ? 1 : 0; ky = dy; kx = g == 3 ? 0 : g; }
  else if (kind == 1) { kz = g < 2 ? 1 : 2; ky = dy; kx = g == 0 ? 1 : (g == 1 ? 2 : (g == 2 ? 0 : 1)); }
  else if (g < 3) { kz = 2; ky = g; kx = 2; }
  if (kz >= 0 && ci >= 0) { s.idx = (co * cin + ci) * 27 + kz * 9 + ky * 3 + kx; s.lo = m & 1; s.hi = hi; }
  return s;
}
// half d of the tail's 8 -> 8 (k = 1) fragment -> its weight of w4 [8][8]
TFL_HD inline M16Src m16_tail_src(int d) {
  const int lane = d >> 2, i = d & 3;
  const int m = lane & 15, g = lane >> 4, j = m >> 1, c = 2 * g + (i & 1);
  M16Src s = {j * 8 + c, m & 1, (i >> 1) == 0};
  return s;
}

// ---- the optimiser's flat parameter space: tensor 2 l = layer l's weight, 2 l + 1 = its bias, off[] their prefix offsets -----
constexpr int kOptimMaxTensors = 2 * kRefreshMaxLayers;
constexpr int kOptimNormBlocks = 64, kOptimThreads = 256;
// the reduce buffer of the data-parallel step: slot i = flat element i, slot total = the guard, then reserved slots (zeros)
constexpr int kOptimReduceTail = 8;
struct OptimPtrs { float* x[kOptimMaxTensors]; float* g[kOptimMaxTensors]; };
// the hyper-parameters of one step, by value: fp32 where the reference hands Torch a scalar for an fp32 tensor operation
// (1 - beta formed in double first), fp64 where it computes in Lua numbers. method 0 = Adam, 1 = RMSprop (b2 / omb2 = alpha / 1 - alpha)
struct OptimArgs { int method; float b1, omb1, b2, omb2, eps, wd; double lr, lrd, beta1, beta2, threshold; };
// the tensor that holds flat element i (off[0] = 0 < off[1] <= ... off[n] = total; empty tensors are skipped)
TFL_HD inline int optim_tensor_of(const long long* off, int n, long long i) {
  int t = 0;
  while (t + 1 < n && off[t + 1] <= i) t++;
  return t;
}
// the flat elements [lo, hi) of norm block b: equal chunks in index order
TFL_HD inline void optim_chunk(long long total, int nblocks, int b, long long* lo, long long* hi) {
  const long long chunk = (total + nblocks - 1) / nblocks;
  *lo = chunk * b < total ? chunk * b : total;
  *hi = *lo + chunk < total ? *lo + chunk : total;
}

}  // namespace tfl
