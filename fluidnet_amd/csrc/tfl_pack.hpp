// tfl_pack.hpp -- the host packers of the projection ConvNet's own weight forms: the split-fp16 A fragments of conv_mfma16.hip
// (conv3_m16_pack_weights / _pack_tail, with the integer float -> half conversion they round with) and the fp32 forms of the
// two default topologies (the MFMA B fragments, the Winograd transform, the tail pack). Plain C++ without a HIP call:
// model_build.cpp packs with them at creation and in tfl_model_set_weights, and a stand-alone host program holds the device
// refresh maps (tfl_refresh.hpp) to them byte for byte (tests/refresh_layout_host.cpp).
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

namespace tfl {

// float -> IEEE binary16 bits, round to nearest even (host side; finite inputs)
inline uint16_t f2h(float f) {
  uint32_t u; memcpy(&u, &f, 4);
  const uint32_t sign = (u >> 16) & 0x8000u;
  u &= 0x7fffffffu;
  if (u >= 0x47800000u) return (uint16_t)(sign | 0x7c00u);            // >= 65536 (callers stay below 65520)
  if (u < 0x38800000u) {                                              // below 2^-14: subnormal half
    if (u < 0x33000000u) return (uint16_t)sign;                       // below 2^-25
    const int e = (int)(u >> 23);                                     // biased exponent, 102..112
    const uint32_t m = (u & 0x7fffffu) | 0x800000u;
    const int shift = 126 - e;                                        // 14..24
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
inline float h2f(uint16_t h) {
  const uint32_t sign = (uint32_t)(h & 0x8000u) << 16;
  uint32_t e = (h >> 10) & 31, m = h & 0x3ffu;
  float v;
  if (e == 0) v = ldexpf((float)m, -24);
  else if (e == 31) v = INFINITY;
  else v = ldexpf((float)(m | 0x400u), (int)e - 25);
  uint32_t u; memcpy(&u, &v, 4); u |= sign; memcpy(&v, &u, 4);
  return v;
}

// out: conv3_m16_frag_halves(cin) halves: (9 * RT * 64 + 1) * 8 (RT = 1 for cin == 3, 2 for cin == 8; the last 16 bytes
// are zero: the source of the kernels' out-of-grid staging slots) and, for cin == 8, the K-packed fragments of
// k_conv3_m16p behind them ((14 * 64 + 1) * 8); returns the post-scale 2^-(11 + e)
inline size_t conv3_m16_frag_halves(int cin) {
  return cin == 3 ? ((size_t)9 * 64 + 1) * 8 + ((size_t)7 * 64 + 1) * 8
                  : ((size_t)9 * 2 * 64 + 1) * 8 + ((size_t)14 * 64 + 1) * 8 + (size_t)64 * 4;   // + the tail's 1 x 1 x 1 A fragment
}
// The A fragment of the tail's 8 -> 8 (k = 1) layer for v_mfma_f32_16x16x16_f16 (k_conv3_m16p<true, true>), written behind the
// K-packed fragments of a cin == 8 layer buffer: lane (m = lane & 15, g = lane >> 4) holds A[m][4g .. 4g + 3]; row m = 2 j + t
// = output channel j as {w_h, w_l} of w4[j][c] 2^e4; column 4g + i = input channel c = 2g + (i & 1), activation term i >> 1
// (0: the high halves, their weights pre-multiplied by 2^11). Returns the post-scale 2^-(11 + e4).
inline float conv3_m16_pack_tail(const float* w4, uint16_t* frag_buf) {
  float mx = 0.0f;
  for (int i = 0; i < 64; i++) mx = fmaxf(mx, fabsf(w4[i]));
  int e = 0;
  if (mx > 0.0f && std::isfinite(mx)) { int ex; (void)frexpf(mx, &ex); e = 4 - ex; }       // mx 2^e in [8, 16)
  uint16_t* o = frag_buf + ((size_t)9 * 2 * 64 + 1) * 8 + ((size_t)14 * 64 + 1) * 8;
  for (int lane = 0; lane < 64; lane++)
    for (int i = 0; i < 4; i++) {
      const int m = lane & 15, g = lane >> 4, j = m >> 1, wt = m & 1, c = 2 * g + (i & 1);
      const float ws = ldexpf(w4[j * 8 + c], e);
      const float wh = h2f(f2h(ws));
      const float base = wt ? h2f(f2h((ws - wh) * 2048.0f)) : wh;
      o[lane * 4 + i] = f2h((i >> 1) == 0 ? base * 2048.0f : base);
    }
  return ldexpf(1.0f, -(11 + e));
}
inline float conv3_m16_pack_weights(const float* w, int cin, uint16_t* out) {
  const int RT = cin == 3 ? 1 : 2;
  float mx = 0.0f;
  for (int i = 0; i < 8 * cin * 27; i++) mx = fmaxf(mx, fabsf(w[i]));
  int e = 0;
  if (mx > 0.0f && std::isfinite(mx)) { int ex; (void)frexpf(mx, &ex); e = 4 - ex; }       // mx 2^e in [8, 16)
  for (int p = 0; p < 9; p++)
    for (int r = 0; r < RT; r++)
      for (int lane = 0; lane < 64; lane++)
        for (int j = 0; j < 8; j++) {
          const int m = lane & 15, g = lane >> 4, co = m >> 1, wt = m & 1;
          int ci = -1; bool act_hi = true;
          if (g < 3) {
            if (cin == 8) { ci = j; act_hi = r == 0; }
            else if (j < 3) { ci = j; act_hi = true; }
            else if (j < 5) { ci = j - 3; act_hi = false; }
          }
          float v = 0.0f;
          if (ci >= 0) {
            const float ws = ldexpf(w[((size_t)(co * cin + ci) * 9 + p) * 3 + g], e);
            const float wh = h2f(f2h(ws));
            const float base = wt ? h2f(f2h((ws - wh) * 2048.0f)) : wh;
            v = act_hi ? base * 2048.0f : base;
          }
          out[(((size_t)p * RT + r) * 64 + lane) * 8 + j] = f2h(v);
        }
  for (int j = 0; j < 8; j++) out[(size_t)9 * RT * 64 * 8 + j] = 0;
  if (cin == 3) {
    // the K-packed fragments of k_conv3_m16p_in behind them: A(dy), B(dy), C (f = 0..6), + 16 zero bytes; K group g of a
    // fragment = one tap as below, its 8 elements = {p_h, d_h, occ, p_l, d_l, 0, 0, 0}
    uint16_t* o2 = out + ((size_t)9 * RT * 64 + 1) * 8;
    for (int f = 0; f < 7; f++)
      for (int lane = 0; lane < 64; lane++)
        for (int j = 0; j < 8; j++) {
          const int m = lane & 15, g = lane >> 4, co = m >> 1, wt = m & 1;
          const int kind = f < 3 ? 0 : (f < 6 ? 1 : 2), dy = kind == 2 ? 0 : f % 3;
          int kz = -1, ky = 0, kx = 0;
          if (kind == 0) { kz = g == 3 ? 1 : 0; ky = dy; kx = g == 3 ? 0 : g; }
          else if (kind == 1) { kz = g < 2 ? 1 : 2; ky = dy; kx = g == 0 ? 1 : (g == 1 ? 2 : (g == 2 ? 0 : 1)); }
          else if (g < 3) { kz = 2; ky = g; kx = 2; }
          const int ci = j < 3 ? j : (j < 5 ? j - 3 : -1);
          const bool act_hi = j < 3;
          float v = 0.0f;
          if (kz >= 0 && ci >= 0) {
            const float ws = ldexpf(w[(size_t)(co * cin + ci) * 27 + kz * 9 + ky * 3 + kx], e);
            const float wh = h2f(f2h(ws));
            const float base = wt ? h2f(f2h((ws - wh) * 2048.0f)) : wh;
            v = act_hi ? base * 2048.0f : base;
          }
          o2[((size_t)f * 64 + lane) * 8 + j] = f2h(v);
        }
    for (int j = 0; j < 8; j++) o2[(size_t)7 * 64 * 8 + j] = 0;
  }
  if (cin == 8) {
    // the K-packed fragments of k_conv3_m16p behind them: A(dy) x term, B(dy) x term, C x term (f = 0..13), + 16 zero bytes.
    // K group g of a fragment = one tap (kz, ky, kx) or none:
    //   A(dy): (0, dy, 0) (0, dy, 1) (0, dy, 2) (1, dy, 0)    B(dy): (1, dy, 1) (1, dy, 2) (2, dy, 0) (2, dy, 1)
    //   C:     (2, 0, 2) (2, 1, 2) (2, 2, 2) -
    uint16_t* o2 = out + ((size_t)9 * RT * 64 + 1) * 8;
    for (int f = 0; f < 14; f++)
      for (int lane = 0; lane < 64; lane++)
        for (int j = 0; j < 8; j++) {
          const int m = lane & 15, g = lane >> 4, co = m >> 1, wt = m & 1;
          const int kind = f < 6 ? 0 : (f < 12 ? 1 : 2), dy = kind == 2 ? 0 : ((f % 6) >> 1), tm = f & 1;
          int kz = -1, ky = 0, kx = 0;
          if (kind == 0) { kz = g == 3 ? 1 : 0; ky = dy; kx = g == 3 ? 0 : g; }
          else if (kind == 1) { kz = g < 2 ? 1 : 2; ky = dy; kx = g == 0 ? 1 : (g == 1 ? 2 : (g == 2 ? 0 : 1)); }
          else if (g < 3) { kz = 2; ky = g; kx = 2; }
          float v = 0.0f;
          if (kz >= 0) {
            const float ws = ldexpf(w[(size_t)(co * cin + j) * 27 + kz * 9 + ky * 3 + kx], e);
            const float wh = h2f(f2h(ws));
            const float base = wt ? h2f(f2h((ws - wh) * 2048.0f)) : wh;
            v = tm == 0 ? base * 2048.0f : base;       // term 0 multiplies the activations' high halves
          }
          o2[((size_t)f * 64 + lane) * 8 + j] = f2h(v);
        }
    for (int j = 0; j < 8; j++) o2[(size_t)14 * 64 * 8 + j] = 0;
  }
  return ldexpf(1.0f, -(11 + e));
}

// ---- the fp32 forms of the two default topologies (model_build.cpp pack_default3 / pack_default2 upload them) --------------
// 3-D default, one k = 3 layer: the per-lane B fragments of conv_mfma.hip, [c][kz][ky][64 lanes]
inline void pack_bfrag3(const float* w, int ci_n, std::vector<float>& frag) {
  frag.assign((size_t)ci_n * 9 * 64, 0.0f);
  for (int c = 0; c < ci_n; c++)
    for (int kz = 0; kz < 3; kz++)
      for (int ky = 0; ky < 3; ky++)
        for (int lane = 0; lane < 64; lane++) {
          const int k = lane >> 4, n = lane & 15, ph = n >> 3, co = n & 7, kx = k - ph;
          float v = 0.0f;
          if (kx >= 0 && kx <= 2) v = w[((((size_t)co * ci_n + c) * 3 + kz) * 3 + ky) * 3 + kx];
          frag[(((size_t)c * 3 + kz) * 3 + ky) * 64 + lane] = v;
        }
}
// 3-D default: {bias3[8], w4[8][8], b4[8], w5[8], b5[1], post4} in one buffer (conv_valu.hip, conv_mfma16.hip kTail*)
constexpr int kTailPackFloats = 8 + 64 + 8 + 8 + 1 + 1;
inline void pack_tail3(const float* const* weights, const float* const* biases, float post16_tail, std::vector<float>& tp) {
  tp.assign(kTailPackFloats, 0.0f);
  for (int i = 0; i < 8; i++) tp[i] = biases[2][i];
  for (int i = 0; i < 64; i++) tp[8 + i] = weights[3][i];
  for (int i = 0; i < 8; i++) { tp[72 + i] = biases[3][i]; tp[80 + i] = weights[4][i]; }
  tp[88] = biases[4][0];
  tp[89] = post16_tail;        // conv_mfma16.hip kTailPost4 (0 on the fp32 paths, which do not read it)
}
// 3-D default, one k = 3 layer, Winograd-transformed along x: U = (g0, (g0 + g1 + g2)/2, (g0 - g1 + g2)/2, g2) over the three
// x-taps of every (dz, dy, c_in, c_out), [dz dy][cin][4][8]
inline void pack_wino3(const float* w, int ci_n, std::vector<float>& u) {
  u.assign((size_t)9 * 4 * ci_n * 8, 0.0f);
  for (int co = 0; co < 8; co++)
    for (int c = 0; c < ci_n; c++)
      for (int zy = 0; zy < 9; zy++) {
        const float* g = w + (((size_t)co * ci_n + c) * 9 + zy) * 3;
        const float uu[4] = {g[0], 0.5f * ((g[0] + g[2]) + g[1]), 0.5f * ((g[0] + g[2]) - g[1]), g[2]};
        for (int p = 0; p < 4; p++) u[(((size_t)zy * ci_n + c) * 4 + p) * 8 + co] = uu[p];
      }
}
// 2-D default, one k = 3 layer: B[k][n] of MFMA (tap, c4): lane = k*16 + n holds w[n][4*c4 + k][dy][dx] (0 for padded channels)
inline void pack_bfrag2(const float* w, int ci_n, std::vector<float>& frag) {
  const int c4n = (ci_n + 3) / 4;
  frag.assign((size_t)9 * c4n * 64, 0.0f);
  for (int tap = 0; tap < 9; tap++)
    for (int c4 = 0; c4 < c4n; c4++)
      for (int lane = 0; lane < 64; lane++) {
        const int k = lane >> 4, n = lane & 15, c = 4 * c4 + k;
        frag[((size_t)tap * c4n + c4) * 64 + lane] = c < ci_n ? w[((size_t)n * ci_n + c) * 9 + tap] : 0.0f;
      }
}

}  // namespace tfl
