// conv.hip -- convolution layers of the projection ConvNet (gfx950).
//
// Replaces cudnn.SpatialConvolution / cudnn.VolumetricConvolution forward as used by
// torch/lib/model_utils.lua:80-116: stride 1, zero padding (k-1)/2, cross-correlation, bias, with the
// following nn.ReLU fused into the epilogue. Activations are channel-planar fp32 [B][C][Z][Y][X].
//
// k_conv_direct is the shape-generic path (any C_in, k; C_out in {1, 2, 4, 8, 16, 32, 64}): one thread
// per voxel holding all C_out accumulators in registers; the weights are re-laid out on the host as
// [tap][c_in][c_out] so every weight address is wave-uniform and travels through the scalar cache
// (s_load), leaving the vector memory path to the activations. The fmaf chain is exact fp32.
//
// The `tog` topologies (lib/model.lua:163-178, 211-218) add two things, both here: 2x average pooling after a layer
// (cudnn.{Spatial,Volumetric}AveragePooling(2,..,2), model_utils.lua:184-208) = k_avg_pool2, and
// nn.{Spatial,Volumetric}ConvolutionUpsample (lib/modules/spatial_convolution_upsample.lua:24-93,
// volumetric_convolution_upsample.lua): a convolution to up^dim * C_out channels whose result is pixel-shuffled,
// out[b][o][z*u+a][y*u+b][x*u+c] = conv[b][((o*u + a)*u + b)*u + c][z][y][x]. The shuffle costs nothing here: the conv
// is launched once per sub-position (a, b, c) with that sub-position's weight slice and a strided store (ConvUp).
//
// The model-graph form (tfl_model_create_graph: banks, dilation, batch norm, max pooling) has kernels of
// its own -- k_conv_direct_ex, k_pool2_ex, k_bank_join -- so k_conv_direct and k_avg_pool2 compile exactly as before.
// A z-slab rank launches k_conv_direct and k_avg_pool2 on the planes of each layer's cone only: the grid covers
// the window's planes, every voxel computes what it computes on the whole grid.
#include "tfl_device.hpp"
#include "tfl_host.hpp"

namespace tfl {

struct ConvUp {      // output placement: voxel (i, j, k) of the conv grid goes to (i*u + a, j*u + b, k*uz + c) of `dout`
  int u, uz, a, b, c;
  int oX, oY, oZ;    // size of the output grid
  int act;           // epilogue: 0 none, 1 ReLU, 2 ReLU6, 3 sigmoid (model_utils.lua:20-34)
  int och;           // channel planes per batch item of `out` (>= COUT: room for a joined skip channel)
};
__device__ __forceinline__ float conv_act(float v, int act) {
  if (act == 1) return fmaxf(v, 0.0f);
  if (act == 2) return fminf(fmaxf(v, 0.0f), 6.0f);
  if (act == 3) return 1.0f / (1.0f + expf(-v));     // nn.Sigmoid (THNN: 1 / (1 + exp(-x)))
  return v;
}

// Options of the model-graph form (tfl_model_create_graph) that the plain instantiations do not carry:
// a dilated conv (banksType 'dilate', model_utils.lua:122-146: taps d apart, zero padding d*(k-1)/2), an output channel
// offset into a wider buffer (a bank writes its slice of a 'concat' join directly) and the inference-form batch norm
// after the activation (model_utils.lua:36-60), folded on the host to y = fmaf(x, bn_s[c], bn_t[c]).
struct ConvEx {
  int dil;                     // tap spacing (1 = plain)
  int c0;                      // first channel plane of `out` this launch writes
  const float* bn_s;           // per-channel BN scale / shift (device), or null
  const float* bn_t;
};

// CPT = output channels per thread: COUT for large grids (each activation is loaded once), COUT/4 for small
// ones where the grid would otherwise leave most CUs idle (2-D 128^2 = 64 blocks of 256 threads).
template <bool IS3D, int COUT, int CPT>
__global__ __launch_bounds__(256) void k_conv_direct(Dom d, int cin, int ksz, const float* __restrict__ in,
                                                     const float* __restrict__ w, const float* __restrict__ bias,
                                                     float* __restrict__ out, ConvUp up) {
  constexpr int G = COUT / CPT;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const int j = blockIdx.y * blockDim.y + threadIdx.y;
  const int zg = blockIdx.z / G, co0 = (blockIdx.z - zg * G) * CPT;
  const int b = zg / d.nw, k = d.w0 + (zg - b * d.nw);        // planes [w0, w0 + nw) of the conv grid
  if (i >= d.X || j >= d.Y) return;
  const long long cells = d.sc;
  const long long ocells = (long long)up.oX * up.oY * up.oZ;
  in += b * cells * cin; out += b * ocells * up.och;
  float acc[CPT];
#pragma unroll
  for (int c = 0; c < CPT; c++) acc[c] = bias[co0 + c];
  const int r = (ksz - 1) / 2;
  const int rz = IS3D ? r : 0;
  int tap = 0;
  for (int dz = -rz; dz <= rz; dz++) {
    for (int dy = -r; dy <= r; dy++) {
      for (int dx = -r; dx <= r; dx++, tap++) {
        const int x = i + dx, y = j + dy, z = k + dz;
        const bool ok = x >= 0 && x < d.X && y >= 0 && y < d.Y && z >= 0 && z < d.Z;
        const int o = ok ? TFL_AT(d, x, y, z) : 0;
        const float* wt = w + (long long)tap * cin * COUT;
        // 8 independent activation loads in flight per batch (a one-load-one-fma loop is a chain of
        // L1 latencies: 144 taps x ~200 cycles made the 2-D 16-channel layers 27 us at 128^2)
        int c = 0;
        for (; c + 8 <= cin; c += 8) {
          float v[8];
#pragma unroll
          for (int q = 0; q < 8; q++) v[q] = ok ? in[o + (c + q) * d.sc] : 0.0f;
#pragma unroll
          for (int q = 0; q < 8; q++)
#pragma unroll
            for (int co = 0; co < CPT; co++) acc[co] = fmaf(v[q], wt[(c + q) * COUT + co0 + co], acc[co]);
        }
        for (; c < cin; c++) {
          const float v = ok ? in[o + c * d.sc] : 0.0f;
#pragma unroll
          for (int co = 0; co < CPT; co++) acc[co] = fmaf(v, wt[c * COUT + co0 + co], acc[co]);
        }
      }
    }
  }
  const long long o = (i * up.u + up.a) + (long long)up.oX * ((j * up.u + up.b) + (long long)up.oY * (k * up.uz + up.c));
#pragma unroll
  for (int c = 0; c < CPT; c++) out[o + (co0 + c) * ocells] = conv_act(acc[c], up.act);
}

// The model-graph form of k_conv_direct (its own kernel: the plain instantiations above compile exactly as before).
// Differs in the tap spacing ex.dil, the channel offset ex.c0 of the output and the batch-norm epilogue; otherwise the
// same loop and the same fmaf order.
template <bool IS3D, int COUT, int CPT>
__global__ __launch_bounds__(256) void k_conv_direct_ex(Dom d, int cin, int ksz, const float* __restrict__ in,
                                                        const float* __restrict__ w, const float* __restrict__ bias,
                                                        float* __restrict__ out, ConvUp up, ConvEx ex) {
  constexpr int G = COUT / CPT;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const int j = blockIdx.y * blockDim.y + threadIdx.y;
  const int zg = blockIdx.z / G, co0 = (blockIdx.z - zg * G) * CPT;
  const int b = zg / d.Z, k = zg - b * d.Z;
  if (i >= d.X || j >= d.Y) return;
  const long long cells = d.sc;
  const long long ocells = (long long)up.oX * up.oY * up.oZ;
  in += b * cells * cin; out += (b * (long long)up.och + ex.c0) * ocells;
  float acc[CPT];
#pragma unroll
  for (int c = 0; c < CPT; c++) acc[c] = bias[co0 + c];
  const int r = (ksz - 1) / 2;
  const int rz = IS3D ? r : 0;
  const int dil = ex.dil;
  int tap = 0;
  for (int dz = -rz; dz <= rz; dz++) {
    for (int dy = -r; dy <= r; dy++) {
      for (int dx = -r; dx <= r; dx++, tap++) {
        const int x = i + dx * dil, y = j + dy * dil, z = k + dz * dil;
        const bool ok = x >= 0 && x < d.X && y >= 0 && y < d.Y && z >= 0 && z < d.Z;
        const int o = ok ? TFL_AT(d, x, y, z) : 0;
        const float* wt = w + (long long)tap * cin * COUT;
        int c = 0;
        for (; c + 8 <= cin; c += 8) {
          float v[8];
#pragma unroll
          for (int q = 0; q < 8; q++) v[q] = ok ? in[o + (c + q) * d.sc] : 0.0f;
#pragma unroll
          for (int q = 0; q < 8; q++)
#pragma unroll
            for (int co = 0; co < CPT; co++) acc[co] = fmaf(v[q], wt[(c + q) * COUT + co0 + co], acc[co]);
        }
        for (; c < cin; c++) {
          const float v = ok ? in[o + c * d.sc] : 0.0f;
#pragma unroll
          for (int co = 0; co < CPT; co++) acc[co] = fmaf(v, wt[c * COUT + co0 + co], acc[co]);
        }
      }
    }
  }
  const long long o = (i * up.u + up.a) + (long long)up.oX * ((j * up.u + up.b) + (long long)up.oY * (k * up.uz + up.c));
#pragma unroll
  for (int c = 0; c < CPT; c++) {
    const float v = conv_act(acc[c], up.act);
    out[o + (co0 + c) * ocells] = ex.bn_s ? fmaf(v, ex.bn_s[co0 + c], ex.bn_t[co0 + c]) : v;
  }
}

// cudnn average pooling, window = stride = 2, no padding: out size floor(n / 2) per pooled axis (z only in 3-D)
// (output planes [k0, k0 + nk) only: a z-slab rank pools the planes of its cone)
template <bool IS3D>
__global__ __launch_bounds__(256) void k_avg_pool2(int rows, int Zo, int Yo, int Xo, int Z, int Y, int X, int k0, int nk,
                                                   const float* __restrict__ in, float* __restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const int j = blockIdx.y * blockDim.y + threadIdx.y;
  const int r = blockIdx.z / nk, k = k0 + (blockIdx.z - r * nk);      // r = b*C + c
  if (i >= Xo || j >= Yo) return;
  const float* p = in + ((long long)r * Z + (IS3D ? 2 * k : 0)) * Y * X + (long long)(2 * j) * X + 2 * i;
  float s = (p[0] + p[1]) + (p[X] + p[X + 1]);
  if (IS3D) {
    const float* q = p + (long long)Y * X;
    s += (q[0] + q[1]) + (q[X] + q[X + 1]);
  }
  out[((long long)r * Zo + k) * Yo * Xo + (long long)j * Xo + i] = s * (IS3D ? 0.125f : 0.25f);
}

// 2x pooling (window = stride = 2) of the model-graph form: average (cudnn / nn *AveragePooling(2)) or max
// (cudnn *MaxPooling(2)), with the stage's batch norm (if any) applied on the way out, and the result placed at channel
// planes [c0, c0 + C) of an `och`-plane output (a bank writing its slice of a 'concat' join).
template <bool IS3D, bool MAX>
__global__ __launch_bounds__(256) void k_pool2_ex(int C, int Zo, int Yo, int Xo, int Z, int Y, int X, const float* __restrict__ in,
                                                  float* __restrict__ out, int och, int c0, const float* __restrict__ bn_s,
                                                  const float* __restrict__ bn_t) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const int j = blockIdx.y * blockDim.y + threadIdx.y;
  const int r = blockIdx.z / Zo, k = blockIdx.z - r * Zo;      // r = b*C + c
  if (i >= Xo || j >= Yo) return;
  const int b = r / C, c = r - b * C;
  const float* p = in + ((long long)r * Z + (IS3D ? 2 * k : 0)) * Y * X + (long long)(2 * j) * X + 2 * i;
  float s;
  if (MAX) {
    s = fmaxf(fmaxf(p[0], p[1]), fmaxf(p[X], p[X + 1]));
    if (IS3D) {
      const float* q = p + (long long)Y * X;
      s = fmaxf(s, fmaxf(fmaxf(q[0], q[1]), fmaxf(q[X], q[X + 1])));
    }
  } else {
    s = (p[0] + p[1]) + (p[X] + p[X + 1]);
    if (IS3D) {
      const float* q = p + (long long)Y * X;
      s += (q[0] + q[1]) + (q[X] + q[X + 1]);
    }
    s *= IS3D ? 0.125f : 0.25f;
  }
  if (bn_s) s = fmaf(s, bn_s[c], bn_t[c]);
  out[(((long long)b * och + c0 + c) * Zo + k) * Yo * Xo + (long long)j * Xo + i] = s;
}

// The join of the banks (model.lua:285-314) in one launch, at bank 1's resolution [Z][Y][X] with C channels per bank.
// Bank i > 1 is read nearest-upsampled by sh[i] = 2^(i-1) (mres; 0 = same resolution: dilate), i.e. at (x >> s, ...).
//  concat (ADD = false): out[b][(i-1)*C + c] = up(bank i)[b][c] for the banks listed (bank 1 and full-resolution banks wrote
//                        their slices themselves); `och` = C * banksNum
//  add (ADD = true):     out[b][c] = ((out + up(b2)) + up(b3)) ... in nn.CAddTable's order, out holding bank 1
struct JoinSrc {
  int n;                       // banks read by this launch
  int slot[kMaxJoinBanks];     // their bank index - 1 (the channel slice for concat)
  int sh[kMaxJoinBanks];       // log2 of their upsampling ratio
  const float* src[kMaxJoinBanks];
};
template <bool IS3D, bool ADD>
__global__ __launch_bounds__(256) void k_bank_join(int C, int Z, int Y, int X, JoinSrc js, float* __restrict__ out, int och) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const int j = blockIdx.y * blockDim.y + threadIdx.y;
  const int r = blockIdx.z / Z, k = blockIdx.z - r * Z;        // r = b*C + c
  if (i >= X || j >= Y) return;
  const int b = r / C, c = r - b * C;
  const long long v = ((long long)k * Y + j) * X + i;
  const long long cells = (long long)Z * Y * X;
  if (ADD) {
    float* o = out + ((long long)b * och + c) * cells + v;
    float s = *o;
    for (int q = 0; q < js.n; q++) {
      const int sh = js.sh[q], Zs = IS3D ? Z >> sh : Z, Ys = Y >> sh, Xs = X >> sh;
      s += js.src[q][(((long long)b * C + c) * Zs + (IS3D ? k >> sh : k)) * Ys * Xs + (long long)(j >> sh) * Xs + (i >> sh)];
    }
    *o = s;
  } else {
    for (int q = 0; q < js.n; q++) {
      const int sh = js.sh[q], Zs = IS3D ? Z >> sh : Z, Ys = Y >> sh, Xs = X >> sh;
      out[((long long)b * och + js.slot[q] * C + c) * cells + v] =
          js.src[q][(((long long)b * C + c) * Zs + (IS3D ? k >> sh : k)) * Ys * Xs + (long long)(j >> sh) * Xs + (i >> sh)];
    }
  }
}

template <bool IS3D, int COUT, bool EX>
static void launch_direct(hipStream_t st, const Dom& d, int B, int cin, int ksz, const float* in,
                          const float* w, const float* bias, float* out, const ConvUp& up, const ConvEx& ex) {
  const dim3 blk(64, 4, 1);
  const unsigned nxy = ((d.X + 63) / 64) * ((d.Y + 3) / 4);
  constexpr int CPT_SMALL = COUT >= 4 ? COUT / 4 : COUT;
  const bool split = COUT >= 4 && (long long)nxy * d.Z * B < 1024;   // fewer than ~4 blocks per CU: split channels
  if (EX) {
    TFL_TIMED("k_conv_direct_ex", st);
    if (split) {
      const dim3 grd((d.X + 63) / 64, (d.Y + 3) / 4, (unsigned)(d.Z * B * (COUT / CPT_SMALL)));
      k_conv_direct_ex<IS3D, COUT, CPT_SMALL><<<grd, blk, 0, st>>>(d, cin, ksz, in, w, bias, out, up, ex);
    } else {
      const dim3 grd((d.X + 63) / 64, (d.Y + 3) / 4, (unsigned)(d.Z * B));
      k_conv_direct_ex<IS3D, COUT, COUT><<<grd, blk, 0, st>>>(d, cin, ksz, in, w, bias, out, up, ex);
    }
    return;
  }
  TFL_TIMED("k_conv_direct", st);
  const bool split_w = COUT >= 4 && (long long)nxy * d.nw * B < 1024;      // (the plain kernel covers the window's planes)
  if (split_w) {
    const dim3 grd((d.X + 63) / 64, (d.Y + 3) / 4, (unsigned)(d.nw * B * (COUT / CPT_SMALL)));
    k_conv_direct<IS3D, COUT, CPT_SMALL><<<grd, blk, 0, st>>>(d, cin, ksz, in, w, bias, out, up);
  } else {
    const dim3 grd((d.X + 63) / 64, (d.Y + 3) / 4, (unsigned)(d.nw * B));
    k_conv_direct<IS3D, COUT, COUT><<<grd, blk, 0, st>>>(d, cin, ksz, in, w, bias, out, up);
  }
}

static bool conv_direct_any(hipStream_t st, bool is3d, int B, int Z, int Y, int X, int cin, int cout, int ksz, int act,
                            const float* in, const float* w, const float* bias, float* out, int upf, int sub, int out_ch,
                            const ConvEx* ex, int z0 = 0, int nz = -1) {
  Dom d = whole_dom(Z, Y, X);
  // the shape-generic path covers the planes it is given and takes no scope: the whole grid, or (z-slab rank) the
  // planes [z0, z0 + nz) of this layer's cone (the model-graph form: always the whole grid)
  if (ex || nz < 0) { z0 = 0; nz = Z; }
  d.w0 = z0; d.n0 = nz; d.w1 = 0; d.nw = nz;
  if (nz == 0) return true;
  ConvUp up;
  up.u = upf; up.uz = is3d ? upf : 1;
  up.a = sub % upf; up.b = (sub / upf) % upf; up.c = is3d ? sub / (upf * upf) : 0;
  up.oX = X * up.u; up.oY = Y * up.u; up.oZ = Z * up.uz;
  up.act = act; up.och = out_ch > 0 ? out_ch : cout;
  const ConvEx plain{1, 0, nullptr, nullptr};
#define TFL_CASE(N)                                                                                                   \
  case N:                                                                                                             \
    if (ex) {                                                                                                         \
      if (is3d) launch_direct<true, N, true>(st, d, B, cin, ksz, in, w, bias, out, up, *ex);                         \
      else launch_direct<false, N, true>(st, d, B, cin, ksz, in, w, bias, out, up, *ex);                             \
    } else {                                                                                                          \
      if (is3d) launch_direct<true, N, false>(st, d, B, cin, ksz, in, w, bias, out, up, plain);                      \
      else launch_direct<false, N, false>(st, d, B, cin, ksz, in, w, bias, out, up, plain);                          \
    }                                                                                                                 \
    return true;
  switch (cout) {
    TFL_CASE(1) TFL_CASE(2) TFL_CASE(4) TFL_CASE(8) TFL_CASE(16) TFL_CASE(32) TFL_CASE(64)
    default: return false;
  }
#undef TFL_CASE
}

// w: device, [tap][cin][cout]. act: 0 none | 1 ReLU | 2 ReLU6 | 3 sigmoid. out_ch: channel planes per batch item of
// `out` (0 = cout). Returns false when cout has no instantiation.
bool conv_direct(hipStream_t st, bool is3d, int B, int Z, int Y, int X, int cin, int cout, int ksz, int act,
                 const float* in, const float* w, const float* bias, float* out, int upf, int sub, int out_ch, int z0, int nz) {
  if (nz >= 0 && (z0 < 0 || z0 + nz > Z)) return false;
  return conv_direct_any(st, is3d, B, Z, Y, X, cin, cout, ksz, act, in, w, bias, out, upf, sub, out_ch, nullptr, z0, nz);
}

bool conv_direct_graph(hipStream_t st, bool is3d, int B, int Z, int Y, int X, int cin, int cout, int ksz, int act,
                       const float* in, const float* w, const float* bias, float* out, int upf, int sub, int out_ch, int c0,
                       int dil, const float* bn_s, const float* bn_t) {
  const ConvEx ex{dil, c0, bn_s, bn_t};
  return conv_direct_any(st, is3d, B, Z, Y, X, cin, cout, ksz, act, in, w, bias, out, upf, sub, out_ch, &ex);
}

void pool2_graph(hipStream_t st, bool is3d, bool max, int B, int C, int Z, int Y, int X, const float* in, float* out, int och,
                 int c0, const float* bn_s, const float* bn_t) {
  const int Zo = is3d ? Z / 2 : Z, Yo = Y / 2, Xo = X / 2;
  const dim3 blk(64, 4, 1), grd((Xo + 63) / 64, (Yo + 3) / 4, (unsigned)(B * C * Zo));
  TFL_TIMED("k_pool2_ex", st);
  if (is3d) {
    if (max) k_pool2_ex<true, true><<<grd, blk, 0, st>>>(C, Zo, Yo, Xo, Z, Y, X, in, out, och, c0, bn_s, bn_t);
    else k_pool2_ex<true, false><<<grd, blk, 0, st>>>(C, Zo, Yo, Xo, Z, Y, X, in, out, och, c0, bn_s, bn_t);
  } else {
    if (max) k_pool2_ex<false, true><<<grd, blk, 0, st>>>(C, Zo, Yo, Xo, Z, Y, X, in, out, och, c0, bn_s, bn_t);
    else k_pool2_ex<false, false><<<grd, blk, 0, st>>>(C, Zo, Yo, Xo, Z, Y, X, in, out, och, c0, bn_s, bn_t);
  }
}

bool bank_join(hipStream_t st, bool is3d, bool add, int B, int C, int Z, int Y, int X, int n, const int* slot, const int* sh,
               const float* const* src, float* out, int och) {
  if (n < 1 || n > kMaxJoinBanks) return false;
  JoinSrc js;
  js.n = n;
  for (int q = 0; q < n; q++) { js.slot[q] = slot[q]; js.sh[q] = sh[q]; js.src[q] = src[q]; }
  const dim3 blk(64, 4, 1), grd((X + 63) / 64, (Y + 3) / 4, (unsigned)(B * C * Z));
  TFL_TIMED("k_bank_join", st);
  if (is3d) {
    if (add) k_bank_join<true, true><<<grd, blk, 0, st>>>(C, Z, Y, X, js, out, och);
    else k_bank_join<true, false><<<grd, blk, 0, st>>>(C, Z, Y, X, js, out, och);
  } else {
    if (add) k_bank_join<false, true><<<grd, blk, 0, st>>>(C, Z, Y, X, js, out, och);
    else k_bank_join<false, false><<<grd, blk, 0, st>>>(C, Z, Y, X, js, out, och);
  }
  return true;
}

void avg_pool2(hipStream_t st, bool is3d, int rows, int Z, int Y, int X, const float* in, float* out, int k0, int nk) {
  const int Zo = is3d ? Z / 2 : Z, Yo = Y / 2, Xo = X / 2;
  if (nk < 0 || k0 < 0 || k0 + nk > Zo) { k0 = 0; nk = Zo; }
  if (nk == 0) return;
  const dim3 blk(64, 4, 1), grd((Xo + 63) / 64, (Yo + 3) / 4, (unsigned)(rows * nk));
  TFL_TIMED("k_avg_pool2", st);
  if (is3d) k_avg_pool2<true><<<grd, blk, 0, st>>>(rows, Zo, Yo, Xo, Z, Y, X, k0, nk, in, out);
  else k_avg_pool2<false><<<grd, blk, 0, st>>>(rows, Zo, Yo, Xo, Z, Y, X, k0, nk, in, out);
}

}  // namespace tfl
