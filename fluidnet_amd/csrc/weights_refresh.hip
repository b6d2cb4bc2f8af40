// weights_refresh.hip -- tfl_model_set_weights_device: every weight form a model holds, rebuilt on the device from the caller's
// cudnn-layout device arrays. At these sizes (7-10 k parameters for the default nets) every launch sits at the launch floor,
// so the launch count is the cost: ONE gather launch covers w / b / wt / ws of all layers (blockIdx.y = layer, the per-model table
// of tfl_refresh.hpp RefreshLayer), ONE covers the fp32 forms of the default topologies (blockIdx.y = packed buffer), ONE
// the split-fp16 fragments (a block per layer: max |w| in LDS, then the pack). Gathers: a thread owns a destination element and
// asks tfl_refresh.hpp for its source, so padded elements are rewritten as zeros and nothing is written twice.
#include <hip/hip_runtime.h>

#include "tfl_host.hpp"
#include "tfl_refresh.hpp"

namespace tfl {
namespace {
constexpr int kRefreshThreads = 256;

__global__ __launch_bounds__(kRefreshThreads) void k_refresh_layers(RefreshSrc src, const RefreshLayer* __restrict__ table) {
  const RefreshLayer L = table[blockIdx.y];
  const float* __restrict__ w = src.w[blockIdx.y];
  const float* __restrict__ b = src.b[blockIdx.y];
  const int n = L.n_w + L.n_b + L.n_wt + L.n_ws;
  for (int d = blockIdx.x * kRefreshThreads + threadIdx.x; d < n; d += gridDim.x * kRefreshThreads) {
    if (d < L.n_w) {
      const long long s = refresh_w_src(L, d);
      L.w[d] = s >= 0 ? w[s] : 0.0f;
    } else if (d < L.n_w + L.n_b) {
      const int e = d - L.n_w, s = refresh_b_src(L, e);
      L.b[e] = s >= 0 ? b[s] : 0.0f;
    } else if (d < L.n_w + L.n_b + L.n_wt) {
      const int e = d - L.n_w - L.n_b;
      const long long s = refresh_wt_src(L, e);
      L.wt[e] = s >= 0 ? w[s] : 0.0f;
    } else {
      const int e = d - L.n_w - L.n_b - L.n_wt;
      L.ws[e] = w[refresh_ws_src(L, e)];
    }
  }
}

__global__ __launch_bounds__(kRefreshThreads) void k_refresh_pack(RefreshSrc src, const PackJob* __restrict__ jobs) {
  const PackJob J = jobs[blockIdx.y];
  const float* __restrict__ w = src.w[J.layer];
  for (int d = blockIdx.x * kRefreshThreads + threadIdx.x; d < J.n; d += gridDim.x * kRefreshThreads) {
    float v = 0.0f;
    if (J.kind == kPackBfrag3) { const int s = pack_bfrag3_src(J.ci_n, d); if (s >= 0) v = w[s]; }
    else if (J.kind == kPackBfrag2) { const int s = pack_bfrag2_src(J.ci_n, d); if (s >= 0) v = w[s]; }
    else if (J.kind == kPackWino3) { int p; const int s = pack_wino3_src(J.ci_n, d, &p); v = pack_wino3_val(w + s, p); }
    else if (J.kind == kPackCopy) v = w[d];
    else {      // kPackTail3 (J.n = 89 where the fp16 launch writes the post-scale behind them, else 90: a zero)
      if (d < 89) { int l, bias, i; pack_tail3_src(d, &l, &bias, &i); v = bias ? src.b[l][i] : src.w[l][i]; }
    }
    J.dst[d] = v;
  }
}

// max |w| over n floats, by the whole block (fmaxf: a NaN never wins, as on the host); every thread gets it
__device__ float block_absmax(const float* __restrict__ w, int n, float* red) {
  float mx = 0.0f;
  for (int i = threadIdx.x; i < n; i += kRefreshThreads) mx = fmaxf(mx, fabsf(w[i]));
  red[threadIdx.x] = mx;
  __syncthreads();
  for (int s = kRefreshThreads / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) red[threadIdx.x] = fmaxf(red[threadIdx.x], red[threadIdx.x + s]);
    __syncthreads();
  }
  mx = red[0];
  __syncthreads();
  return mx;
}

struct Pack16Args { uint16_t* frag[3]; float* post; float* tail_pack; };
// block l: layer l's A fragments with the layer's own exponent; block 2 also packs the tail's 8 -> 8 (k = 1) layer behind them.
// post[0..2] = the layers' post-scales, post[3] = the tail's (also tail_pack[89], where the kernels read it).
__global__ __launch_bounds__(kRefreshThreads) void k_refresh_pack16(RefreshSrc src, Pack16Args a) {
  __shared__ float red[kRefreshThreads];
  const int l = blockIdx.x, cin = l == 0 ? 3 : 8;
  const float* __restrict__ w = src.w[l];
  const int e = m16_exp(block_absmax(w, 8 * cin * 27, red));
  uint16_t* out = a.frag[l];
  const int n = m16_frag_halves(cin);
  for (int d = threadIdx.x; d < n; d += kRefreshThreads) {
    const M16Src s = m16_frag_src(cin, d);
    out[d] = s.idx >= 0 ? m16_half(w[s.idx], e, s.lo, s.hi) : (uint16_t)0;
  }
  if (threadIdx.x == 0) a.post[l] = m16_post(e);
  if (l != 2) return;
  const float* __restrict__ w4 = src.w[3];
  const int e4 = m16_exp(block_absmax(w4, 64, red));
  for (int d = threadIdx.x; d < kM16TailHalves; d += kRefreshThreads) {
    const M16Src s = m16_tail_src(d);
    out[n + d] = m16_half(w4[s.idx], e4, s.lo, s.hi);
  }
  if (threadIdx.x == 0) { a.post[3] = m16_post(e4); a.tail_pack[89] = m16_post(e4); }
}
}  // namespace

void refresh_layers(hipStream_t st, const RefreshSrc& src, const RefreshLayer* d_table, int nlayers, int max_elems) {
  int gx = (max_elems + kRefreshThreads - 1) / kRefreshThreads;
  gx = gx < 1 ? 1 : (gx > 64 ? 64 : gx);
  TFL_TIMED("k_refresh_layers", st);
  hipLaunchKernelGGL(k_refresh_layers, dim3(gx, nlayers), dim3(kRefreshThreads), 0, st, src, d_table);
}
void refresh_pack(hipStream_t st, const RefreshSrc& src, const PackJob* d_jobs, int njobs, int max_elems) {
  int gx = (max_elems + kRefreshThreads - 1) / kRefreshThreads;
  gx = gx < 1 ? 1 : (gx > 64 ? 64 : gx);
  TFL_TIMED("k_refresh_pack", st);
  hipLaunchKernelGGL(k_refresh_pack, dim3(gx, njobs), dim3(kRefreshThreads), 0, st, src, d_jobs);
}
void refresh_pack16(hipStream_t st, const RefreshSrc& src, void* const* wfrag16, float* d_post, float* tail_pack) {
  Pack16Args a = {{(uint16_t*)wfrag16[0], (uint16_t*)wfrag16[1], (uint16_t*)wfrag16[2]}, d_post, tail_pack};
  TFL_TIMED("k_refresh_pack16", st);
  hipLaunchKernelGGL(k_refresh_pack16, dim3(3), dim3(kRefreshThreads), 0, st, src, a);
}

}  // namespace tfl
