// frames.hip -- the resident frame store of the training loop and its one-launch mini-batch gather (tfl_frames_*).
// The reference caches every frame on disk and rebuilds each mini-batch on CPU threads, then copies it to the GPU
// (lib/data_binary.lua:190-251, 413-453, lib/run_epoch.lua:131). Here the frames stay resident: slots [0, device_frames) in one
// HBM allocation, the overflow in one pinned, device-mapped host allocation, and k_frames_gather writes the seven tensors of a
// mini-batch from the selected slots wherever they lie -- no staging copy, no launch per plane.
// blockIdx.z = batch item, blockIdx.y = plane of the record, threads over the plane (tfl_frames.hpp: the layout, and the split
// of a thread's four floats into stores). Source planes always start on 16 bytes, so every load is 128-bit; a destination
// plane of a [B][C][Z][Y][X] tensor starts on 16 bytes only where Z Y X is a multiple of 4, and takes narrower stores otherwise.
// A thread issues all its loads before its first store: reads of host-mapped slots cross the host link, are latency-bound, and
// need many loads in flight. Nothing passes through arithmetic: the copy is bit-exact (NaN payloads, -0, denormals).
// The slot indices travel by value as kernel arguments (at most kFramesMaxSlots per launch): no host read, no synchronisation,
// and a gather captured into a graph replays the slots it was recorded with.
// k_frames_scatter is the same map run backwards (tfl_frames_put_device): device tensors into the planes of
// slots, for a producer that lives on the device -- the data-set generator -- so that a frame never passes through the host.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "tfl_abi.hpp"
#include "tfl_frames.hpp"

struct tfl_frames {
  tfl::FramesLayout L{};
  int is3d = 0, Z = 0, Y = 0, X = 0, device = 0;
  long long capacity = 0, device_frames = 0;
  float* d_dev = nullptr;       // slots [0, device_frames)
  float* h_host = nullptr;      // slots [device_frames, capacity): pinned, mapped
  float* d_host = nullptr;      // the device address of h_host
};

namespace tfl {
namespace {

struct FramesGatherArgs {
  const float* dev;
  const float* host;
  long long device_frames;
  FramesLayout L;
  float* out[kFramesOutputs];       // item 0 of this launch; null: the tensor is skipped
  int slots[kFramesMaxSlots];
};

__global__ __launch_bounds__(kFramesThreads) void k_frames_gather(const FramesGatherArgs a) {
  const int item = blockIdx.z, pl = blockIdx.y;
  int t, ch;
  frames_plane_dst(a.L.C, pl, &t, &ch);
  float* out = a.out[t];
  if (!out) return;      // (block-uniform)
  int on_host;
  const long long local = frames_slot_local(a.slots[item], a.device_frames, &on_host);
  const float* __restrict__ src = (on_host ? a.host : a.dev) + frames_src_offset(a.L, local, pl);
  float* __restrict__ dst = out + frames_dst_offset(a.L, item, frames_out_channels(a.L.C, t), ch);
  const int mis = frames_mis(dst);
  const long long nvec = a.L.plane / 4;
  float4 q[kFramesVecs];
  // unconditional loads (a predicated one compiles to a branch that drains the load queue): a thread beyond the plane reads
  // the plane's first vector and drops it
#pragma unroll
  for (int k = 0; k < kFramesVecs; k++) {
    const long long v = frames_vec((int)blockIdx.x, k, (int)threadIdx.x);
    q[k] = *reinterpret_cast<const float4*>(src + 4 * (v < nvec ? v : 0));
  }
#pragma unroll
  for (int k = 0; k < kFramesVecs; k++) {
    const long long v = frames_vec((int)blockIdx.x, k, (int)threadIdx.x);
    if (v >= nvec) continue;
    const FramesSplit s = frames_split(a.L.cells, mis, v);
    float* d = dst + 4 * v;
    // (the three forms write the same 16 bytes, and left alone the compiler sinks them into ONE common tail of the weakest
    // alignment -- a 96-bit and a 32-bit store on every path. An empty asm statement of its own at the end of each arm keeps
    // the arms apart, so that an aligned plane gets its 128-bit store. What the source states is the alignment each store
    // NEEDS; hipcc may still fuse the narrower ones into dword-aligned wide stores, which gfx950 takes for global memory.)
    if (s.kind == kFramesStore16) {
      *reinterpret_cast<float4*>(d) = q[k];
      asm volatile("; frames: 128-bit store");
    } else if (s.kind == kFramesStore8) {
      *reinterpret_cast<float2*>(d) = make_float2(q[k].x, q[k].y);
      *reinterpret_cast<float2*>(d + 2) = make_float2(q[k].z, q[k].w);
      asm volatile("; frames: 64-bit stores");
    } else if (s.kind == kFramesStore484) {
      d[0] = q[k].x;
      *reinterpret_cast<float2*>(d + 1) = make_float2(q[k].y, q[k].z);
      d[3] = q[k].w;
      asm volatile("; frames: 32-, 64-, 32-bit stores");
    } else {
      if (s.n > 0) d[0] = q[k].x;
      if (s.n > 1) d[1] = q[k].y;
      if (s.n > 2) d[2] = q[k].z;
    }
  }
}

// The scatter (tfl_frames_put_device): item z of every non-null tensor into the planes it feeds of slot slots[z], the map of
// tfl_frames.hpp run backwards on the gather's launch geometry. The slot side is aligned and padded: one 128-bit store per
// vector, the padding as zero. The tensor side takes the loads its alignment allows; all of a thread's loads before its first
// store, as above (a store into a host-mapped slot is posted and needs no such care). Bit-exact like the gather.
struct FramesScatterArgs {
  float* dev;
  float* host;
  long long device_frames;
  FramesLayout L;
  const float* in[kFramesOutputs];  // item 0 of this launch; null: the tensor's planes keep what they hold
  int slots[kFramesMaxSlots];
};

__global__ __launch_bounds__(kFramesThreads) void k_frames_scatter(const FramesScatterArgs a) {
  const int item = blockIdx.z, pl = blockIdx.y;
  int t, ch;
  frames_plane_dst(a.L.C, pl, &t, &ch);
  const float* in = a.in[t];
  if (!in) return;      // (block-uniform)
  int on_host;
  const long long local = frames_slot_local(a.slots[item], a.device_frames, &on_host);
  float* __restrict__ dst = (on_host ? a.host : a.dev) + frames_scatter_dst_offset(a.L, local, pl);
  const float* __restrict__ src = in + frames_scatter_src_offset(a.L, item, t, ch);
  const int mis = frames_mis(src);
  const long long nvec = a.L.plane / 4;
  float4 q[kFramesVecs];
#pragma unroll
  for (int k = 0; k < kFramesVecs; k++) {
    const long long v = frames_vec((int)blockIdx.x, k, (int)threadIdx.x);
    q[k] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (v >= nvec) continue;
    const FramesSplit s = frames_scatter_split(a.L.cells, mis, v);
    const float* p = src + 4 * v;
    if (s.kind == kFramesStore16) {
      q[k] = *reinterpret_cast<const float4*>(p);
    } else if (s.kind == kFramesStore8) {
      const float2 lo = *reinterpret_cast<const float2*>(p), hi = *reinterpret_cast<const float2*>(p + 2);
      q[k] = make_float4(lo.x, lo.y, hi.x, hi.y);
    } else if (s.kind == kFramesStore484) {
      const float2 mid = *reinterpret_cast<const float2*>(p + 1);
      q[k] = make_float4(p[0], mid.x, mid.y, p[3]);
    } else {
      // the plane's last cells: what lies behind them in the slot is padding and is written as zero
      if (frames_scatter_is_cell(a.L.cells, v, 0)) q[k].x = p[0];
      if (frames_scatter_is_cell(a.L.cells, v, 1)) q[k].y = p[1];
      if (frames_scatter_is_cell(a.L.cells, v, 2)) q[k].z = p[2];
    }
  }
#pragma unroll
  for (int k = 0; k < kFramesVecs; k++) {
    const long long v = frames_vec((int)blockIdx.x, k, (int)threadIdx.x);
    if (v < nvec) *reinterpret_cast<float4*>(dst + 4 * v) = q[k];
  }
}

const char* const kOutName[kFramesOutputs] = {"pDiv", "UDiv", "flags", "densityDiv", "pTarget", "UTarget", "densityTarget"};

// what tfl_frames_gather and tfl_frames_put_device ask of a call before anything is launched: the slots in range, every
// non-null tensor 4-byte aligned device memory of the context's device, of the store's shape, with at least n items
int check_frames_call(tfl_ctx* c, const char* who, const tfl_frames* f, int n, const int32_t* h_slots,
                      const tfl_tensor* const ts[kFramesOutputs], bool* any) {
  if (!f) return fail(c, TFL_EINVAL, "%s: null store", who);
  if (n < 0 || (n > 0 && !h_slots)) return fail(c, TFL_EINVAL, "%s: n = %d slots, or a null slot array", who, n);
  if (f->device != c->device) return fail(c, TFL_EINVAL, "%s: the store lives on device %d, the context on device %d", who, f->device, c->device);
  for (int i = 0; i < n; i++)
    if (h_slots[i] < 0 || h_slots[i] >= f->capacity)
      return fail(c, TFL_EINVAL, "%s: slot %d (item %d) is out of range [0, %lld)", who, (int)h_slots[i], i, (long long)f->capacity);
  const int C = f->L.C;
  *any = false;
  // (a tfl_tensor is contiguous by definition -- it carries no strides; a binding checks that before it builds one)
  for (int t = 0; t < kFramesOutputs; t++) {
    const tfl_tensor* o = ts[t];
    if (!o) continue;
    const char* name = kOutName[t];
    if (!o->data || ((uintptr_t)o->data & 3) != 0) return fail(c, TFL_EINVAL, "%s: %s has no data or is not 4-byte aligned", who, name);
    const int ch = frames_out_channels(C, t);
    if (o->C != ch || o->Z != f->Z || o->Y != f->Y || o->X != f->X)
      return fail(c, TFL_EINVAL, "%s: %s has shape [%d][%d][%d][%d] per item, the store holds [%d][%d][%d][%d] (wrong shape)", who, name,
                  o->C, o->Z, o->Y, o->X, ch, f->Z, f->Y, f->X);
    if (n > o->B) return fail(c, TFL_EINVAL, "%s: n = %d exceeds the batch size B = %d of %s", who, n, o->B, name);
    hipPointerAttribute_t at;
    if (hipPointerGetAttributes(&at, o->data) != hipSuccess) {
      (void)hipGetLastError();
      return fail(c, TFL_EINVAL, "%s: %s is not device memory (a host array? there is no CPU path)", who, name);
    }
    if (at.type != hipMemoryTypeDevice || at.device != c->device)
      return fail(c, TFL_EINVAL, "%s: %s is not device memory of this context's device %d", who, name, c->device);
    *any = true;
  }
  return TFL_OK;
}

}  // namespace
}  // namespace tfl

using tfl::fail;

extern "C" {

tfl_frames* tfl_frames_create(tfl_ctx* c, int is3D, int Z, int Y, int X, int64_t capacity, int64_t device_frames) {
  if (!c) return nullptr;
  const char* who = "frames_create";
  if (Z < 1 || Y < 1 || X < 1) { fail(c, TFL_EINVAL, "%s: empty grid", who); return nullptr; }
  if (!is3D && Z != 1) { fail(c, TFL_EINVAL, "%s: 2D domains should have unary z-dimension", who); return nullptr; }
  if ((long long)Z * Y * X * 3 >= (1ll << 31)) { fail(c, TFL_EINVAL, "%s: grid too large for 32-bit cell offsets", who); return nullptr; }
  if (capacity < 1 || capacity > 0x7fffffffll) { fail(c, TFL_EINVAL, "%s: capacity %lld is not in [1, 2^31)", who, (long long)capacity); return nullptr; }
  if (device_frames < 0 || device_frames > capacity) {
    fail(c, TFL_EINVAL, "%s: device_frames %lld is not in [0, capacity = %lld]", who, (long long)device_frames, (long long)capacity);
    return nullptr;
  }
  tfl_frames* f = new tfl_frames();
  f->L = tfl::frames_layout(is3D, Z, Y, X);
  f->is3d = is3D ? 1 : 0; f->Z = Z; f->Y = Y; f->X = X; f->device = c->device;
  f->capacity = capacity; f->device_frames = device_frames;
  const size_t rec = sizeof(float) * (size_t)f->L.record;
  bool ok = true;
  if (device_frames > 0) ok = hipMalloc((void**)&f->d_dev, rec * (size_t)device_frames) == hipSuccess;
  if (ok && capacity > device_frames)
    ok = hipHostMalloc((void**)&f->h_host, rec * (size_t)(capacity - device_frames), hipHostMallocMapped) == hipSuccess &&
         hipHostGetDevicePointer((void**)&f->d_host, f->h_host, 0) == hipSuccess;
  if (!ok) {
    (void)hipGetLastError();
    fail(c, TFL_EHIP, "%s: could not allocate %lld device and %lld host slots of %lld bytes", who, (long long)device_frames,
         (long long)(capacity - device_frames), (long long)rec);
    tfl_frames_destroy(c, f);
    return nullptr;
  }
  return f;
}

void tfl_frames_destroy(tfl_ctx* c, tfl_frames* f) {
  (void)c;
  if (!f) return;
  if (f->d_dev) (void)hipFree(f->d_dev);
  if (f->h_host) (void)hipHostFree(f->h_host);
  delete f;
}

int64_t tfl_frames_record_floats(const tfl_frames* f) { return f ? (int64_t)f->L.record : -1; }

int tfl_frames_put(tfl_ctx* c, tfl_frames* f, int64_t slot, const float* h_record) {
  if (!c) return TFL_EINVAL;
  const char* who = "frames_put";
  if (!f || !h_record) return fail(c, TFL_EINVAL, "%s: null store or record", who);
  if (slot < 0 || slot >= f->capacity) return fail(c, TFL_EINVAL, "%s: slot %lld is out of range [0, %lld)", who, (long long)slot, (long long)f->capacity);
  const size_t rec = sizeof(float) * (size_t)f->L.record;
  int on_host;
  const long long local = tfl::frames_slot_local(slot, f->device_frames, &on_host);
  if (!on_host) {
    HIP_TRY(c, hipMemcpyAsync(f->d_dev + local * f->L.record, h_record, rec, hipMemcpyHostToDevice, c->stream));
    return TFL_OK;
  }
  HIP_TRY(c, hipStreamSynchronize(c->stream));      // a gather enqueued earlier may still be reading the slot
  std::memcpy(f->h_host + local * f->L.record, h_record, rec);
  return TFL_OK;
}

int tfl_frames_gather(tfl_ctx* c, tfl_frames* f, int n, const int32_t* h_slots, const tfl_tensor* pDiv, const tfl_tensor* UDiv,
                      const tfl_tensor* flags, const tfl_tensor* densityDiv, const tfl_tensor* pTarget, const tfl_tensor* UTarget,
                      const tfl_tensor* densityTarget) {
  if (!c) return TFL_EINVAL;
  const char* who = "frames_gather";
  const tfl_tensor* outs[tfl::kFramesOutputs] = {pDiv, UDiv, flags, densityDiv, pTarget, UTarget, densityTarget};
  bool any = false;
  TRY(tfl::check_frames_call(c, who, f, n, h_slots, outs, &any));
  const int C = f->L.C;
  if (n == 0 || !any) return TFL_OK;
  tfl::FramesGatherArgs a;
  a.dev = f->d_dev; a.host = f->d_host; a.device_frames = f->device_frames; a.L = f->L;
  const int bx = tfl::frames_blocks_x(f->L), planes = tfl::frames_planes(C);
  for (int i0 = 0; i0 < n; i0 += tfl::kFramesMaxSlots) {
    const int m = n - i0 < tfl::kFramesMaxSlots ? n - i0 : tfl::kFramesMaxSlots;
    for (int t = 0; t < tfl::kFramesOutputs; t++)
      a.out[t] = outs[t] ? (float*)outs[t]->data + tfl::frames_dst_offset(f->L, i0, tfl::frames_out_channels(C, t), 0) : nullptr;
    for (int i = 0; i < tfl::kFramesMaxSlots; i++) a.slots[i] = i < m ? (int)h_slots[i0 + i] : 0;
    TFL_TIMED("k_frames_gather", c->stream);
    hipLaunchKernelGGL(tfl::k_frames_gather, dim3((unsigned)bx, (unsigned)planes, (unsigned)m), dim3(tfl::kFramesThreads), 0, c->stream, a);
  }
  return tfl::check_launch(c, who);
}

int tfl_frames_put_device(tfl_ctx* c, tfl_frames* f, int n, const int32_t* h_slots, const tfl_tensor* pDiv, const tfl_tensor* UDiv,
                          const tfl_tensor* flags, const tfl_tensor* densityDiv, const tfl_tensor* pTarget, const tfl_tensor* UTarget,
                          const tfl_tensor* densityTarget) {
  if (!c) return TFL_EINVAL;
  const char* who = "frames_put_device";
  const tfl_tensor* ins[tfl::kFramesOutputs] = {pDiv, UDiv, flags, densityDiv, pTarget, UTarget, densityTarget};
  bool any = false;
  TRY(tfl::check_frames_call(c, who, f, n, h_slots, ins, &any));
  // two items of one call into one slot would race: refused (the gather may read a slot twice, nobody may write it twice)
  if (n > 1) {
    std::vector<int32_t> sorted(h_slots, h_slots + n);
    std::sort(sorted.begin(), sorted.end());
    for (int i = 1; i < n; i++)
      if (sorted[i] == sorted[i - 1]) return fail(c, TFL_EINVAL, "%s: slot %d appears twice in one call (duplicate slot)", who, (int)sorted[i]);
  }
  if (n == 0 || !any) return TFL_OK;
  const int C = f->L.C;
  tfl::FramesScatterArgs a;
  a.dev = f->d_dev; a.host = f->d_host; a.device_frames = f->device_frames; a.L = f->L;
  const int bx = tfl::frames_blocks_x(f->L), planes = tfl::frames_planes(C);
  for (int i0 = 0; i0 < n; i0 += tfl::kFramesMaxSlots) {
    const int m = n - i0 < tfl::kFramesMaxSlots ? n - i0 : tfl::kFramesMaxSlots;
    for (int t = 0; t < tfl::kFramesOutputs; t++)
      a.in[t] = ins[t] ? (const float*)ins[t]->data + tfl::frames_scatter_src_offset(f->L, i0, t, 0) : nullptr;
    for (int i = 0; i < tfl::kFramesMaxSlots; i++) a.slots[i] = i < m ? (int)h_slots[i0 + i] : 0;
    TFL_TIMED("k_frames_scatter", c->stream);
    hipLaunchKernelGGL(tfl::k_frames_scatter, dim3((unsigned)bx, (unsigned)planes, (unsigned)m), dim3(tfl::kFramesThreads), 0, c->stream, a);
  }
  return tfl::check_launch(c, who);
}

}  // extern "C"
