// tfl_frames.hpp -- the layout arithmetic of the resident frame store (tfl_frames_*, frames.hip): where a plane
// of a slot lies, which plane of a record feeds which channel of which of the gather's seven output tensors, and how one thread
// of k_frames_gather splits the four floats it has loaded into stores. Plain C++ without a HIP call: the kernel calls these
// functions on the device, and a stand-alone host program walks them over exactly sized buffers under a sanitizer and counts
// that every destination element is written exactly once (tests/frames_layout_host.cpp).
//
// A record = one training frame pair as lib/data_binary.lua:93-114 keeps it: 2 C + 5 fp32 planes of Z Y X cells,
//   pDiv, UDiv[C], flags, densityDiv, p, U[C], density          (C = 3 in 3-D, 2 in 2-D)
// the flags plane stored ONCE (the two files of a frame carry equal flags, :77), as the floats loadMantaFile makes of the int32
// words. Every plane is padded to a multiple of 4 floats, so every plane of every slot starts on 16 bytes and the kernel's
// source loads are 128-bit whatever the grid. The seven output tensors of a gather, in the order of the C entry:
//   0 pDiv  1 UDiv  2 flags  3 densityDiv  4 pTarget (<- p)  5 UTarget (<- U)  6 densityTarget (<- density)
// Ingest (tfl_frames_put) is not a hot path: one copy per frame, once per data set.
#pragma once
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

constexpr int kFramesOutputs = 7;
constexpr int kFramesMaxSlots = 128;      // slot indices per launch: they travel by value as kernel arguments
constexpr int kFramesThreads = 256;
constexpr int kFramesVecs = 4;            // 128-bit loads per thread, all issued before its first store

struct FramesLayout {
  int C;                  // velocity channels
  long long cells;        // Z Y X
  long long plane;        // floats from one plane of a slot to the next: cells rounded up to a multiple of 4
  long long record;       // floats per slot: (2 C + 5) plane
};
TFL_HD inline int frames_planes(int C) { return 2 * C + 5; }
TFL_HD inline FramesLayout frames_layout(int is3D, int Z, int Y, int X) {
  FramesLayout L;
  L.C = is3D ? 3 : 2;
  L.cells = (long long)Z * Y * X;
  L.plane = (L.cells + 3) & ~3ll;
  L.record = frames_planes(L.C) * L.plane;
  return L;
}
// the channels of output tensor t
TFL_HD inline int frames_out_channels(int C, int t) { return t == 1 || t == 5 ? C : 1; }
// the record's plane that holds channel 0 of output tensor t
TFL_HD inline int frames_out_first_plane(int C, int t) {
  return t == 0 ? 0 : t == 1 ? 1 : t == 2 ? C + 1 : t == 3 ? C + 2 : t == 4 ? C + 3 : t == 5 ? C + 4 : 2 * C + 4;
}
// plane pl of a record -> the output tensor it feeds (*t) and the channel there (*ch)
TFL_HD inline void frames_plane_dst(int C, int pl, int* t, int* ch) {
  int k = kFramesOutputs - 1;
  while (k > 0 && frames_out_first_plane(C, k) > pl) k--;
  *t = k;
  *ch = pl - frames_out_first_plane(C, k);
}
// the float offset of plane pl of slot s inside the allocation that holds the slot (the device part holds slots [0, device_frames),
// the host part the rest: frames_slot_local)
TFL_HD inline long long frames_src_offset(const FramesLayout& L, long long local_slot, int pl) { return local_slot * L.record + pl * L.plane; }
TFL_HD inline long long frames_slot_local(long long slot, long long device_frames, int* on_host) {
  *on_host = slot >= device_frames;
  return *on_host ? slot - device_frames : slot;
}
// the float offset of channel ch of item b in a contiguous [B][chans][Z][Y][X] output tensor
TFL_HD inline long long frames_dst_offset(const FramesLayout& L, long long b, int chans, int ch) { return (b * chans + ch) * L.cells; }

// ---- one thread's stores ---------------------------------------------------------------------------------------------------
// Thread `tid` of block `bx` loads the source vectors frames_vec(bx, k, tid), k < kFramesVecs (vector v = floats [4 v, 4 v + 4)
// of the padded source plane; a vector at or beyond plane / 4 is not loaded). What it stores of vector v depends on the
// destination plane's address: mis = (address / 4) mod 4, the floats the plane starts behind a 16-byte boundary.
//   kFramesStore16     one 128-bit store                                       (mis 0: Z Y X a multiple of 4, or channel 0 of item 0)
//   kFramesStore8      two 64-bit stores: floats {0, 1}, {2, 3}                (mis 2)
//   kFramesStore484    32-, 64-, 32-bit: floats {0}, {1, 2}, {3}               (mis 1, 3: float 1 of every vector sits on 8 bytes)
//   kFramesStoreTail   n < 4 scalar stores: the vector that holds the plane's last cells; the padding is never stored
enum { kFramesStore16 = 0, kFramesStore8 = 1, kFramesStore484 = 2, kFramesStoreTail = 3 };
struct FramesSplit { int kind, n; };      // n: the floats stored (4 but for the tail; 0: nothing)
TFL_HD inline long long frames_vec(int bx, int k, int tid) { return ((long long)bx * kFramesVecs + k) * kFramesThreads + tid; }
TFL_HD inline int frames_blocks_x(const FramesLayout& L) {
  const long long per = (long long)kFramesVecs * kFramesThreads;
  return (int)((L.plane / 4 + per - 1) / per);
}
TFL_HD inline int frames_mis(const void* dst_plane) { return (int)(((uintptr_t)dst_plane >> 2) & 3); }
TFL_HD inline FramesSplit frames_split(long long cells, int mis, long long v) {
  FramesSplit s;
  const long long left = cells - 4 * v;
  if (left <= 0) { s.kind = kFramesStoreTail; s.n = 0; return s; }
  if (left < 4) { s.kind = kFramesStoreTail; s.n = (int)left; return s; }
  s.n = 4;
  s.kind = mis == 0 ? kFramesStore16 : mis == 2 ? kFramesStore8 : kFramesStore484;
  return s;
}

// ---- the scatter: device tensors into slots (tfl_frames_put_device, k_frames_scatter) -----------------------------------------
// The gather's map run backwards, on the same launch geometry (grid x = frames_blocks_x, y = plane of the record, z = item;
// thread `tid` of block `bx` owns the vectors frames_vec(bx, k, tid) < plane / 4 of the SLOT's plane). Plane pl of the record is
// fed by channel ch of input tensor t (frames_plane_dst); a NULL tensor leaves its planes as they are. The slot side starts on
// 16 bytes and is padded, so every vector is ONE 128-bit store, the padding floats included (as zero); the tensor side is
// where the alignment varies: the four floats of vector v are read as frames_split says -- the kinds name loads here -- and the
// vector that holds the plane's last cells reads n < 4 scalars and fills the rest with zero.
TFL_HD inline long long frames_scatter_src_offset(const FramesLayout& L, long long item, int t, int ch) {
  return frames_dst_offset(L, item, frames_out_channels(L.C, t), ch);
}
TFL_HD inline long long frames_scatter_dst_offset(const FramesLayout& L, long long local_slot, int pl) { return frames_src_offset(L, local_slot, pl); }
// how a thread reads vector v of a tensor plane that starts `mis` floats behind a 16-byte boundary (v < plane / 4, so n >= 1)
TFL_HD inline FramesSplit frames_scatter_split(long long cells, int mis, long long v) { return frames_split(cells, mis, v); }
// float e of vector v of a slot's plane: a cell (read from the tensor) or padding (written as zero)
TFL_HD inline bool frames_scatter_is_cell(long long cells, long long v, int e) { return 4 * v + e < cells; }

}  // namespace tfl
