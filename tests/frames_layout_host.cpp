// A stand-alone host program over the layout arithmetic of the resident frame store (fluidnet_amd/csrc/tfl_frames.hpp; DESIGN.md
// 3.21): the plane and slot offsets of a record, the map from a record's planes to the gather's seven output tensors, and the
// split of each thread's four loaded floats into 128- / 64- / 32-bit stores and a scalar tail -- walked exactly as
// k_frames_gather walks them (grid x = frames_blocks_x, y = plane, z = item; kFramesThreads threads; kFramesVecs vectors each),
// on host buffers sized exactly, so that AddressSanitizer / UBSan see any index that leaves them. Counted: every source float a
// thread loads lies inside its slot's plane, every store is aligned to its width, and every destination element is written
// exactly once with its own source value. For every cell count 1 ... 70, C = 2 and 3, and destination tensors that start 0 / 4 /
// 8 / 12 bytes behind a 16-byte boundary. No GPU, no HIP call.
// Built and run by tests/test_frames_layout_cpu.py:  g++ -std=c++17 -fsanitize=address,undefined frames_layout_host.cpp
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../fluidnet_amd/csrc/tfl_frames.hpp"

#define CHECK(c) do { if (!(c)) { std::fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #c); std::exit(1); } } while (0)

using namespace tfl;

// a store of `cap` slots, the first `dev` of them in the "device" buffer; value of float i of plane pl of slot s = a code of
// (s, pl, i), the padding a code of its own that must never arrive
static float code(long long s, int pl, long long i) { return (float)(s * 4096 + pl * 256 + i); }
static const float kPad = -1.0f;

struct Dst {
  std::vector<float> raw;      // exactly off + B * chans * cells floats
  std::vector<int> hits;
  float* base;                 // 16-byte aligned + off floats
};

static void run(int C, long long cells, int off_floats) {
  FramesLayout L;
  // frames_layout takes a grid: a 2-D one of `cells` x 1 has C = 2, a 3-D one C = 3
  L = frames_layout(C == 3, 1, 1, (int)cells);
  CHECK(L.C == C && L.cells == cells && L.plane % 4 == 0 && L.plane >= cells && L.plane < cells + 4);
  const int planes = frames_planes(C);
  CHECK(L.record == planes * L.plane);
  // the plane -> output map is a bijection onto the channels of the seven outputs, in record order
  {
    int next = 0;
    for (int t = 0; t < kFramesOutputs; t++) {
      CHECK(frames_out_first_plane(C, t) == next);
      for (int ch = 0; ch < frames_out_channels(C, t); ch++) {
        int tt, cc;
        frames_plane_dst(C, next, &tt, &cc);
        CHECK(tt == t && cc == ch);
        next++;
      }
    }
    CHECK(next == planes);
  }
  const long long cap = 5, dev = 2;
  const int B = 4, n = 3;
  const int slots[n] = {4, 0, 4};      // host, device, and a repeated slot
  std::vector<float> dbuf((size_t)(dev * L.record)), hbuf((size_t)((cap - dev) * L.record));
  for (long long s = 0; s < cap; s++) {
    int on_host;
    const long long local = frames_slot_local(s, dev, &on_host);
    CHECK(on_host == (s >= dev) && local >= 0 && local < (on_host ? cap - dev : dev));
    std::vector<float>& buf = on_host ? hbuf : dbuf;
    for (int pl = 0; pl < planes; pl++) {
      const long long o = frames_src_offset(L, local, pl);
      CHECK(o % 4 == 0);      // every plane of every slot on 16 bytes (the allocations are)
      for (long long i = 0; i < L.plane; i++) buf[(size_t)(o + i)] = i < cells ? code(s, pl, i) : kPad;
    }
  }
  // the seven outputs: each in a buffer of its own exact size, its first float `off_floats` behind a 16-byte boundary
  std::vector<Dst> out(kFramesOutputs);
  for (int t = 0; t < kFramesOutputs; t++) {
    const long long numel = (long long)B * frames_out_channels(C, t) * cells;
    out[t].raw.assign((size_t)(numel + off_floats), 7.0f);
    out[t].hits.assign((size_t)numel, 0);
    out[t].base = out[t].raw.data() + off_floats;
  }
  const long long nvec = L.plane / 4;
  const int bxn = frames_blocks_x(L);
  CHECK((long long)bxn * kFramesVecs * kFramesThreads >= nvec && (long long)(bxn - 1) * kFramesVecs * kFramesThreads < nvec);
  for (int item = 0; item < n; item++)
    for (int pl = 0; pl < planes; pl++) {
      int t, ch;
      frames_plane_dst(C, pl, &t, &ch);
      int on_host;
      const long long local = frames_slot_local(slots[item], dev, &on_host);
      const std::vector<float>& sbuf = on_host ? hbuf : dbuf;
      const long long so = frames_src_offset(L, local, pl);
      const long long doff = frames_dst_offset(L, item, frames_out_channels(C, t), ch);
      // the kernel reads the address's low bits; here the buffer's own alignment is whatever the allocator gave, so the
      // misalignment is formed from the offsets the test controls (base = a 16-byte boundary + off_floats)
      const int mis = (int)((off_floats + doff) & 3);
      float* dst = out[t].base + doff;
      int* hit = out[t].hits.data() + doff;
      for (int bx = 0; bx < bxn; bx++)
        for (int tid = 0; tid < kFramesThreads; tid++) {
          float q[kFramesVecs][4];
          for (int k = 0; k < kFramesVecs; k++) {
            const long long v = frames_vec(bx, k, tid);
            const long long lv = v < nvec ? v : 0;
            for (int e = 0; e < 4; e++) q[k][e] = sbuf[(size_t)(so + 4 * lv + e)];      // (the vector: one aligned 16-byte load)
            CHECK((so + 4 * lv) % 4 == 0 && 4 * lv + 4 <= L.plane);
          }
          for (int k = 0; k < kFramesVecs; k++) {
            const long long v = frames_vec(bx, k, tid);
            if (v >= nvec) continue;
            const FramesSplit s = frames_split(cells, mis, v);
            const long long e0 = 4 * v;
            auto store = [&](int first, int count) {      // one store of `count` floats: aligned to its width, inside the plane
              CHECK(((off_floats + doff + e0 + first) * 4) % (4 * count) == 0);
              for (int e = first; e < first + count; e++) {
                CHECK(e0 + e < cells);
                dst[e0 + e] = q[k][e];
                hit[e0 + e]++;
              }
            };
            if (s.kind == kFramesStore16) { CHECK(s.n == 4 && mis == 0); store(0, 4); }
            else if (s.kind == kFramesStore8) { CHECK(s.n == 4 && mis == 2); store(0, 2); store(2, 2); }
            else if (s.kind == kFramesStore484) { CHECK(s.n == 4 && (mis & 1)); store(0, 1); store(1, 2); store(3, 1); }
            else { CHECK(s.kind == kFramesStoreTail && s.n >= 0 && s.n < 4); for (int e = 0; e < s.n; e++) store(e, 1); }
          }
        }
    }
  for (int t = 0; t < kFramesOutputs; t++) {
    const int chans = frames_out_channels(C, t);
    for (int b = 0; b < B; b++)
      for (int ch = 0; ch < chans; ch++)
        for (long long i = 0; i < cells; i++) {
          const long long o = frames_dst_offset(L, b, chans, ch) + i;
          CHECK(out[t].hits[(size_t)o] == (b < n ? 1 : 0));
          const float want = b < n ? code(slots[b], frames_out_first_plane(C, t) + ch, i) : 7.0f;
          CHECK(out[t].base[o] == want);
        }
    for (int i = 0; i < off_floats; i++) CHECK(out[t].raw[(size_t)i] == 7.0f);
  }
}

int main() {
  for (int C = 2; C <= 3; C++)
    for (long long cells = 1; cells <= 70; cells++)
      for (int off = 0; off < 4; off++) run(C, cells, off);
  // more than one block along x, and a plane whose last block is partly idle
  for (long long cells : {4096ll, 4099ll, 5000ll}) {
    run(2, cells, 0);
    run(3, cells, 1);
  }
  // the reference's shapes: 2-D 128^2 (9 planes of 16384 floats), 3-D 64^3 (11 planes of 262144)
  const FramesLayout a = frames_layout(0, 1, 128, 128), b = frames_layout(1, 64, 64, 64);
  CHECK(a.record == 9 * 16384 && frames_blocks_x(a) == 4 && b.record == 11 * 262144 && frames_blocks_x(b) == 64);
  // 20 k frames of 64^3: float offsets beyond 2^31 stay exact
  CHECK(frames_src_offset(b, 19999, 10) == 19999ll * 11 * 262144 + 10ll * 262144);
  std::puts("frames layout OK");
  return 0;
}
