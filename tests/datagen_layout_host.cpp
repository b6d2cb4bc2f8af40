// A stand-alone host program over the arithmetic the data-set generator added: the scatter map of
// fluidnet_amd/csrc/tfl_frames.hpp -- device tensors into the slots of the frame store, walked exactly as k_frames_scatter
// walks it (grid x = frames_blocks_x, y = plane, z = item; kFramesThreads threads; kFramesVecs vectors each) -- and the
// primitive, hash and curl arithmetic of fluidnet_amd/csrc/tfl_datagen.hpp, on host buffers sized exactly, so that
// AddressSanitizer / UBSan see any index that leaves them. Counted: every load lies inside its tensor's plane and is aligned to
// its width, every float of a record is written by exactly one (tensor, item, element) or is padding (and then zero), the planes
// of a null tensor and the slots nobody named keep their floats. Cell counts 35, 192 and 1 (and a few more), C = 2 and 3, tensors
// that start 0 / 4 / 8 / 12 bytes behind a 16-byte boundary. No GPU, no HIP call.
// Built and run by tests/test_datagen_layout_cpu.py:  g++ -std=c++17 -fsanitize=address,undefined datagen_layout_host.cpp
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../fluidnet_amd/csrc/tfl_datagen.hpp"
#include "../fluidnet_amd/csrc/tfl_frames.hpp"

#define CHECK(c) do { if (!(c)) { std::fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #c); std::exit(1); } } while (0)

using namespace tfl;

static float code(int t, long long item, int ch, long long i) { return (float)(1 + t * 100000 + item * 10000 + ch * 1000 + i); }
static const float kOld = -7.0f;

// `present`: bit t set = input tensor t is given
static void run_scatter(int C, long long cells, int off_floats, unsigned present) {
  const FramesLayout L = frames_layout(C == 3, 1, 1, (int)cells);
  const int planes = frames_planes(C);
  const long long cap = 5, dev = 2;
  const int B = 4, n = 3;
  const int slots[n] = {4, 0, 3};      // host, device, host: no slot twice
  std::vector<float> dbuf((size_t)(dev * L.record), kOld), hbuf((size_t)((cap - dev) * L.record), kOld);
  std::vector<int> dhit(dbuf.size(), 0), hhit(hbuf.size(), 0);
  // the inputs: each in a buffer of its own exact size, its first float `off_floats` behind a 16-byte boundary
  std::vector<std::vector<float>> in(kFramesOutputs);
  for (int t = 0; t < kFramesOutputs; t++) {
    const int chans = frames_out_channels(C, t);
    in[t].assign((size_t)(off_floats + (long long)B * chans * cells), 0.0f);
    for (int b = 0; b < B; b++)
      for (int ch = 0; ch < chans; ch++)
        for (long long i = 0; i < cells; i++) in[t][(size_t)(off_floats + frames_scatter_src_offset(L, b, t, ch) + i)] = code(t, b, ch, i);
  }
  const long long nvec = L.plane / 4;
  const int bxn = frames_blocks_x(L);
  for (int item = 0; item < n; item++)
    for (int pl = 0; pl < planes; pl++) {
      int t, ch;
      frames_plane_dst(C, pl, &t, &ch);
      if (!(present >> t & 1)) continue;
      int on_host;
      const long long local = frames_slot_local(slots[item], dev, &on_host);
      std::vector<float>& dbase = on_host ? hbuf : dbuf;
      std::vector<int>& hits = on_host ? hhit : dhit;
      const long long dof = frames_scatter_dst_offset(L, local, pl);
      CHECK(dof % 4 == 0);
      const long long sof = frames_scatter_src_offset(L, item, t, ch);
      const int mis = (int)((off_floats + sof) & 3);      // (the kernel reads the address's low bits: frames_mis)
      const std::vector<float>& src = in[t];
      for (int bx = 0; bx < bxn; bx++)
        for (int tid = 0; tid < kFramesThreads; tid++)
          for (int k = 0; k < kFramesVecs; k++) {
            const long long v = frames_vec(bx, k, tid);
            if (v >= nvec) continue;
            const FramesSplit s = frames_scatter_split(cells, mis, v);
            CHECK(s.n >= 1 && s.n <= 4);
            float q[4] = {0.0f, 0.0f, 0.0f, 0.0f};
            auto load = [&](int first, int count) {      // one load of `count` floats: aligned to its width, inside the plane
              CHECK(((off_floats + sof + 4 * v + first) * 4) % (4 * count) == 0);
              for (int e = first; e < first + count; e++) {
                CHECK(4 * v + e < cells);
                q[e] = src[(size_t)(off_floats + sof + 4 * v + e)];
              }
            };
            if (s.kind == kFramesStore16) { CHECK(mis == 0 && s.n == 4); load(0, 4); }
            else if (s.kind == kFramesStore8) { CHECK(mis == 2 && s.n == 4); load(0, 2); load(2, 2); }
            else if (s.kind == kFramesStore484) { CHECK((mis & 1) && s.n == 4); load(0, 1); load(1, 2); load(3, 1); }
            else {
              CHECK(s.kind == kFramesStoreTail && s.n < 4);
              for (int e = 0; e < 3; e++)
                if (frames_scatter_is_cell(cells, v, e)) load(e, 1);
              CHECK(!frames_scatter_is_cell(cells, v, 3) && frames_scatter_is_cell(cells, v, s.n - 1) && !frames_scatter_is_cell(cells, v, s.n));
            }
            CHECK(4 * v + 4 <= L.plane);
            for (int e = 0; e < 4; e++) {      // (the vector: one aligned 16-byte store)
              dbase[(size_t)(dof + 4 * v + e)] = q[e];
              hits[(size_t)(dof + 4 * v + e)]++;
            }
          }
    }
  // every float of every record: written once by its own (tensor, item, element), written once as zero padding, or untouched
  for (long long s = 0; s < cap; s++) {
    int on_host, item = -1;
    const long long local = frames_slot_local(s, dev, &on_host);
    for (int i = 0; i < n; i++)
      if (slots[i] == s) item = i;
    const std::vector<float>& buf = on_host ? hbuf : dbuf;
    const std::vector<int>& hits = on_host ? hhit : dhit;
    for (int pl = 0; pl < planes; pl++) {
      int t, ch;
      frames_plane_dst(C, pl, &t, &ch);
      const bool written = item >= 0 && (present >> t & 1);
      for (long long i = 0; i < L.plane; i++) {
        const size_t o = (size_t)(frames_scatter_dst_offset(L, local, pl) + i);
        CHECK(hits[o] == (written ? 1 : 0));
        const float want = !written ? kOld : i < cells ? code(t, item, ch, i) : 0.0f;
        CHECK(buf[o] == want);
      }
    }
  }
}

static void run_datagen() {
  // the mixer: its fixed point, and 1 through the chain written out
  CHECK(noise_mix(0u) == 0u);
  uint32_t x = 1u;
  x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16;
  CHECK(noise_mix(1u) == x);
  // values: multiples of 2^-23 in [-1, 1), the ends reached by the extreme words
  CHECK(noise_value(0u) == -1.0f && noise_value(0xffffffffu) == 1.0f - 1.0f / 8388608.0f && noise_value(0x80000000u) == 0.0f);
  for (uint32_t c = 0; c < 4096; c++) {
    const float v = noise_value(noise_hash(7u, 3u, c & 3u, c));
    CHECK(v >= -1.0f && v < 1.0f && v * 8388608.0f == std::floor(v * 8388608.0f));
  }
  CHECK(noise_hash(7u, 3u, 0u, 5u) != noise_hash(7u, 3u, 1u, 5u) && noise_hash(7u, 3u, 0u, 5u) != noise_hash(7u, 4u, 0u, 5u));
  CHECK(noise_hash(0xffffffffu, 0xffffffffu, 2u, 0xffffffffu) == noise_hash(0xffffffffu, 0xffffffffu, 2u, 0xffffffffu));      // (wraps, no UB)
  // the rasteriser: a sphere and a box on a 2-D and a 3-D grid against the centre test written out
  SceneTable obs;
  std::memset(&obs, 0, sizeof(obs));
  obs.n = 2;
  obs.p[0].kind = kScenePrimSphere; obs.p[0].a[0] = 4.0f; obs.p[0].a[1] = 3.5f; obs.p[0].a[2] = 2.5f; obs.p[0].b[0] = 1.5f;
  obs.p[1].kind = kScenePrimBox; obs.p[1].a[0] = 6.0f; obs.p[1].a[1] = 1.0f; obs.p[1].a[2] = 1.0f; obs.p[1].b[0] = 8.0f; obs.p[1].b[1] = 3.0f; obs.p[1].b[2] = 2.0f;
  SceneTable blobs = obs;
  blobs.p[0].val = 0.25f; blobs.p[1].val = 0.75f;
  blobs.p[0].b[0] = 3.0f;      // a blob larger than the obstacle sphere around the same centre
  for (int is3D = 0; is3D <= 1; is3D++) {
    const int Z = is3D ? 5 : 1, Y = 7, X = 10;
    int obstacles = 0, dense = 0;
    for (int k = 0; k < Z; k++)
      for (int j = 0; j < Y; j++)
        for (int i = 0; i < X; i++) {
          const float f = scene_flag(obs, is3D, Z, Y, X, i, j, k);
          const bool border = i == 0 || i == X - 1 || j == 0 || j == Y - 1 || (is3D && (k == 0 || k == Z - 1));
          const float dx = i + 0.5f - 4.0f, dy = j + 0.5f - 3.5f, dz = k + 0.5f - 2.5f;
          const bool sph = dx * dx + dy * dy + (is3D ? dz * dz : 0.0f) <= 2.25f;
          const bool box = i + 0.5f >= 6.0f && i + 0.5f <= 8.0f && j + 0.5f >= 1.0f && j + 0.5f <= 3.0f && (!is3D || (k + 0.5f >= 1.0f && k + 0.5f <= 2.0f));
          CHECK(f == ((border || sph || box) ? kSceneObstacle : kSceneFluid));
          obstacles += f == kSceneObstacle;
          const float rho = scene_density(blobs, f, is3D, i, j, k);
          CHECK(f == kSceneFluid || rho == 0.0f);
          CHECK(rho == 0.0f || rho == 0.25f || rho == 0.75f);
          dense += rho != 0.0f;
        }
    CHECK(obstacles > 2 * (X + Y) - 4 && dense > 0);
  }
  // the curl: every index inside an exactly sized potential, clamped at the grid's end; the divergence of an integer potential
  // (no rounding anywhere) is exactly zero
  for (int is3D = 0; is3D <= 1; is3D++) {
    const int Z = is3D ? 4 : 1, Y = 5, X = 6, C = is3D ? 3 : 2, Cpsi = is3D ? 3 : 1;
    const long long cells = (long long)Z * Y * X;
    std::vector<float> psi((size_t)(Cpsi * cells)), U((size_t)(C * cells));
    for (size_t i = 0; i < psi.size(); i++) psi[i] = (float)((int)(noise_hash(1u, 2u, 3u, (uint32_t)i) >> 20) - 2048);
    for (int c = 0; c < C; c++)
      for (int k = 0; k < Z; k++)
        for (int j = 0; j < Y; j++)
          for (int i = 0; i < X; i++) U[(size_t)(c * cells + ((long long)k * Y + j) * X + i)] = curl_mac(psi.data(), is3D, Z, Y, X, c, i, j, k, 2.0f);
    for (int k = 0; k + 1 < (is3D ? Z : 2); k++)
      for (int j = 0; j + 1 < Y; j++)
        for (int i = 0; i + 1 < X; i++) {
          const long long o = ((long long)k * Y + j) * X + i;
          float div = (U[(size_t)(o + 1)] - U[(size_t)o]) + (U[(size_t)(cells + o + X)] - U[(size_t)(cells + o)]);
          if (is3D) div += U[(size_t)(2 * cells + o + (long long)X * Y)] - U[(size_t)(2 * cells + o)];
          CHECK(div == 0.0f);
        }
  }
}

int main() {
  // the cell counts of the three alignment cases of a tail (35 = 4 * 8 + 3, 192 = a multiple of 4, 1), both C, every
  // misalignment, all seven tensors / the two halves of a record / a single tensor
  for (int C = 2; C <= 3; C++)
    for (long long cells : {35ll, 192ll, 1ll, 2ll, 6ll, 4099ll})
      for (int off = 0; off < 4; off++)
        for (unsigned present : {0x7fu, 0x0fu, 0x70u, 0x20u, 0u}) run_scatter(C, cells, off, present);
  run_datagen();
  std::puts("datagen layout OK");
  return 0;
}
