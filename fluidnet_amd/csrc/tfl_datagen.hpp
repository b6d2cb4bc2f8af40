// tfl_datagen.hpp -- the host-checkable arithmetic of the data-set generator's scene kernels (datagen.hip): the
// primitive rasteriser of k_scene_flags, the counter-based noise of k_noise_potential and the staggered curl of k_curl_mac.
// Plain C++ without a HIP call: the kernels call these functions on the device, a stand-alone host program walks them under a
// sanitizer (tests/datagen_layout_host.cpp), and tests/datagen_ref.py restates them in numpy float32 / uint32. Everything is
// fp32 (or uint32) in ONE stated operation order, and the library is built -ffp-contract=off, so the three agree bit for bit.
#pragma once
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

constexpr int kSceneMaxPrims = 32;        // primitives per table: they travel by value as kernel arguments
constexpr int kScenePrimSphere = 0, kScenePrimBox = 1;
constexpr float kSceneFluid = 1.0f, kSceneObstacle = 2.0f;      // TypeFluid, TypeObstacle as the float words of a flags grid

// One primitive in cell units; a cell (i, j, k) is tested at its centre (i + 0.5, j + 0.5, k + 0.5), x first.
//   sphere: a = centre, b[0] = radius           inside: ((dx dx + dy dy) + dz dz) <= r r    (2-D: no dz term)
//   box:    a = lo, b = hi                      inside: lo <= centre <= hi on every axis    (2-D: x and y only)
// val: the density of a blob (the obstacle table does not read it).
struct ScenePrim { int kind; float a[3]; float b[3]; float val; };
struct SceneTable { int n; ScenePrim p[kSceneMaxPrims]; };

TFL_HD inline bool scene_inside(const ScenePrim& q, int is3D, int i, int j, int k) {
  const float cx = (float)i + 0.5f, cy = (float)j + 0.5f, cz = (float)k + 0.5f;
  if (q.kind == kScenePrimSphere) {
    const float dx = cx - q.a[0], dy = cy - q.a[1];
    float d2 = dx * dx + dy * dy;
    if (is3D) { const float dz = cz - q.a[2]; d2 = d2 + dz * dz; }
    return d2 <= q.b[0] * q.b[0];
  }
  const bool in2 = cx >= q.a[0] && cx <= q.b[0] && cy >= q.a[1] && cy <= q.b[1];
  return is3D ? (in2 && cz >= q.a[2] && cz <= q.b[2]) : in2;
}
// emptyDomain(bnd = 1) (generic/tfluids.cc:136-167) plus the obstacle table: the flag word of cell (i, j, k)
TFL_HD inline float scene_flag(const SceneTable& obs, int is3D, int Z, int Y, int X, int i, int j, int k) {
  const bool border = i < 1 || i > X - 2 || j < 1 || j > Y - 2 || (is3D && (k < 1 || k > Z - 2));
  if (border) return kSceneObstacle;
  for (int n = 0; n < obs.n; n++)
    if (scene_inside(obs.p[n], is3D, i, j, k)) return kSceneObstacle;
  return kSceneFluid;
}
// the density of a cell: the value of the LAST blob of the table that holds its centre, +0 outside all of them and in obstacles
TFL_HD inline float scene_density(const SceneTable& blobs, float flag, int is3D, int i, int j, int k) {
  float rho = 0.0f;
  if (flag != kSceneFluid) return rho;
  for (int n = 0; n < blobs.n; n++)
    if (scene_inside(blobs.p[n], is3D, i, j, k)) rho = blobs.p[n].val;
  return rho;
}

// ---- white noise: a counter-based integer hash (a lowbias32-style mixer), pure uint32 arithmetic --------------------------------
TFL_HD inline uint32_t noise_mix(uint32_t x) {
  x ^= x >> 16; x *= 0x7feb352du;
  x ^= x >> 15; x *= 0x846ca68bu;
  x ^= x >> 16;
  return x;
}
// (seed, run, component, cell index inside ONE item's grid) -> 32 bits; nothing of the launch geometry enters
TFL_HD inline uint32_t noise_hash(uint32_t seed, uint32_t run, uint32_t comp, uint32_t cell) {
  uint32_t h = noise_mix(seed + 0x9e3779b9u);
  h = noise_mix(h ^ run);
  h = noise_mix(h ^ comp);
  return noise_mix(h ^ cell);
}
// the top 24 bits as a multiple of 2^-23 in [-1, 1): exactly representable, so the conversion rounds nowhere
TFL_HD inline float noise_value(uint32_t h) { return (float)((int32_t)(h >> 8) - (1 << 23)) * (1.0f / 8388608.0f); }

// ---- the MAC-staggered curl of an edge-located potential ----------------------------------------------------------------------
// psi: [Cpsi][Z][Y][X], Cpsi = 1 in 2-D (psi_z at the cell's lower corner), 3 in 3-D (psi_x, psi_y, psi_z on the edges through
// that corner). A neighbour index beyond the grid's end is clamped to the last one. With d_a f = f(+1 along a) - f:
//   2-D:  u = d_y psi,  v = -(d_x psi)
//   3-D:  u = d_y psi_z - d_z psi_y,  v = d_z psi_x - d_x psi_z,  w = d_x psi_y - d_y psi_x
// each difference rounded once, then the difference of the two, then the product with `amp`: the discrete MAC divergence
// d_x u + d_y v (+ d_z w) of the unrounded field is identically zero.
TFL_HD inline float curl_mac(const float* psi, int is3D, int Z, int Y, int X, int comp, int i, int j, int k, float amp) {
  const long long sy = X, sz = (long long)X * Y, sc = sz * Z;
  const long long o = k * sz + j * sy + i;
  const long long ox = i + 1 < X ? 1 : 0, oy = j + 1 < Y ? sy : 0, oz = k + 1 < Z ? sz : 0;
  if (!is3D) {
    if (comp == 0) return amp * (psi[o + oy] - psi[o]);
    return amp * (-(psi[o + ox] - psi[o]));
  }
  const float* px = psi; const float* py = psi + sc; const float* pz = psi + 2 * sc;
  if (comp == 0) { const float a = pz[o + oy] - pz[o], b = py[o + oz] - py[o]; return amp * (a - b); }
  if (comp == 1) { const float a = px[o + oz] - px[o], b = pz[o + ox] - pz[o]; return amp * (a - b); }
  const float a = py[o + ox] - py[o], b = px[o + oy] - px[o];
  return amp * (a - b);
}

}  // namespace tfl
