// tfl_pcg_mg.hpp -- the multigrid preconditioner of solveLinearSystemPCG (precondType = "mg", pcg_mg.hip): its parameters, the
// geometry of the level hierarchy and the index maps between a level and the next coarser one. Plain C++ without a HIP header:
// the kernels, the host code (pcg.hip), the workspace table (tfl_pcg_ws.hpp) and a stand-alone host program
// (tests/pcg_mg_ws_host.cpp) read the same expressions. tests/pcg_mg_ref64.py mirrors the constants.
//
// One symmetric V-cycle of aggregation multigrid per CG iteration, matrix-free from the flag grid, for one fluid component:
//   level 0   the component's cells; diag = number of non-obstacle neighbours, coupling 1 to every face neighbour in the component,
//             stored as one "plus-face" coupling per axis (cx, cy, cz: the coupling of a cell to its neighbour at +1);
//   coarser   2x per pooled axis (y, x in 2-D; z, y, x in 3-D), extent = ceil(fine / 2), piecewise-constant P, the exact Galerkin
//             product P^T A P: diag_c = sum of the children's diag - 2 * the couplings inside the aggregate, plus-face coupling =
//             sum of the children's couplings across that face. A cell with diag = 0 (inactive, or an isolated aggregate) keeps 0;
//   cycle     from z = 0: kMgNu damped-Jacobi sweeps (weight kMgOmega), r_c = P^T (r - A z), recurse, z += kMgAlpha P z_c,
//             kMgNu sweeps; kMgNuCoarse sweeps from 0 on the coarsest level (no direct solve: a pure Neumann component is no
//             special case). Equal pre- and post-smoothing, R = P^T and Galerkin operators make M^-1 symmetric positive
//             semi-definite for any kMgAlpha > 0 and kMgOmega rho(D^-1 A) < 2; rho(D^-1 A) <= 2 here, so kMgOmega < 1 is safe.
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define TFL_MG_HD __host__ __device__
#else
#define TFL_MG_HD
#endif

namespace tfl {

// chosen on the cases of tests/test_pcg_mg_ref_cpu.py with the fp64 restatement (profiles/pcg_mg.md, "parameters")
constexpr float kMgOmega = 0.8f;       // Jacobi weight
constexpr int kMgNu = 2;               // pre- and post-smoothing sweeps per level
constexpr int kMgNuCoarse = 8;         // sweeps on the coarsest level
constexpr float kMgAlpha = 1.6f;       // over-correction of the piecewise-constant prolongation
constexpr int kMgCoarsestExtent = 4;   // coarsen while every pooled axis is longer than this
constexpr int kMgMaxLevels = 10;
constexpr int kMgBlockCells = 4096;    // levels of at most this many cells run inside ONE single-block kernel (k_mg_coarse)
static_assert(kMgNu >= 1 && kMgNuCoarse >= 1, "the first sweep of a level starts from z = 0");

struct MgLevelGeom {
  int Z, Y, X;
  long long n;      // cells
  long long off;    // cells of the coarser levels before this one (levels >= 1 are stacked; 0 for levels 0 and 1)
};
struct MgLevels {
  int count;                    // levels, level 0 = the grid
  int is3d;
  int first_block_level;        // the first level k_mg_coarse owns: >= 1, == count when no level is small enough
  long long coarse_cells;       // sum of n over the levels >= 1
  MgLevelGeom lv[kMgMaxLevels];
};

inline MgLevels mg_levels(int Z, int Y, int X, bool is3d) {
  MgLevels m{};
  m.is3d = is3d ? 1 : 0;
  m.lv[0] = {Z, Y, X, (long long)Z * Y * X, 0};
  m.count = 1;
  while (m.count < kMgMaxLevels) {
    const MgLevelGeom& f = m.lv[m.count - 1];
    if (f.X <= kMgCoarsestExtent || f.Y <= kMgCoarsestExtent || (is3d && f.Z <= kMgCoarsestExtent)) break;
    MgLevelGeom c;
    c.X = (f.X + 1) / 2; c.Y = (f.Y + 1) / 2; c.Z = is3d ? (f.Z + 1) / 2 : f.Z;
    c.n = (long long)c.Z * c.Y * c.X;
    c.off = m.coarse_cells;
    m.coarse_cells += c.n;
    m.lv[m.count++] = c;
  }
  m.first_block_level = m.count;
  for (int l = m.count - 1; l >= 1 && m.lv[l].n <= kMgBlockCells; l--) m.first_block_level = l;
  return m;
}

// the parent of fine cell (k, j, i) as an index of the coarse level
TFL_MG_HD inline long long mg_parent(const MgLevelGeom& c, bool is3d, int k, int j, int i) {
  return ((long long)(is3d ? k >> 1 : k) * c.Y + (j >> 1)) * c.X + (i >> 1);
}
// The children of coarse cell (K, J, I) in summation order: z outermost, then y, then x, the lower child first. Child q
// (0 .. mg_child_slots - 1) sits at offset (q >> 2 & 1, q >> 1 & 1, q & 1); children outside the fine grid do not exist.
TFL_MG_HD inline int mg_child_slots(bool is3d) { return is3d ? 8 : 4; }
TFL_MG_HD inline bool mg_child(const MgLevelGeom& f, bool is3d, int K, int J, int I, int q, int& k, int& j, int& i) {
  k = is3d ? 2 * K + ((q >> 2) & 1) : K;
  j = 2 * J + ((q >> 1) & 1);
  i = 2 * I + (q & 1);
  return k < f.Z && j < f.Y && i < f.X;
}

// What the kernels get of one level: its geometry and its arrays in the workspace. diag, invd (1 / diag, 0 where diag = 0), the
// plus-face couplings, the right-hand side r and the two iterates za / zb (a cycle leaves the level's z in zb). On level 0
// r and zb are the CG's r and z.
struct MgLv {
  MgLevelGeom g;
  int n;
  float *diag, *invd, *cx, *cy, *cz, *r, *za, *zb;
};
struct MgDev {
  int count, first_block_level;
  MgLv lv[kMgMaxLevels];
};

}  // namespace tfl
