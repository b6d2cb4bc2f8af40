// A stand-alone host program over fluidnet_amd/csrc/tfl_step_ws.hpp -- the workspace table of the un-cut native step
// (tfl_simulate_step). It is the record of what the layout was when the table replaced the literals in simulate.cpp: (a) every
// region's offset and length against the expression the step used to write out, (b) every region inside the total and the
// total against the size formula tfl_simulate_workspace_floats used to restate, (c) the regions that are live at the same time
// pairwise disjoint. No GPU, no HIP call. Built and run by tests/test_step_ws_cpu.py:
//   g++ -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all step_ws_host.cpp
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <initializer_list>

#include "../fluidnet_amd/csrc/tfl_step_ws.hpp"

#define CHECK(c) do { if (!(c)) { std::fprintf(stderr, "%s:%d: CHECK(%s) failed (%s)\n", __FILE__, __LINE__, #c, g_case); std::exit(1); } } while (0)

using namespace tfl;

static char g_case[160];

static bool is(WsRegion r, long long off, long long floats) { return r.off == off && r.floats == floats; }
static bool disjoint(WsRegion a, WsRegion b) { return a.off + a.floats <= b.off || b.off + b.floats <= a.off; }
static void check_disjoint(std::initializer_list<WsRegion> live) {
  for (const WsRegion* a = live.begin(); a != live.end(); a++) {
    CHECK(a->floats > 0);      // a group names only regions that exist in the case
    for (const WsRegion* b = a + 1; b != live.end(); b++) CHECK(disjoint(*a, *b));
  }
}

static void check_case(int B, int Z, int Y, int X, int C, StepProj proj, long long pcg_floats) {
  std::snprintf(g_case, sizeof(g_case), "B %d, %d x %d x %d, C %d, proj %d, pcg %lld", B, Z, Y, X, C, (int)proj, pcg_floats);
  const long long N = (long long)B * Z * Y * X;
  const bool is3d = C == 3;
  const StepWs w = step_ws(B, Z, Y, X, C, proj, pcg_floats);

  // ---- (a) the layout as the step wrote it out ------------------------------------------------------------------------------
  // vfwd | vbwd | Uadv at 0 | C N | 2C N
  CHECK(is(w.vfwd, 0, C * N) && is(w.vbwd, C * N, C * N) && is(w.Uadv, 2 * C * N, C * N));
  // the scalar temporaries in front of advectVel: 0 | N | 2N | (2 + C) N | (2 + 2C) N
  CHECK(is(w.scal.fwd, 0, N) && is(w.scal.bwd, N, N) && is(w.scal.fwdPos, 2 * N, C * N) && is(w.scal.bwdPos, (2 + C) * N, C * N));
  CHECK(is(w.sout, (2 + 2 * C) * N, N));
  // ... behind pass A of advectVel (3-D only): fwd 9N, bwd 3N, fwdPos 6N, bwdPos 3N, the last two as three-channel fields
  if (is3d) CHECK(is(w.scal_first.fwd, 9 * N, N) && is(w.scal_first.bwd, 3 * N, N) && is(w.scal_first.fwdPos, 6 * N, 3 * N) && is(w.scal_first.bwdPos, 3 * N, 3 * N));
  else CHECK(is(w.scal_first.fwd, 0, 0) && is(w.scal_first.bwd, 0, 0) && is(w.scal_first.fwdPos, 0, 0) && is(w.scal_first.bwdPos, 0, 0));
  // curl (three planes) / cnorm: 3N and 9N in 3-D, 0 and 3N in 2-D
  CHECK(is(w.curl, is3d ? 3 * N : 0, 3 * N) && is(w.cnorm, is3d ? 9 * N : 3 * N, N));
  // Utmp at 0; centered / force at 4N and (4 + C) N
  CHECK(is(w.Utmp, 0, C * N) && is(w.centered, 4 * N, C * N) && is(w.force, (4 + C) * N, C * N));
  // div at 0; Jacobi's pPrev | pDelta | norm (B floats) at N | 2N | 3N; PCG's workspace behind (N + 1) & ~1
  CHECK(is(w.div, 0, N));
  if (proj == StepProj::jacobi) CHECK(is(w.pPrev, N, N) && is(w.pDelta, 2 * N, N) && is(w.norm, 3 * N, B));
  else CHECK(is(w.pPrev, 0, 0) && is(w.pDelta, 0, 0) && is(w.norm, 0, 0));
  if (proj == StepProj::pcg) CHECK(is(w.pcg, (N + 1) & ~1ll, pcg_floats) && w.pcg.off % 2 == 0 && w.pcg.off >= N);
  else CHECK(is(w.pcg, 0, 0));

  // ---- (b) the total: max((3 + 2C) N, 3C N, (2C + 4) N, method term) + 2 ------------------------------------------------------
  long long need = std::max(std::max((3 + 2 * C) * N, 3 * C * N), (2 * C + 4) * N);
  if (proj == StepProj::jacobi) need = std::max(need, 3 * N + B);
  if (proj == StepProj::pcg) need = std::max(need, N + 2 + pcg_floats);
  CHECK(w.total == need + 2);
  for (WsRegion r : {w.vfwd, w.vbwd, w.Uadv, w.scal.fwd, w.scal.bwd, w.scal.fwdPos, w.scal.bwdPos, w.scal_first.fwd, w.scal_first.bwd,
                     w.scal_first.fwdPos, w.scal_first.bwdPos, w.sout, w.curl, w.cnorm, w.Utmp, w.centered, w.force, w.div, w.pPrev,
                     w.pDelta, w.norm, w.pcg})
    CHECK(r.off >= 0 && r.floats >= 0 && r.off + r.floats <= w.total);

  // ---- (c) what is live at the same time is disjoint --------------------------------------------------------------------------
  // the temporaries of one advectScalar call in front of advectVel, with the channel's output
  check_disjoint({w.scal.fwd, w.scal.bwd, w.scal.fwdPos, w.scal.bwdPos, w.sout});
  // pass A of advectVel first: vfwd is live together with the four scalar temporaries (Uadv is written only after the last
  // scalar pass, so fwdPos may sit on its planes). bwd is exempt against bwdPos alone: the operator does not touch `bwd` on
  // any path, and on this one the min / max grid is not used either, so the two share the `vbwd` planes on purpose
  if (is3d) {
    check_disjoint({w.vfwd, w.scal_first.fwd, w.scal_first.fwdPos, w.scal_first.bwdPos});
    check_disjoint({w.vfwd, w.scal_first.fwd, w.scal_first.fwdPos, w.scal_first.bwd});
  }
  // advectVel itself
  check_disjoint({w.vfwd, w.vbwd, w.Uadv});
  // after the advection: the confinement's arrays and both places the velocity may sit in (3-D); 2-D has no scratch velocity.
  // centered / force are arguments the kernels do not read, and exempt
  if (is3d) check_disjoint({w.Uadv, w.curl, w.cnorm, w.Utmp});
  else check_disjoint({w.Uadv, w.curl, w.cnorm});
  if (proj == StepProj::jacobi) check_disjoint({w.div, w.pPrev, w.pDelta, w.norm});
  if (proj == StepProj::pcg && pcg_floats > 0) check_disjoint({w.div, w.pcg});
}

int main() {
  const int shapes2[][3] = {{1, 5, 7}, {1, 4, 6}, {1, 1, 1}}, shapes3[][3] = {{3, 5, 7}, {4, 6, 8}, {1, 5, 7}, {1, 1, 1}};
  int cases = 0;
  for (int C : {2, 3})
    for (int B : {1, 3})
      for (StepProj proj : {StepProj::convnet, StepProj::jacobi, StepProj::pcg, StepProj::unknown})
        for (int i = 0; i < (C == 2 ? 3 : 4); i++) {
          const int* d = C == 2 ? shapes2[i] : shapes3[i];
          const long long N = (long long)B * d[0] * d[1] * d[2];
          // a PCG workspace smaller than the step's other terms, one that sets the total, and an odd one
          for (long long pcg : {0ll, 3ll, 20 * N + 13})
            if (proj == StepProj::pcg || pcg == 0) { check_case(B, d[0], d[1], d[2], C, proj, pcg); cases++; }
        }
  std::printf("step workspace OK (%d cases)\n", cases);
  return 0;
}
