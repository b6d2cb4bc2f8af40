// A stand-alone host program over the workspace table of the step on batch items (tfl_simulate_step_items;
// fluidnet_amd/csrc/tfl_step_ws.hpp step_items_ws): the step's table with the PCG region sized for the batched solver. For
// B = 1, 2, 4, 32 at odd 2-D and 3-D sizes, 'mg' and 'none': (a) every region of the step's table sits where step_ws puts it --
// no offset moves, only the PCG region's length and the total grow --, and step_ws itself gives the totals of the size formula
// written out here; (b) the PCG region starts on 8 bytes behind the divergence, holds pcg_batched_ws(B, ...).total floats and
// ends inside the total; (c) the divergence, every region of the batched solver's table at its place inside the PCG region and
// the slack are written once into a buffer of exactly `total` floats (AddressSanitizer sees a region that leaves it, the marks
// see two that overlap); (d) a preconditioner that does not batch (batched_floats < 0) gives the step's own table. No GPU, no
// HIP call. Built and run by tests/test_datagen_batched_cpu.py:
//   g++ -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all step_items_ws_host.cpp
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../fluidnet_amd/csrc/tfl_pcg_ws.hpp"
#include "../fluidnet_amd/csrc/tfl_step_ws.hpp"

#define CHECK(c) do { if (!(c)) { std::fprintf(stderr, "%s:%d: CHECK(%s) failed (%s)\n", __FILE__, __LINE__, #c, g_case); std::exit(1); } } while (0)

using namespace tfl;

static char g_case[160];

static bool same(tfl::WsRegion a, tfl::WsRegion b) { return a.off == b.off && a.floats == b.floats; }

static void check_case(int B, int Z, int Y, int X, bool mg) {
  const bool is3d = Z > 1;
  const int C = is3d ? 3 : 2;
  std::snprintf(g_case, sizeof(g_case), "B %d, %d x %d x %d, mg %d", B, Z, Y, X, (int)mg);
  const long long N = (long long)B * Z * Y * X;
  const long long seq = pcg_ws(Z, Y, X, false, mg, is3d).total;
  const PcgBatchedWs bt = pcg_batched_ws(B, Z, Y, X, mg, is3d);
  const StepWs old = step_ws(B, Z, Y, X, C, StepProj::pcg, seq);
  const StepWs w = step_items_ws(B, Z, Y, X, C, StepProj::pcg, seq, bt.total);

  // (a) nothing of the step's table moves
  CHECK(same(w.vfwd, old.vfwd) && same(w.vbwd, old.vbwd) && same(w.Uadv, old.Uadv) && same(w.sout, old.sout));
  CHECK(same(w.scal.fwd, old.scal.fwd) && same(w.scal.bwd, old.scal.bwd) && same(w.scal.fwdPos, old.scal.fwdPos) && same(w.scal.bwdPos, old.scal.bwdPos));
  CHECK(same(w.scal_first.fwd, old.scal_first.fwd) && same(w.scal_first.bwd, old.scal_first.bwd) && same(w.scal_first.fwdPos, old.scal_first.fwdPos) &&
        same(w.scal_first.bwdPos, old.scal_first.bwdPos));
  CHECK(same(w.curl, old.curl) && same(w.cnorm, old.cnorm) && same(w.Utmp, old.Utmp) && same(w.centered, old.centered) && same(w.force, old.force));
  CHECK(same(w.div, old.div) && w.pcg.off == old.pcg.off && old.pcg.floats == seq);
  // ... and step_ws gives the total of the size formula it replaced
  long long need = (3 + 2 * C) * N;
  if (3 * C * N > need) need = 3 * C * N;
  if ((2 * C + 4) * N > need) need = (2 * C + 4) * N;
  long long need_old = need, need_new = need;
  if (N + 2 + seq > need_old) need_old = N + 2 + seq;
  if (N + 2 + bt.total > need_new) need_new = N + 2 + bt.total;
  CHECK(old.total == need_old + kStepWsSlack && w.total == need_new + kStepWsSlack);

  // (b) the PCG region: on 8 bytes behind the divergence, the batched table's size, inside the total
  CHECK(w.pcg.off % 2 == 0 && w.pcg.off >= w.div.off + w.div.floats && w.pcg.floats == bt.total);
  CHECK(w.pcg.off + w.pcg.floats + kStepWsSlack <= w.total);
  CHECK(bt.total >= B * seq && bt.stride % 2 == 0 && bt.states.off % 2 == 0);

  // (c) written once each into exactly `total` floats
  std::vector<float> ws(w.total, 0.0f);
  std::vector<unsigned char> mark(w.total, 0);
  auto touch = [&](long long off, long long floats) {
    CHECK(off >= 0 && floats >= 0 && off + floats <= w.total);
    for (long long e = 0; e < floats; e++) { ws[off + e] = 1.0f; CHECK(mark[off + e] == 0); mark[off + e] = 1; }
  };
  touch(w.div.off, w.div.floats);
  for (int b = 0; b < B; b++) touch(w.pcg.off + bt.items.off + b * bt.stride, bt.item.total);
  touch(w.pcg.off + bt.states.off, bt.states.floats);
  touch(w.pcg.off + bt.recs.off, bt.recs.floats);
  touch(w.pcg.off + bt.cc.off, bt.cc.floats);
  touch(w.pcg.off + bt.comps.off, bt.comps.floats);
  touch(w.total - kStepWsSlack, kStepWsSlack);

  // (d) a preconditioner that does not batch: the step's own table
  const StepWs q = step_items_ws(B, Z, Y, X, C, StepProj::pcg, seq, -1);
  CHECK(q.total == old.total && same(q.pcg, old.pcg));
  const StepWs j = step_items_ws(B, Z, Y, X, C, StepProj::jacobi, 0, -1), j0 = step_ws(B, Z, Y, X, C, StepProj::jacobi, 0);
  CHECK(j.total == j0.total && same(j.pPrev, j0.pPrev) && same(j.pDelta, j0.pDelta) && same(j.norm, j0.norm));
}

int main() {
  const int shapes[][3] = {{1, 9, 13}, {1, 16, 16}, {1, 32, 32}, {1, 128, 128}, {5, 6, 7}, {12, 16, 20}, {6, 8, 12}, {33, 17, 9}};
  for (const auto& s : shapes)
    for (int B : {1, 2, 4, 32})
      for (int mg = 0; mg < 2; mg++) check_case(B, s[0], s[1], s[2], mg != 0);
  std::printf("step items workspace OK\n");
  return 0;
}
