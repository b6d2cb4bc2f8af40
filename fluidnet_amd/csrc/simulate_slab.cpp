// simulate_slab.cpp -- the z-slab rank-step: tfl_simulate_step (simulate.cpp) on one slab of a grid cut along z, as one native
// call (tfl_simulate_step_slab), with the slab geometry, the neighbour messages, the reach checks, the stand-alone halo
// exchange (tfl_slab_exchange), the cut divergence norm and the rank-step as one HIP graph (tfl_slab_graph_*). Besides the
// operators it launches the plane kernels of its Jacobi projection and its halo bookkeeping (reach absmax / publication,
// message packing). What it shares with the un-cut step is tfl_step.hpp. Tested bit for bit against the un-cut step
// (tests/test_hip_simulate.py, tests/test_hip_slab_*.py).
#include "../../include/tfluids_hip.h"
#include "tfl_abi.hpp"
#include "tfl_host.hpp"
#include "tfl_ops.hpp"
#include "tfl_step.hpp"

#include <cstddef>
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <chrono>
#include <cstring>
#include <thread>
#include <string>

extern "C" {

// ================================================================================================================
// z-slab decomposition: tfl_simulate_step on one slab of a grid cut along z (include/tfluids_hip.h, "z-slab" section).
//
// Valid-plane bookkeeping. Write (a, b) for "planes [own_lo - a, own_hi + b)", clipped to the local array (at a domain
// end the slab simply ends there). With R = back-trace reach in cells (max|u_z|*dt < R) the per-phase z-dependencies are
//   3^3 min/max grid of rho  +-1      pass A of MacCormack  rho +-(R+1) incl. the min/max lookup, U +-(R+1)
//   pass B                   fwd +-R, U +-(R+1)             buoyancy  rho -1         curl  U -1..+2
//   confinement              curl -1, |curl| -2..+1         divergence  U +1 (flags +2)
//   3 conv layers            +-1 each                       velocity update  p -1
// so, working backwards from "owned planes exact":
//   project (0,0) <- conv3 (1,0) <- conv2 (2,1) <- conv1 (3,2) <- {p, div} (4,3)            [T1: p, T3: div]
//   divergence (0,0) <- confine (0,1) <- curl (2,2) <- buoyancy/gravity (3,4) <- {U_adv (3,4), rho (4,4)}   [T2]
//   pass B (0,0) <- pass A (R,R) <- min/max (2R,2R) <- {rho (2R+1,2R+1), U (max(R+1,2R), same): trace velocity R+1,
//                                                       advected field 2R}                    [T0: U; rho is still
//                                                                                             valid from T2]
// Local array ends are treated by the kernels as the domain's border shell (zeros); with halo >= max(4, 2R+1) no window
// above ever evaluates a tap there except through data that is exchanged instead (div, p).
// The other advection methods (one dependency cone per method) need no more: single-pass methods write (0,0)
// from s +-R and U (R,R); Manta maccormack pass A (R,R) reads s (2R,2R) and U (R,R+1), its velocity pass A U (2R,2R); their
// passes B (0,0) read fwd, s / U and flags +-R. Their density goes through the workspace (no in-place kernels) and its owned
// planes are copied back before T2, which carries every density channel.
//
// Every other projection net that is not a graph model (tog, yang, tfl_model_opts, the default topology on the
// shape-generic kernels): its cone (model_cone) replaces the conv rows above -- p and div travel with the net input's (lo, hi)
// planes, the halo is tfl_slab_halo_model, and the whole net runs as one stage under per-layer windows.
//
// Jacobi projection (simMethod = 'jacobi', state->model = NULL), the un-cut branch's order: setWallBcs on (0,1), setConstVals,
// divergence (0,0) -> div halos (J-1, J-1) [T3], then maxIter sweeps from p = 0, then velocity update (0,0) <- p (1,0).
// J = the stored halo depth (own_lo; the smaller of the two sides on a middle rank -- every rank must store the same depth).
// A sweep turns p valid on (d,d) into p valid on (d-1,d-1); p = 0 is valid on (J,J) at the start, so the first round needs no
// exchange. Rounds of J sweeps each end at (0,0) and refill (J,J) by a p exchange [T1]; the last round, r < J sweeps, ends at
// (1,0) or wider. Sweep n of a round of r (n = 1..r) computes the window (min(d-1, r-n+f), min(d-1, r-n)), f = 1 in the last
// round (the velocity update's plane below), 0 otherwise -- so a window never reaches the array end of a cut (d-1 < J). Per
// step: maxIter sweep launches and floor(maxIter / J) p exchanges of J planes a side, plus the div exchange.
namespace {

struct Halo { const tfl_tensor* t; int below, above; };   // planes of `t` refreshed below / above the owned range

struct Msg {                 // one neighbour exchange: buffers inside the workspace
  int tag, n;
  Halo f[10];                // T2: the advected U + up to 8 density channels
  float *send_lo, *recv_lo, *send_hi, *recv_hi;
  long long n_send_lo, n_recv_lo, n_send_hi, n_recv_hi;   // floats
};

struct SlabGeom {
  int Zl, o0, o1, R, H;
  int J;                     // the stored halo depth: planes between two p exchanges of the Jacobi projection
  bool lower, upper;
  long long yx, N;           // Y*X, B*Zl*Y*X
  int B;
  bool gen;                  // the model runs the shape-generic forward under per-layer windows
  tfl::ModelCone cone;       // its cone (s->model != NULL)
};

int slab_geom(tfl_ctx* c, const tfl_sim_state* s, const tfl_slab* sl, SlabGeom* g) {
  if (!s || !s->flags || !s->U || !sl) return TFL_EINVAL;
  if (s->n_density < 0 || s->n_density > 8) { if (c) c->err = "simulate_step_slab: 0 to 8 density channels"; return TFL_EINVAL; }
  g->Zl = s->flags->Z; g->B = s->flags->B;
  g->o0 = sl->own_lo; g->o1 = sl->own_hi;
  g->R = sl->reach > 0 ? sl->reach : 1;
  g->H = tfl_slab_halo(g->R);
  g->gen = false;
  g->cone = tfl::ModelCone{};
  g->cone.F = 1;
  // (a model without a cone -- graph models, 2-D -- keeps the plain halo here: the step's entry gate refuses it with its reason)
  if (s->model && tfl::model_cone(s->model, &g->cone)) {
    g->gen = g->cone.windowed;
    g->H = tfl_slab_halo_model(s->model, g->R);
    // pooling windows of the cut grid must be those of the un-cut grid: every cut, owned boundary and local depth on the
    // model's downsampling factor
    const int F = g->cone.F;
    if (F > 1 && (sl->z_first % F || g->o0 % F || g->o1 % F || g->Zl % F || sl->z_total % F)) {
      if (c) {
        char buf[240];
        snprintf(buf, sizeof(buf), "simulate_step_slab: the model pools by %d along z: z_first %d, owned planes [%d, %d), local depth %d "
                                   "and z_total %d must be multiples of %d", F, sl->z_first, g->o0, g->o1, g->Zl, sl->z_total, F);
        c->err = buf;
      }
      return TFL_EINVAL;
    }
  }
  g->yx = (long long)s->flags->Y * s->flags->X;
  g->N = (long long)g->B * g->Zl * g->yx;
  g->lower = sl->z_first + sl->own_lo > 0;
  g->upper = sl->z_first + sl->own_hi < sl->z_total;
  g->J = g->lower ? (g->upper ? std::min(g->o0, g->Zl - g->o1) : g->o0) : (g->upper ? g->Zl - g->o1 : 0);
  const bool ok = g->o0 >= 0 && g->o1 > g->o0 && g->o1 <= g->Zl && sl->z_first >= 0 && sl->z_first + g->Zl <= sl->z_total &&
                  (g->lower ? g->o0 >= g->H : (g->o0 == 0 && sl->z_first == 0)) &&
                  (g->upper ? g->Zl - g->o1 >= g->H : (g->o1 == g->Zl && sl->z_first + g->Zl == sl->z_total)) &&
                  ((!g->lower && !g->upper) || g->o1 - g->o0 >= g->H);
  if (!ok) {
    if (c) {
      char buf[240];
      snprintf(buf, sizeof(buf), "simulate_step_slab: inconsistent slab description (halo too thin, or owned range thinner than the halo: "
                                 "%d planes needed next to each neighbour, tfl_slab_halo_model)", g->H);
      c->err = buf;
    }
    return TFL_EINVAL;
  }
  return TFL_OK;
}

long long msg_floats(const SlabGeom& g, const Halo* f, int n, bool to_lower, bool send) {
  // to lower neighbour: I send what it needs ABOVE its range (my lowest `above` planes) and receive my `below` planes
  long long planes = 0;
  for (int i = 0; i < n; i++) {
    const int cnt = (to_lower == send) ? f[i].above : f[i].below;
    planes += (long long)f[i].t->B * f[i].t->C * cnt;
  }
  return planes * g.yx;
}

// carve the four buffers of each message out of `base`; returns the floats used
long long msg_layout(const SlabGeom& g, Msg* m, int count, float* base) {
  long long off = 0;
  auto take = [&](long long n) { float* p = base ? base + off : nullptr; off += (n + 3) & ~3ll; return p; };
  for (int i = 0; i < count; i++) {
    Msg& q = m[i];
    q.n_send_lo = g.lower ? msg_floats(g, q.f, q.n, true, true) : 0;
    q.n_recv_lo = g.lower ? msg_floats(g, q.f, q.n, true, false) : 0;
    q.n_send_hi = g.upper ? msg_floats(g, q.f, q.n, false, true) : 0;
    q.n_recv_hi = g.upper ? msg_floats(g, q.f, q.n, false, false) : 0;
    q.send_lo = take(q.n_send_lo); q.recv_lo = take(q.n_recv_lo); q.send_hi = take(q.n_send_hi); q.recv_hi = take(q.n_recv_hi);
  }
  return off;
}

// the planes of one message that leave (unpack = false: owned planes -> send buffers) or arrive (unpack = true: receive
// buffers -> halo planes), BOTH neighbours in one launch
void pack_msg(tfl_ctx* c, const SlabGeom& g, const Msg& q, bool unpack) {
  float* ptrs[20]; float* bufs[20]; int rows[20], zlo[20], np[20];
  int n = 0;
  for (int side = 0; side < 2; side++) {
    const bool lower = side == 0;
    if (lower ? !g.lower : !g.upper) continue;
    float* buf = unpack ? (lower ? q.recv_lo : q.recv_hi) : (lower ? q.send_lo : q.send_hi);
    for (int i = 0; i < q.n; i++) {
      const Halo& h = q.f[i];
      ptrs[n] = h.t->data; rows[n] = h.t->B * h.t->C;
      if (!unpack) { np[n] = lower ? h.above : h.below; zlo[n] = lower ? g.o0 : g.o1 - h.below; }     // owned planes out
      else { np[n] = lower ? h.below : h.above; zlo[n] = lower ? g.o0 - h.below : g.o1; }              // halo planes in
      bufs[n] = buf;
      buf += (long long)rows[n] * np[n] * g.yx;
      n++;
    }
  }
  for (int i = 0; i < n; i += 8)        // (a launch takes 8 fields: more only with several density channels)
    tfl::pack_planes(c->stream, std::min(8, n - i), ptrs + i, rows + i, zlo + i, np + i, g.yx * g.Zl, g.yx, nullptr, unpack ? 1 : 0, bufs + i);
}

// the same planes as contiguous runs of the fields themselves, one per (batch item, channel): what exchange_start_v moves
int msg_chunks(const SlabGeom& g, const Msg& q, bool lower, bool send, tfl_comm_chunk* out) {
  if (lower ? !g.lower : !g.upper) return 0;
  int n = 0;
  for (int i = 0; i < q.n; i++) {
    const Halo& h = q.f[i];
    int np, zlo;
    if (send) { np = lower ? h.above : h.below; zlo = lower ? g.o0 : g.o1 - h.below; }      // owned planes out
    else { np = lower ? h.below : h.above; zlo = lower ? g.o0 - h.below : g.o1; }           // halo planes in
    for (int row = 0; row < h.t->B * h.t->C; row++) {
      out[n].ptr = h.t->data + ((long long)row * g.Zl + zlo) * g.yx;
      out[n].n = (long long)np * g.yx;
      n++;
    }
  }
  return n;
}
constexpr int kMaxChunks = 64;     // per neighbour and message: (B * C) of every field of the message

// the optional in-place transport, read only when the host's struct is large enough to hold it (tfl_comm::size)
static inline decltype(tfl_comm::exchange_start_v) start_v_of(const tfl_comm* comm) {
  return comm->size >= (int32_t)(offsetof(tfl_comm, exchange_start_v) + sizeof(comm->exchange_start_v)) ? comm->exchange_start_v : nullptr;
}

int msg_start(tfl_ctx* c, const SlabGeom& g, const tfl_comm* comm, const Msg& q) {
  if ((!g.lower && !g.upper) || q.n == 0) return TFL_OK;
  if (auto start_v = start_v_of(comm)) {
    int rows = 0;
    for (int i = 0; i < q.n; i++) rows += q.f[i].t->B * q.f[i].t->C;
    if (q.n > 0 && rows <= kMaxChunks) {
      tfl_comm_chunk slo[kMaxChunks], rlo[kMaxChunks], shi[kMaxChunks], rhi[kMaxChunks];
      const int n_lo = msg_chunks(g, q, true, true, slo), n_hi = msg_chunks(g, q, false, true, shi);
      msg_chunks(g, q, true, false, rlo); msg_chunks(g, q, false, false, rhi);
      if (start_v(comm->user, q.tag, n_lo, slo, rlo, n_hi, shi, rhi) != 0) { c->err = "simulate_step_slab: comm callback failed (exchange_start_v)"; return TFL_EINVAL; }
      return TFL_OK;
    }
  }
  pack_msg(c, g, q, false);
  if (comm->exchange_start(comm->user, q.tag, q.send_lo, q.n_send_lo, q.recv_lo, q.n_recv_lo, q.send_hi, q.n_send_hi,
                           q.recv_hi, q.n_recv_hi) != 0) { c->err = "simulate_step_slab: comm callback failed (exchange_start)"; return TFL_EINVAL; }
  return TFL_OK;
}
int msg_finish(tfl_ctx* c, const SlabGeom& g, const tfl_comm* comm, const Msg& q) {
  if ((!g.lower && !g.upper) || q.n == 0) return TFL_OK;
  if (comm->exchange_wait(comm->user, q.tag) != 0) { c->err = "simulate_step_slab: comm callback failed (exchange_wait)"; return TFL_EINVAL; }
  int rows = 0;
  for (int i = 0; i < q.n; i++) rows += q.f[i].t->B * q.f[i].t->C;
  if (start_v_of(comm) && q.n > 0 && rows <= kMaxChunks) return TFL_OK;      // delivered in place
  pack_msg(c, g, q, true);
  return TFL_OK;
}

// the messages of a step (slot 1: Jacobi only); for the layout alone any tensors with the B and C of `Uadv` / `div` will do
void slab_messages(const SlabGeom& g, const tfl_sim_state* s, const tfl_tensor* Uadv, const tfl_tensor* div, Msg m[4]) {
  const int rr = 2 * g.R + 1;
  // U feeds pass A twice: as the trace velocity (window (R,R) reads it out to +-(R+1)) and as the ADVECTED field of the
  // velocity's self-advection, sampled at positions up to R cells away from the window: +-2R. The projection only
  // rewrites the owned planes, so everything out to max(R+1, 2R) must be refreshed (R = 1: 2 planes either way).
  const int ur = std::max(g.R + 1, 2 * g.R);
  // U and p leave together at the end of a step (ONE message, one packing launch) and are consumed at the start of the
  // next one: nothing writes either field's halo planes in between (p is only read by the first conv layer)
  // (the net reads its input on the cone of the owned planes: (4, 3) for the default topology, (in_lo, in_hi) of the model_cone
  // walk for every other net)
  const int nlo = g.gen ? g.cone.in_lo : 4, nhi = g.gen ? g.cone.in_hi : 3;
  m[0].tag = 0; m[0].n = 2; m[0].f[0] = Halo{s->U, ur, ur}; m[0].f[1] = Halo{s->p, nlo, nhi};
  m[1].tag = 1; m[1].n = 0;
  if (!s->model) { m[1].n = 1; m[1].f[0] = Halo{s->p, g.J, g.J}; }       // Jacobi: p between two rounds of sweeps (either buffer)
  m[2].tag = 2; m[2].n = 1 + s->n_density; m[2].f[0] = Halo{Uadv, 3, 4};
  for (int i = 0; i < s->n_density; i++) m[2].f[1 + i] = Halo{s->density[i], rr > 4 ? rr : 4, rr > 4 ? rr : 4};
  m[3].tag = 3; m[3].n = 1; m[3].f[0] = Halo{div, nlo, nhi};
  // a net whose input holds UDiv also reads SetWallBcs(U) there: tfl_model_begin has left it in U's owned planes
  if (g.gen && g.cone.reads_U) { m[3].n = 2; m[3].f[1] = Halo{s->U, nlo, nhi}; }
  if (!s->model) m[3].f[0] = Halo{div, g.J > 1 ? g.J - 1 : 0, g.J > 1 ? g.J - 1 : 0};     // what the first round of sweeps reads
}

constexpr int kReachPrimed = 0x100;  // tfl_slab::in_flight, beside the message bits: this run has reset the context's sticky reach word
constexpr int kReachFlags = 8;       // check_reach = 2 resolves reaches 1 .. 8 (a 16-plane slab can hold the halo of 7)
struct SlabWs { float* msg; double* stats; float* compute; long long compute_floats; };

// workspace = [message buffers][stats: 2*B doubles][compute region]
long long slab_ws(const SlabGeom& g, const tfl_sim_state* s, float* ws, SlabWs* out) {
  Msg m[4];
  slab_messages(g, s, s->U, s->flags, m);
  long long off = msg_layout(g, m, 4, nullptr);
  off = (off + 3) & ~3ll;
  const long long stats_off = off;
  off += 4ll * g.B + 2ll * (kReachFlags + 1);         // 2*B doubles + the reach / range flags of check_reach = 2 (behind the stats)
  off = (off + 3) & ~3ll;
  long long model = s->model ? tfl_model_workspace_floats(s->model, g.B, g.Zl, s->flags->Y, s->flags->X) : 0;
  const long long comp = std::max<long long>(13 * g.N, model) + 4;
  if (out) { out->msg = ws; out->stats = ws ? (double*)(ws + stats_off) : nullptr; out->compute = ws ? ws + off : nullptr; out->compute_floats = comp; }
  return off + comp;
}

// How the rank-step runs an advection method (the dependency cones). maccormackOurs advects in place
// through the pair kernels; every other method goes through tfl_advectScalar / tfl_advectVel, the density into the workspace
// first. Two-pass: a pass A on (R, R) before the pass that writes the owned planes. rk2Ours / rk3Ours advect the velocity
// with maccormackOurs (tfluids.cc:799-802), so only their scalar advection is single-pass.
struct AdvPlan { bool known, ours, scalar2, vel2; };
AdvPlan adv_plan(const char* m) {
  static const char* names[] = {"euler", "maccormack", "eulerOurs", "rk2Ours", "rk3Ours", "maccormackOurs"};
  int k = -1;
  for (int i = 0; i < 6; i++) if (std::strcmp(m, names[i]) == 0) k = i;
  return AdvPlan{k >= 0, k == 5, k == 1 || k == 5, k == 1 || k >= 3};
}

// owned planes [o0, o1) of `src` into `dst` (two [B][1][Zl][Y][X] fields): the advected density out of the workspace
int copy_owned(tfl_ctx* c, const SlabGeom& g, const tfl_tensor* dst, const tfl_tensor* src) {
  const long long off = (long long)g.o0 * g.yx, n = (long long)(g.o1 - g.o0) * g.yx;
  for (int b = 0; b < g.B; b++) {
    const long long row = (long long)b * g.Zl * g.yx + off;
    if (hipMemcpyAsync(dst->data + row, src->data + row, sizeof(float) * (size_t)n, hipMemcpyDeviceToDevice, c->stream) != hipSuccess) {
      (void)hipGetLastError(); c->err = "simulate_step_slab: hipMemcpyAsync failed"; return TFL_EHIP;
    }
  }
  return TFL_OK;
}

struct Win { int a, b; };
Win ext(const SlabGeom& g, int below, int above) {
  Win w;
  const int widen = tfl::sw::num(tfl::Sw::SLAB_WIDEN, 0);   // development aid
  below += widen; above += widen; w.a = g.o0 - below < 0 ? 0 : g.o0 - below; w.b = g.o1 + above > g.Zl ? g.Zl : g.o1 + above; return w;
}

// the pinned publication count has reached `target` (wrap-safe); spins without an API call, gives the core away after a while,
// and gives up after 30 s (a dead device must not hang the host here: the next HIP call reports it)
void reach_wait(tfl_ctx* c, unsigned target) {
  volatile unsigned* tick = reinterpret_cast<volatile unsigned*>(c->h_reach) + 1;
  if ((int)(*tick - target) >= 0) return;
  const auto t0 = std::chrono::steady_clock::now();
  for (unsigned long i = 0; (int)(*tick - target) < 0; i++) {
    if (i < 4096) { __builtin_ia32_pause(); continue; }
    std::this_thread::yield();
    if ((i & 1023) == 0 && std::chrono::steady_clock::now() - t0 > std::chrono::seconds(30)) return;
  }
}
// check_reach = 1, host side: has a step that the device has certainly started (two calls back) -- or any later one it has got
// to since -- found max|u_z| dt >= R? Waits only when the host is more than two steps ahead of the device.
bool reach_violated(tfl_ctx* c, float dt, int R, char* msg, size_t msg_len) {
  if (c->reach_hist[0]) reach_wait(c, c->reach_hist[0]);
  const float v = *(volatile float*)c->h_reach;
  if (!(v * dt >= (float)R)) return false;
  snprintf(msg, msg_len, "simulate_step_slab: max|u_z|*dt = %.3f cells reached the slab's back-trace reach %d (found up to three steps after the fact: "
                         "check_reach = 2 refuses such a step BEFORE it runs)", v * dt, R);
  // acknowledged: the sticky maximum starts again (the state is past saving; a host that carries on gets the next report afresh)
  c->h_reach[0] = 0.0f;
  (void)hipMemsetAsync(c->d_reach, 0, sizeof(float), c->stream);
  return true;
}
// ... device side: the sticky word and the publication count reach the host through the step's LAST kernel (k_project writes
// them into the mapped pinned mirror: Ask::reach_via_project) -- not through hipMemcpyAsync (a 4-byte D2H copy on the stream makes
// the HOST wait until the stream has drained on this stack, tools/ubench/host_costs.hip) and not behind an event (4 us of
// device time per hipEventRecord): the host counts the publishing launches it has enqueued (tfl_model_finish) and keeps the
// count as it stood at the end of the last two steps
void reach_mark(tfl_ctx* c) {      // at the end of a step whose projection published (eager, or behind the launch of a recorded step)
  c->reach_hist[0] = c->reach_hist[1]; c->reach_hist[1] = c->reach_issued;
}
// the first step of a run on this context (the host initialised in_flight to 0): the sticky maximum of whatever ran on the
// context before must not speak for this run
void reach_prime(tfl_ctx* c, tfl_slab* sl) {
  c->h_reach[0] = 0.0f;
  (void)hipMemsetAsync(c->d_reach, 0, sizeof(float), c->stream);
  sl->in_flight |= kReachPrimed;
}
void reach_quiesce(tfl_ctx* c) {   // every publication enqueued so far has landed
  if (c->reach_issued) reach_wait(c, c->reach_issued);
}

// the U / p messages (T0, T1) an earlier eager step left in flight are finished (a failed one is not waited for again)
int finish_in_flight(tfl_ctx* c, const SlabGeom& g, const tfl_comm* comm, const Msg* m, tfl_slab* sl) {
  for (int t = 0; t < 2; t++)
    if (sl->in_flight & (1 << t)) { const int rc = msg_finish(c, g, comm, m[t]); sl->in_flight &= ~(1 << t); if (rc) return rc; }
  return TFL_OK;
}

}  // namespace

int32_t tfl_slab_halo(int32_t reach) {
  const int r = reach > 0 ? reach : 1;
  return 2 * r + 1 > 4 ? 2 * r + 1 : 4;
}

int32_t tfl_slab_halo_model(const tfl_model* model, int32_t reach) {
  const int h = tfl_slab_halo(reach);
  if (!model) return h;
  tfl::ModelCone cone;
  if (!tfl::model_cone(model, &cone)) return TFL_EUNSUPPORTED;
  const int need = cone.fused ? h : std::max(h, cone.depth);      // (the fused default topology: its (4, 3) cone, always <= h)
  return (need + cone.F - 1) / cone.F * cone.F;
}

int64_t tfl_simulate_slab_workspace_floats(tfl_ctx* c, const tfl_sim_params* prm, const tfl_sim_state* s, const tfl_slab* sl) {
  (void)prm;
  SlabGeom g;
  if (slab_geom(c, s, sl, &g) != TFL_OK) return 0;
  return slab_ws(g, s, nullptr, nullptr);
}

int tfl_slab_drain(tfl_ctx* c, const tfl_sim_state* s, tfl_slab* sl, const tfl_comm* comm, float* ws, int64_t ws_floats) {
  if (!c) return TFL_EINVAL;
  if (!s || !sl || !comm || !ws) { c->err = "slab_drain: null state, slab, comm or workspace"; return TFL_EINVAL; }
  SlabGeom g;
  int rc = slab_geom(c, s, sl, &g);
  if (rc) return rc;
  // (the step's own test: a workspace the step would refuse cannot hold its messages)
  if (((uintptr_t)ws & 15) != 0 || ws_floats < slab_ws(g, s, nullptr, nullptr)) { c->err = "slab_drain: workspace too small or misaligned"; return TFL_EINVAL; }
  Msg m[4];
  slab_messages(g, s, s->U, s->flags, m);
  msg_layout(g, m, 4, ws);
  return finish_in_flight(c, g, comm, m, sl);
}

// The divergence norm of the whole grid from its slabs (include/tfluids_hip.h; divnorm.hip). Bit-equal to the un-cut
// tfl_velocityDivergenceNorm: each plane's sum is formed by the rank that owns it, by the un-cut call's kernel in the un-cut
// call's order (it depends on (Y, X) only), the all-reduce adds zeros to it, and stage 2 adds the planes as the un-cut call does.
int tfl_slab_divergence_norm(tfl_ctx* c, const tfl_sim_state* s, tfl_slab* sl, const tfl_comm* comm, float* ws, int64_t ws_floats,
                             double* norm) {
  if (!c) return TFL_EINVAL;
  if (!s || !sl || !ws || !norm || ((uintptr_t)norm & 7) != 0) { c->err = "slab_divergence_norm: null state, slab, workspace or norm"; return TFL_EINVAL; }
  SlabGeom g;
  TRY(slab_geom(c, s, sl, &g));
  if (!sizes_of(s).is3d) { c->err = "slab_divergence_norm: 2-D grids have no z to cut (run replicas)"; return TFL_EUNSUPPORTED; }
  const bool multi = g.lower || g.upper;
  if (multi && (!comm || comm->size < (int32_t)(offsetof(tfl_comm, allreduce_sum) + sizeof(comm->allreduce_sum)) ||
                !comm->exchange_wait || !comm->allreduce_sum)) {
    c->err = "slab_divergence_norm: tfl_comm is null, has no size or lacks a required callback";
    return TFL_EINVAL;
  }
  if (((uintptr_t)ws & 15) != 0 || ws_floats < slab_ws(g, s, nullptr, nullptr)) { c->err = "slab_divergence_norm: workspace too small or misaligned"; return TFL_EINVAL; }
  SlabWs W;
  slab_ws(g, s, ws, &W);
  // the plane sums live in the compute region (13 fields of the local array or the model's workspace: dead between steps)
  const long long n_sums = (long long)g.B * sl->z_total;
  if (2 * n_sums > W.compute_floats) { c->err = "slab_divergence_norm: the plane sums (B * z_total doubles) do not fit the workspace's compute region"; return TFL_EINVAL; }
  Msg m[4];
  slab_messages(g, s, s->U, s->flags, m);
  msg_layout(g, m, 4, W.msg);
  TRY(finish_in_flight(c, g, comm, m, sl));          // U on the plane above the owned range
  double* sums = reinterpret_cast<double*>(W.compute);
  if (hipMemsetAsync(sums, 0, sizeof(double) * (size_t)n_sums, c->stream) != hipSuccess) {
    (void)hipGetLastError(); c->err = "slab_divergence_norm: hipMemsetAsync failed"; return TFL_EHIP;
  }
  tfl::Scope sc;
  sc.win = tfl::ZWin{g.o0, g.o1, 0, 0}; sc.origin = tfl::ZOrigin{sl->z_first, sl->z_total};
  tfl::divergence_norm_planes(c->stream, sc, true, g.B, g.Zl, s->flags->Y, s->flags->X, s->U->data, s->flags->data, sums, sl->z_total,
                              sl->z_first);
  if (multi && comm->allreduce_sum(comm->user, sums, n_sums) != 0) { c->err = "slab_divergence_norm: comm callback failed (allreduce_sum)"; return TFL_EINVAL; }
  tfl::divergence_norm_finish(c->stream, g.B, sl->z_total, sums, norm);
  if (hipGetLastError() != hipSuccess) { c->err = "slab_divergence_norm: a launch failed"; return TFL_EHIP; }
  return TFL_OK;
}

namespace {

// One rank-step, phase by phase. The phases share the call's arguments, the slab's geometry, the workspace views and messages,
// and what one phase hands to the next (which pairs pass B applied, where the velocity lives).
struct SlabStep {
  tfl_ctx* c; const tfl_sim_params* prm; const tfl_sim_state* s; tfl_slab* sl; const tfl_comm* comm;
  float* ws; int64_t ws_floats;
  bool capturing;                      // tfl_slab_graph_create is recording the step on the context's stream: no host waits, no host reads
  SlabGeom g; SlabWs W; Msg m[4];
  const char* method; AdvPlan ap;
  bool multi, jac, ovl;                // a slab with neighbours; the Jacobi projection; boundary strips first (tfl_slab::overlap)
  bool buoyant, vort, vfused;
  const tfl_tensor* rho;               // density channel 0 (null without density)
  // compute region: scalar temps [fwd N][fwdPos 3N][bwdPos 3N] | velocity temps [vfwd 3N][Uadv 3N]; the vorticity temps
  // and the model workspace re-use the region once the advection is done (Uadv lives until addBuoyancy)
  tfl_tensor fwd, fwdPos, bwdPos, vfwd, Uadv, curl, cnorm, div, Utmp;
  bool rho_done = true, Uadv_done = true;  // pass B applied the setConstVals pair of density channel 0 / of the advected U
  unsigned extra_done = 0;                 // ... of density channels 1.. (bit i)
  bool paired = false;                 // both advections' passes run as pairs (advect_pair3.hip)
  bool U_folded = false;               // the last force applied the U pair of the second setConstVals
  bool reach_via_project = false;      // the projection kernel of this step publishes the reach word (check_reach = 1)
  const tfl_tensor* cur = nullptr;     // where the velocity of the step currently lives

  int validate();                      // the refusals that come before anything is enqueued, then the views and messages
  int gates();                         // reach checks (check_reach 1 / 2), the fp16 range gate, the previous step's U / p halos
  int advect();                        // passes A, passes B under message T2, the first setConstVals
  int forces();                        // buoyancy, gravity, confinement; Jacobi's setWallBcs, the second setConstVals
  int project_jacobi();                // divergence under T3, the rounds of sweeps and p exchanges, velocity update
  int project_net();                   // tfl_model_begin under T3, input statistics, the conv stages, the projection
  int end_step();                      // the next step's U / p halos leave (message T0)

  tfl_tensor view(float* base, int C) const { tfl_tensor t = *s->flags; t.data = base; t.C = C; return t; }
  // The scope of one operator call: stage mask `mask` on the planes [a0, a1) and [b0, b1) of the local array, which sits at
  // z_first of the whole grid; dx is the whole grid's, the advect mode the context's.
  tfl::Scope planes(int mask, int a0, int a1, int b0, int b1) const {
    tfl::Scope sc;
    sc.win = tfl::ZWin{a0, a1, b0, b1}; sc.origin = tfl::ZOrigin{sl->z_first, sl->z_total}; sc.stages = mask;
    sc.advect_fast = c->advect_fast;
    sc.dx_cells = std::max(std::max(s->flags->X, s->flags->Y), sl->z_total);   // tfluids.getDx of the WHOLE grid
    return sc;
  }
  // ... on the planes (below, above) around the owned ones
  tfl::Scope stage(int mask, int below, int above) const { const Win w = ext(g, below, above); return planes(mask, w.a, w.b, 0, 0); }
  using Op = int (SlabStep::*)(const tfl::Scope&);
  int run_then_send(int mask, int k, const Msg& q, Op op);
  // (a: what the call is asked, step_ask; null: nothing)
  int adv_scalar(const tfl::Scope& sc, const tfl_tensor* d, const tfl_tensor* dst, tfl::Ask* a = nullptr) {
    tfl::Ask none = step_ask(nullptr);
    return tfl::advectScalar(c, prm->dt, d, s->U, s->flags, &fwd, &fwd, 1, method, &fwdPos, &bwdPos, 1, 0, prm->maccormackStrength, dst,
                             sc, a ? *a : none);
  }
  int adv_vel(const tfl::Scope& sc, tfl::Ask* a = nullptr) {
    tfl::Ask none = step_ask(nullptr);
    return tfl::advectVel(c, prm->dt, s->U, s->flags, &vfwd, &vfwd, 1, method, 1, prm->maccormackStrength, &Uadv, sc, a ? *a : none);
  }
  int adv_pair(const tfl::Scope& sc, bool with_folds);
  int pass_b(const tfl::Scope& sc);
  int model_begin(const tfl::Scope& sc) {
    tfl::Ask a = step_ask(nullptr);
    return tfl::model_begin(c, s->model, s->U, s->flags, s->U, W.compute, ws_floats - (W.compute - ws), g.o0, g.o1, W.stats, sc, a);
  }
};

// `op` on the owned planes under stage mask `mask`, then message `q` starts. Overlapped: `op` on the boundary strips (k planes
// next to each neighbour) first, then the message starts and `op` runs on the interior while it travels.
int SlabStep::run_then_send(int mask, int k, const Msg& q, Op op) {
  const int a1 = g.lower ? std::min(g.o0 + k, g.o1) : g.o0, b0 = g.upper ? std::max(g.o1 - k, a1) : g.o1;   // strips [o0, a1), [b0, o1)
  if (!ovl || (a1 == g.o0 && b0 == g.o1) || b0 == a1) {
    TRY((this->*op)(stage(mask, 0, 0)));
    return msg_start(c, g, comm, q);
  }
  TRY((this->*op)(planes(mask, g.o0, a1, b0, g.o1)));
  TRY(msg_start(c, g, comm, q));
  return (this->*op)(planes(mask, a1, b0, 0, 0));
}

int SlabStep::validate() {
  auto bad = [&](const char* why) { c->err = std::string("simulate_step_slab: ") + why; return TFL_EUNSUPPORTED; };
  if (tfl::model_is_graph(s->model)) return bad("banked, batch-norm and max-pool models run un-sharded only (tfl_simulate_step)");
  TRY(slab_geom(c, s, sl, &g));
  multi = g.lower || g.upper;
  if (multi && (!comm || comm->size < (int32_t)(offsetof(tfl_comm, allreduce_sum) + sizeof(comm->allreduce_sum)) ||
                !comm->exchange_start || !comm->exchange_wait || !comm->allreduce_sum)) {
    c->err = "simulate_step_slab: tfl_comm is null, has no size (ABI 3: size = sizeof(tfl_comm)) or lacks a required callback";
    return TFL_EINVAL;
  }
  if (!sizes_of(s).is3d) return bad("2-D grids have no z to cut (run replicas)");
  method = (prm->advectionMethod && prm->advectionMethod[0]) ? prm->advectionMethod : "maccormackOurs";
  ap = adv_plan(method);
  if (!ap.known) { c->err = std::string("simulate_step_slab: unknown advection method '") + method + "'"; return TFL_EINVAL; }
  const std::string sm = method_of(prm);
  if (sm == "pcg")
    return bad("the PCG projection cannot be cut along z: its dot products need an all-reduce per iteration and its IC(0) "
               "preconditioner is a lexicographic wavefront over the whole grid (use simMethod 'jacobi' or 'convnet')");
  jac = sm == "jacobi";
  if (jac && s->model) return bad("the Jacobi projection takes no model (state->model = NULL: the workspace layout follows it)");
  if (!jac && (sm != "convnet" || !s->model)) return bad("only the ConvNet projection (with a model) or 'jacobi' (without one)");
  if (jac && multi && g.o1 - g.o0 < g.J) return bad("Jacobi: the owned range is thinner than the halo depth it sends");
  if (!ws || ((uintptr_t)ws & 15) != 0 || ws_floats < slab_ws(g, s, nullptr, nullptr)) { c->err = "simulate_step_slab: workspace too small or misaligned"; return TFL_EINVAL; }
  const long long N = g.N;
  slab_ws(g, s, ws, &W);
  float* cw = W.compute;
  fwd = view(cw, 1); fwdPos = view(cw + N, 3); bwdPos = view(cw + 4 * N, 3); vfwd = view(cw + 7 * N, 3); Uadv = view(cw + 10 * N, 3);
  curl = view(cw, 3); cnorm = view(cw + 3 * N, 1);
  div = view(jac ? cw : tfl_model_div(s->model, g.B, g.Zl, s->flags->Y, s->flags->X, cw), 1);
  Utmp = view(cw + 4 * N, 3);          // the scalar advection's bwdPos planes, dead once the advection is done
  slab_messages(g, s, &Uadv, &div, m);
  msg_layout(g, m, 4, W.msg);
  ovl = sl->overlap && multi;
  rho = s->n_density > 0 ? s->density[0] : nullptr;
  buoyant = s->n_density > 0 && prm->buoyancyScale > 0.0;
  // as tfl_simulate_step: the fused vorticity confinement delivers into U, so buoyancy / gravity work on a scratch velocity
  vort = prm->vorticityConfinementAmp > 0.0;
  vfused = vort && tfl::vorticity_confinement_fused_ok(true, g.Zl, s->flags->Y, s->flags->X);
  return TFL_OK;
}

int SlabStep::gates() {
  // ---- reach check of the PREVIOUS step's velocity (no host sync: the word was copied back behind that step) ---------
  if (sl->check_reach == 1 && !capturing) {  // (a captured step: tfl_slab_graph_step makes both checks before it launches)
    char buf[256];
    if (reach_violated(c, prm->dt, g.R, buf, sizeof(buf))) {
      // the neighbours' matching receives of the U / p messages are already posted: finish ours before giving up
      if (multi) (void)finish_in_flight(c, g, comm, m, sl);
      c->err = buf;
      return TFL_EINVAL;
    }
  }
  // The fp16 range gate of tfl_simulate_step -- only where refusing cannot strand a neighbour: a slab WITHOUT
  // neighbours, or (below) collectively under check_reach = 2. A rank that refused on its own word would leave the others
  // waiting for its halos; the host of a cut run polls tfl_model_range_flag / tfl_model_range_errors and stops every rank.
  if (!capturing && !multi && s->model && tfl_model_range_flag(c, s->model) > 0) return range_refusal(c, "simulate_step_slab");
  TRY(finish_in_flight(c, g, comm, m, sl));      // U and p halos
  // (the state a run starts from has been through no projection of ours)
  if (sl->check_reach == 1 && !(sl->in_flight & kReachPrimed)) { reach_prime(c, sl); c->reach_folded = false; }
  // mode 1, from the second step on: the projection kernel of the step before has folded max |u_z| of the planes it wrote -- this
  // rank's OWNED planes; the halo planes are their owners' to report -- into the sticky word (k_project_v4, reach_acc): no launch
  // of our own (round 6: k_absmax was 5-6 us of a 0.1 ms rank-step). Mode 2 needs THIS step's exact maximum and keeps it.
  const bool reach_known = sl->check_reach == 1 && c->reach_folded;
  c->reach_folded = false;
  if (sl->check_reach && !reach_known) {
    for (int b = 0; b < g.B; b++)                                                                            // u_z of every batch item
      tfl::absmax(c->stream, (long long)g.Zl * g.yx, s->U->data + (3ll * b + 2) * g.Zl * g.yx, c->d_reach,
                  sl->check_reach == 2 && b == 0);      // (mode 1: a sticky maximum over the steps, see tfl_ctx.hpp)
  }
  if (sl->check_reach == 2) {
    // "exact" (round 6): the reach THIS step needs, agreed by all ranks, before anything is written. One-hot flags
    // (max|u_z| dt >= r, r = 1 .. 8) so that the transport's SUM all-reduce can combine them; one host synchronisation.
    if (capturing) { c->err = "simulate_step_slab: check_reach = 2 synchronises with the host and cannot be recorded into a graph"; return TFL_EUNSUPPORTED; }
    if (!c->h_reach_flags && hipHostMalloc((void**)&c->h_reach_flags, sizeof(double) * (kReachFlags + 1), hipHostMallocDefault) != hipSuccess) {
      c->h_reach_flags = nullptr; c->err = "simulate_step_slab: hipHostMalloc failed"; return TFL_EHIP;
    }
    double* d_flags = W.stats + 2 * g.B;
    tfl::reach_flags(c->stream, c->d_reach, prm->dt, kReachFlags, d_flags, tfl::model_range_counter(s->model));
    // (without a model there is no range word: the Jacobi step all-reduces the reach flags alone)
    if (multi && comm->allreduce_sum(comm->user, d_flags, kReachFlags + (s->model ? 1 : 0)) != 0) { c->err = "simulate_step_slab: comm callback failed (allreduce_sum, reach)"; return TFL_EINVAL; }
    if (hipMemcpyAsync(c->h_reach_flags, d_flags, sizeof(double) * (kReachFlags + 1), hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
        hipStreamSynchronize(c->stream) != hipSuccess) { c->err = "simulate_step_slab: reading the reach flags failed"; (void)hipGetLastError(); return TFL_EHIP; }
    // some rank's conv stack left the fp16 range: EVERY rank refuses this step
    if (c->h_reach_flags[kReachFlags] > 0.0) return range_refusal(c, "simulate_step_slab", true);
    int need = 1;
    for (int r = 0; r < kReachFlags; r++) if (c->h_reach_flags[r] > 0.0) need = r + 2;
    if (need > g.R) {
      char buf[200];
      snprintf(buf, sizeof(buf), "simulate_step_slab: this step's back-traces reach %d cells along z%s, the slab is laid out for %d; nothing has been written",
               need, need > kReachFlags ? " or more" : "", g.R);
      c->err = buf; c->needed_reach = need;
      return TFL_EREACH;
    }
  } else if (sl->check_reach && jac) {
    // no projection kernel to ride on: the word k_absmax has just folded goes to the pinned mirror by a launch of its own
    tfl::reach_publish(c->stream, c->d_reach, c->d_reach_host, c->d_reach_tick);
    c->reach_issued++;
  } else if (sl->check_reach) {
    reach_via_project = true;              // the projection kernel of THIS step publishes the word
  }
  return TFL_OK;
}

// Round 6: the two advections' passes as PAIRS -- passes A in one launch, passes B in one launch (advect_pair3.hip; they are
// independent here: the slab step does not fold the buoyancy force into pass B). TFL_EUNSUPPORTED = the shape is not the pair
// kernels': the four launches as before.
int SlabStep::adv_pair(const tfl::Scope& sc, bool with_folds) {
  const tfl::BcFoldArg fs = with_folds ? fold_arg(s->densityBC[0]) : tfl::no_fold(), fv = with_folds ? fold_arg(s->UBC) : tfl::no_fold();
  const int r = tfl::advect_pair(c, prm->dt, prm->maccormackStrength, rho, s->U, s->flags, &fwd, &fwdPos, rho, &vfwd, &Uadv, fs, fv, sc);
  if (r == TFL_OK && with_folds) { rho_done = rho_done && fs.dev != nullptr; Uadv_done = Uadv_done && fv.dev != nullptr; }
  return r;
}

// the passes B of both operators on the window of `sc` (other methods: the velocity's). They apply the pairs of the
// setConstVals that follows on the planes they write -- the owned ones, which is what message T2 carries to the neighbours'
// halos (step_ask)
int SlabStep::pass_b(const tfl::Scope& sc) {
  if (ap.ours && paired) { const int r = adv_pair(sc, true); if (r != TFL_EUNSUPPORTED) return r; paired = false; }
  if (ap.ours && rho) {
    tfl::Ask a = step_ask(s->densityBC[0]);
    const int r = adv_scalar(sc, rho, rho, &a);
    rho_done = a.fold.bc_took && rho_done;
    if (r) return r;
  }
  tfl::Ask a = step_ask(s->UBC);
  const int r = adv_vel(sc, &a);
  Uadv_done = a.fold.bc_took && Uadv_done;
  return r;
}

int SlabStep::advect() {
  const int R = g.R;
  // (Round 6 measured the scalar advection on a second stream beside the velocity's -- they are independent, simulate.lua:183-200
  // -- and dropped it: an event hop between two streams costs 12-15 us of GPU-side latency on this stack
  // (tools/ubench/host_costs.hip), more than the overlap of two 8 us kernels returns; profiles/r06_slab_host_cost.txt.)
  paired = ap.ours && rho != nullptr;
  if (ap.ours) {
    // density channels 1.. (RGB): each one complete -- min/max (2R, 2R), pass A (R, R), pass B (0, 0) in place -- before channel 0
    // and the velocity, so that the pair kernels below run as with one channel and T2 finds every channel's owned planes written
    for (int i = 1; i < s->n_density; i++) {
      const tfl_tensor* di = s->density[i];
      TRY(adv_scalar(stage(1, 2 * R, 2 * R), di, di));
      TRY(adv_scalar(stage(2, R, R), di, di));
      tfl::Ask a = step_ask(s->densityBC[i]);
      const int rc = adv_scalar(stage(4, 0, 0), di, di, &a);
      if (a.fold.bc_took) extra_done |= 1u << i;
      if (rc) return rc;
    }
    const tfl::Scope pass_a = stage(2, R, R);
    const int rc = paired ? adv_pair(pass_a, false) : TFL_OK;
    if (rc == TFL_EUNSUPPORTED) {
      paired = false;
      TRY(adv_scalar(stage(1, 2 * R, 2 * R), rho, rho));
    } else if (rc) return rc;
    if (!paired) {
      if (rho) TRY(adv_scalar(pass_a, rho, rho));
      TRY(adv_vel(pass_a));
    }
  } else {
    // every other method: the generic gather kernels (and the LDS-tiled single pass of eulerOurs) under the windows of the
    // cones -- a two-pass method's pass A on (R, R), the pass that writes on (0, 0). Those kernels cannot advect in place:
    // each density channel goes to `sout` (the fwdPos planes, which only maccormackOurs uses) and its owned planes are copied
    // back before T2 leaves. Its setConstVals pair is left to the launch after T2 (on every plane: halos arrive unpaired).
    tfl_tensor sout = view(W.compute + g.N, 1);
    for (int i = 0; i < s->n_density; i++) {
      const tfl_tensor* di = s->density[i];
      if (ap.scalar2) TRY(adv_scalar(stage(2, R, R), di, &sout));
      TRY(adv_scalar(stage(ap.scalar2 ? 4 : 2, 0, 0), di, &sout));
      TRY(copy_owned(c, g, di, &sout));
    }
    rho_done = false;
    if (ap.vel2) TRY(adv_vel(stage(2, R, R)));
  }
  // the velocity's pass that writes the owned planes (single-pass methods: stage 2); strips as deep as message T2 sends
  TRY(run_then_send(ap.vel2 ? 4 : 2, std::max(4, 2 * R + 1), m[2], &SlabStep::pass_b));
  TRY(msg_finish(c, g, comm, m[2]));
  cur = &Uadv;
  if (!buoyant && !vfused) { TRY(tfl_copy(c, s->U, &Uadv)); cur = s->U; }
  return set_const_vals(c, s, cur, !Uadv_done, Unchanged{false, false, false}, ((rho && rho_done) ? 1u : 0u) | extra_done);
}

int SlabStep::forces() {
  const tfl::Scope force_sc = stage(0, 3, 4);
  const double dx = tfl::get_dx_double(c, force_sc, s->flags);
  // as tfl_simulate_step: the last force's kernel applies the U pair of the setConstVals that follows, on the planes it writes
  // (they include every plane the projection reads: (0, 1)); the launch below then skips U. Not before the Jacobi projection:
  // its setWallBcs comes between the last force and the pair (as in tfl_simulate_step)
  const bool fold_forces = !prm->outputDiv && !jac;
  const bool gravity_on = prm->gravityScale > 0.0;
  float gv[3];
  if (buoyant) {
    scaled_gravity(prm, dx, prm->buoyancyScale, gv);
    const tfl_tensor* dst = vfused ? &Utmp : s->U;
    const bool last = fold_forces && !gravity_on && !vort;
    tfl::Ask a = step_ask(last ? s->UBC : nullptr);
    const int rc = tfl::addBuoyancyFrom(c, cur, dst, s->flags, rho, gv, prm->dt, 1, force_sc, a);
    U_folded = a.fold.bc_took;
    if (rc) return rc;
    cur = dst;
  }
  if (gravity_on) {
    scaled_gravity(prm, dx, prm->gravityScale, gv);
    TRY(tfl::addGravity(c, cur, s->flags, gv, prm->dt, 1, force_sc));
  }
  if (vort) {
    // fused: one launch, curl (2,2) and |curl| live in LDS, the planes (0,1) of U are written (inputs: planes (3,3) of `cur`);
    // otherwise curl on (2, 2), then the force on (0, 1)
    const float strength = (float)(dx * prm->vorticityConfinementAmp);
    if (!vfused) {
      tfl::Ask none;
      TRY(tfl::vorticityConfinement(c, s->U, s->flags, strength, &curl, &curl, &cnorm, &curl, 1, stage(2, 2, 2), none));
    }
    const tfl::Scope sc = stage(vfused ? 0 : 4, 0, 1);
    tfl::Ask a = step_ask(fold_forces ? s->UBC : nullptr);
    const int rc = vfused ? tfl::vorticityConfinementFrom(c, cur, s->U, s->flags, strength, &curl, &cnorm, 1, sc, a)
                          : tfl::vorticityConfinement(c, s->U, s->flags, strength, &curl, &curl, &cnorm, &curl, 1, sc, a);
    U_folded = a.fold.bc_took;
    if (rc) return rc;
  }
  if (prm->outputDiv) return TFL_OK;
  if (jac) {
    const Win w = ext(g, 0, 1);            // what the divergence reads
    tfl::set_wall_bcs_planes(c->stream, g.B, g.Zl, s->flags->Y, s->flags->X, w.a, w.b, s->U->data, s->flags->data);
  }
  return set_const_vals(c, s, s->U, !U_folded, Unchanged{true, false, true});
}

// (window schedule: the bookkeeping comment above)
int SlabStep::project_jacobi() {
  const int Y = s->flags->Y, X = s->flags->X;
  tfl::velocity_divergence_planes(c->stream, g.B, g.Zl, Y, X, g.o0, g.o1, s->U->data, s->flags->data, div.data);
  TRY(msg_start(c, g, comm, m[3]));
  TRY(msg_finish(c, g, comm, m[3]));
  const int M = prm->maxIter > 0 ? prm->maxIter : 100;
  tfl_tensor pPrev = view(W.compute + g.N, 1);
  const tfl_tensor* buf[2] = {s->p, &pPrev};
  int in = M & 1;                        // p^0's buffer, so that p^M lands in s->p
  if (hipMemsetAsync(buf[in]->data, 0, sizeof(float) * (size_t)g.N, c->stream) != hipSuccess) {
    (void)hipGetLastError(); c->err = "simulate_step_slab: hipMemsetAsync failed"; return TFL_EHIP;
  }
  auto exchange_p = [&]() -> int { Msg q = m[1]; q.f[0].t = buf[in]; TRY(msg_start(c, g, comm, q)); return msg_finish(c, g, comm, q); };
  const int J = multi ? g.J : M + 1;     // (no neighbour: one round, windows clipped to the array)
  int d = J;                             // p is valid on (d, d)
  for (int n = 0; n < M; n++) {
    if (d == 0) { TRY(exchange_p()); d = J; }
    const int left = M - n;              // sweeps still to run, this one included
    const bool last_round = left < d;    // no exchange follows: end at (1, 0)
    const int r = std::min(d, left) - 1; // sweeps of this round after this one
    const Win w = ext(g, std::min(d - 1, r + (last_round ? 1 : 0)), std::min(d - 1, r));
    tfl::jacobi_sweep_slab(c->stream, g.B, g.Zl, Y, X, sl->z_first, sl->z_total, w.a, w.b, buf[in]->data, s->flags->data,
                           div.data, buf[in ^ 1]->data);
    in ^= 1; d--;
  }
  if (d == 0) TRY(exchange_p());
  tfl::velocity_update_planes(c->stream, g.B, g.Zl, Y, X, g.o0, g.o1, s->U->data, s->flags->data, s->p->data);
  if (hipPeekAtLastError() != hipSuccess) { c->err = std::string("simulate_step_slab: ") + hipGetErrorString(hipGetLastError()); return TFL_EHIP; }
  TRY(set_const_vals(c, s, s->U, true, Unchanged{false, false, true}));
  return tfl_applyBCs(c, s->U, nullptr, nullptr, 1, -1e6f, 1e6f);
}

int SlabStep::project_net() {
  TRY(run_then_send(2, g.gen ? std::max(g.cone.in_lo, g.cone.in_hi) : 4, m[3], &SlabStep::model_begin));  // (strips: what T3 sends)
  double count = 3.0 * (double)sl->z_total * (double)g.yx;
  if (g.cone.norm == 0) {        // std(UDiv): tfl_model_begin's partial sums over the owned planes
    TRY(model_begin(stage(4, 0, 0)));
  } else {                       // another field / the l2 norm / none: the same over the owned planes
    tfl::model_slab_stats(c->stream, s->model, g.B, g.Zl, g.yx, g.o0, g.o1, sl->z_total, s->p->data, s->U->data, div.data, W.stats, &count);
  }
  // (no input scale: every rank holds (0, 1) already -- a sum would make it (0, world))
  if (multi && g.cone.norm != 2 && comm->allreduce_sum(comm->user, W.stats, 2ll * g.B) != 0) { c->err = "simulate_step_slab: comm callback failed (allreduce_sum)"; return TFL_EINVAL; }
  const LateUbc lu = late_ubc_of(s);
  auto finish = [&](const tfl::Scope& sc, tfl::Ask* a = nullptr) {
    tfl::Ask none = step_ask(nullptr);
    return tfl::model_finish(c, s->model, s->p, s->flags, s->p, s->U, W.compute, ws_floats - (W.compute - ws), W.stats, count,
                             lu.bc, lu.mask, 1, -1e6f, 1e6f, sc, a ? *a : none);
  };
  const Win w1 = ext(g, 3, 2);
  if (g.gen) {
    // every other net: the whole shape-generic forward as stage 1, each launch on its layer's cone of the owned planes (the
    // window names the owned planes; tfl_model_finish widens it layer by layer)
    TRY(msg_finish(c, g, comm, m[3])); TRY(finish(stage(1, 0, 0)));
  } else if (ovl && g.o1 - 1 > g.o0 + 1) {
    // interior of conv 1 needs only owned planes of div / p: it runs while the div halos travel
    TRY(finish(planes(1, g.lower ? g.o0 + 1 : w1.a, g.upper ? g.o1 - 1 : w1.b, 0, 0)));
    TRY(msg_finish(c, g, comm, m[3]));
    TRY(finish(planes(1, g.lower ? w1.a : 0, g.lower ? g.o0 + 1 : 0, g.upper ? g.o1 - 1 : 0, g.upper ? w1.b : 0)));
  } else {
    TRY(msg_finish(c, g, comm, m[3])); TRY(finish(stage(1, 3, 2)));
  }
  if (!g.gen) { TRY(finish(stage(2, 2, 1))); TRY(finish(stage(4, 1, 0))); }
  tfl::Ask a = step_ask(lu.late ? s->UBC : nullptr);   // the projection kernel applies the sparse U pair itself (owned planes: what T0 sends)
  a.reach_via_project = reach_via_project;
  const int rc = finish(stage(8, 0, 0), &a);
  if (a.reach_published) { c->reach_folded = a.reach_folded; c->reach_issued++; }   // (tfl_slab_graph_create counts these)
  if (rc) return rc;
  return set_const_vals(c, s, s->U, lu.late && !a.fold.bc_took, Unchanged{false, false, true});
}

// the end of every step: the next step's U and p halos leave now; they are consumed at its start / before its first conv layer
int SlabStep::end_step() {
  if (sl->check_reach == 1 && !capturing) reach_mark(c);      // behind the kernel that published this step's reach word
  if (!multi) return TFL_OK;
  TRY(msg_start(c, g, comm, m[0]));
  // a captured step must end with every stream joined: the message is finished here instead of by the next call (nothing
  // of the next step could have run beside it anyway -- its first kernels read these halos)
  if (capturing) return msg_finish(c, g, comm, m[0]);
  sl->in_flight |= 1;
  return TFL_OK;
}

// the rank-step, eager (tfl_simulate_step_slab) or while tfl_slab_graph_create records it (capturing)
int slab_step(tfl_ctx* c, const tfl_sim_params* prm, const tfl_sim_state* s, tfl_slab* sl, const tfl_comm* comm, float* ws,
              int64_t ws_floats, bool capturing) {
  if (!c || !prm || !s || !s->p || !s->U || !s->flags || !sl) return TFL_EINVAL;
  SlabStep S{c, prm, s, sl, comm, ws, ws_floats, capturing};
  TRY(S.validate());
  TRY(S.gates());
  TRY(S.advect());
  TRY(S.forces());
  if (prm->outputDiv) return TFL_OK;
  TRY(S.jac ? S.project_jacobi() : S.project_net());
  return S.end_step();
}

}  // namespace

// Every operator call of the step carries its own scope (planes, stage mask, the slab's origin in the whole grid, the whole
// grid's dx): whatever tfl_set_z_window / tfl_set_stages / tfl_set_z_origin left on the context is neither read nor changed
// (tfl_set_advect_mode is honoured).
int tfl_simulate_step_slab(tfl_ctx* c, const tfl_sim_params* prm, const tfl_sim_state* s, tfl_slab* sl, const tfl_comm* comm,
                           float* ws, int64_t ws_floats) {
  return slab_step(c, prm, s, sl, comm, ws, ws_floats, false);
}

int32_t tfl_slab_needed_reach(const tfl_ctx* c) { return c ? c->needed_reach : 0; }

namespace {
// geometry + message of a stand-alone halo exchange (tfl_slab_exchange): every field has the slab's local depth
int exchange_setup(const tfl_ctx* c, int n, const tfl_tensor* const* fields, const int32_t* below, const int32_t* above, const tfl_slab* sl,
                   SlabGeom* g, Msg* q) {
  (void)c;
  if (n < 1 || n > 4 || !fields || !below || !above || !sl || !fields[0]) return TFL_EINVAL;     // (4 fields x 2 sides = the 8 plane runs of one packing launch)
  g->Zl = fields[0]->Z; g->B = fields[0]->B;
  g->o0 = sl->own_lo; g->o1 = sl->own_hi; g->R = sl->reach > 0 ? sl->reach : 1; g->H = 0;
  g->yx = (long long)fields[0]->Y * fields[0]->X;
  g->N = (long long)g->B * g->Zl * g->yx;
  g->lower = sl->z_first + sl->own_lo > 0;
  g->upper = sl->z_first + sl->own_hi < sl->z_total;
  if (g->o0 < 0 || g->o1 <= g->o0 || g->o1 > g->Zl) return TFL_EINVAL;
  q->tag = 4; q->n = n;
  for (int i = 0; i < n; i++) {
    const tfl_tensor* t = fields[i];
    if (!t || !t->data || t->Z != g->Zl || (long long)t->Y * t->X != g->yx || below[i] < 0 || above[i] < 0) return TFL_EINVAL;
    // a neighbour sends out of its OWNED planes: no deeper than the thinnest slab (the caller keeps own >= halo, as slab_geom demands)
    if ((g->lower && (below[i] > g->o0 || above[i] > g->o1 - g->o0)) || (g->upper && (above[i] > g->Zl - g->o1 || below[i] > g->o1 - g->o0))) return TFL_EINVAL;
    q->f[i] = Halo{t, below[i], above[i]};
  }
  return TFL_OK;
}
}  // namespace

int64_t tfl_slab_exchange_floats(int n, const tfl_tensor* const* fields, const int32_t* below, const int32_t* above, const tfl_slab* sl) {
  SlabGeom g; Msg q;
  if (exchange_setup(nullptr, n, fields, below, above, sl, &g, &q) != TFL_OK) return 0;
  return msg_layout(g, &q, 1, nullptr) + 4;
}

int tfl_slab_exchange(tfl_ctx* c, int n, const tfl_tensor* const* fields, const int32_t* below, const int32_t* above, const tfl_slab* sl,
                      const tfl_comm* comm, float* scratch, int64_t scratch_floats) {
  if (!c) return TFL_EINVAL;
  SlabGeom g; Msg q;
  if (exchange_setup(c, n, fields, below, above, sl, &g, &q) != TFL_OK) { c->err = "slab_exchange: bad fields / plane counts"; return TFL_EINVAL; }
  if (!g.lower && !g.upper) return TFL_OK;
  if (!comm || comm->size < (int32_t)(offsetof(tfl_comm, allreduce_sum) + sizeof(comm->allreduce_sum)) || !comm->exchange_start || !comm->exchange_wait) {
    c->err = "slab_exchange: tfl_comm is null or lacks a required callback"; return TFL_EINVAL;
  }
  if (!scratch || ((uintptr_t)scratch & 15) != 0 || scratch_floats < msg_layout(g, &q, 1, nullptr)) { c->err = "slab_exchange: scratch too small or misaligned"; return TFL_EINVAL; }
  msg_layout(g, &q, 1, scratch);
  // always staged (pack -> send | receive -> unpack): the in-place form needs the transport's chunk lists, and this is a one-off
  pack_msg(c, g, q, false);
  if (comm->exchange_start(comm->user, q.tag, q.send_lo, q.n_send_lo, q.recv_lo, q.n_recv_lo, q.send_hi, q.n_send_hi, q.recv_hi, q.n_recv_hi) != 0) {
    c->err = "slab_exchange: comm callback failed (exchange_start)"; return TFL_EINVAL;
  }
  if (comm->exchange_wait(comm->user, q.tag) != 0) { c->err = "slab_exchange: comm callback failed (exchange_wait)"; return TFL_EINVAL; }
  pack_msg(c, g, q, true);
  return TFL_OK;
}

// ---- the rank-step as ONE host call: a HIP graph of tfl_simulate_step_slab (round 6; include/tfluids_hip.h) -------------
struct tfl_slab_graph {
  hipGraphExec_t exec = nullptr;
  hipStream_t cap = nullptr;          // the stream the step was recorded on (kept: RCCL's captured work refers to it)
  const tfl_sim_params* prm = nullptr;
  const tfl_sim_state* s = nullptr;
  tfl_slab* sl = nullptr;
  int reach = 1;
  bool multi = false;                 // the slab has neighbours
  unsigned reach_pubs = 0;            // reach publications one replay makes (counted while recording)
  size_t nodes = 0;
};

tfl_slab_graph* tfl_slab_graph_create(tfl_ctx* c, const tfl_sim_params* prm, const tfl_sim_state* s, tfl_slab* sl, const tfl_comm* comm,
                                      float* ws, int64_t ws_floats) {
  if (!c || !prm || !s || !sl) return nullptr;
  SlabGeom g;
  if (slab_geom(c, s, sl, &g) != TFL_OK) return nullptr;
  const bool multi = g.lower || g.upper;
  if (multi) {
    const bool can = comm && comm->size >= (int32_t)(offsetof(tfl_comm, capturable) + sizeof(comm->capturable)) && comm->capturable != 0;
    if (!can) { c->err = "slab_graph_create: this transport's calls are not stream operations (tfl_comm.capturable = 0): step eagerly"; return nullptr; }
  }
  if (sl->check_reach == 2) { c->err = "slab_graph_create: check_reach = 2 synchronises with the host every step: step eagerly"; return nullptr; }
  // the U / p message the last eager step left in flight is consumed now: a captured step starts and ends with none
  if ((sl->in_flight & 0xF) && tfl_slab_drain(c, s, sl, comm, ws, ws_floats) != TFL_OK) return nullptr;
  // (a host that records before its first eager step: the reset of the sticky reach word must not become a node of the graph)
  if (sl->check_reach == 1 && !(sl->in_flight & kReachPrimed)) reach_prime(c, sl);
  tfl_slab_graph* G = new tfl_slab_graph();
  G->prm = prm; G->s = s; G->sl = sl; G->reach = g.R; G->multi = multi;
  if (hipStreamCreateWithFlags(&G->cap, hipStreamNonBlocking) != hipSuccess) { c->err = "slab_graph_create: hipStreamCreate failed"; delete G; return nullptr; }
  hipStream_t user = c->stream;
  // everything queued so far on the caller's stream happens before the recording stream is used at all (warm-up steps)
  (void)hipStreamSynchronize(user);
  reach_quiesce(c);
  hipGraph_t graph = nullptr;
  // relaxed: the transport's library may call into the runtime from its own threads while we record
  if (hipStreamBeginCapture(G->cap, hipStreamCaptureModeRelaxed) != hipSuccess) {
    c->err = "slab_graph_create: hipStreamBeginCapture failed"; (void)hipStreamDestroy(G->cap); delete G; return nullptr;
  }
  c->stream = G->cap;
  const unsigned issued0 = c->reach_issued;
  const int rc = slab_step(c, prm, s, sl, comm, ws, ws_floats, true);
  G->reach_pubs = c->reach_issued - issued0; c->reach_issued = issued0;      // recorded, not run: every REPLAY makes them
  c->stream = user;
  const hipError_t ec = hipStreamEndCapture(G->cap, &graph);
  std::string why;
  if (rc != TFL_OK) why = "the step failed while being recorded: " + c->err;
  else if (ec != hipSuccess || !graph) why = std::string("hipStreamEndCapture: ") + hipGetErrorString(ec);
  else if (hipGraphInstantiate(&G->exec, graph, nullptr, nullptr, 0) != hipSuccess) why = "hipGraphInstantiate failed";
  if (graph) { (void)hipGraphGetNodes(graph, nullptr, &G->nodes); (void)hipGraphDestroy(graph); }
  (void)hipGetLastError();
  if (!why.empty()) {
    c->err = "slab_graph_create: " + why;
    if (G->exec) (void)hipGraphExecDestroy(G->exec);
    (void)hipStreamDestroy(G->cap);
    delete G;
    return nullptr;
  }
  return G;
}

int64_t tfl_slab_graph_nodes(const tfl_slab_graph* G) { return G ? (int64_t)G->nodes : 0; }

int tfl_slab_graph_step(tfl_ctx* c, tfl_slab_graph* G) {
  if (!c || !G || !G->exec) return TFL_EINVAL;
  // the two gates of the eager call, read from the words the PREVIOUS step left in pinned memory
  if (G->sl->check_reach) {
    char buf[256];
    if (reach_violated(c, G->prm->dt, G->reach, buf, sizeof(buf))) { c->err = buf; return TFL_EINVAL; }
  }
  // (a slab with neighbours never refuses on its own word: see the eager step)
  if (!G->multi && G->s->model && tfl_model_range_flag(c, G->s->model) > 0) return range_refusal(c, "simulate_step_slab");
  if (hipGraphLaunch(G->exec, c->stream) != hipSuccess) { c->err = "slab_graph_step: hipGraphLaunch failed"; (void)hipGetLastError(); return TFL_EHIP; }
  if (G->sl->check_reach) { c->reach_issued += G->reach_pubs; reach_mark(c); }
  return TFL_OK;
}

void tfl_slab_graph_destroy(tfl_ctx* c, tfl_slab_graph* G) {
  (void)c;
  if (!G) return;
  if (G->exec) (void)hipGraphExecDestroy(G->exec);
  if (G->cap) (void)hipStreamDestroy(G->cap);
  delete G;
}

}  // extern "C"
