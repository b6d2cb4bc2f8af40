// context.cpp -- the context behind the opaque tfl_ctx* of include/tfluids_hip.h: its creation and destruction, what the
// tfl_set_* calls store on it (and scope_of / get_dx, which read that back for the operators), the per-kernel event
// profiler, and the error return every entry point of the library shares (fail, tfl_abi.hpp).
// No torch / Lua / C++ types cross the boundary; errors come back as codes + tfl_last_error().
#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "tfl_abi.hpp"
#include "tfl_ops.hpp"

using tfl::fail;

// ---- per-kernel event profiler (TFL_TIMED in the launchers) ---------------------------------------
namespace tfl {
struct ProfRec { const char* name; hipEvent_t e0, e1; };
struct Profiler { std::vector<ProfRec> recs; };
static thread_local Profiler* g_prof = nullptr;

KernelTimer::KernelTimer(const char* name, hipStream_t st, bool ext) : slot_(-1), st_(st), ext_(ext) {
  if (!g_prof) return;
  ProfRec r; r.name = name;
  if (hipEventCreate(&r.e0) != hipSuccess) return;
  if (hipEventCreate(&r.e1) != hipSuccess) { (void)hipEventDestroy(r.e0); return; }
  if (!ext_) (void)hipEventRecord(r.e0, st);
  g_prof->recs.push_back(r);
  slot_ = (int)g_prof->recs.size() - 1;
}
KernelTimer::~KernelTimer() {
  if (slot_ >= 0 && g_prof && !ext_) (void)hipEventRecord(g_prof->recs[slot_].e1, st_);
}
hipEvent_t KernelTimer::start() const { return (slot_ >= 0 && g_prof) ? g_prof->recs[slot_].e0 : nullptr; }
hipEvent_t KernelTimer::stop() const { return (slot_ >= 0 && g_prof) ? g_prof->recs[slot_].e1 : nullptr; }

int fail(tfl_ctx* ctx, int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  if (ctx) ctx->err = buf;
  return code;
}

// What the tfl_set_* calls left on the context, as the one value a public operator that honours them forms at its entry and
// passes down (the operators that ignore them never call this). A null context gives the empty scope: the operator's own
// checks refuse it.
Scope scope_of(const tfl_ctx* c) {
  Scope sc;
  if (c) { sc.win = c->zwin; sc.origin = c->zorigin; sc.stages = c->stages; sc.advect_fast = c->advect_fast; }
  return sc;
}
static int dx_cells(const Scope& sc, const tfl_tensor* f) {
  return sc.dx_cells > 0 ? sc.dx_cells : std::max(std::max(f->X, f->Y), f->Z);
}
float get_dx(const tfl_ctx* c, const Scope& sc, const tfl_tensor* f) {  // grid.cc:37-40
  if (sc.dx_cells <= 0 && c && c->dx_override > 0.0f) return c->dx_override;
  return 1.0f / (float)dx_cells(sc, f);
}
double get_dx_double(const tfl_ctx* c, const Scope& sc, const tfl_tensor* f) {
  if (sc.dx_cells <= 0 && c && c->dx_override > 0.0f) return (double)c->dx_override;
  return 1.0 / (double)dx_cells(sc, f);
}

static void scal3_sparse_free(Scal3SparseState* p) {
  if (p->buf.nz) (void)hipFree(p->buf.nz);
  if (p->buf.lists) (void)hipFree(p->buf.lists);
  if (p->buf.counts) (void)hipFree(p->buf.counts);
  if (p->h_mirror) (void)hipHostFree(p->h_mirror);
  delete p;
}
Scal3SparseState* scal3_sparse_state(tfl_ctx* c, const float* key, int B, int Z, int Y, int X, int bricks) {
  for (Scal3SparseState* p : c->scal3_sparse)
    if (p->key == key && p->B == B && p->Z == Z && p->Y == Y && p->X == X) return p;
  if ((int)c->scal3_sparse.size() >= kScal3SparseFields) {      // the oldest field goes (hipFree waits for the kernels that use it)
    if (c->scal3_last == c->scal3_sparse.front()) c->scal3_last = nullptr;
    scal3_sparse_free(c->scal3_sparse.front());
    c->scal3_sparse.erase(c->scal3_sparse.begin());
  }
  Scal3SparseState* p = new Scal3SparseState();
  p->key = key; p->B = B; p->Z = Z; p->Y = Y; p->X = X;
  const size_t n = (size_t)B * (size_t)bricks;
  // (the tags hold scan numbers and are never cleared between scans: zero, the number no scan has, at allocation)
  p->scans = (unsigned)sw::num(Sw::SCAL3_SEQ0, 0);
  if (hipMalloc((void**)&p->buf.nz, sizeof(unsigned) * (n + B)) != hipSuccess || hipMemset(p->buf.nz, 0, sizeof(unsigned) * (n + B)) != hipSuccess ||
      hipMalloc((void**)&p->buf.lists, sizeof(int) * 2 * n) != hipSuccess ||
      hipMalloc((void**)&p->buf.counts, sizeof(int) * 4 * B) != hipSuccess || hipMemset(p->buf.counts, 0, sizeof(int) * 4 * B) != hipSuccess ||
      hipHostMalloc((void**)&p->h_mirror, sizeof(unsigned) * 8 * B, hipHostMallocMapped) != hipSuccess ||
      hipHostGetDevicePointer((void**)&p->buf.mirror, p->h_mirror, 0) != hipSuccess) {
    (void)hipGetLastError();
    scal3_sparse_free(p);
    return nullptr;
  }
  memset(p->h_mirror, 0, sizeof(unsigned) * 8 * B);      // the scan's number 0: nothing known yet
  c->scal3_sparse.push_back(p);
  return p;
}
}  // namespace tfl

extern "C" {

int tfl_abi_version(void) { return TFL_ABI_VERSION; }

tfl_ctx* tfl_create(int device) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || device < 0 || device >= n) return nullptr;
  if (hipSetDevice(device) != hipSuccess) return nullptr;
  tfl_ctx* c = new tfl_ctx();
  c->device = device;
  if (hipMalloc((void**)&c->d_trace_err, 3 * sizeof(unsigned long long)) != hipSuccess ||      // [1], [2]: tfl_scal3_zero_blocks
      hipMemset(c->d_trace_err, 0, 3 * sizeof(unsigned long long)) != hipSuccess ||
      hipMalloc((void**)&c->d_resid, sizeof(double) * kMaxBatch) != hipSuccess ||
      hipHostMalloc((void**)&c->h_resid, sizeof(double) * kMaxBatch, hipHostMallocDefault) != hipSuccess ||
      hipMalloc((void**)&c->d_reach, sizeof(float)) != hipSuccess ||
      hipMemset(c->d_reach, 0, sizeof(float)) != hipSuccess ||      // (a sticky maximum since round 6: nothing resets it per step)
      hipHostMalloc((void**)&c->h_reach, 2 * sizeof(float), hipHostMallocMapped) != hipSuccess ||
      hipHostGetDevicePointer((void**)&c->d_reach_host, c->h_reach, 0) != hipSuccess ||
      hipMalloc((void**)&c->d_reach_tick, sizeof(unsigned)) != hipSuccess ||
      hipMemset(c->d_reach_tick, 0, sizeof(unsigned)) != hipSuccess) {
    tfl_destroy(c);
    return nullptr;
  }
  c->h_reach[0] = 0.0f; reinterpret_cast<unsigned*>(c->h_reach)[1] = 0u;
  if (const char* m = tfl::sw::text(tfl::Sw::ADVECT_MODE)) c->advect_fast = (strcmp(m, "fast") == 0 || strcmp(m, "1") == 0) ? 1 : 0;
  return c;
}

int tfl_set_advect_mode(tfl_ctx* c, int mode) {
  if (!c) return TFL_EINVAL;
  if (mode != TFL_ADVECT_EXACT && mode != TFL_ADVECT_FAST) return fail(c, TFL_EINVAL, "set_advect_mode: unknown mode %d", mode);
  c->advect_fast = mode == TFL_ADVECT_FAST ? 1 : 0;
  return TFL_OK;
}
int tfl_get_advect_mode(const tfl_ctx* c) { return c ? (c->advect_fast ? TFL_ADVECT_FAST : TFL_ADVECT_EXACT) : TFL_EINVAL; }

void tfl_destroy(tfl_ctx* c) {
  if (!c) return;
  { std::lock_guard<std::mutex> lock(c->wall_mu); for (tfl_wall_plan* p : c->wall_plans) p->owner = nullptr; c->wall_plans.clear(); }      // the host still owns (and frees) them
  for (Scal3SparseState* p : c->scal3_sparse) tfl::scal3_sparse_free(p);
  if (c->d_reach) (void)hipFree(c->d_reach);
  if (c->h_reach) (void)hipHostFree(c->h_reach);
  if (c->d_reach_tick) (void)hipFree(c->d_reach_tick);
  if (c->h_reach_flags) (void)hipHostFree(c->h_reach_flags);
  if (c->d_trace_err) (void)hipFree(c->d_trace_err);
  if (c->d_resid) (void)hipFree(c->d_resid);
  if (c->h_resid) (void)hipHostFree(c->h_resid);
  delete c;
}

int tfl_set_stream(tfl_ctx* c, void* s) {
  if (!c) return TFL_EINVAL;
  c->stream = (hipStream_t)s;
  return TFL_OK;
}

const char* tfl_last_error(const tfl_ctx* c) { return c ? c->err.c_str() : "null context"; }

int tfl_set_dx_override(tfl_ctx* c, float dx) {
  if (!c) return TFL_EINVAL;
  c->dx_override = dx > 0.0f ? dx : 0.0f;
  return TFL_OK;
}

int tfl_set_z_window(tfl_ctx* c, int a0, int a1, int b0, int b1) {
  if (!c) return TFL_EINVAL;
  if (a0 < 0 || a1 < a0 || b0 < 0 || b1 < b0 || (a1 > a0 && b1 > b0 && b0 < a1))
    return fail(c, TFL_EINVAL, "set_z_window: [%d,%d) [%d,%d) is not an ordered pair of plane runs", a0, a1, b0, b1);
  c->zwin = tfl::ZWin{a0, a1, b0, b1};
  return TFL_OK;
}

int tfl_set_z_origin(tfl_ctx* c, int z_first, int z_total) {
  if (!c || z_first < 0 || z_total < 0 || (z_total > 0 && z_first >= z_total)) return TFL_EINVAL;
  c->zorigin = tfl::ZOrigin{z_total > 0 ? z_first : 0, z_total};
  return TFL_OK;
}

int tfl_set_stages(tfl_ctx* c, int mask) {
  if (!c || mask < 0) return TFL_EINVAL;
  c->stages = mask;
  return TFL_OK;
}

int tfl_synchronize(tfl_ctx* c) {
  if (!c) return TFL_EINVAL;
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return TFL_OK;
}

int tfl_profile_begin(tfl_ctx* c) {
  if (!c) return TFL_EINVAL;
  if (tfl::g_prof) return fail(c, TFL_EINVAL, "profile_begin: a profile is already active on this thread");
  tfl::g_prof = new tfl::Profiler();
  return TFL_OK;
}

int tfl_profile_end(tfl_ctx* c, char* buf, int64_t cap) {
  if (!c) return TFL_EINVAL;
  tfl::Profiler* p = tfl::g_prof;
  if (!p) return fail(c, TFL_EINVAL, "profile_end: no active profile");
  tfl::g_prof = nullptr;
  (void)hipStreamSynchronize(c->stream);
  (void)hipDeviceSynchronize();
  std::vector<std::string> names;
  std::vector<double> ms;
  std::vector<long long> calls;
  for (auto& r : p->recs) {
    float t = 0.0f;
    if (hipEventElapsedTime(&t, r.e0, r.e1) != hipSuccess) t = 0.0f;
    (void)hipEventDestroy(r.e0);
    (void)hipEventDestroy(r.e1);
    size_t i = 0;
    for (; i < names.size(); i++) if (names[i] == r.name) break;
    if (i == names.size()) { names.push_back(r.name); ms.push_back(0.0); calls.push_back(0); }
    ms[i] += t; calls[i] += 1;
  }
  delete p;
  std::string js = "{";
  for (size_t i = 0; i < names.size(); i++) {
    char tmp[256];
    snprintf(tmp, sizeof(tmp), "%s\"%s\": {\"calls\": %lld, \"ms\": %.6f}", i ? ", " : "", names[i].c_str(), calls[i], ms[i]);
    js += tmp;
  }
  js += "}";
  if (buf && cap > 0) {
    const size_t n = js.size() < (size_t)cap - 1 ? js.size() : (size_t)cap - 1;
    memcpy(buf, js.data(), n);
    buf[n] = 0;
  }
  return (int)names.size();
}

int64_t tfl_trace_errors(tfl_ctx* c) {
  if (!c) return -1;
  unsigned long long v = 0;
  if (hipMemcpyAsync(&v, c->d_trace_err, sizeof(v), hipMemcpyDeviceToHost, c->stream) != hipSuccess) return -1;
  if (hipMemsetAsync(c->d_trace_err, 0, sizeof(v), c->stream) != hipSuccess) return -1;
  if (hipStreamSynchronize(c->stream) != hipSuccess) return -1;
  return (int64_t)v;
}

int tfl_scal3_zero_blocks(tfl_ctx* c, int64_t* blocks) {
  if (!c || !blocks) return TFL_EINVAL;
  unsigned long long v[2] = {0, 0};
  HIP_TRY(c, hipMemcpyAsync(v, c->d_trace_err + 1, sizeof(v), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipMemsetAsync(c->d_trace_err + 1, 0, sizeof(v), c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  blocks[0] = (int64_t)v[0]; blocks[1] = (int64_t)v[1];
  return TFL_OK;
}

int tfl_scal3_sparse_stats(tfl_ctx* c, int64_t* out) {
  if (!c || !out) return TFL_EINVAL;
  HIP_TRY(c, hipStreamSynchronize(c->stream));      // the last lists kernel has published its counts
  for (int i = 0; i < 3; i++) { out[i] = (int64_t)c->scal3_counts[i]; c->scal3_counts[i] = 0; }
  out[3] = out[4] = 0;
#ifdef TFL_EXPERIMENTS
  if (const Scal3SparseState* p = c->scal3_last)
    for (int b = 0; b < p->B; b++) { out[3] += p->h_mirror[8 * b + 3]; out[4] += p->h_mirror[8 * b]; }
#endif
  return TFL_OK;
}

double tfl_getDx(tfl_ctx* c, const tfl_tensor* flags) {
  if (!flags) return 0.0;
  return tfl::get_dx_double(c, tfl::Scope{}, flags);
}

}  // extern "C"
