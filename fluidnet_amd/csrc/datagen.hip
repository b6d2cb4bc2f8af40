// datagen.hip -- the scene kernels of the data-set generator (tfl_scene_flags, tfl_noise_potential, tfl_curl_mac; DESIGN.md 3.22,
// fluidnet_amd/datagen.py). The reference's training sets come from a Mantaflow scene script that is not part of its tree; these
// kernels build this project's own random scenes where the simulation runs: a flags grid and a density field from a table of
// primitives (k_scene_flags), white noise from a counter-based hash (k_noise_potential), and -- behind the existing
// rectangularBlur -- the staggered curl of the smoothed potential as the initial velocity (k_curl_mac).
// None is a hot path (once per run); what matters is that each value is a function of its arguments alone, in the stated fp32 /
// uint32 order of tfl_datagen.hpp, so that tests/datagen_ref.py restates them bit for bit. One thread per cell, x fastest;
// the tables travel by value as kernel arguments.
#include <hip/hip_runtime.h>

#include <cstring>

#include "tfl_abi.hpp"
#include "tfl_datagen.hpp"

namespace tfl {
namespace {

constexpr int kGenThreads = 256;

static_assert(sizeof(tfl_scene_prim) == sizeof(ScenePrim), "tfl_scene_prim is ScenePrim");

__global__ __launch_bounds__(kGenThreads) void k_scene_flags(const SceneTable obs, const SceneTable blobs, int is3D, int B, int Z, int Y, int X,
                                                             float* __restrict__ flags, float* __restrict__ density) {
  const long long cells = (long long)Z * Y * X;
  const long long t = (long long)blockIdx.x * kGenThreads + threadIdx.x;
  if (t >= cells) return;
  const int i = (int)(t % X), j = (int)((t / X) % Y), k = (int)(t / ((long long)X * Y));
  const float f = scene_flag(obs, is3D, Z, Y, X, i, j, k);
  const float rho = density ? scene_density(blobs, f, is3D, i, j, k) : 0.0f;
  for (int b = 0; b < B; b++) {
    flags[b * cells + t] = f;
    if (density) density[b * cells + t] = rho;
  }
}

__global__ __launch_bounds__(kGenThreads) void k_noise_potential(uint32_t seed, uint32_t run, int C, long long cells, float* __restrict__ psi) {
  const long long t = (long long)blockIdx.x * kGenThreads + threadIdx.x;
  if (t >= cells) return;
  const int b = blockIdx.z, comp = blockIdx.y;
  psi[((long long)b * C + comp) * cells + t] = noise_value(noise_hash(seed, run + (uint32_t)b, (uint32_t)comp, (uint32_t)t));
}

__global__ __launch_bounds__(kGenThreads) void k_curl_mac(const float* __restrict__ psi, float amp, int is3D, int Z, int Y, int X,
                                                          float* __restrict__ U) {
  const long long cells = (long long)Z * Y * X;
  const long long t = (long long)blockIdx.x * kGenThreads + threadIdx.x;
  if (t >= cells) return;
  const int b = blockIdx.z, comp = blockIdx.y;
  const int C = is3D ? 3 : 2, Cpsi = is3D ? 3 : 1;
  const int i = (int)(t % X), j = (int)((t / X) % Y), k = (int)(t / ((long long)X * Y));
  U[((long long)b * C + comp) * cells + t] = curl_mac(psi + (long long)b * Cpsi * cells, is3D, Z, Y, X, comp, i, j, k, amp);
}

int check_grid(tfl_ctx* c, const char* who, const char* name, const tfl_tensor* t, int C) {
  if (!t || !t->data) return fail(c, TFL_EINVAL, "%s: %s is null", who, name);
  if (t->B < 1 || t->Z < 1 || t->Y < 1 || t->X < 1) return fail(c, TFL_EINVAL, "%s: empty grid", who);
  if (t->C != C) return fail(c, TFL_EINVAL, "%s: %s has %d channels, %d expected", who, name, t->C, C);
  if ((long long)t->Z * t->Y * t->X * 3 >= (1ll << 31)) return fail(c, TFL_EINVAL, "%s: grid too large for 32-bit cell offsets", who);
  if (t->B > 65535) return fail(c, TFL_EINVAL, "%s: B exceeds the launch grid limit", who);
  return TFL_OK;
}

int table_of(tfl_ctx* c, const char* who, const char* name, const tfl_scene_prim* p, int n, SceneTable* out) {
  if (n < 0 || n > kSceneMaxPrims || (n > 0 && !p)) return fail(c, TFL_EINVAL, "%s: %d %s, at most %d fit one table (or a null table)", who, n, name, kSceneMaxPrims);
  std::memset(out, 0, sizeof(*out));
  out->n = n;
  for (int i = 0; i < n; i++) {
    if (p[i].kind != kScenePrimSphere && p[i].kind != kScenePrimBox) return fail(c, TFL_EINVAL, "%s: %s %d is of unknown kind %d", who, name, i, (int)p[i].kind);
    std::memcpy(&out->p[i], &p[i], sizeof(ScenePrim));
  }
  return TFL_OK;
}

}  // namespace
}  // namespace tfl

using tfl::fail;

extern "C" {

int tfl_scene_flags(tfl_ctx* c, const tfl_scene_prim* obstacles, int n_obstacles, const tfl_scene_prim* blobs, int n_blobs, int is3D,
                    const tfl_tensor* flags, const tfl_tensor* density) {
  if (!c) return TFL_EINVAL;
  const char* who = "scene_flags";
  TRY(tfl::check_grid(c, who, "flags", flags, 1));
  if (!is3D && flags->Z != 1) return fail(c, TFL_EINVAL, "%s: 2D domain but zdepth > 1", who);
  if (density) {
    TRY(tfl::check_grid(c, who, "density", density, 1));
    if (!tfl::same_dims(density, flags)) return fail(c, TFL_EINVAL, "%s: density size mismatch", who);
  }
  tfl::SceneTable obs, bl;
  TRY(tfl::table_of(c, who, "obstacles", obstacles, n_obstacles, &obs));
  TRY(tfl::table_of(c, who, "blobs", blobs, n_blobs, &bl));
  const long long cells = (long long)flags->Z * flags->Y * flags->X;
  const unsigned blocks = (unsigned)((cells + tfl::kGenThreads - 1) / tfl::kGenThreads);
  TFL_TIMED("k_scene_flags", c->stream);
  hipLaunchKernelGGL(tfl::k_scene_flags, dim3(blocks), dim3(tfl::kGenThreads), 0, c->stream, obs, bl, is3D ? 1 : 0, flags->B, flags->Z, flags->Y,
                     flags->X, flags->data, density ? density->data : nullptr);
  return tfl::check_launch(c, who);
}

int tfl_noise_potential(tfl_ctx* c, uint32_t seed, uint32_t run, const tfl_tensor* psi) {
  if (!c) return TFL_EINVAL;
  const char* who = "noise_potential";
  if (!psi || (psi->C != 1 && psi->C != 3)) return fail(c, TFL_EINVAL, "%s: psi is null or has neither 1 (2-D) nor 3 (3-D) channels", who);
  TRY(tfl::check_grid(c, who, "psi", psi, psi->C));
  const long long cells = (long long)psi->Z * psi->Y * psi->X;
  const unsigned blocks = (unsigned)((cells + tfl::kGenThreads - 1) / tfl::kGenThreads);
  TFL_TIMED("k_noise_potential", c->stream);
  hipLaunchKernelGGL(tfl::k_noise_potential, dim3(blocks, (unsigned)psi->C, (unsigned)psi->B), dim3(tfl::kGenThreads), 0, c->stream, seed, run, psi->C,
                     cells, psi->data);
  return tfl::check_launch(c, who);
}

int tfl_curl_mac(tfl_ctx* c, const tfl_tensor* psi, float amp, int is3D, const tfl_tensor* U) {
  if (!c) return TFL_EINVAL;
  const char* who = "curl_mac";
  TRY(tfl::check_grid(c, who, "psi", psi, is3D ? 3 : 1));
  TRY(tfl::check_grid(c, who, "U", U, is3D ? 3 : 2));
  if (!tfl::same_dims(psi, U)) return fail(c, TFL_EINVAL, "%s: U size mismatch", who);
  if (!is3D && U->Z != 1) return fail(c, TFL_EINVAL, "%s: 2D velocity field but zdepth > 1", who);
  if (psi->data == U->data) return fail(c, TFL_EINVAL, "%s: psi and U must not alias", who);
  const long long cells = (long long)U->Z * U->Y * U->X;
  const unsigned blocks = (unsigned)((cells + tfl::kGenThreads - 1) / tfl::kGenThreads);
  TFL_TIMED("k_curl_mac", c->stream);
  hipLaunchKernelGGL(tfl::k_curl_mac, dim3(blocks, (unsigned)U->C, (unsigned)U->B), dim3(tfl::kGenThreads), 0, c->stream, psi->data, amp, is3D ? 1 : 0,
                     U->Z, U->Y, U->X, U->data);
  return tfl::check_launch(c, who);
}

}  // extern "C"
