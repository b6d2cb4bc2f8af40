// tfl_abi.hpp -- what the .cpp files behind include/tfluids_hip.h share (context.cpp, abi.cpp, model_build.cpp, model_host.cpp,
// model_train.cpp, optim_host.cpp, simulate.cpp, simulate_slab.cpp; private to them -- of the .hip files only frames.hip, which holds its entries' host side, includes it): the batch limit, the error return, the argument checks that mirror
// torch/tfluids/init.lua's asserts, and the two early-return macros. The checks are inline: every operator runs several per call,
// and as calls into another translation unit they measured 0.1 - 0.5 % on the benchmark's step. fail() is context.cpp's.
// (What only the two native steps share is tfl_step.hpp, inline for the same reason.)
#pragma once
#include "../../include/tfluids_hip.h"
#include "tfl_ctx.hpp"

static const int kMaxBatch = 1024;

namespace tfl {
int fail(tfl_ctx* ctx, int code, const char* fmt, ...);      // stores the message for tfl_last_error, returns code
inline int check_launch(tfl_ctx* ctx, const char* what) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(ctx, TFL_EHIP, "%s: %s", what, hipGetErrorString(e));
  return TFL_OK;
}

inline bool same_dims(const tfl_tensor* a, const tfl_tensor* b) {
  return a->B == b->B && a->Z == b->Z && a->Y == b->Y && a->X == b->X;
}

// init.lua's shape asserts (e.g. :99-120): flags scalar, U has 2 (2-D, Z==1) or 3 channels, all same B/Z/Y/X.
inline int check_flags(tfl_ctx* ctx, const char* op, const tfl_tensor* flags) {
  if (!ctx) return TFL_EINVAL;
  if (!flags || !flags->data) return fail(ctx, TFL_EINVAL, "%s: flags is null", op);
  if (flags->C != 1) return fail(ctx, TFL_EINVAL, "%s: flags is not scalar", op);
  if (flags->B < 1 || flags->Z < 1 || flags->Y < 1 || flags->X < 1) return fail(ctx, TFL_EINVAL, "%s: empty grid", op);
  if ((long long)flags->Z * flags->Y * flags->X * 3 >= (1ll << 31))
    return fail(ctx, TFL_EINVAL, "%s: grid too large for 32-bit cell offsets", op);
  if ((long long)flags->Z * flags->B > 65535) return fail(ctx, TFL_EINVAL, "%s: B*Z exceeds the launch grid limit", op);
  return TFL_OK;
}
inline int check_vel(tfl_ctx* ctx, const char* op, const char* name, const tfl_tensor* U, const tfl_tensor* flags, int is3D) {
  if (!U || !U->data) return fail(ctx, TFL_EINVAL, "%s: %s is null", op, name);
  if (!same_dims(U, flags)) return fail(ctx, TFL_EINVAL, "%s: %s size mismatch", op, name);
  if (is3D) {
    if (U->C != 3) return fail(ctx, TFL_EINVAL, "%s: 3D velocity field must have 3 channels", op);
  } else {
    if (flags->Z != 1) return fail(ctx, TFL_EINVAL, "%s: 2D velocity field but zdepth > 1", op);
    if (U->C != 2) return fail(ctx, TFL_EINVAL, "%s: 2D velocity field must have only 2 channels", op);
  }
  return TFL_OK;
}
inline int check_scalar(tfl_ctx* ctx, const char* op, const char* name, const tfl_tensor* s, const tfl_tensor* flags) {
  if (!s || !s->data) return fail(ctx, TFL_EINVAL, "%s: %s is null", op, name);
  if (s->C != 1 || !same_dims(s, flags)) return fail(ctx, TFL_EINVAL, "%s: %s size mismatch", op, name);
  return TFL_OK;
}
}  // namespace tfl

#define HIP_TRY(ctx, call)                                                                     \
  do {                                                                                         \
    hipError_t e_ = (call);                                                                    \
    if (e_ != hipSuccess) return ::tfl::fail(ctx, TFL_EHIP, "%s: %s", #call, hipGetErrorString(e_)); \
  } while (0)
#define TRY(x) do { int rc_ = (x); if (rc_ != TFL_OK) return rc_; } while (0)
