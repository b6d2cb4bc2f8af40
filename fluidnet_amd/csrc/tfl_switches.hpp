// tfl_switches.hpp -- every TFL_* environment variable the library reads: one table, one reader. This is the only file of
// csrc that calls getenv. Plain C++ (no HIP headers): tfl_device.hpp, tfl_host.hpp and comm_rccl.cpp include it, and
// tests/switches_host.cpp compiles it alone.
//
//   sw::present(Sw::X)      the variable is set (to anything, "0" included)
//   sw::num(Sw::X, dflt)    atoi of its value, dflt when it is not set
//   sw::text(Sw::X)         its text or null (PER_CALL rows only: a pointer getenv returned is never kept)
//
// Columns: id, variable, flavour, when, meaning (value convention first).
//   flavour  PRODUCT = both libraries read it; EXP = only the EXPERIMENTS flavour (-DTFL_EXPERIMENTS, `make exp`) does: the
//            product library holds no such name, the row reads as "not set" there and what it guards folds away
//   when     ONCE = parsed at the first read of the row and kept for the life of the process (function-local static: lazy,
//            thread-safe); PER_CALL = getenv at every read (the tests flip these inside one process)
// INTEGRATION.md 4e shows this table to hosts and tests/flavours.py takes the EXP names from it (tests/test_switches_cpu.py
// holds the three together), so a row is one line of the form below.
#pragma once
#include <cstdlib>

// clang-format off
#define TFL_SWITCH_TABLE(X) \
  X(ADVECT_MODE,     "TFL_ADVECT_MODE",     PRODUCT, PER_CALL, "text, at context creation: fast or 1 = the tolerance mode of the 3-D advection kernels, anything else = exact (tfl_set_advect_mode is the API)") \
  X(ADV_PAIR,        "TFL_ADV_PAIR",        PRODUCT, ONCE,     "=0 turns the pair kernels of the z-slab step off (advectScalar and advectVel as launches of their own)") \
  X(BC_FOLD,         "TFL_BC_FOLD",         PRODUCT, PER_CALL, "=0 keeps every sparse setConstVals pair in its own launch (the A/B parity test switches it inside one process)") \
  X(BUOY_FOLD,       "TFL_BUOY_FOLD",       PRODUCT, PER_CALL, "=0 keeps the buoyancy force in its own launch instead of pass B of advectVel") \
  X(CONV_PATH,       "TFL_CONV_PATH",       PRODUCT, PER_CALL, "text, at model creation: mfma16 or unset = split-operand fp16 MFMA, mfma = fp32 MFMA, direct = the shape-generic kernels, anything else (winograd) = strict fp32 on the vector ALUs") \
  X(DEBUG,           "TFL_DEBUG",           PRODUCT, PER_CALL, "set at all: launch geometry and occupancy of the conv kernels on stderr") \
  X(JACOBI_LDS,      "TFL_JACOBI_LDS",      PRODUCT, ONCE,     "=0 turns the one-launch LDS Jacobi solve of small 2-D grids off (one launch per iteration)") \
  X(PCG_HYPERPLANES, "TFL_PCG_HYPERPLANES", PRODUCT, ONCE,     "set at all (=0 too): the PCG triangular solves as one launch per hyperplane instead of the wavefront pipeline") \
  X(RCCL_LIBRARY,    "TFL_RCCL_LIBRARY",    PRODUCT, PER_CALL, "text, at the first native transport: path of the librccl to dlopen (empty = as unset)") \
  X(RCCL_PACKED,     "TFL_RCCL_PACKED",     PRODUCT, PER_CALL, "set at all, at transport creation: one staged buffer per neighbour (pack / unpack kernels) instead of chunk lists") \
  X(SCAL3_TZ,        "TFL_SCAL3_TZ",        PRODUCT, ONCE,     "1 / 2 / 12 / 14 force the block shape of the tiled advectScalar passes, 0 or unset = by pass and grid size; set at all: no pair kernels") \
  X(STATS_CONSUMER,  "TFL_STATS_CONSUMER",  PRODUCT, PER_CALL, "=0 runs k_reduce_stats as its own launch instead of summing the partials in the first conv layer (the parity test flips it inside one process)") \
  X(VEL3_KZ,         "TFL_VEL3_KZ",         PRODUCT, ONCE,     "1 / >=2 force the one- / two-plane advectVel tile kernels, 0 or unset = by grid size; set at all: no pair kernels") \
  X(VORT_FUSED,      "TFL_VORT_FUSED",      PRODUCT, ONCE,     "0 = never, 1 = always take the fused confinement; unset (-1) = by grid size") \
  X(VORT_PIPE,       "TFL_VORT_PIPE",       PRODUCT, ONCE,     "=0 the three-barrier k_vort_fused instead of the pipelined k_vort_pipe; unset (-1) = pipelined") \
  X(ADVECT_GATHER,   "TFL_ADVECT_GATHER",   EXP,     ONCE,     "set at all: the round-2 gather kernels for advectVel and advectScalar, no pair kernels") \
  X(SCALAR_GATHER,   "TFL_SCALAR_GATHER",   EXP,     ONCE,     "set at all: the round-2 gather kernels for advectScalar only, no pair kernels") \
  X(CONV_DEBUG,      "TFL_CONV_DEBUG",      EXP,     ONCE,     "the debug word handed to k_conv3_mfma under TFL_CONV_TRACE (unset = 0)") \
  X(CONV_TRACE,      "TFL_CONV_TRACE",      EXP,     ONCE,     "set at all: per-block phase timestamps of every k_conv3_mfma launch on stderr (synchronises)") \
  X(M16_CZ,          "TFL_M16_CZ",          EXP,     PER_CALL, ">0 overrides the chosen chunk length of the 8 -> 8 and tail fp16 conv kernels (k_conv3_m16q / m16p / m16z)") \
  X(M16_CZ_F2,       "TFL_M16_CZ_F2",       EXP,     PER_CALL, ">0 overrides the chosen chunk length of k_conv3_m16p_f2 (the tests switch it inside one process)") \
  X(M16_CZ_IN,       "TFL_M16_CZ_IN",       EXP,     PER_CALL, ">0 overrides the chosen chunk length of k_conv3_m16p_in") \
  X(M16_FUSE12,      "TFL_M16_FUSE12",      EXP,     PER_CALL, "=1 runs conv layers 1 + 2 in one launch, k_conv3_m16p_f2 (the tests switch it inside one process)") \
  X(M16_KPACK,       "TFL_M16_KPACK",       EXP,     ONCE,     "0 = k_conv3_m16z and the tile kernel for the first layer, 2 = the tile kernel for the first layer only; unset = 1, the K-packed kernels") \
  X(M16_NT,          "TFL_M16_NT",          EXP,     PER_CALL, ">0 overrides the chosen z-tiles per block of the tile kernel k_conv3_m16") \
  X(M16_PIPE,        "TFL_M16_PIPE",        EXP,     PER_CALL, "=0 the un-pipelined k_conv3_m16p instead of k_conv3_m16q (the tests switch it inside one process)") \
  X(M16_STAGGER,     "TFL_M16_STAGGER",     EXP,     PER_CALL, "de-phased block starts of k_conv3_m16p in units of 64 clocks per wave slot (unset = 0, none)") \
  X(M16_STAGGER_F2,  "TFL_M16_STAGGER_F2",  EXP,     PER_CALL, "the same for k_conv3_m16p_f2") \
  X(M16_STAGGER_IN,  "TFL_M16_STAGGER_IN",  EXP,     PER_CALL, "the same for k_conv3_m16p_in") \
  X(M16_TAIL_MFMA,   "TFL_M16_TAIL_MFMA",   EXP,     PER_CALL, "=0 the tail's 1 x 1 x 1 layers on the vector ALUs, k_conv3_m16p (the tests switch it inside one process)") \
  X(M16_TILED,       "TFL_M16_TILED",       EXP,     PER_CALL, "bit 0 / bit 1 = the tile kernel k_conv3_m16 for the mid / tail layer (the tests switch it inside one process)") \
  X(NO_VEC4,         "TFL_NO_VEC4",         EXP,     ONCE,     "set at all: the one-cell-per-thread kernels instead of the four-cells-per-thread ones") \
  X(SCAL3M_CZ_A,     "TFL_SCAL3M_CZ_A",     EXP,     PER_CALL, ">0 overrides the chosen chunk length of pass A of the z-marched advectScalar") \
  X(SCAL3M_CZ_B,     "TFL_SCAL3M_CZ_B",     EXP,     PER_CALL, ">0 overrides the chosen chunk length of pass B of the z-marched advectScalar") \
  X(SCAL3_MARCH,     "TFL_SCAL3_MARCH",     EXP,     ONCE,     "=1 the z-marched advectScalar kernels (not under a forced TFL_SCAL3_TZ)") \
  X(SCAL3_SPARSE,    "TFL_SCAL3_SPARSE",    EXP,     ONCE,     "advectScalar of tfl_simulate_step over the list of non-empty bricks: 0 = never, 2 = always, 1 or unset = by the host policy (same bits either way)") \
  X(SCAL3_SEQ0,      "TFL_SCAL3_SEQ0",      EXP,     ONCE,     "the number of scans a density field's brick-list state starts from, as a 32-bit word (tests: -3 puts the wrap of the scan's number three scans away; unset = 0)") \
  X(SCAL3_ZSKIP,   "TFL_SCAL3_ZSKIP",     EXP,     ONCE,     "=0 turns the short path of all-zero advectScalar tiles off: every block traces (same bits either way)") \
  X(SLAB_WIDEN,      "TFL_SLAB_WIDEN",      EXP,     ONCE,     "planes added below and above every phase window of the z-slab step (development aid; unset = 0)") \
  X(STATS_FOLD,      "TFL_STATS_FOLD",      EXP,     PER_CALL, "=1 folds k_reduce_stats into the last block of k_bcs_div_stats (the tests switch it inside one process)") \
  X(VEL3_KZ_B,       "TFL_VEL3_KZ_B",       EXP,     ONCE,     "=2 keeps pass B of advectVel on the two-plane kernel when the buoyancy fold is asked for") \
  X(VORT_CZ,         "TFL_VORT_CZ",         EXP,     PER_CALL, ">0 overrides the chosen chunk length of k_vort_pipe / k_vort_fused") \
  X(VORT_TILE,       "TFL_VORT_TILE",       EXP,     ONCE,     "=32 k_vort_pipe on 32 x 16 tiles, two blocks per CU (unset = 64)") \
  X(WF_MAX_BLOCKS,   "TFL_WF_MAX_BLOCKS",   EXP,     ONCE,     ">0 caps the blocks per launch of the PCG wavefront pipeline, at least 1 (tests: small launches)") \
  X(WF_TEST_TIMEOUT, "TFL_WF_TEST_TIMEOUT", EXP,     ONCE,     "set at all: the wavefront pipeline reports a timeout (tests: the caller's fallback)") \
  X(WF_TRACE,        "TFL_WF_TRACE",        EXP,     ONCE,     "set at all: start and finish of every sub-box of the last PCG sweeps on stdout") \
  X(XCD_ORDER,       "TFL_XCD_ORDER",       EXP,     ONCE,     "=0 the hardware's block order everywhere, 1 = one run per XCD, unset (2) = an eighth of a plane per XCD") \
  X(XCD_RUN,         "TFL_XCD_RUN",         EXP,     ONCE,     ">0 tiles per run of the XCD-contiguous block order")
// clang-format on

namespace tfl {

#define TFL_SW_ID(id, name, flavour, when, meaning) id,
enum class Sw : int { TFL_SWITCH_TABLE(TFL_SW_ID) COUNT };
#undef TFL_SW_ID

namespace sw {

enum Flavour { PRODUCT, EXP };
enum When { ONCE, PER_CALL };
struct Row { const char* name; Flavour flavour; When when; };      // name == nullptr: not read by this flavour of the library

#define TFL_SW_NAME_PRODUCT(name) name
#ifdef TFL_EXPERIMENTS
#define TFL_SW_NAME_EXP(name) name
#else
#define TFL_SW_NAME_EXP(name) nullptr
#endif
#define TFL_SW_ROW(id, name, flavour, when, meaning) {TFL_SW_NAME_##flavour(name), flavour, when},
constexpr Row kRows[] = {TFL_SWITCH_TABLE(TFL_SW_ROW)};
#undef TFL_SW_ROW
#undef TFL_SW_NAME_EXP
#undef TFL_SW_NAME_PRODUCT
constexpr const Row& row(Sw s) { return kRows[(int)s]; }

// (forced inline: the row is a constant at every site, so the look-up folds to one getenv, one static or, for an EXP row in
// the product library, to "not set")
#define TFL_SW_INLINE inline __attribute__((always_inline))
struct Val { bool set; int num; };
inline Val read(const char* name) {
  const char* e = getenv(name);
  return Val{e != nullptr, e ? atoi(e) : 0};
}
template <Sw S>
inline Val once() {
  static const Val v = read(row(S).name);
  return v;
}
TFL_SW_INLINE Val get(Sw s) {
  if (!row(s).name) return Val{false, 0};
  if (row(s).when == PER_CALL) return read(row(s).name);
  switch (s) {
#define TFL_SW_CASE(id, var, flavour, mode, meaning) \
  case Sw::id:                                      \
    if constexpr (row(Sw::id).name != nullptr && row(Sw::id).when == ONCE) return once<Sw::id>(); else break;
    TFL_SWITCH_TABLE(TFL_SW_CASE)
#undef TFL_SW_CASE
    case Sw::COUNT: break;
  }
  return Val{false, 0};
}

TFL_SW_INLINE bool present(Sw s) { return get(s).set; }
TFL_SW_INLINE int num(Sw s, int dflt) {
  const Val v = get(s);
  return v.set ? v.num : dflt;
}
TFL_SW_INLINE const char* text(Sw s) { return row(s).name && row(s).when == PER_CALL ? getenv(row(s).name) : nullptr; }

#undef TFL_SW_INLINE

}  // namespace sw
}  // namespace tfl
