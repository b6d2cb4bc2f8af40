// A stand-alone host program over fluidnet_amd/csrc/tfl_switches.hpp, the library's one table and one reader of its TFL_*
// environment variables: it sets and clears every variable of the table and checks what sw::present / sw::num / sw::text
// answer -- a ONCE row keeps what its first read saw, a PER_CALL row follows the environment, num is atoi of the text or
// the default, "0" counts as set, and without -DTFL_EXPERIMENTS every EXP row reads as not set. No GPU, no HIP call.
// Built twice and run by tests/test_switches_cpu.py:  g++ -std=c++17 -pthread -fsanitize=address,undefined [-DTFL_EXPERIMENTS]
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <vector>

#include "../fluidnet_amd/csrc/tfl_switches.hpp"

#define CHECK(c) do { if (!(c)) { std::fprintf(stderr, "%s:%d: CHECK(%s) failed (row %s)\n", __FILE__, __LINE__, #c, g_row); std::exit(1); } } while (0)

using namespace tfl;

static const char* g_row = "-";

// the table again, with every name (the reader's own rows hold no EXP name in the plain build)
struct Named { Sw id; const char* name; sw::Flavour flavour; sw::When when; };
#define NAMED(id, var, flavour, mode, meaning) {Sw::id, var, sw::flavour, sw::mode},
static const Named kNamed[] = {TFL_SWITCH_TABLE(NAMED)};
#undef NAMED
constexpr int kCount = (int)Sw::COUNT;

#ifdef TFL_EXPERIMENTS
constexpr bool kExperiments = true;
#else
constexpr bool kExperiments = false;
#endif

static void put(const char* name, const char* value) {
  if (value) CHECK(setenv(name, value, 1) == 0);
  else CHECK(unsetenv(name) == 0);
}
// what row i holds before its first read: nothing, "0", or a number with a tail atoi stops at
static const char* first_value(int i) {
  if (kNamed[i].id == Sw::VORT_FUSED) return "1";            // the row the threads read first
  if (kNamed[i].id == Sw::PCG_HYPERPLANES) return "0";       // (its site tests presence: =0 selects hyperplanes too)
  static const char* const v[3] = {nullptr, "0", "-12abc"};
  return v[i % 3];
}
static void check_reads(int i, const char* value) {        // the row answers as for `value` in the environment
  const Sw s = kNamed[i].id;
  CHECK(sw::present(s) == (value != nullptr));
  CHECK(sw::num(s, 7) == (value ? atoi(value) : 7));
  CHECK(sw::num(s, -3) == (value ? atoi(value) : -3));
}

int main() {
  static_assert(sizeof(sw::kRows) / sizeof(sw::kRows[0]) == (size_t)kCount, "one reader row per id");
  static_assert(sizeof(kNamed) / sizeof(kNamed[0]) == (size_t)kCount, "one named row per id");
  int n_once = 0, n_exp = 0;
  for (int i = 0; i < kCount; i++) {
    g_row = kNamed[i].name;
    const sw::Row& r = sw::row(kNamed[i].id);
    CHECK((int)kNamed[i].id == i && strncmp(kNamed[i].name, "TFL_", 4) == 0);
    CHECK(r.flavour == kNamed[i].flavour && r.when == kNamed[i].when);
    const bool readable = kExperiments || r.flavour == sw::PRODUCT;
    CHECK(readable ? (r.name && strcmp(r.name, kNamed[i].name) == 0) : r.name == nullptr);
    n_once += r.when == sw::ONCE; n_exp += r.flavour == sw::EXP;
    put(kNamed[i].name, first_value(i));
  }
  CHECK(n_once > 0 && n_once < kCount && n_exp > 0 && n_exp < kCount);

  // concurrent first reads of one ONCE row agree (nothing writes the environment meanwhile)
  g_row = "TFL_VORT_FUSED";
  CHECK(sw::row(Sw::VORT_FUSED).when == sw::ONCE && sw::row(Sw::VORT_FUSED).flavour == sw::PRODUCT);
  {
    int seen[8][2];
    std::vector<std::thread> th;
    for (int t = 0; t < 8; t++) th.emplace_back([&seen, t] { seen[t][0] = sw::present(Sw::VORT_FUSED); seen[t][1] = sw::num(Sw::VORT_FUSED, -1); });
    for (auto& t : th) t.join();
    for (int t = 0; t < 8; t++) CHECK(seen[t][0] == 1 && seen[t][1] == 1);
  }

  for (int i = 0; i < kCount; i++) {
    g_row = kNamed[i].name;
    const Named& r = kNamed[i];
    const bool readable = kExperiments || r.flavour == sw::PRODUCT;
    const char* v0 = first_value(i);
    // first read
    check_reads(i, readable ? v0 : nullptr);
    // the variable changes: a ONCE row keeps its first value, a PER_CALL row follows
    const char* v1 = v0 && atoi(v0) == 91 ? "19" : "91";
    put(r.name, v1);
    check_reads(i, !readable ? nullptr : (r.when == sw::ONCE ? v0 : v1));
    put(r.name, "0");        // set to "0" is set
    check_reads(i, !readable ? nullptr : (r.when == sw::ONCE ? v0 : "0"));
    // text: PER_CALL rows only, and never a kept pointer
    const char* t = sw::text(r.id);
    if (readable && r.when == sw::PER_CALL) CHECK(t && strcmp(t, "0") == 0);
    else CHECK(t == nullptr);
    put(r.name, nullptr);
    check_reads(i, !readable ? nullptr : (r.when == sw::ONCE ? v0 : nullptr));
    CHECK(sw::text(r.id) == nullptr);
  }

  // the text-valued rows
  const Sw texts[3] = {Sw::CONV_PATH, Sw::ADVECT_MODE, Sw::RCCL_LIBRARY};
  for (Sw s : texts) {
    g_row = kNamed[(int)s].name;
    CHECK(sw::row(s).when == sw::PER_CALL && sw::row(s).flavour == sw::PRODUCT);
    put(kNamed[(int)s].name, "winograd");
    CHECK(sw::text(s) && strcmp(sw::text(s), "winograd") == 0 && sw::present(s) && sw::num(s, 5) == 0);
    put(kNamed[(int)s].name, "");
    CHECK(sw::text(s) && sw::text(s)[0] == 0 && sw::present(s));
    put(kNamed[(int)s].name, nullptr);
    CHECK(sw::text(s) == nullptr && !sw::present(s));
  }
  std::printf("switches OK (%d rows, %d ONCE, %d EXP, %s)\n", kCount, n_once, n_exp, kExperiments ? "EXPERIMENTS" : "product");
  return 0;
}
