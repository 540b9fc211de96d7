// lane_conf_emul.cpp -- TEST INFRASTRUCTURE ONLY.
// The cases of lane_cases.h on the wave emulator's vocabulary (tests/emul/lane_ops_emul.h), behind the C ABI that
// lane_conf.hip gives the GPU's: tests/test_lane_ops_emul.py, tests/test_gpu_lane_ops.py.
#include "../emul/lane_ops_emul.h"
#include "../../deciphon_amd/csrc/viterbi_body.h" // lane_shift_up_again as the emulated kernels have it
#include "../../deciphon_amd/csrc/traceback.h"    // DcpLanesHost

thread_local long em_fallback_rows = 0;
thread_local long em_row_range_zeros = 0;
thread_local long em_votes = 0, em_votes_true = 0;

#define LANE_POLICY DcpLanesHost

struct ConfArgs
{
  uint32_t const *in;   // [nvec][nin][lanes]
  uint32_t *out;        // [nvec][nout][lanes]
  uint32_t const *scal; // [nvec][nscal]
  uint32_t const *mem;  // shared, read-only
  uint32_t *omem;       // [nvec][omem_words]
  int nin, nout, nscal, omem_words, lanes;
};

static float as_f(uint32_t u)
{
  float f;
  memcpy(&f, &u, 4);
  return f;
}
static uint32_t as_u(float f)
{
  uint32_t u;
  memcpy(&u, &f, 4);
  return u;
}

struct LaneIO
{
  ConfArgs const &a;
  int vec;
  uint32_t const *inp(int j) const { return a.in + ((size_t)vec * a.nin + j) * a.lanes; }
  uint32_t *outp(int j) const { return a.out + ((size_t)vec * a.nout + j) * a.lanes; }
  lf f(int j) const
  {
    lf r;
    memcpy(r.v, inp(j), 4 * (size_t)a.lanes);
    return r;
  }
  lu u(int j) const
  {
    lu r;
    memcpy(r.v, inp(j), 4 * (size_t)a.lanes);
    return r;
  }
  void of(int j, lf const &x) const { memcpy(outp(j), x.v, 4 * (size_t)a.lanes); }
  void ou(int j, lu const &x) const { memcpy(outp(j), x.v, 4 * (size_t)a.lanes); }
  void om(int j, lm const &x) const
  {
    for (int i = 0; i < a.lanes; ++i) outp(j)[i] = x.v[i] ? 1u : 0u;
  }
  void osu(int j, uint32_t x) const
  {
    for (int i = 0; i < a.lanes; ++i) outp(j)[i] = x;
  }
  void osf(int j, float x) const { osu(j, as_u(x)); }
  void osb(int j, bool x) const { osu(j, x ? 1u : 0u); }
  void os64(int j, uint64_t x) const
  {
    osu(j, (uint32_t)x);
    osu(j + 1, (uint32_t)(x >> 32));
  }
  uint32_t su(int s) const { return a.scal[(size_t)vec * a.nscal + s]; }
  int si(int s) const { return (int)su(s); }
  float sf(int s) const { return as_f(su(s)); }
  float const *mem() const { return reinterpret_cast<float const *>(a.mem); }
  uint32_t const *memu() const { return a.mem; }
  float *omem() const { return reinterpret_cast<float *>(a.omem + (size_t)vec * a.omem_words); }
  uint32_t *omemu() const { return a.omem + (size_t)vec * a.omem_words; }
  lds_float const *lds(int) const { return mem(); }
};

#include "lane_cases.h"

template <class Case> static int run_case(ConfArgs const &a, int nvec)
{
  static thread_local Case c; // 64 W-lane vectors are large: off the stack
  if (a.lanes != 64 * Case::W) return -2;
  for (int v = 0; v < nvec; ++v)
  {
    em_lanes = a.lanes;
    LaneIO io{a, v};
    c.run(io);
  }
  em_lanes = 64;
  return 0;
}

struct CaseInfo
{
  char const *name, *ops;
  int W, nin, nout;
  int (*run)(ConfArgs const &, int);
};
#define LC_ENTRY(NAME, OPS, NIN, NOUT, ...) {NAME, OPS, __VA_ARGS__::W, NIN, NOUT, run_case<__VA_ARGS__>},
static CaseInfo const cases[] = {LANE_CASES(LC_ENTRY)};
static int const ncases = (int)(sizeof cases / sizeof cases[0]);

extern "C" int lane_conf_count(void) { return ncases; }
extern "C" char const *lane_conf_name(int i) { return i >= 0 && i < ncases ? cases[i].name : nullptr; }
extern "C" char const *lane_conf_ops(int i) { return i >= 0 && i < ncases ? cases[i].ops : nullptr; }
// dims[3] = wavefronts of the group (64 W lanes), per-lane inputs, per-lane outputs
extern "C" int lane_conf_dims(int i, int *dims)
{
  if (i < 0 || i >= ncases) return -1;
  dims[0] = cases[i].W;
  dims[1] = cases[i].nin;
  dims[2] = cases[i].nout;
  return 0;
}
// 0, or negative: no such case / the arrays are not the case's.  `out` is zeroed first.
extern "C" int lane_conf_run(int i, int nvec, uint32_t const *in, uint32_t *out, uint32_t const *scal, int nscal,
                             uint32_t const *mem, long mem_words, uint32_t *omem, int omem_words)
{
  if (i < 0 || i >= ncases || nvec < 1 || nscal < 1 || mem_words < 1 || omem_words < 1) return -1;
  CaseInfo const &c = cases[i];
  ConfArgs a{in, out, scal, mem, omem, c.nin, c.nout, nscal, omem_words, 64 * c.W};
  memset(out, 0, 4 * (size_t)nvec * (size_t)c.nout * (size_t)a.lanes);
  return c.run(a, nvec);
}
// reads that load_row_q / load_row_chunks answered by the range rule since the last call
extern "C" long lane_conf_row_range_zeros(void)
{
  long const n = em_row_range_zeros;
  em_row_range_zeros = 0;
  return n;
}
