// lane_conf.hip -- TEST INFRASTRUCTURE ONLY.
// The cases of lane_cases.h on the GPU's own vocabulary (deciphon_amd/csrc/lane_ops_gpu.h): every case a kernel of
// 64 W threads, one workgroup per input vector, behind the C ABI of lane_conf_emul.cpp (tests/test_gpu_lane_ops.py).
#include "../../deciphon_amd/csrc/lane_ops_gpu.h"

#define LANE_POLICY DcpLanesWave
#define CONF_LDS_WORDS 2048

struct ConfArgs
{
  uint32_t const *in;   // [nvec][nin][lanes]
  uint32_t *out;        // [nvec][nout][lanes]
  uint32_t const *scal; // [nvec][nscal]
  uint32_t const *mem;  // shared, read-only
  uint32_t *omem;       // [nvec][omem_words]
  int nin, nout, nscal, omem_words, lanes;
};

struct LaneIO
{
  ConfArgs const &a;
  uint32_t vec, tid;
  DCP_FN uint32_t const *inp(int j) const { return a.in + ((size_t)vec * a.nin + j) * a.lanes + tid; }
  DCP_FN uint32_t *outp(int j) const { return a.out + ((size_t)vec * a.nout + j) * a.lanes + tid; }
  DCP_FN lf f(int j) const { return __uint_as_float(*inp(j)); }
  DCP_FN lu u(int j) const { return *inp(j); }
  DCP_FN void of(int j, lf x) const { *outp(j) = __float_as_uint(x); }
  DCP_FN void ou(int j, lu x) const { *outp(j) = x; }
  DCP_FN void om(int j, lm x) const { *outp(j) = x ? 1u : 0u; }
  DCP_FN void osu(int j, uint32_t x) const { *outp(j) = x; }
  DCP_FN void osf(int j, float x) const { *outp(j) = __float_as_uint(x); }
  DCP_FN void osb(int j, bool x) const { *outp(j) = x ? 1u : 0u; }
  DCP_FN void os64(int j, uint64_t x) const
  {
    osu(j, (uint32_t)x);
    osu(j + 1, (uint32_t)(x >> 32));
  }
  DCP_FN uint32_t su(int s) const { return a.scal[(size_t)vec * a.nscal + s]; }
  DCP_FN int si(int s) const { return (int)su(s); }
  DCP_FN float sf(int s) const { return __uint_as_float(su(s)); }
  DCP_FN float const *mem() const { return reinterpret_cast<float const *>(a.mem); }
  DCP_FN uint32_t const *memu() const { return a.mem; }
  DCP_FN float *omem() const { return reinterpret_cast<float *>(a.omem + (size_t)vec * a.omem_words); }
  DCP_FN uint32_t *omemu() const { return a.omem + (size_t)vec * a.omem_words; }
  DCP_FN lds_float const *lds(int n) const
  {
    __shared__ __attribute__((aligned(16))) float table[CONF_LDS_WORDS];
    for (int i = (int)tid; i < n && i < CONF_LDS_WORDS; i += a.lanes) table[i] = mem()[i];
    __syncthreads();
    return (lds_float const *)table;
  }
};

#include "lane_cases.h"

template <class Case> __global__ void __launch_bounds__(64 * Case::W) conf_kernel(ConfArgs a)
{
  LaneIO io{a, blockIdx.x, threadIdx.x};
  Case c;
  c.run(io);
}

template <class Case> static void launch_case(ConfArgs const &a, int nvec)
{
  hipLaunchKernelGGL(conf_kernel<Case>, dim3((unsigned)nvec), dim3(64 * Case::W), 0, 0, a);
}

struct CaseInfo
{
  char const *name, *ops;
  int W, nin, nout;
  void (*launch)(ConfArgs const &, int);
};
#define LC_ENTRY(NAME, OPS, NIN, NOUT, ...) {NAME, OPS, __VA_ARGS__::W, NIN, NOUT, launch_case<__VA_ARGS__>},
static CaseInfo const cases[] = {LANE_CASES(LC_ENTRY)};
static int const ncases = (int)(sizeof cases / sizeof cases[0]);

extern "C" int lane_conf_count(void) { return ncases; }
extern "C" char const *lane_conf_name(int i) { return i >= 0 && i < ncases ? cases[i].name : nullptr; }
extern "C" char const *lane_conf_ops(int i) { return i >= 0 && i < ncases ? cases[i].ops : nullptr; }
extern "C" int lane_conf_dims(int i, int *dims)
{
  if (i < 0 || i >= ncases) return -1;
  dims[0] = cases[i].W;
  dims[1] = cases[i].nin;
  dims[2] = cases[i].nout;
  return 0;
}

// 0, negative (no such case), or the HIP error of the first call that failed.  `out` is zeroed first.
extern "C" int lane_conf_run(int i, int nvec, uint32_t const *in, uint32_t *out, uint32_t const *scal, int nscal,
                             uint32_t const *mem, long mem_words, uint32_t *omem, int omem_words)
{
  if (i < 0 || i >= ncases || nvec < 1 || nscal < 1 || mem_words < 1 || omem_words < 1) return -1;
  CaseInfo const &c = cases[i];
  int const lanes = 64 * c.W;
  size_t const b_in = 4 * (size_t)nvec * (size_t)c.nin * lanes, b_out = 4 * (size_t)nvec * (size_t)c.nout * lanes;
  size_t const b_scal = 4 * (size_t)nvec * (size_t)nscal, b_mem = 4 * (size_t)mem_words;
  size_t const b_omem = 4 * (size_t)nvec * (size_t)omem_words;
  uint32_t *d_in = nullptr, *d_out = nullptr, *d_scal = nullptr, *d_mem = nullptr, *d_omem = nullptr;
  hipError_t e = hipSuccess;
  auto step = [&](hipError_t r) {
    if (e == hipSuccess) e = r;
    return e == hipSuccess;
  };
  // (a zero-sized array of the case still gets a word, so that no pointer is null)
  step(hipMalloc(&d_in, b_in + 4)) && step(hipMalloc(&d_out, b_out + 4)) && step(hipMalloc(&d_scal, b_scal)) &&
      step(hipMalloc(&d_mem, b_mem)) && step(hipMalloc(&d_omem, b_omem)) &&
      step(b_in ? hipMemcpy(d_in, in, b_in, hipMemcpyHostToDevice) : hipSuccess) &&
      step(hipMemset(d_out, 0, b_out + 4)) && step(hipMemcpy(d_scal, scal, b_scal, hipMemcpyHostToDevice)) &&
      step(hipMemcpy(d_mem, mem, b_mem, hipMemcpyHostToDevice)) &&
      step(hipMemcpy(d_omem, omem, b_omem, hipMemcpyHostToDevice));
  if (e == hipSuccess)
  {
    ConfArgs a{d_in, d_out, d_scal, d_mem, d_omem, c.nin, c.nout, nscal, omem_words, lanes};
    c.launch(a, nvec);
    step(hipGetLastError()) && step(hipDeviceSynchronize()) &&
        step(b_out ? hipMemcpy(out, d_out, b_out, hipMemcpyDeviceToHost) : hipSuccess) &&
        step(hipMemcpy(omem, d_omem, b_omem, hipMemcpyDeviceToHost));
  }
  (void)hipFree(d_in);
  (void)hipFree(d_out);
  (void)hipFree(d_scal);
  (void)hipFree(d_mem);
  (void)hipFree(d_omem);
  return (int)e;
}
