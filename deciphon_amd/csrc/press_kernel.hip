// press_kernel.hip -- the emission tables of press on the GPU.
//
// What imm_score_table_scores does per state in the reference (c-core/protein.c:98-106, on the CPU, one node at a
// time): log P(z) of each of the 1364 quasi-codon codes z (1..5 nucleotides; code = offset[|z| - 1] + z read as a
// base-4 number, first nucleotide most significant; offsets 0, 4, 20, 84, 340) for a frame state with nucleotide
// distribution p = exp(nucltp[4]), codon marginals M = exp(codonm[125]) and error rate e.  The formula is the
// marginal form of the quasi-codon model (host_logic.h, oracle/pydecode.py: emission_prob), which reproduces the
// reference's pressed tables (tests/test_decoder.py).
//
// One workgroup per entry (a node, or the null or background model): its 129 inputs are exponentiated once into
// LDS, lanes stride over the codes and each row of 1364 floats is stored coalesced.
//
// Every code length's P(z) is a sum of at most three terms c e^a f^b poly(p, M), f = 1 - e, a + b <= 4.  In fp32
// probability space these products underflow long before log P(z) leaves its range: e^2 at e < 1e-19 (log P is
// still about -100 at e = 1e-22), and p p M of an almost one-hot emission at any e.  So each term is taken as its
// log, ln c + a ln e + b ln f + ln poly, in double, and the terms are combined by a max-shifted sum.  The
// polynomials are sums of products of at most three probabilities, in double from the fp32 log inputs.  A zero power is left out of its term, never written as 0 * ln 0: with e = 0 or
// e = 1 the terms that vanish are -inf (a positive multiple of -inf, or ln 0), nothing is NaN, and a code whose
// terms all vanish is -inf exactly.  No term is ever +inf.  The result is rounded to fp32 once, at the end.
#include "press_kernel.h"

#include <hip/hip_runtime.h>

namespace
{

constexpr int ANY = 4;
constexpr int THREADS = 256;

struct State
{
  double const *p; // [4]
  double const *M; // [125]
  __device__ double m(int a, int b, int c) const { return M[a * 25 + b * 5 + c]; }
  __device__ double del1(int a, int b) const { return m(ANY, a, b) + m(a, ANY, b) + m(a, b, ANY); }
  __device__ double one(int a) const { return m(a, ANY, ANY) + m(ANY, a, ANY) + m(ANY, ANY, a); }
};

// ln(exp(x) + exp(y)) and ln(exp(x) + exp(y) + exp(z)); -inf when every argument is
__device__ double log_sum(double x, double y)
{
  double const hi = fmax(x, y);
  if (hi == -INFINITY) return hi;
  return hi + log(exp(x - hi) + exp(y - hi));
}

__device__ double log_sum(double x, double y, double z)
{
  double const hi = fmax(fmax(x, y), z);
  if (hi == -INFINITY) return hi;
  return hi + log(exp(x - hi) + exp(y - hi) + exp(z - hi));
}

// ln P(z) for n = |z| nucleotides; le = ln e, lf = ln(1 - e)
__device__ double emission_lprob(State const &s, double le, double lf, int n, int const *z)
{
  double const *p = s.p;
  if (n == 1) return log(1.0 / 3.0) + 2.0 * le + 2.0 * lf + log(s.one(z[0]));
  if (n == 2)
    return log_sum(log(2.0 / 3.0) + le + 3.0 * lf + log(s.del1(z[0], z[1])),
                   log(1.0 / 3.0) + 3.0 * le + lf + log(p[z[0]] * s.one(z[1]) + p[z[1]] * s.one(z[0])));
  if (n == 3)
    return log_sum(4.0 * lf + log(s.m(z[0], z[1], z[2])),
                   log(4.0 / 9.0) + 2.0 * le + 2.0 * lf +
                       log(p[z[0]] * s.del1(z[1], z[2]) + p[z[1]] * s.del1(z[0], z[2]) + p[z[2]] * s.del1(z[0], z[1])),
                   4.0 * le + log(p[z[0]] * p[z[1]] * p[z[2]]));
  if (n == 4)
  {
    // one base inserted (j) into a codon, or two inserted (i, j) into a codon with one base deleted
    double a = p[z[0]] * s.m(z[1], z[2], z[3]) + p[z[1]] * s.m(z[0], z[2], z[3]) + p[z[2]] * s.m(z[0], z[1], z[3]) +
               p[z[3]] * s.m(z[0], z[1], z[2]);
    double b = 0.0;
    for (int i = 0; i < 4; ++i)
      for (int j = i + 1; j < 4; ++j)
      {
        int r[2], k = 0;
        for (int t = 0; t < 4; ++t)
          if (t != i && t != j) r[k++] = z[t];
        b += p[z[i]] * p[z[j]] * s.del1(r[0], r[1]);
      }
    return log_sum(log(1.0 / 2.0) + le + 3.0 * lf + log(a), log(1.0 / 9.0) + 3.0 * le + lf + log(b));
  }
  double v = 0.0; // n == 5: two bases inserted (i, j) into a codon
  for (int i = 0; i < 5; ++i)
    for (int j = i + 1; j < 5; ++j)
    {
      int r[3], k = 0;
      for (int t = 0; t < 5; ++t)
        if (t != i && t != j) r[k++] = z[t];
      v += p[z[i]] * p[z[j]] * s.m(r[0], r[1], r[2]);
    }
  return log(1.0 / 10.0) + 2.0 * le + 2.0 * lf + log(v);
}

__global__ __launch_bounds__(THREADS) void emission_kernel(float const *__restrict__ in, float *__restrict__ out,
                                                           float epsilon)
{
  __shared__ double prob[DCP_PRESS_IN_STRIDE];
  int const tid = (int)threadIdx.x;
  size_t const entry = blockIdx.x;
  if (tid < 4 + 125) prob[tid] = exp((double)in[entry * DCP_PRESS_IN_STRIDE + (size_t)tid]);
  __syncthreads();
  State const s{prob, prob + 4};
  double const le = log((double)epsilon), lf = log1p(-(double)epsilon);
  float *row = out + entry * DCP_PRESS_TABLE;
  for (int code = tid; code < DCP_PRESS_TABLE; code += THREADS)
  {
    int n, idx;
    if (code < 4) n = 1, idx = code;
    else if (code < 20) n = 2, idx = code - 4;
    else if (code < 84) n = 3, idx = code - 20;
    else if (code < 340) n = 4, idx = code - 84;
    else n = 5, idx = code - 340;
    int z[5];
    for (int j = n - 1; j >= 0; --j, idx >>= 2) z[j] = idx & 3;
    row[code] = (float)emission_lprob(s, le, lf, n, z);
  }
}

} // namespace

int dcp_press_emission_launch(float const *in, float *out, int entries, float epsilon, hipStream_t stream)
{
  if (entries <= 0) return 0;
  hipLaunchKernelGGL(emission_kernel, dim3((unsigned)entries), dim3(THREADS), 0, stream, in, out, epsilon);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}
