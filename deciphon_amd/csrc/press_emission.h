// press_emission.h -- the arithmetic of one emission table entry, for the kernels that make them: emission_kernel
// (press_kernel.hip: node-major tables, for press and for a load) and reemit_kernel (press_reemit.hip: a resident
// profile's rows at a new error rate, in place).  Device code only, and one source for both: everything is computed in
// double and rounded to fp32 once, so the same source under the same flags (-ffp-contract=off -fno-honor-nans) gives
// the same words in either kernel.  The formula and its treatment of e = 0 and e = 1 are described at press_kernel.hip.
#pragma once
#include <hip/hip_runtime.h>

namespace dcp_emission
{

constexpr int ANY = 4;
constexpr int INPUTS = 4 + 125; // nucltp[4], codonm[125] of an input entry (press_kernel.h)

struct State
{
  double const *p; // [4]
  double const *M; // [125]
  __device__ double m(int a, int b, int c) const { return M[a * 25 + b * 5 + c]; }
  __device__ double del1(int a, int b) const { return m(ANY, a, b) + m(a, ANY, b) + m(a, b, ANY); }
  __device__ double one(int a) const { return m(a, ANY, ANY) + m(ANY, a, ANY) + m(ANY, ANY, a); }
};

// an input (a log-probability, fp32) as the probability the formulas take
__device__ inline double input_prob(float lprob) { return exp((double)lprob); }

// ln(exp(x) + exp(y)) and ln(exp(x) + exp(y) + exp(z)); -inf when every argument is
__device__ inline double log_sum(double x, double y)
{
  double const hi = fmax(x, y);
  if (hi == -INFINITY) return hi;
  return hi + log(exp(x - hi) + exp(y - hi));
}

__device__ inline double log_sum(double x, double y, double z)
{
  double const hi = fmax(fmax(x, y), z);
  if (hi == -INFINITY) return hi;
  return hi + log(exp(x - hi) + exp(y - hi) + exp(z - hi));
}

// ln P(z) for n = |z| nucleotides; le = ln e, lf = ln(1 - e)
__device__ inline double emission_lprob(State const &s, double le, double lf, int n, int const *z)
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

// code -> its nucleotides z[0..n), first most significant; returns n (offsets 0, 4, 20, 84, 340)
__device__ inline int decode(int code, int *z)
{
  int n, idx;
  if (code < 4) n = 1, idx = code;
  else if (code < 20) n = 2, idx = code - 4;
  else if (code < 84) n = 3, idx = code - 20;
  else if (code < 340) n = 4, idx = code - 84;
  else n = 5, idx = code - 340;
  for (int j = n - 1; j >= 0; --j, idx >>= 2) z[j] = idx & 3;
  return n;
}

} // namespace dcp_emission
