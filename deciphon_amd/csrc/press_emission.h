// press_emission.h -- the arithmetic of one emission table entry, for the kernels that make them: emission_kernel
// (press_kernel.hip: node-major tables, for press and for a load) and reemit_kernel (press_reemit.hip: a resident
// profile's rows at a new error rate, in place).  Device code only, and one source for both: everything is computed in
// double and rounded to fp32 once, so the same source under the same flags (-ffp-contract=off -fno-honor-nans) gives
// the same words in either kernel.  The formula and its treatment of e = 0 and e = 1 are described at press_kernel.hip.
//
// The two terms that stand alone in a 3-mer at small and at large e are (1 - e)^4 M and e^4 p p p, and there ln P falls
// on or beside the midpoint of two fp32 values as a matter of structure, not of chance: a sum of three fp32 values at
// e = 1, x - 2^-23 - 2^-49 + .. at e = 2^-25.  Three things keep a 3-mer's word the nearest fp32 there
// (tests/test_gpu_emission_exact.py; without them 14 of 21 770 words went to the other neighbour at e = 2^-25, 4 of 1024
// at e = 1).  The log of a polynomial that is a single input, or a product of inputs, is never log(exp(x)): it is the
// fp32 input itself, or the sum of the inputs, which is exact in double.  The largest term t is split into that exact
// part and the rest, ln P = exact + (rest + log1p(sum of the other terms / t)), so that only one sum is rounded at the
// size of ln P.  And that one sum is narrowed by narrow_sum: rounded to odd in double, then to nearest in fp32, which
// rounds as from the exact sum.
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
  float const *lp; // [INPUTS]: the inputs themselves, log-probabilities, where the kernel was given them
  __device__ double log_p(int a) const { return (double)lp[a]; }
  __device__ double log_m(int a, int b, int c) const { return (double)lp[4 + a * 25 + b * 5 + c]; }
  __device__ double m(int a, int b, int c) const { return M[a * 25 + b * 5 + c]; }
  __device__ double del1(int a, int b) const { return m(ANY, a, b) + m(a, ANY, b) + m(a, b, ANY); }
  __device__ double one(int a) const { return m(a, ANY, ANY) + m(ANY, a, ANY) + m(ANY, ANY, a); }
};

// an input (a log-probability, fp32) as the probability the formulas take
__device__ inline double input_prob(float lprob) { return exp((double)lprob); }

// ln(exp(x) + exp(y)); -inf when both arguments are
__device__ inline double log_sum(double x, double y)
{
  double const hi = fmax(x, y);
  if (hi == -INFINITY) return hi;
  return hi + log(exp(x - hi) + exp(y - hi));
}

// The fp32 nearest base + small.  The double sum is rounded to odd -- Fast2Sum gives its error exactly, and an inexact
// sum with an even last bit moves one step towards the error -- so the narrowing, with 29 bits to spare, rounds as from
// the exact sum.  -inf when the sum is.
__device__ inline float narrow_sum(double base, double small)
{
  double const sum = base + small;
  if (sum == -INFINITY) return (float)sum;
  double const err = fabs(base) >= fabs(small) ? small - (sum - base) : base - (sum - small);
  if (err == 0.0) return (float)sum;
  long long bits = __double_as_longlong(sum);
  if ((bits & 1) == 0) bits += (err > 0.0) == (sum > 0.0) ? 1 : -1;
  return (float)__longlong_as_double(bits);
}

// ln P(z) for n = |z| nucleotides, as fp32; le = ln e, lf = ln(1 - e)
__device__ inline float emission_lprob(State const &s, double le, double lf, int n, int const *z)
{
  double const *p = s.p;
  if (n == 1) return (float)(log(1.0 / 3.0) + 2.0 * le + 2.0 * lf + log(s.one(z[0])));
  if (n == 2)
    return (float)log_sum(log(2.0 / 3.0) + le + 3.0 * lf + log(s.del1(z[0], z[1])),
                          log(1.0 / 3.0) + 3.0 * le + lf + log(p[z[0]] * s.one(z[1]) + p[z[1]] * s.one(z[0])));
  if (n == 3)
  {
    // each term as (what e gives) + (what the inputs give); the latter is exact for the first and the last
    double const e0 = 4.0 * lf, i0 = s.log_m(z[0], z[1], z[2]);
    double const e1 = log(4.0 / 9.0) + 2.0 * le + 2.0 * lf;
    double const i1 =
        log(p[z[0]] * s.del1(z[1], z[2]) + p[z[1]] * s.del1(z[0], z[2]) + p[z[2]] * s.del1(z[0], z[1]));
    double const e2 = 4.0 * le, i2 = s.log_p(z[0]) + s.log_p(z[1]) + s.log_p(z[2]);
    double const t0 = e0 + i0, t1 = e1 + i1, t2 = e2 + i2;
    double const hi = fmax(fmax(t0, t1), t2);
    if (hi == -INFINITY) return (float)hi;
    if (t0 == hi) return narrow_sum(i0, e0 + log1p(exp(t1 - hi) + exp(t2 - hi)));
    if (t1 == hi) return narrow_sum(i1, e1 + log1p(exp(t0 - hi) + exp(t2 - hi)));
    return narrow_sum(i2, e2 + log1p(exp(t0 - hi) + exp(t1 - hi)));
  }
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
    return (float)log_sum(log(1.0 / 2.0) + le + 3.0 * lf + log(a), log(1.0 / 9.0) + 3.0 * le + lf + log(b));
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
  return (float)(log(1.0 / 10.0) + 2.0 * le + 2.0 * lf + log(v));
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
