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
// LDS, lanes stride over the codes and each row of 1364 floats is stored coalesced.  Sums are taken in probability
// space -- every term is a product of probabilities, so nothing cancels -- and the log is the accurate logf.  With
// e = 0 every term of a code of length != 3 is 0 * (a finite probability) = 0, and logf(0) = -inf exactly.
#include "press_kernel.h"

#include <hip/hip_runtime.h>

namespace
{

constexpr int ANY = 4;
constexpr int THREADS = 256;

struct State
{
  float const *p; // [4]
  float const *M; // [125]
  __device__ float m(int a, int b, int c) const { return M[a * 25 + b * 5 + c]; }
  __device__ float del1(int a, int b) const { return m(ANY, a, b) + m(a, ANY, b) + m(a, b, ANY); }
  __device__ float one(int a) const { return m(a, ANY, ANY) + m(ANY, a, ANY) + m(ANY, ANY, a); }
};

__device__ float emission_prob(State const &s, float e, int n, int const *z)
{
  float const f = 1.0f - e;
  float const *p = s.p;
  if (n == 1) return e * e * f * f / 3.0f * s.one(z[0]);
  if (n == 2)
    return 2.0f * e * f * f * f / 3.0f * s.del1(z[0], z[1]) +
           e * e * e * f / 3.0f * (p[z[0]] * s.one(z[1]) + p[z[1]] * s.one(z[0]));
  if (n == 3)
  {
    float v = f * f * f * f * s.m(z[0], z[1], z[2]);
    v += 4.0f * e * e * f * f / 9.0f *
         (p[z[0]] * s.del1(z[1], z[2]) + p[z[1]] * s.del1(z[0], z[2]) + p[z[2]] * s.del1(z[0], z[1]));
    return v + e * e * e * e * p[z[0]] * p[z[1]] * p[z[2]];
  }
  if (n == 4)
  {
    // one base inserted (j) into a codon, or two inserted (i, j) into a codon with one base deleted
    float a = p[z[0]] * s.m(z[1], z[2], z[3]) + p[z[1]] * s.m(z[0], z[2], z[3]) + p[z[2]] * s.m(z[0], z[1], z[3]) +
              p[z[3]] * s.m(z[0], z[1], z[2]);
    float b = 0.0f;
    for (int i = 0; i < 4; ++i)
      for (int j = i + 1; j < 4; ++j)
      {
        int r[2], k = 0;
        for (int t = 0; t < 4; ++t)
          if (t != i && t != j) r[k++] = z[t];
        b += p[z[i]] * p[z[j]] * s.del1(r[0], r[1]);
      }
    return e * f * f * f / 2.0f * a + e * e * e * f / 9.0f * b;
  }
  float v = 0.0f; // n == 5: two bases inserted (i, j) into a codon
  for (int i = 0; i < 5; ++i)
    for (int j = i + 1; j < 5; ++j)
    {
      int r[3], k = 0;
      for (int t = 0; t < 5; ++t)
        if (t != i && t != j) r[k++] = z[t];
      v += p[z[i]] * p[z[j]] * s.m(r[0], r[1], r[2]);
    }
  return e * e * f * f / 10.0f * v;
}

__global__ __launch_bounds__(THREADS) void emission_kernel(float const *__restrict__ in, float *__restrict__ out,
                                                           float epsilon)
{
  __shared__ float prob[DCP_PRESS_IN_STRIDE];
  int const tid = (int)threadIdx.x;
  size_t const entry = blockIdx.x;
  if (tid < 4 + 125) prob[tid] = expf(in[entry * DCP_PRESS_IN_STRIDE + (size_t)tid]);
  __syncthreads();
  State const s{prob, prob + 4};
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
    row[code] = logf(emission_prob(s, epsilon, n, z));
  }
}

} // namespace

int dcp_press_emission_launch(float const *in, float *out, int entries, float epsilon, hipStream_t stream)
{
  if (entries <= 0) return 0;
  hipLaunchKernelGGL(emission_kernel, dim3((unsigned)entries), dim3(THREADS), 0, stream, in, out, epsilon);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}
