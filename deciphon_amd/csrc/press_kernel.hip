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
// polynomials are sums of products of at most three probabilities, in double from the fp32 log inputs; a 3-mer, whose
// ln P lies beside fp32 midpoints by structure, keeps its exact parts apart to the end (press_emission.h).  A zero
// power is left out of its term, never written as 0 * ln 0: with e = 0 or
// e = 1 the terms that vanish are -inf (a positive multiple of -inf, or ln 0), nothing is NaN, and a code whose
// terms all vanish is -inf exactly.  No term is ever +inf.  The result is rounded to fp32 once, at the end.
// (The arithmetic itself is in press_emission.h, shared with press_reemit.hip.)
#include "press_kernel.h"
#include "press_emission.h"

#include <hip/hip_runtime.h>

namespace
{

using namespace dcp_emission;

constexpr int THREADS = 256;

__global__ __launch_bounds__(THREADS) void emission_kernel(float const *__restrict__ in, float *__restrict__ out,
                                                           float epsilon)
{
  __shared__ double prob[DCP_PRESS_IN_STRIDE];
  int const tid = (int)threadIdx.x;
  size_t const entry = blockIdx.x;
  if (tid < INPUTS) prob[tid] = input_prob(in[entry * DCP_PRESS_IN_STRIDE + (size_t)tid]);
  __syncthreads();
  State const s{prob, prob + 4, in + entry * DCP_PRESS_IN_STRIDE};
  double const le = log((double)epsilon), lf = log1p(-(double)epsilon);
  float *row = out + entry * DCP_PRESS_TABLE;
  for (int code = tid; code < DCP_PRESS_TABLE; code += THREADS)
  {
    int z[5];
    int const n = decode(code, z);
    row[code] = emission_lprob(s, le, lf, n, z);
  }
}

} // namespace

int dcp_press_emission_launch(float const *in, float *out, int entries, float epsilon, hipStream_t stream)
{
  if (entries <= 0) return 0;
  hipLaunchKernelGGL(emission_kernel, dim3((unsigned)entries), dim3(THREADS), 0, stream, in, out, epsilon);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}
