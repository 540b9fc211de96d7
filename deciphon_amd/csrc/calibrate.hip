// calibrate.hip -- the Gumbel fit of every profile's scores against the random reads of dcp_hip_calibrate (the reads'
// code rows: code_rows.hip).
#include "viterbi_kernels.h"

namespace
{

// neither infinite nor NaN, by the bits (this unit is built like the others: the compiler may assume no NaN in arithmetic)
__device__ inline bool finite_bits(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }

__device__ inline double wave_sum(double v)
{
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
  return v;
}

} // namespace

// One wavefront per profile (see dcp_launch_gumbel_fit, viterbi_kernels.h).  Two passes over the profile's n pairs: the
// minimum of the finite scores and their count, then the sum of exp(-lambda (x - m)) in fp64.  Lane 0 stores.
__global__ __launch_bounds__(64) void dcp_gumbel_fit_kernel(float const *__restrict__ out, int n, float lambda,
                                                            uint32_t *__restrict__ mu_bits, int32_t *__restrict__ excluded)
{
  int const p = (int)blockIdx.x, lane = (int)threadIdx.x;
  float const *pairs = out + 2 * (size_t)n * (size_t)p;
  float const inf = __uint_as_float(0x7f800000u);
  float m = inf;
  int kept = 0;
  for (int i = lane; i < n; i += 64)
  {
    float const x = dcp_lrt(-pairs[2 * (size_t)i], -pairs[2 * (size_t)i + 1]);
    if (finite_bits(x))
    {
      m = x < m ? x : m;
      ++kept;
    }
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1)
  {
    float const o = __shfl_xor(m, d);
    m = o < m ? o : m;
    kept += __shfl_xor(kept, d);
  }
  double sum = 0;
  if (kept > 0) // (uniform: every lane holds the wave's count)
    for (int i = lane; i < n; i += 64)
    {
      float const x = dcp_lrt(-pairs[2 * (size_t)i], -pairs[2 * (size_t)i + 1]);
      if (finite_bits(x)) sum += exp(-(double)lambda * ((double)x - (double)m));
    }
  sum = wave_sum(sum);
  if (lane == 0)
  {
    uint32_t bits = 0x7fc00000u; // NaN: no score kept
    if (kept > 0) bits = __float_as_uint((float)((double)m - log(sum / (double)kept) / (double)lambda));
    mu_bits[p] = bits;
    excluded[p] = n - kept;
  }
}

hipError_t dcp_launch_gumbel_fit(float const *out, int nprof, int n, float lambda, uint32_t *mu_bits, int32_t *excluded,
                                 hipStream_t stream)
{
  if (nprof <= 0) return hipSuccess;
  hipLaunchKernelGGL(dcp_gumbel_fit_kernel, dim3((unsigned)nprof), dim3(64), 0, stream, out, n, lambda, mu_bits, excluded);
  return hipGetLastError();
}
