// calibrate.hip -- the kernels of dcp_hip_calibrate: the code rows of random reads, written without the reads, and the
// Gumbel fit of every profile's scores against them.
#include "calibrate.h"
#include "viterbi_kernels.h"

// Code rows of nseq random sequences of len nucleotides (dcp_code_rows_of, include/deciphon_host.h, states the rows of a
// read; calibrate.h the read).  The thread of row r draws the up to five bases r-5..r-1 again from the generator and
// extends the t-mers to the left as dcp_encode_kernel does; the row goes out as two 16-byte stores.  Sequence s has its
// rows at s * (len + 1); row 0 is all zeros.
__global__ void dcp_random_code_rows_kernel(int nseq, int len, uint64_t seed, uint32_t t0, uint32_t t1, uint32_t t2,
                                            DcpCodeRow *__restrict__ rows)
{
  // gridDim.y is capped at 65535: stride over the sequences
  for (int s = (int)blockIdx.y; s < nseq; s += (int)gridDim.y)
  {
    uint4 *out = reinterpret_cast<uint4 *>(rows + (int64_t)s * ((int64_t)len + 1)); // (rows are 32 bytes from a 256-byte base)
    uint64_t const first = (uint64_t)s * (uint64_t)len; // idx of the sequence's nucleotide 0
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r <= len; r += (int64_t)gridDim.x * blockDim.x)
    {
      unsigned const off[5] = {0u, 4u, 20u, 84u, 340u};
      unsigned c[5], idx = 0;
#pragma unroll
      for (int t = 1; t <= 5; ++t)
      {
        // the new symbol is the t-mer's leftmost, the most significant digit
        bool const ok = r - t >= 0;
        unsigned const sym = ok ? dcp_random_base(seed, t0, t1, t2, first + (uint64_t)(r - t)) : 0u;
        idx += sym << (2 * (t - 1));
        c[t - 1] = ok ? off[t - 1] + idx : 0u;
      }
      out[2 * r] = make_uint4(c[0], c[1], c[2], c[3]);
      out[2 * r + 1] = make_uint4(c[4], 0u, 0u, 0u);
    }
  }
}

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
    // c-core/lrt.h:6-9, the fp32 operations of dcp_lrt_filter_kernel
    float const null_loglik = -pairs[2 * (size_t)i], alt_loglik = -pairs[2 * (size_t)i + 1];
    float const x = -2 * (null_loglik - alt_loglik);
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
      float const null_loglik = -pairs[2 * (size_t)i], alt_loglik = -pairs[2 * (size_t)i + 1];
      float const x = -2 * (null_loglik - alt_loglik);
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

hipError_t dcp_launch_random_code_rows(int nseq, int len, uint64_t seed, uint32_t const t[3], DcpCodeRow *rows,
                                       hipStream_t stream)
{
  if (nseq <= 0) return hipSuccess;
  unsigned bx = (unsigned)(((int64_t)len + 1 + 255) / 256);
  if (bx < 1) bx = 1;
  if (bx > 1024) bx = 1024;
  hipLaunchKernelGGL(dcp_random_code_rows_kernel, dim3(bx, (unsigned)(nseq < 65535 ? nseq : 65535)), dim3(256), 0, stream,
                     nseq, len, seed, t[0], t[1], t[2], rows);
  return hipGetLastError();
}

hipError_t dcp_launch_gumbel_fit(float const *out, int nprof, int n, float lambda, uint32_t *mu_bits, int32_t *excluded,
                                 hipStream_t stream)
{
  if (nprof <= 0) return hipSuccess;
  hipLaunchKernelGGL(dcp_gumbel_fit_kernel, dim3((unsigned)nprof), dim3(64), 0, stream, out, n, lambda, mu_bits, excluded);
  return hipGetLastError();
}
