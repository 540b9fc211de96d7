// calibrate.hip -- the scores of a calibration's ladder of read lengths (dcp_hip_calibrate_lengths; the reads' code rows:
// code_rows.hip) gathered out of the cost pass's results, and the Gumbel fit of every profile's scores: the location of
// every rung at a fixed lambda, or lambda as well by maximum likelihood.
#include "../../include/deciphon_hip.h" // DCP_CALIB_MAX_LENS
#include "viterbi_kernels.h"

namespace
{

// neither infinite nor NaN, by the bits (this unit is built like the others: the compiler may assume no NaN in arithmetic)
__device__ inline bool finite_bits(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }

// every lane gets the sum, and the same bits: a butterfly adds the same two values on either side
__device__ inline double wave_sum(double v)
{
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
  return v;
}

// The minimum of the finite scores among x[0 .. n) and their count, in every lane.
__device__ inline void kept_scores(float const *x, int n, int lane, float &m, int &kept)
{
  m = __uint_as_float(0x7f800000u);
  kept = 0;
  for (int i = lane; i < n; i += 64)
  {
    float const v = x[i];
    if (finite_bits(v))
    {
      m = v < m ? v : m;
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
}

// T0 = sum exp(-lambda (x - m)) over the finite scores, in fp64 (every term <= 1): a lane sums its scores i = lane,
// lane + 64, .. in that order, the wave sums the lanes.  The one summation behind every mu, at a fixed lambda and at a
// fitted one.
__device__ inline double gumbel_t0(float const *x, int n, int lane, double lambda, float m)
{
  double sum = 0;
  for (int i = lane; i < n; i += 64)
  {
    float const v = x[i];
    if (finite_bits(v)) sum += exp(-lambda * ((double)v - (double)m));
  }
  return wave_sum(sum);
}

// mu = m - log(T0 / kept) / lambda, as fp32 bits
__device__ inline uint32_t gumbel_mu_bits(float m, double t0, int kept, double lambda)
{
  return __float_as_uint((float)((double)m - log(t0 / (double)kept) / lambda));
}

// T0, T1 = sum y exp(-lambda y) and T2 = sum y^2 exp(-lambda y), y = x - m, over the finite scores; the order of
// gumbel_t0
__device__ inline void gumbel_moments(float const *x, int n, int lane, double lambda, float m, double &t0, double &t1, double &t2)
{
  t0 = t1 = t2 = 0;
  for (int i = lane; i < n; i += 64)
  {
    float const v = x[i];
    if (finite_bits(v))
    {
      double const y = (double)v - (double)m, e = exp(-lambda * y), ye = y * e;
      t0 += e;
      t1 += ye;
      t2 += y * ye;
    }
  }
  t0 = wave_sum(t0);
  t1 = wave_sum(t1);
  t2 = wave_sum(t2);
}

// sum y and sum y^2, y = x - m, over the finite scores, and the largest of them (m <= xmax)
__device__ inline void shifted_sums(float const *x, int n, int lane, float m, double &s1, double &s2, float &xmax)
{
  s1 = s2 = 0;
  xmax = m;
  for (int i = lane; i < n; i += 64)
  {
    float const v = x[i];
    if (finite_bits(v))
    {
      double const y = (double)v - (double)m;
      s1 += y;
      s2 += y * y;
      xmax = v > xmax ? v : xmax;
    }
  }
  s1 = wave_sum(s1);
  s2 = wave_sum(s2);
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1)
  {
    float const o = __shfl_xor(xmax, d);
    xmax = o > xmax ? o : xmax;
  }
}

constexpr int NEWTON_MAX = 64; // steps of the search for lambda: samples of 2 to 800 scores took 8 at the most on the CPU

} // namespace

// Window i of a chunk of whole profiles, profile-major with nseq windows each, is read i % nseq of the chunk's profile
// i / nseq: its score goes to rung `rung` of that profile in scores[profile][nlen][nseq] (scores: at the chunk's first
// profile).
__global__ __launch_bounds__(256) void dcp_calib_gather_kernel(float const *__restrict__ out, int n, int nseq, int nlen, int rung,
                                                               float *__restrict__ scores)
{
  int64_t const i = (int64_t)blockIdx.x * 256 + (int64_t)threadIdx.x;
  if (i >= (int64_t)n) return;
  size_t const p = (size_t)(i / nseq), s = (size_t)(i % nseq);
  scores[(p * (size_t)nlen + (size_t)rung) * (size_t)nseq + s] = dcp_lrt(-out[2 * (size_t)i], -out[2 * (size_t)i + 1]);
}

// One wavefront per profile (see dcp_launch_gumbel_ladder_fit, viterbi_kernels.h).  Every value the control flow depends
// on is the wave's (kept_scores, wave_sum), so the lanes stay together; lane 0 stores.
__global__ __launch_bounds__(64) void dcp_gumbel_ladder_fit_kernel(float const *__restrict__ scores, int nlen, int n, float lambda,
                                                                   uint32_t *__restrict__ mu_bits, int32_t *__restrict__ excluded,
                                                                   uint32_t *__restrict__ lambda_bits)
{
  int const p = (int)blockIdx.x, lane = (int)threadIdx.x;
  float const *const x = scores + (size_t)p * (size_t)nlen * (size_t)n;
  mu_bits += (size_t)p * (size_t)nlen;
  excluded += (size_t)p * (size_t)nlen;
  uint32_t const nan_bits = 0x7fc00000u;
  // what the passes below keep of each rung: the same in every lane, so it lies in LDS and not in registers indexed by j
  __shared__ float s_m[DCP_CALIB_MAX_LENS];
  __shared__ int s_kept[DCP_CALIB_MAX_LENS];
  __shared__ double s_sum_y[DCP_CALIB_MAX_LENS];
  __shared__ int s_informative[DCP_CALIB_MAX_LENS];

  if (lambda > 0.0f) // fixed: rung by rung
  {
    for (int j = 0; j < nlen; ++j)
    {
      float m;
      int kept;
      kept_scores(x + (size_t)j * (size_t)n, n, lane, m, kept);
      double const t0 = kept > 0 ? gumbel_t0(x + (size_t)j * (size_t)n, n, lane, (double)lambda, m) : 0.0;
      if (lane == 0)
      {
        mu_bits[j] = kept > 0 ? gumbel_mu_bits(m, t0, kept, (double)lambda) : nan_bits;
        excluded[j] = n - kept;
      }
    }
    if (lane == 0) lambda_bits[p] = __float_as_uint(lambda);
    return;
  }

  // fitted: the rungs that say something about the scale, and the variance within them for a first lambda
  double ss = 0, dof = 0;
  for (int j = 0; j < nlen; ++j)
  {
    float m, xmax = 0;
    int kept;
    double s1 = 0, s2 = 0;
    kept_scores(x + (size_t)j * (size_t)n, n, lane, m, kept);
    if (kept > 0) shifted_sums(x + (size_t)j * (size_t)n, n, lane, m, s1, s2, xmax);
    bool const informative = kept >= 2 && xmax > m; // not all equal
    if (informative)
    {
      ss += s2 - s1 * s1 / (double)kept;
      dof += (double)(kept - 1);
    }
    if (lane == 0)
    {
      s_m[j] = m;
      s_kept[j] = kept;
      s_sum_y[j] = s1;
      s_informative[j] = informative;
      excluded[j] = n - kept;
    }
  }
  __syncthreads();
  if (!(dof > 0)) // no informative rung: not calibrated
  {
    if (lane == 0)
    {
      for (int j = 0; j < nlen; ++j) mu_bits[j] = nan_bits;
      lambda_bits[p] = nan_bits;
    }
    return;
  }

  // Newton's method on g(lambda) = sum_j kept_j (1 / lambda - mean_j y + T1_j / T0_j), strictly decreasing from +inf to
  // a negative limit, inside the bracket (lo, hi) of the values seen with g > 0 and g <= 0: a step that leaves it is
  // replaced by the middle, or by twice lambda while nothing bounds it above
  double lam = ss > 0 ? 3.14159265358979323846 / sqrt(6.0 * ss / dof) : 1.0;
  double lo = 0, hi = 0; // hi = 0: none yet
  for (int it = 0; it < NEWTON_MAX; ++it)
  {
    double g = 0, dg = 0;
    for (int j = 0; j < nlen; ++j)
    {
      if (!s_informative[j]) continue;
      double t0, t1, t2;
      gumbel_moments(x + (size_t)j * (size_t)n, n, lane, lam, s_m[j], t0, t1, t2);
      double const k = (double)s_kept[j], r = t1 / t0;
      g += k * (1.0 / lam - s_sum_y[j] / k + r);
      dg += k * (-1.0 / (lam * lam) - t2 / t0 + r * r);
    }
    if (g > 0)
      lo = lam;
    else
      hi = lam;
    double const step = g / dg, next = lam - step;
    bool const inside = next > lo && (hi == 0 || next < hi);
    if (fabs(step) <= 1e-13 * lam) // (a last step that rounding takes out of the bracket is not made)
    {
      if (inside) lam = next;
      break;
    }
    lam = inside ? next : hi > 0 ? 0.5 * (lo + hi) : 2.0 * lam;
  }
  for (int j = 0; j < nlen; ++j)
  {
    int const kept = s_kept[j];
    double const t0 = kept > 0 ? gumbel_t0(x + (size_t)j * (size_t)n, n, lane, lam, s_m[j]) : 0.0;
    if (lane == 0) mu_bits[j] = kept > 0 ? gumbel_mu_bits(s_m[j], t0, kept, lam) : nan_bits;
  }
  if (lane == 0) lambda_bits[p] = __float_as_uint((float)lam);
}

hipError_t dcp_launch_calib_gather(float const *out, int nprof, int nseq, int nlen, int rung, float *scores, hipStream_t stream)
{
  int64_t const n = (int64_t)nprof * (int64_t)nseq;
  if (n <= 0) return hipSuccess;
  if (n > (int64_t)INT32_MAX || rung < 0 || rung >= nlen) return hipErrorInvalidValue;
  hipLaunchKernelGGL(dcp_calib_gather_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, out, (int)n, nseq, nlen, rung,
                     scores);
  return hipGetLastError();
}

hipError_t dcp_launch_gumbel_ladder_fit(float const *scores, int nprof, int nlen, int n, float lambda, uint32_t *mu_bits,
                                        int32_t *excluded, uint32_t *lambda_bits, hipStream_t stream)
{
  if (nprof <= 0) return hipSuccess;
  if (nlen < 1 || nlen > DCP_CALIB_MAX_LENS || n < 1) return hipErrorInvalidValue;
  hipLaunchKernelGGL(dcp_gumbel_ladder_fit_kernel, dim3((unsigned)nprof), dim3(64), 0, stream, scores, nlen, n, lambda, mu_bits,
                     excluded, lambda_bits);
  return hipGetLastError();
}
