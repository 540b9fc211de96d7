// calibrate.h -- the random reads a calibration scores (dcp_hip_calibrate, include/deciphon_hip.h), stated once for the
// host and for the kernel that writes their code rows (calibrate.hip).
//
// Nucleotide i of random sequence s, in a set of sequences of `len` nucleotides, has the 64-bit index idx = s * len + i.
// Its base is splitmix64 addressed by position, the upper half of the word against three cumulative thresholds:
//   z = seed + (idx + 1) * 0x9E3779B97F4A7C15            (mod 2^64)
//   z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9
//   z = (z ^ z >> 27) * 0x94D049BB133111EB
//   u = (z ^ z >> 31) >> 32
//   base = (u >= t[0]) + (u >= t[1]) + (u >= t[2])
// The thresholds are integers the host makes from the caller's frequencies (dcp_random_thresholds_of); the device sees
// only them, so no float crosses the line.  This definition is part of the interface: a seed gives the same reads in
// every later version.
#pragma once
#include "dcp_types.h"

DCP_HDI uint32_t dcp_random_u32(uint64_t seed, uint64_t idx)
{
  uint64_t z = seed + (idx + 1u) * 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return (uint32_t)((z ^ (z >> 31)) >> 32);
}

DCP_HDI uint32_t dcp_random_base(uint64_t seed, uint32_t t0, uint32_t t1, uint32_t t2, uint64_t idx)
{
  uint32_t const u = dcp_random_u32(seed, idx);
  return (uint32_t)(u >= t0) + (uint32_t)(u >= t1) + (uint32_t)(u >= t2);
}

// t[j] = min(floor(cum_j * 2^32), 2^32 - 1), cum_j the sum of the first j + 1 frequencies over the sum of all four, in
// double; freq == nullptr: uniform.  A frequency of 0 leaves its base no value of u: equal neighbouring thresholds for
// bases 1 and 2, t[0] = 0 for base 0; for base 3 the clamp leaves it the single value u = 2^32 - 1 (one draw in 2^32).
// False for a negative, non-finite or all-zero freq: t is then not written.
inline bool dcp_random_thresholds_of(float const *freq, uint32_t t[3])
{
  double f[4] = {1, 1, 1, 1}, sum = 0;
  for (int j = 0; j < 4; ++j)
  {
    if (freq) f[j] = (double)freq[j];
    if (!(f[j] >= 0.0) || !(f[j] <= 3.5e38)) return false; // negative, NaN, infinite
    sum += f[j];
  }
  if (!(sum > 0.0)) return false;
  double cum = 0;
  for (int j = 0; j < 3; ++j)
  {
    cum += f[j] / sum;
    double const v = __builtin_floor(cum * 4294967296.0);
    t[j] = v >= 4294967295.0 ? 4294967295u : (uint32_t)v;
  }
  return true;
}
