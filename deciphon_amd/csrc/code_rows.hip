// code_rows.hip -- the kernels that write code rows (code_rows.h states a row) and their launches: the rows of reads as
// given, of reads on both strands, and of random reads that exist nowhere but in their rows.  One thread per row; a row
// goes out as two 16-byte stores (rows are 32 bytes from a 256-byte base).
#include "calibrate.h"
#include "code_rows.h"
#include "viterbi_kernels.h"

namespace
{

__device__ __forceinline__ void store_row(uint4 *__restrict__ out, int64_t r, uint32_t const c[5])
{
  out[2 * r] = make_uint4(c[0], c[1], c[2], c[3]);
  out[2 * r + 1] = make_uint4(c[4], 0u, 0u, 0u);
}

// The launch of all three kernels, blocks of 256 threads: x over the max_len + 1 rows of the longest sequence, 1024
// blocks at the most, y over the nseq sequences (reads, for both strands), 65535 at the most -- what a grid's y extent
// stops at, and a batch of metagenomic reads is larger.  The kernels stride over what is left in either direction.
template <class... Params, class... Args>
hipError_t launch_rows(void (*kernel)(Params...), int nseq, int64_t max_len, hipStream_t stream, Args... args)
{
  if (nseq <= 0) return hipSuccess;
  int64_t const bx = (max_len + 1 + 255) / 256;
  dim3 const grid((unsigned)(bx < 1 ? 1 : bx > 1024 ? 1024 : bx), (unsigned)(nseq < 65535 ? nseq : 65535));
  hipLaunchKernelGGL(kernel, grid, dim3(256), 0, stream, args...);
  return hipGetLastError();
}

} // namespace

// Sequence s: nt[seq_off[s] .. seq_off[s + 1]), its rows from row_off[s].
__global__ void dcp_encode_kernel(unsigned char const *__restrict__ nt, int64_t const *__restrict__ seq_off,
                                  int64_t const *__restrict__ row_off, int nseq, DcpCodeRow *__restrict__ rows)
{
  for (int s = (int)blockIdx.y; s < nseq; s += (int)gridDim.y)
  {
    int64_t const n = seq_off[s + 1] - seq_off[s];
    unsigned char const *x = nt + seq_off[s];
    uint4 *out = reinterpret_cast<uint4 *>(rows + row_off[s]);
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r <= n; r += (int64_t)gridDim.x * blockDim.x)
    {
      uint32_t c[5];
      dcp_code_row_words(r, [&](int t) { return x[r - t]; }, c);
      store_row(out, r, c);
    }
  }
}

// Both strands of every read from one pass over its nucleotides: read s becomes sequence 2s as given and sequence
// 2s + 1, its reverse complement y[i] = 3 - x[n-1-i], which is never materialised.  Row j of the reverse complement
// holds the t-mers y[j-t..j-1] = 3 - x[n-j+t-1..n-j]: the thread of position r = n - j finds the symbol t places to
// the left of that row t - 1 places to the RIGHT of r on the given strand, so it reads x[r-5..r+4], writes plus row r
// and minus row n - r.
// seq_off[nreads + 1]: the reads in nt; row_off[2 nreads + 1]: the rows in front of each of the 2 nreads sequences.
__global__ void dcp_encode_strands_kernel(unsigned char const *__restrict__ nt, int64_t const *__restrict__ seq_off,
                                          int64_t const *__restrict__ row_off, int nreads, DcpCodeRow *__restrict__ rows)
{
  for (int s = (int)blockIdx.y; s < nreads; s += (int)gridDim.y)
  {
    int64_t const n = seq_off[s + 1] - seq_off[s];
    unsigned char const *x = nt + seq_off[s];
    uint4 *plus = reinterpret_cast<uint4 *>(rows + row_off[2 * (int64_t)s]);
    uint4 *minus = reinterpret_cast<uint4 *>(rows + row_off[2 * (int64_t)s + 1]);
    if (n == 0) // an empty read: row 0 of either strand, and nothing to load
    {
      if (blockIdx.x == 0 && threadIdx.x == 0) plus[0] = plus[1] = minus[0] = minus[1] = make_uint4(0u, 0u, 0u, 0u);
      continue;
    }
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r <= n; r += (int64_t)gridDim.x * blockDim.x)
    {
      // a symbol beyond either end is read from the nearest position inside, n > 0, and never asked for: ten loads in
      // flight at once, none behind a branch
      unsigned lp[5], lm[5];
#pragma unroll
      for (int t = 1; t <= 5; ++t)
      {
        lp[t - 1] = x[r - t >= 0 ? r - t : 0];
        lm[t - 1] = x[r + t <= n ? r + t - 1 : n - 1];
      }
      uint32_t cp[5], cm[5];
      dcp_code_row_words(r, [&](int t) { return lp[t - 1]; }, cp);
      dcp_code_row_words(n - r, [&](int t) { return 3u - lm[t - 1]; }, cm);
      store_row(plus, r, cp);
      store_row(minus, n - r, cm);
    }
  }
}

// nseq random sequences of len nucleotides (calibrate.h states the read): the thread of row r draws the up to five
// bases r-5..r-1 again from the generator, so there is no nt buffer and there are no loads.  Sequence s has its rows at
// s * (len + 1).
__global__ void dcp_random_code_rows_kernel(int nseq, int len, uint64_t seed, uint32_t t0, uint32_t t1, uint32_t t2,
                                            DcpCodeRow *__restrict__ rows)
{
  for (int s = (int)blockIdx.y; s < nseq; s += (int)gridDim.y)
  {
    uint4 *out = reinterpret_cast<uint4 *>(rows + (int64_t)s * ((int64_t)len + 1));
    uint64_t const first = (uint64_t)s * (uint64_t)len; // idx of the sequence's nucleotide 0
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r <= len; r += (int64_t)gridDim.x * blockDim.x)
    {
      uint32_t c[5];
      dcp_code_row_words(r, [&](int t) { return dcp_random_base(seed, t0, t1, t2, first + (uint64_t)(r - t)); }, c);
      store_row(out, r, c);
    }
  }
}

hipError_t dcp_launch_encode(unsigned char const *nt, int64_t const *seq_off, int64_t const *row_off, int nreads,
                             bool both, int64_t max_len, DcpCodeRow *rows, hipStream_t stream)
{
  return launch_rows(both ? dcp_encode_strands_kernel : dcp_encode_kernel, nreads, max_len, stream, nt, seq_off, row_off,
                     nreads, rows);
}

hipError_t dcp_launch_random_code_rows(int nseq, int len, uint64_t seed, uint32_t const t[3], DcpCodeRow *rows,
                                       hipStream_t stream)
{
  return launch_rows(dcp_random_code_rows_kernel, nseq, len, stream, nseq, len, seed, t[0], t[1], t[2], rows);
}
