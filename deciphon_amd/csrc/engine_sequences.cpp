// engine_sequences.cpp -- the engine's sequences (struct Sequences, engine_internal.h): reads on one strand or on both,
// and random sequences that exist only as code rows.  Every kind is checked, laid out by one routine and installed by
// one path; the kernels that write the rows: code_rows.hip.
#include "calibrate.h"
#include "engine_internal.h"
#include <limits.h>

namespace dcp_engine
{

namespace
{

// Internal sequences of nreads reads, `per` of each (2: a read and its reverse complement), back to back
struct Layout
{
  std::vector<int64_t> seq_off{0}, row_off{0};
  int64_t max_len = 0;
};

// len_of(i): the length of read i.  False when one is negative.
template <class LenOf> bool lay_out(int nreads, int per, LenOf len_of, Layout &l)
{
  l.seq_off.reserve((size_t)nreads * (size_t)per + 1);
  l.row_off.reserve((size_t)nreads * (size_t)per + 1);
  for (int i = 0; i < nreads; ++i)
  {
    int64_t const len = len_of(i);
    if (len < 0) return false;
    l.max_len = std::max(l.max_len, len);
    for (int k = 0; k < per; ++k)
    {
      l.seq_off.push_back(l.seq_off.back() + len);
      l.row_off.push_back(l.row_off.back() + len + 1);
    }
  }
  return true;
}

// The sequences of `l` replace the engine's, the checks having passed.  enqueue(stream): what writes their rows -- the
// caller's uploads, into buffers it reserves first, and its kernel; 0 or a return code.
// From the second line to the last the engine holds no sequences, so that is what any failure leaves: never offsets
// whose rows are absent (a reserve that fails has freed the old buffer) or half written.
template <class Enqueue> int install(dcp_hip *x, Layout &l, Enqueue enqueue)
{
  Sequences &q = x->seqs;
  hipStream_t const stream = x->cost_set.stream;
  ++x->gen;
  q.seq_off = q.row_off = {0};
  HIP_TRY(x, hipStreamSynchronize(stream), DCP_EFUNCUSE);
  HIP_TRY(x, q.d_rows.reserve((size_t)std::max<int64_t>(l.row_off.back(), 1)), DCP_ENOMEM);
  if (int rc = enqueue(stream)) return rc;
  HIP_TRY(x, hipStreamSynchronize(stream), DCP_EFUNCUSE);
  q.seq_off = std::move(l.seq_off);
  q.row_off = std::move(l.row_off);
  return 0;
}

} // namespace

int check_random(dcp_hip *x, int nseq, int len, float const *freq, uint32_t t[3])
{
  if (outstanding_batches(x)) return refuse_outstanding(x);
  if (nseq < 0 || len < 0) return fail(x, DCP_EFUNCUSE, "nseq and len must not be negative");
  if (!dcp_random_thresholds_of(freq, t)) return fail(x, DCP_EFUNCUSE, "freq must hold four non-negative frequencies, not all zero");
  if ((uint64_t)nseq * ((uint64_t)len + 1) >= ((uint64_t)1 << 32)) return fail(x, DCP_EFUNCUSE, "more than 2^32 - 1 code rows");
  return 0;
}

int install_random(dcp_hip *x, int nseq, int len, uint64_t seed, uint32_t const t[3])
{
  HIP_TRY(x, hipSetDevice(x->device), DCP_EFUNCUSE);
  Layout l;
  lay_out(nseq, 1, [&](int) { return (int64_t)len; }, l);
  return install(x, l, [&](hipStream_t stream) {
    HIP_TRY(x, dcp_launch_random_code_rows(nseq, len, seed, t, x->seqs.d_rows.p, stream), DCP_EFUNCUSE);
    return 0;
  });
}

} // namespace dcp_engine

extern "C" {

// Plus strand: internal sequence i is read i.  Both: sequences 2s and 2s + 1 are read s and its reverse complement, which
// exists only as code rows (dcp_encode_strands_kernel); seq_off and row_off count 2 nseq sequences, the device's copy of
// the offsets stays the reads' (what the kernel walks nt by).
int dcp_hip_set_sequences_strands(struct dcp_hip *x, int nseq, uint8_t const *nt, int64_t const *offsets, int strands)
{
  if (!x || nseq < 0 || !offsets || (nseq > 0 && !nt)) return DCP_EFUNCUSE;
  if (strands != DCP_STRANDS_PLUS && strands != DCP_STRANDS_BOTH) return fail(x, DCP_EFUNCUSE, "strands must be DCP_STRANDS_PLUS or DCP_STRANDS_BOTH");
  bool const both = strands == DCP_STRANDS_BOTH;
  if (both && nseq > INT_MAX / 2) return fail(x, DCP_EFUNCUSE, "more than INT_MAX / 2 reads on both strands");
  if (outstanding_batches(x)) return refuse_outstanding(x);
  HIP_TRY(x, hipSetDevice(x->device), DCP_EFUNCUSE);
  // everything is checked before anything is replaced: a refused call leaves the previous reads in force
  if (offsets[0] != 0) return fail(x, DCP_EFUNCUSE, "offsets[0] must be 0");
  Layout l;
  if (!lay_out(nseq, both ? 2 : 1, [&](int i) { return offsets[i + 1] - offsets[i]; }, l))
    return fail(x, DCP_EFUNCUSE, "offsets must not decrease");
  int64_t const total = offsets[nseq];
  for (int64_t i = 0; i < total; ++i)
    if (nt[i] > 3) return fail(x, DCP_ESEQABC, "nucleotide index above 3");
  return install(x, l, [&](hipStream_t stream) {
    Sequences &q = x->seqs;
    HIP_TRY(x, q.d_nt.reserve((size_t)std::max<int64_t>(total, 1)), DCP_ENOMEM);
    HIP_TRY(x, q.d_seq_off.reserve((size_t)nseq + 1), DCP_ENOMEM);
    HIP_TRY(x, q.d_row_off.reserve(l.row_off.size()), DCP_ENOMEM);
    if (total) HIP_TRY(x, hipMemcpyAsync(q.d_nt.p, nt, (size_t)total, hipMemcpyHostToDevice, stream), DCP_EFUNCUSE);
    // (the caller's offsets, and the layout's: install waits for the copies before either goes)
    HIP_TRY(x, hipMemcpyAsync(q.d_seq_off.p, offsets, ((size_t)nseq + 1) * sizeof(int64_t), hipMemcpyHostToDevice, stream), DCP_EFUNCUSE);
    HIP_TRY(x, hipMemcpyAsync(q.d_row_off.p, l.row_off.data(), l.row_off.size() * sizeof(int64_t), hipMemcpyHostToDevice, stream),
            DCP_EFUNCUSE);
    HIP_TRY(x, dcp_launch_encode(q.d_nt.p, q.d_seq_off.p, q.d_row_off.p, nseq, both, l.max_len, q.d_rows.p, stream), DCP_EFUNCUSE);
    return 0;
  });
}

int dcp_hip_set_sequences(struct dcp_hip *x, int nseq, uint8_t const *nt, int64_t const *offsets)
{
  return dcp_hip_set_sequences_strands(x, nseq, nt, offsets, DCP_STRANDS_PLUS);
}

int dcp_hip_set_random_sequences(struct dcp_hip *x, int nseq, int len, uint64_t seed, float const freq[4])
{
  if (!x) return DCP_EFUNCUSE;
  uint32_t t[3];
  if (int rc = check_random(x, nseq, len, freq, t)) return rc;
  return install_random(x, nseq, len, seed, t);
}

int dcp_hip_num_sequences(struct dcp_hip const *x) { return x ? x->seqs.count() : 0; }

int dcp_hip_code_rows_read(struct dcp_hip const *x, int seq, uint32_t *out, int64_t rows)
{
  if (!x || !out || seq < 0 || seq >= x->seqs.count()) return DCP_EFUNCUSE;
  int64_t const first = x->seqs.row_off[(size_t)seq];
  if (rows != x->seqs.row_off[(size_t)seq + 1] - first) return DCP_EFUNCUSE;
  // (the install has waited for its kernel before it returned)
  if (hipSetDevice(x->device) != hipSuccess) return DCP_EFUNCUSE;
  if (hipMemcpy(out, x->seqs.d_rows.p + first, (size_t)rows * sizeof(DcpCodeRow), hipMemcpyDeviceToHost) != hipSuccess) return DCP_EFUNCUSE;
  return 0;
}

} // extern "C"
