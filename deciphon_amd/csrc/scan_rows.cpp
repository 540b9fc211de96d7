// scan_rows.cpp -- see scan_rows.h
#include "scan_rows.h"
#include "code_rows.h"
#include "dcp_errors.h"
#include "parallel_for.h"
#include "press_kernel.h"
#include <algorithm>
#include <math.h>
#include <stdio.h>
#include <string.h>

namespace
{

// product_thread_add_match + write_match (c-core/product_thread.c:40-79,112-148) without HMMER: every step of the
// hit as "<nucleotides>,<state>,<codon>,<amino>", the last two from decoder_decode / imm_gencode_decode
// (c-core/match.c:66-89, c-core/decoder.c:38-58) for the emitting states.  *rc receives DCP_EDECODON when a step
// cannot be decoded (the reference fails the scan there).
// text, nt: the scanned strand of the read (the read's own, or its reverse complement); strand: '+' or '-' for the 13th
// column of a scan of both strands, 0 for none.
std::string format_row(dcp_batch::Seq const &seq, std::string const &text, uint8_t const *nt, char strand, int window,
                       int wstart, int wstop, DcpHit const &hit, char const *accession, char const *abc, float lrt,
                       double evalue, uint32_t const *steps, DcpDecoder const &dec, std::atomic<int> *rc)
{
  // a step: state id in the low 16 bits, emission length above (dcp_hip_path_steps_packed)
  auto step_id = [&](int i) { return (int)(steps[i] & 0xffffu); };
  auto step_size = [&](int i) { return (int)(steps[i] >> 16); };
  char const *sym = seq.has_u ? "ACGU" : "ACGT";
  // the evalue column: "nan" for a profile that is not calibrated, the literal string as ever; else c-core/product_thread.c:60
  char head[256], ev[32] = "nan";
  if (!isnan(evalue)) snprintf(ev, sizeof ev, "%.2g", evalue);
  snprintf(head, sizeof head, "%ld\t%d\t%d\t%d\t%d\t%d\t%d\t%s\t%s\t%.1f\t%s\t", seq.id, window, wstart, wstop, 0,
           hit.hit_start, hit.hit_stop, accession, abc, (double)lrt, ev);
  std::string out = head;
  out.reserve(out.size() + (size_t)(hit.end_step - hit.begin_step) * 12);
  int pos = 0;
  for (int i = 0; i < hit.begin_step; ++i) pos += step_size(i);
  for (int i = hit.begin_step; i < hit.end_step; ++i)
  {
    if (i > hit.begin_step) out += ';';
    char name[8];
    int const n = step_size(i), id = step_id(i);
    dcp_state_name(id, name);
    out.append(text, (size_t)(wstart + pos), (size_t)n);
    out += ',';
    out += name;
    out += ',';
    if (!dcp_state_is_mute(id))
    {
      // insert states decode against the background, match states against their node, N / J / C against the
      // null model (c-core/decoder.c:43-49)
      int const kind = id >> 14, k = (id & 0x3FFF) - 1;
      size_t const entry = kind == 1 ? 1 : kind == 0 ? 2 + (size_t)k : 0;
      uint8_t codon[3] = {0, 0, 0};
      bool ok = !(kind <= 1 && (k < 0 || k > dec.core_size)) && n >= 1 && n <= 5;
      if (ok)
      {
        // the code of the n-mer (imm_eseq's indexing: SURVEY 8a row S) keys the decoder's memo
        unsigned code = 0;
        for (int t = 0; t < n; ++t) code = code * 4 + nt[(size_t)(wstart + pos + t)];
        std::atomic<uint8_t> &slot = dec.memo[entry * DCP_TABLE_SIZE + dcp_code_off(n) + code];
        uint8_t m = slot.load(std::memory_order_relaxed);
        if (m == 0xFF)
        {
          bool const found = dcp_decode_codon_prob((double)dec.epsilon, dec.base.data() + 4 * entry, dec.prior.data() + 64 * entry,
                                                   nt + wstart + pos, n, codon);
          m = found ? (uint8_t)(codon[0] * 16 + codon[1] * 4 + codon[2]) : (uint8_t)0xFE;
          slot.store(m, std::memory_order_relaxed);
        }
        ok = m != 0xFE;
        codon[0] = (uint8_t)(m >> 4);
        codon[1] = (uint8_t)((m >> 2) & 3);
        codon[2] = (uint8_t)(m & 3);
      }
      char const amino = ok ? dcp_gencode_amino(dec.gencode, codon) : 0;
      if (!ok || !amino)
      {
        int expected = 0;
        rc->compare_exchange_strong(expected, !ok ? DCP_EDECODON : DCP_EGENCODEID);
      }
      else
      {
        out += sym[codon[0]];
        out += sym[codon[1]];
        out += sym[codon[2]];
        out += ',';
        out += amino;
      }
      if (!ok || !amino) out += ',';
    }
    else
      out += ',';
    pos += n;
  }
  if (strand)
  {
    out += '\t';
    out += strand;
  }
  return out;
}

} // namespace

// the engine's kept entries are the nodes of the scan's profiles, in order: one load, nothing else resident
void DcpHmmDecoders::entries(size_t, size_t n, float const *in)
{
  for (size_t e = 0; e < n; ++e, in += DCP_PRESS_IN_STRIDE)
  {
    while (at_profile < nodes.size() && at_node == nodes[at_profile].size()) ++at_profile, at_node = 0;
    if (at_profile == nodes.size()) return;
    DcpNucltDist &d = nodes[at_profile][at_node++];
    memcpy(d.nucltp, in, sizeof d.nucltp);
    memcpy(d.codonm, in + 4, sizeof d.codonm);
  }
}

int DcpHmmDecoders::read_decoder(int i, DcpDecoder &x) const
{
  if (i < 0 || (size_t)i >= nodes.size()) return DCP_EINVALPART;
  std::vector<DcpNucltDist> const &nd = nodes[(size_t)i];
  size_t const K = nd.size();
  x.gencode = gencode;
  x.core_size = (int)K;
  x.epsilon = epsilon;
  x.nucltp.resize((K + 3) * 4);
  x.codonm.resize((K + 3) * 125);
  for (size_t e = 0; e < K + 3; ++e)
  {
    DcpNucltDist const &d = e == 0 ? null : e == 1 ? bg : nd[std::min(e - 2, K - 1)];
    memcpy(x.nucltp.data() + 4 * e, d.nucltp, sizeof d.nucltp);
    memcpy(x.codonm.data() + 125 * e, d.codonm, sizeof d.codonm);
  }
  x.prepare();
  return 0;
}

DcpScanRows::DcpScanRows(dcp_hip const *eng, DcpDecoderSource const *db, int index_offset, char const *abc,
                         dcp_batch const *batch, DcpProductRuns *runs, bool both_strands, DcpEvalueRule evalue)
    : eng_(eng), db_(db), index_offset_(index_offset), abc_(abc), batch_(batch), runs_(runs), both_(both_strands),
      evalue_(evalue),
      decoders_((size_t)std::max(dcp_hip_num_profiles(eng), 0)), minus_(both_strands ? batch->seqs.size() : 0)
{
}

// The minus strand of a read: the reverse complement of the text and of the indices dcp_batch_add keeps (A<->T, or
// A<->U in the text of an RNA read, C<->G; an index i becomes 3 - i), once per read that has a minus hit.
DcpScanRows::MinusStrand const &DcpScanRows::minus_strand(size_t read) const
{
  MinusStrand &m = minus_[read];
  std::call_once(m.once, [&]() {
    dcp_batch::Seq const &s = batch_->seqs[read];
    size_t const n = s.nt.size();
    char const *sym = s.has_u ? "ACGU" : "ACGT";
    m.text.resize(n);
    m.nt.resize(n);
    for (size_t i = 0; i < n; ++i)
    {
      m.nt[i] = (uint8_t)(3 - s.nt[n - 1 - i]);
      m.text[i] = sym[m.nt[i]];
    }
  });
  return m;
}

void DcpScanRows::fill(LazyDecoder &ld, int profile) const
{
  std::call_once(ld.once, [&]() { ld.rc = db_->read_decoder(index_offset_ + profile, ld.dec); });
}

void DcpScanRows::warm_decoders(std::vector<dcp_hip_window> const &wins)
{
  std::vector<std::pair<int, std::shared_ptr<LazyDecoder>>> warm;
  for (dcp_hip_window const &w : wins)
  {
    std::shared_ptr<LazyDecoder> &d = decoders_[(size_t)w.profile];
    if (d) continue;
    d = std::make_shared<LazyDecoder>();
    warm.emplace_back(w.profile, d);
  }
  if (!warm.empty())
    threads_.emplace_back([this, warm = std::move(warm)]() {
      dcp_parallel_for(warm.size(), 16, 4, 1, [&](size_t k) { fill(*warm[k].second, warm[k].first); });
    });
}

int DcpScanRows::spans(size_t n, std::vector<uint8_t> &is_hit, std::vector<int32_t> &last_hit_pos)
{
  // a few threads: 6 M steps to walk for the headline's 2301 hits
  found_.assign(n, Job());
  is_hit.assign(n, 0);
  last_hit_pos.assign(n, -1);
  std::atomic<int> steps_rc{0};
  dcp_parallel_for(n, 8, 64, 16, [&](size_t i) {
    Job &j = found_[i];
    if (int const src = dcp_hip_path_steps_packed(eng_, (int)i, &j.steps, &j.nsteps))
    {
      int expected = 0;
      steps_rc.compare_exchange_strong(expected, src);
      return;
    }
    is_hit[i] = dcp_find_hit_packed(j.steps, j.nsteps, j.hit) ? 1 : 0;
    last_hit_pos[i] = j.hit.last_hit_pos;
  });
  return steps_rc;
}

void DcpScanRows::format(std::vector<dcp_walk_hit> const &hits)
{
  if (hits.empty()) return;
  std::vector<Job> jobs;
  jobs.reserve(hits.size());
  for (dcp_walk_hit const &h : hits)
  {
    Job &j = found_[(size_t)h.batch_index];
    j.at = h;
    std::shared_ptr<LazyDecoder> &d = decoders_[(size_t)h.profile];
    if (!d) d = std::make_shared<LazyDecoder>();
    j.dec = d;
    jobs.push_back(std::move(j));
  }
  int64_t const serial = batches_++ << 32;
  std::promise<void> copied;
  steps_copied_ = copied.get_future();
  // up to 16 host threads: a row is a few thousand short appends
  threads_.emplace_back([this, serial, jobs = std::move(jobs), copied = std::move(copied)]() mutable {
    // the steps out of the engine's buffers first: the scan's next path pass waits for that, not for the rows
    dcp_parallel_for(jobs.size(), 16, 8, 1, [&](size_t k) {
      Job &j = jobs[k];
      j.owned.assign(j.steps, j.steps + j.nsteps);
      j.steps = j.owned.data();
    });
    copied.set_value();
    std::vector<DcpProductRuns::Row> out(jobs.size());
    std::vector<uint8_t> dropped(jobs.size(), 0); // rows at or beyond the E-value limit (DcpEvalueRule)
    dcp_parallel_for(jobs.size(), 16, 8, 1, [&](size_t k) {
      Job const &j = jobs[k];
      // mu of the profile at the window's length (dcp_calib_mu_at: one rung is a constant), and the profile's lambda
      float const mu = (float)dcp_hip_profile_mu_at(eng_, j.at.profile, (int64_t)j.at.stop - (int64_t)j.at.start);
      double const evalue = dcp_lrt_evalue(j.at.lrt, mu, dcp_hip_profile_lambda(eng_, j.at.profile), evalue_.z);
      if (evalue >= evalue_.max) // (never for NaN: a profile that is not calibrated keeps its rows)
      {
        dropped[k] = 1;
        return;
      }
      LazyDecoder &ld = *j.dec;
      fill(ld, j.at.profile); // decoder_setup, c-core/decoder.c:21-36, once per profile
      if (ld.rc)
      {
        int expected = 0;
        decode_rc_.compare_exchange_strong(expected, ld.rc);
        return;
      }
      // on both strands the walk's sequence 2s is read s as given, 2s + 1 its reverse complement
      size_t const read = both_ ? (size_t)j.at.seq / 2 : (size_t)j.at.seq;
      bool const minus = both_ && (j.at.seq & 1);
      dcp_batch::Seq const &seq = batch_->seqs[read];
      MinusStrand const *m = minus ? &minus_strand(read) : nullptr;
      out[k] = DcpProductRuns::Row{j.at.profile, j.at.seq, j.at.window, serial + (int64_t)k,
                                   format_row(seq, m ? m->text : seq.text, m ? m->nt.data() : seq.nt.data(),
                                              !both_ ? (char)0 : minus ? '-' : '+', j.at.window, j.at.start, j.at.stop, j.hit,
                                              dcp_hip_profile_accession(eng_, j.at.profile), abc_.c_str(), j.at.lrt,
                                              evalue, j.steps, ld.dec, &decode_rc_)};
    });
    if (decode_rc_) return; // (the scan fails: its rows are not written)
    size_t kept = 0;
    for (size_t k = 0; k < out.size(); ++k)
      if (!dropped[k])
      {
        if (kept != k) out[kept] = std::move(out[k]);
        ++kept;
      }
    out.resize(kept);
    if (int const rc = runs_->add(std::move(out)))
    {
      int expected = 0;
      decode_rc_.compare_exchange_strong(expected, rc);
    }
  });
}

void DcpScanRows::release_decoders(int first, int last)
{
  for (int p = first; p < last; ++p) decoders_[(size_t)p].reset();
}

int DcpScanRows::join()
{
  for (std::thread &t : threads_) t.join();
  threads_.clear();
  return decode_rc_;
}
