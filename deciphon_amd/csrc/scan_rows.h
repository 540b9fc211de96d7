// scan_rows.h -- from the walked paths of a scan to products.tsv: replaces the products.tsv writer (c-core/product.c,
// product_thread.c) and the quasi-codon decoding of the match column (c-core/decoder.c, match.c), minus HMMER: the
// evalue column is "nan" and no row is dropped, unless the profiles are calibrated (DcpEvalueRule).
#pragma once
#include "../../include/deciphon_hip.h"
#include "../../include/deciphon_host.h"
#include "dcp_db.h"
#include "engine_hmm.h"
#include "host_logic.h"
#include "product_runs.h"
#include <atomic>
#include <future>
#include <math.h>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

struct dcp_batch
{
  struct Seq
  {
    long id;
    std::string name;
    std::string text;        // uppercased + disambiguated (what dcp_batch_add stores, c-core/sequence.c:15-45)
    std::vector<uint8_t> nt; // indices 0..3
    bool has_t = false, has_u = false;
  };
  std::vector<Seq> seqs;
};

// Where the rows take a profile's distributions from: "fill a DcpDecoder for profile i" (global index), entries in the
// order of the pressed file -- 0 = null, 1 = background, 2 + n = node n, node K repeating node K - 1 -- with the scan's
// translation table and error rate, prepare()d.  0 or a DCP_E* code; called from several threads at once.
struct DcpDecoderSource
{
  virtual ~DcpDecoderSource() = default;
  virtual int read_decoder(int i, DcpDecoder &out) const = 0;
};

// the mapped database of a scan set up from a pressed file
struct DcpDbDecoders : DcpDecoderSource
{
  DcpDbReader db;
  int read_decoder(int i, DcpDecoder &out) const override { return db.read_decoder(i, out); }
};

// A scan set up from a HMMER3 file (dcp_scan_setup_hmm) has no file to read them back from: it keeps the fp32 nucltp
// and codonm of every node, 516 bytes each, as the load shows them (engine_hmm.h).
// dcp_scan_set_gencode: the engine shows the entries it recomputes (DcpGencodeSink) and they replace the kept ones.
struct DcpHmmDecoders : DcpDecoderSource, DcpHmmSink, DcpGencodeSink
{
  int gencode = 0;
  float epsilon = 0; // of the engine's tables: dcp_scan_set_epsilon moves both, between runs (a run's decoders copy it)
  DcpNucltDist null{}, bg{};
  std::vector<std::vector<DcpNucltDist>> nodes; // by profile: [K]
  void models(DcpNucltDist const &n, DcpNucltDist const &b) override { null = n, bg = b; }
  void profile(DcpHmmProfile const &p) override { nodes.emplace_back(p.nodes.begin(), p.nodes.begin() + p.core_size); }
  void regencoded(int gencode_id, DcpNucltDist const &n, DcpNucltDist const &b) override
  {
    gencode = gencode_id, null = n, bg = b;
    at_profile = at_node = 0;
  }
  void entries(size_t first, size_t n, float const *in) override;
  int read_decoder(int i, DcpDecoder &out) const override;

private:
  size_t at_profile = 0, at_node = 0; // where the next entry of a dcp_scan_set_gencode goes
};

// The evalue column of a run and its row filter.  A row whose profile has a Gumbel location at the length of the row's
// window (dcp_hip_profile_mu_at of window_stop - window_start is not NaN) prints E = dcp_lrt_evalue(lrt, that mu as fp32,
// dcp_hip_profile_lambda of the profile, z) with %.2g, as c-core/product_thread.c:60 prints
// HMMER's, and is left out when E >= max (c-core/thread.c:192-201 drops E >= 1).  Any other row prints "nan" and stays.
// The walk has moved on by then either way: last_hit_pos does not depend on it (thread.c:162 against thread.c:201).
struct DcpEvalueRule
{
  double z = 1;              // targets: the sequences the run scans, or what dcp_scan_set_evalue was given
  double max = HUGE_VAL;     // +inf: every row stays
};

// The rows of one dcp_scan_run.  Per path batch, in this order: warm_decoders, wait_steps_copied, dcp_hip_path, spans,
// format.  Its threads read the batch's sequences, the scan's decoder source and the engine -- the profiles' accessions, and
// the step buffers of the last dcp_hip_path until they hold copies (wait_steps_copied) -- and hand their rows to
// `runs`, so it is declared after all of them; its destructor joins the threads.
class DcpScanRows
{
public:
  // both_strands: the walk's sequences are 2 x reads (dcp_hip_set_sequences_strands: 2s is read s, 2s + 1 its reverse
  // complement) and every row ends in a strand column.  A minus row takes its nucleotides, the text of its match column
  // and its codons from the reverse complement of what dcp_batch_add keeps of the read (uppercased and disambiguated
  // first, then reversed and complemented -- that is the definition of the minus strand), built once per read that has
  // a minus hit; its coordinates are the walk's, on that strand.
  DcpScanRows(dcp_hip const *eng, DcpDecoderSource const *db, int index_offset, char const *abc, dcp_batch const *batch,
              DcpProductRuns *runs, bool both_strands = false, DcpEvalueRule evalue = DcpEvalueRule());
  ~DcpScanRows() { join(); }
  // decoder_setup (c-core/decoder.c:21-36) for the profiles of this batch -- reading a profile's distributions out of
  // the database and exponentiating them (a fraction of a millisecond, times hundreds of profiles with hits) -- by host
  // threads WHILE the GPU walks the paths; the formatters find them ready
  void warm_decoders(std::vector<dcp_hip_window> const &wins);
  // until the formatters of the batch before hold copies of its steps: dcp_hip_path overwrites the engine's
  void wait_steps_copied()
  {
    if (steps_copied_.valid()) steps_copied_.get();
  }
  // the hit spans of the n paths (c-core/thread.c:130-166): whether each holds a hit, and its last_hit_pos
  int spans(size_t n, std::vector<uint8_t> &is_hit, std::vector<int32_t> &last_hit_pos);
  // the rows of these hits of the batch, formatted off the calling thread while the GPU goes on and handed to `runs`
  // by the formatter (which also writes them to a run file when they are beyond the budget: never this thread).  A
  // row's serial -- batch number, then index in the batch -- is fixed here, whichever formatter finishes first.
  void format(std::vector<dcp_walk_hit> const &hits);
  // the decoders of profiles [first, last) go (a memo of (K + 3) * 1364 bytes each; the formatter jobs hold their own
  // references, and a profile that hits again makes a new one)
  void release_decoders(int first, int last);
  // joins the formatters; 0, or the first error of quasi-codon decoding (c-core/match.c:66-89 fails the scan the same
  // way) or of handing rows to `runs`
  int join();
  // product_close (c-core/product.c:34-88): rows in profile, read, window order, to `file`; they stay in `runs`
  int write(std::string const &file) { return runs_->close(file); }

private:
  // a decoder is handed out empty and filled by whichever thread needs it first
  struct LazyDecoder
  {
    std::once_flag once;
    int rc = 0;
    DcpDecoder dec;
  };
  struct Job
  {
    dcp_walk_hit at;
    DcpHit hit;
    // the path: first where the engine holds it (dcp_hip_path_steps_packed), then a copy of the job's own
    uint32_t const *steps = nullptr;
    int32_t nsteps = 0;
    std::vector<uint32_t> owned;
    std::shared_ptr<LazyDecoder> dec;
  };
  struct MinusStrand
  {
    std::once_flag once;
    std::string text;
    std::vector<uint8_t> nt;
  };
  void fill(LazyDecoder &ld, int profile) const;
  MinusStrand const &minus_strand(size_t read) const;

  dcp_hip const *eng_;
  DcpDecoderSource const *db_;
  int index_offset_;
  std::string abc_;
  dcp_batch const *batch_;
  DcpProductRuns *runs_;
  bool both_;
  DcpEvalueRule evalue_;
  int64_t batches_ = 0;                                // with hits, so far
  std::vector<std::shared_ptr<LazyDecoder>> decoders_; // by local profile
  mutable std::vector<MinusStrand> minus_;             // by read, on both strands (empty otherwise)
  std::vector<Job> found_;                             // of the batch between spans and format
  std::future<void> steps_copied_;                     // of the last batch with hits
  std::atomic<int> decode_rc_{0};
  std::vector<std::thread> threads_;
};
