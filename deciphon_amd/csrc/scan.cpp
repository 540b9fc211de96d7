// scan.cpp -- the reference's outer API (include/deciphon.h) on top of the engine.
//
// Replaces c-core/scan.c (orchestration), thread.c (thread_run / process_window), workload.c / work.c (profile
// iteration) and batch.c (reads).  The window chains are scan_walk.cpp's, the rows of products.tsv scan_rows.cpp's;
// what is here is the C API and the pipeline that feeds the GPU.
//
// The reference walks profile-major: for each profile, for each read, for each
// window -- one DP at a time per thread.  Windows of ONE (profile, read) pair form
// a chain (the next window starts after the previous window's hit,
// c-core/window.c:21-31), but different pairs are independent and hits are rare:
// dcp_scan_run scores the no-hit chain of every pair in one launch and then lets
// only the pairs that did hit walk their real chains (see there).  Rows are emitted
// in the reference's order (profile, then read, then window) whatever the order of work.
#include "../../include/deciphon.h"
#include "../../include/deciphon_hip.h"
#include "../../include/deciphon_host.h"
#include "dcp_db.h"
#include "dcp_errors.h"
#include "engine_hmm.h"
#include "hmm_model.h"
#include "host_logic.h"
#include "scan_rows.h"
#include "scan_walk.h"

#include <algorithm>
#include <atomic>
#include <chrono>
#include <errno.h>
#include <limits.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <deque>
#include <memory>
#include <string>
#include <sys/stat.h>
#include <vector>

struct dcp_scan
{
  dcp_hip *eng = nullptr;
  int device = 0;
  bool multi_hits = true, hmmer3_compat = false;
  void (*callback)(void *) = nullptr;
  void *userdata = nullptr;
  std::atomic<bool> interrupted{false};
  std::atomic<int> done_proteins{0};
  int num_proteins = 0;   // of this partition
  int index_offset = 0;   // global index of local profile 0 (workload_index, c-core/workload.c:95)
  std::string abc_name = "dna";
  std::unique_ptr<DcpProductRuns> runs; // the rows of the last dcp_scan_run (dcp_scan_product), until the next one
  double timing[DCP_SCAN_TIMING_VALUES] = {0}; // dcp_scan_last_timing
  // the rows read the distributions of the profiles with hits from it: the database, which stays mapped, or what a
  // load from a HMMER3 file left in memory
  std::unique_ptr<DcpDecoderSource> db;
  int strands = DCP_STRANDS_PLUS; // dcp_scan_set_strands: what the next dcp_scan_run scans of every read
  DcpHmmDecoders *hmm = nullptr; // `db`, when dcp_scan_setup_hmm set it: the error rate moves with the tables (dcp_scan_set_epsilon)
  // dcp_scan_set_evalue: the targets of the evalue column (<= 0: the sequences a run scans) and the limit of its rows.
  // The calibration itself is the engine's (dcp_scan_calibrate), and goes with whatever changes its scores.
  double evalue_z = 0, evalue_max = HUGE_VAL;
};

namespace
{

int loglevel() // c-core/loglevel.c:9-16
{
  static thread_local int level = 2;
  static thread_local bool cached = false;
  if (!cached)
  {
    char const *x = getenv("DECIPHON_LOGLEVEL");
    if (x) level = atoi(x);
    cached = true;
  }
  return level;
}

int raise(int rc, char const *func, char const *detail = nullptr) // c-core/error.c:103-121
{
  if (rc && loglevel() <= 2)
    fprintf(stderr, "%s %s%s%s.\n", func, dcp_error_string(rc), detail ? ". Detail: " : "", detail ? detail : "");
  return rc;
}

int mkdir_p(std::string const &dir)
{
  if (mkdir(dir.c_str(), 0755) == 0 || errno == EEXIST) return 0;
  return DCP_EMKDIR;
}

// the phase times of dcp_scan_run (dcp_scan_last_timing, DECIPHON_HIP_TIMING)
struct Phase
{
  double reads = 0, windows = 0, cost = 0, path = 0, rows = 0, write = 0, callbacks = 0;
  std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now(), t = t0;
  double total() const { return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(); }
  double lap()
  {
    auto n = std::chrono::steady_clock::now();
    double d = std::chrono::duration<double>(n - t).count();
    t = n;
    return d;
  }
};

// a fresh engine on `device`, with HBM set aside for the path pass
int new_engine(dcp_scan *x, int device)
{
  if (x->eng) dcp_hip_del(x->eng);
  x->eng = dcp_hip_new(device);
  if (!x->eng) return DCP_EFUNCUSE;
  x->device = device;
  {
    // HBM for the path pass's DP tables, first: VRAM is cleared on allocation, in the background,
    // and the clearing then overlaps the database load and the first cost pass.  Best effort:
    // dcp_hip_path allocates what it needs anyway.  16 GB (never more than a quarter of what is free) hold the
    // tables of ~8000 hit windows of a median profile at once: the path pass of a scan's first hits is then one slice.
    char const *mb = getenv("DECIPHON_HIP_PATH_BUDGET_MB");
    (void)dcp_hip_path_reserve(x->eng, mb ? (int64_t)std::max(atol(mb), 1L) << 20 : (int64_t)16 << 30);
  }
  return 0;
}

// the last step of every setup, the profiles resident
int set_mode(dcp_scan *x, char const *func, bool multi_hits, bool hmmer3_compat, void (*callback)(void *), void *userdata)
{
  if (int const rc = dcp_hip_set_mode(x->eng, multi_hits, hmmer3_compat)) return raise(rc, func);
  x->multi_hits = multi_hits;
  x->hmmer3_compat = hmmer3_compat;
  x->callback = callback;
  x->userdata = userdata;
  x->interrupted = false;
  x->done_proteins = 0;
  return 0;
}

int setup_common(dcp_scan *x, char const *dbfile, int device, int index, int nparts, bool balanced, bool multi_hits,
                 bool hmmer3_compat, void (*callback)(void *), void *userdata)
{
  if (!x || !dbfile) return raise(DCP_EFUNCUSE, __func__);
  if (nparts < 1) return raise(DCP_EZEROPART, __func__);
  if (index < 0 || index >= nparts) return raise(DCP_EINVALPART, __func__);
  DcpDbReader db;
  int rc = db.open(dbfile);
  if (rc) return raise(rc, __func__, dbfile);
  int const abc = db.header().abc_typeid;
  if (!(abc == 4 || abc == 5)) return raise(DCP_ENUCLTNOSUPPORT, __func__); // IMM_DNA / IMM_RNA
  x->abc_name = abc == 4 ? "dna" : "rna";
  int const N = db.num_proteins();
  nparts = std::min(nparts, std::max(N, 1)); // c-core/scan.c:102
  if (index >= nparts)
  {
    x->num_proteins = 0;
    x->index_offset = N;
  }
  else
  {
    // contiguous partitions, in database order: by count as the reference does (c-core/partition_size.c:13-16,
    // c-core/protein_reader.c:112-128), or -- balanced -- by the running sum of core sizes
    std::vector<int32_t> K, first((size_t)nparts + 1);
    if (balanced)
    {
      K.resize((size_t)N);
      std::string acc;
      for (int i = 0; i < N; ++i)
      {
        int k = 0;
        if ((rc = db.read_protein_head(i, k, acc))) return raise(rc, __func__, dbfile);
        K[(size_t)i] = k;
      }
    }
    dcp_partition_bounds(N, balanced ? K.data() : nullptr, nparts, balanced, first.data());
    x->index_offset = first[(size_t)index];
    x->num_proteins = first[(size_t)index + 1] - first[(size_t)index];
  }
  {
    std::unique_ptr<DcpDbDecoders> mapped(new DcpDbDecoders);
    if ((rc = mapped->db.open(dbfile))) return raise(rc, __func__, dbfile);
    x->hmm = nullptr;
    x->db = std::move(mapped);
  }
  if ((rc = new_engine(x, device))) return raise(rc, __func__, "no usable HIP device (there is no CPU fallback)");
  if (x->num_proteins > 0)
  {
    if ((rc = dcp_hip_load_dcp(x->eng, dbfile, x->index_offset, x->num_proteins)))
      return raise(rc, __func__, dcp_hip_strerror(x->eng));
    if ((rc = dcp_hip_commit_profiles(x->eng))) return raise(rc, __func__, dcp_hip_strerror(x->eng));
  }
  return set_mode(x, __func__, multi_hits, hmmer3_compat, callback, userdata);
}


// the DECIPHON_HIP_* knobs of dcp_scan_run, read once per scan
struct Knobs
{
  bool speculate = true;    // DECIPHON_HIP_SPECULATE=0: nothing is assumed, every pair goes round by round (the tests compare the two)
  bool path_beside = false; // DECIPHON_HIP_PATH_BESIDE=1 (experiment): path passes beside the cost batches in flight
  double chunk_cells = 0;   // DECIPHON_HIP_CHUNK_CELLS: cells per chunk (experiments)
  double chunk_windows = 0; // DECIPHON_HIP_CHUNK_WINDOWS: windows per chunk
  size_t drain_hits = 32768; // DECIPHON_HIP_PATH_DRAIN_HITS: see dcp_scan_run
  // DECIPHON_HIP_PRODUCT_MB: the row text a scan holds before it sorts it into a run file (csrc/product_runs.h); 0:
  // every path batch is a run.  The default keeps the rows of some 30000 hits in memory, as every scan did before.
  double product_mb = 1024;
  bool timing = false;      // DECIPHON_HIP_TIMING=1: phase times of dcp_scan_run on stderr
  Knobs()
  {
    if (char const *e = getenv("DECIPHON_HIP_SPECULATE")) speculate = e[0] != '0';
    if (char const *e = getenv("DECIPHON_HIP_PATH_BESIDE")) path_beside = e[0] == '1';
    if (char const *e = getenv("DECIPHON_HIP_CHUNK_CELLS")) chunk_cells = atof(e);
    if (char const *e = getenv("DECIPHON_HIP_CHUNK_WINDOWS")) chunk_windows = atof(e);
    if (char const *e = getenv("DECIPHON_HIP_PATH_DRAIN_HITS")) drain_hits = (size_t)std::max(atol(e), 0L);
    if (char const *e = getenv("DECIPHON_HIP_PRODUCT_MB")) product_mb = atof(e);
    timing = getenv("DECIPHON_HIP_TIMING") != nullptr;
  }
};

// a chunk whose cost batch is outstanding on the engine
struct InFlight
{
  int chunk;
  std::vector<dcp_hip_window> wins;
  std::vector<int64_t> base; // DcpScanWalk::chunk_windows
};

// a scan that fails keeps no rows and leaves no run file (declared before the rows: their threads end first)
struct DropRuns
{
  dcp_scan *x;
  bool keep = false;
  ~DropRuns()
  {
    if (!keep) x->runs.reset();
  }
};

// whatever happens, no batch stays outstanding on the engine
struct Drain
{
  dcp_hip *eng;
  std::deque<InFlight> *flight;
  ~Drain()
  {
    int nh = 0;
    for (InFlight &f : *flight)
    {
      std::vector<int32_t> hw(f.wins.size() + 1);
      std::vector<float> hl(f.wins.size() + 1);
      (void)dcp_hip_cost_hits_end(eng, &nh, hw.data(), hl.data());
    }
  }
};

// one dcp_scan_run: the walk, the rows, and what dcp_scan_last_timing reports of the engine calls between them
struct Run
{
  dcp_scan *x;
  DcpScanWalk &walk;
  DcpScanRows &rows;
  Phase &ph;
  int rounds = 0, chunks_begun = 0, path_batches = 0;
  size_t nhits = 0;
  int64_t largest_chunk = 0;
  // one callback per window queued for scoring (c-core/thread.c:74)
  void progress(size_t n, bool until_interrupted = false)
  {
    if (x->callback)
      for (size_t i = 0; i < n && !(until_interrupted && x->interrupted); ++i) x->callback(x->userdata);
  }
};
char const RUN[] = "dcp_scan_run";

// the no-hit chains of a chunk's pairs go to the engine; the progress callbacks are made while the GPU scores them.
// (A window of a pair that hit earlier in its chain may turn out not to be the chain's -- it was scored all the same.)
int begin_chunk(Run &r, std::deque<InFlight> &flight, DcpChunk const &chunk, int c)
{
  InFlight f;
  f.chunk = c;
  f.wins.resize((size_t)chunk.windows); // (dcp_plan_chunks counted them)
  f.base.resize((size_t)(chunk.p1 - chunk.p0) * (size_t)(chunk.s1 - chunk.s0) + 1);
  if (r.walk.chunk_windows(chunk, f.wins.data(), f.base.data()))
    return raise(DCP_EFUNCUSE, RUN, "chunk plan and window chains disagree");
  ++r.chunks_begun;
  r.largest_chunk = std::max(r.largest_chunk, chunk.windows);
  r.ph.windows += r.ph.lap();
  ++r.rounds;
  if (int const rc = dcp_hip_cost_hits_begin(r.x->eng, (int)f.wins.size(), f.wins.data()))
    return raise(rc, RUN, dcp_hip_strerror(r.x->eng));
  flight.push_back(std::move(f));
  r.progress((size_t)chunk.windows, true);
  r.ph.callbacks += r.ph.lap();
  return 0;
}

// c-core/thread.c:123-166 for a batch of windows that passed the filter: viterbi_path, trellis_unzip, the hit span,
// last_hit_pos; their rows go to the formatter threads; their pairs move on
int path_batch(Run &r)
{
  std::vector<dcp_hip_window> const &wins = r.walk.take_path_batch();
  r.nhits += wins.size();
  r.rows.warm_decoders(wins);
  r.ph.windows += r.ph.lap();
  r.rows.wait_steps_copied();
  if (wins.size() > (size_t)INT_MAX) return raise(DCP_ENOMEM, RUN, "more than INT_MAX windows for one path pass");
  ++r.path_batches;
  if (int const rc = dcp_hip_path(r.x->eng, (int)wins.size(), wins.data())) return raise(rc, RUN, dcp_hip_strerror(r.x->eng));
  r.ph.path += r.ph.lap();
  std::vector<uint8_t> is_hit;
  std::vector<int32_t> last_hit_pos;
  if (int const rc = r.rows.spans(wins.size(), is_hit, last_hit_pos)) return raise(rc, RUN);
  r.ph.rows += r.ph.lap();
  std::vector<dcp_walk_hit> const &hits = r.walk.path_walked(is_hit.data(), last_hit_pos.data());
  r.progress(r.walk.take_queued());
  r.ph.windows += r.ph.lap();
  r.rows.format(hits);
  r.ph.rows += r.ph.lap();
  return 0;
}

// c-core/thread.c:114-121 for windows nobody has scored yet (only with no batch in flight)
int cost_batch(Run &r)
{
  std::vector<dcp_hip_window> const &wins = r.walk.take_cost_round();
  std::vector<int32_t> hit_index(wins.size());
  std::vector<float> lrts(wins.size());
  int nh = 0;
  ++r.rounds;
  r.ph.windows += r.ph.lap();
  if (wins.size() > (size_t)INT_MAX) return raise(DCP_ENOMEM, RUN, "more than INT_MAX windows to score again");
  if (int const rc = dcp_hip_cost_hits(r.x->eng, (int)wins.size(), wins.data(), &nh, hit_index.data(), lrts.data()))
    return raise(rc, RUN, dcp_hip_strerror(r.x->eng));
  r.ph.cost += r.ph.lap();
  r.walk.cost_scored(nh, hit_index.data(), lrts.data());
  r.progress(r.walk.take_queued());
  r.ph.windows += r.ph.lap();
  return 0;
}

} // namespace

extern "C" {

struct dcp_scan *dcp_scan_new(void) { return new (std::nothrow) dcp_scan; }

void dcp_scan_del(struct dcp_scan const *cx)
{
  dcp_scan *x = const_cast<dcp_scan *>(cx);
  if (!x) return;
  if (x->eng) dcp_hip_del(x->eng);
  delete x;
}

int dcp_scan_setup(struct dcp_scan *x, char const *dbfile, int port, int num_threads, bool multi_hits,
                   bool hmmer3_compat, bool cache, void (*callback)(void *), void *userdata)
{
  (void)port;
  (void)cache;
  if (num_threads > 128) return raise(DCP_EMANYTHREADS, __func__); // THREAD_MAX, c-core/thread.h:7
  int device = 0;
  if (char const *d = getenv("DECIPHON_HIP_DEVICE")) device = atoi(d);
  return setup_common(x, dbfile, device, 0, 1, false, multi_hits, hmmer3_compat, callback, userdata);
}

int dcp_scan_setup_partition(struct dcp_scan *x, char const *dbfile, int device, int index, int nparts,
                             bool multi_hits, bool hmmer3_compat, void (*callback)(void *), void *userdata)
{
  return setup_common(x, dbfile, device, index, nparts, false, multi_hits, hmmer3_compat, callback, userdata);
}

int dcp_scan_setup_partition_balanced(struct dcp_scan *x, char const *dbfile, int device, int index, int nparts,
                                      bool multi_hits, bool hmmer3_compat, void (*callback)(void *), void *userdata)
{
  return setup_common(x, dbfile, device, index, nparts, true, multi_hits, hmmer3_compat, callback, userdata);
}

int dcp_scan_setup_hmm(struct dcp_scan *x, char const *hmm, int gencode_id, float epsilon, bool multi_hits,
                       bool hmmer3_compat, void (*callback)(void *), void *userdata)
{
  if (!x || !hmm) return raise(DCP_EFUNCUSE, __func__);
  // the arguments first, in the order of dcp_hip_load_hmm: without a GPU they are still told apart
  {
    DcpNucltDist probe;
    float const zero[20] = {};
    if (!dcp_setup_nuclt_dist(gencode_id, zero, probe)) return raise(DCP_EGENCODEID, __func__);
  }
  if (!(epsilon >= 0.0f && epsilon <= 1.0f)) return raise(DCP_EFUNCUSE, __func__, "epsilon must lie in [0, 1]");
  if (FILE *f = fopen(hmm, "rb")) fclose(f);
  else return raise(DCP_EOPENHMM, __func__, hmm);
  int device = 0;
  if (char const *d = getenv("DECIPHON_HIP_DEVICE")) device = atoi(d);
  if (new_engine(x, device)) return raise(DCP_EFUNCUSE, __func__, "no usable HIP device (there is no CPU fallback)");
  std::unique_ptr<DcpHmmDecoders> kept(new DcpHmmDecoders);
  kept->gencode = gencode_id;
  kept->epsilon = epsilon;
  x->hmm = nullptr;
  x->db.reset();
  x->abc_name = "dna"; // what press writes
  x->index_offset = 0;
  x->num_proteins = 0;
  int rc = dcp_hip_load_hmm_sink(x->eng, hmm, gencode_id, epsilon, 0, -1, kept.get());
  if (rc) return raise(rc, __func__, dcp_hip_strerror(x->eng)); // (what the sink was shown goes with `kept`)
  if ((rc = dcp_hip_commit_profiles(x->eng))) return raise(rc, __func__, dcp_hip_strerror(x->eng));
  x->num_proteins = dcp_hip_num_profiles(x->eng);
  x->hmm = kept.get();
  x->db = std::move(kept);
  return set_mode(x, __func__, multi_hits, hmmer3_compat, callback, userdata);
}

int dcp_scan_set_epsilon(struct dcp_scan *x, float epsilon)
{
  // the arguments first: without a GPU the codes are still told apart
  if (!x) return raise(DCP_EFUNCUSE, __func__);
  if (!x->eng || !x->hmm) return raise(DCP_EFUNCUSE, __func__, "the scan was not set up by dcp_scan_setup_hmm");
  if (!(epsilon >= 0.0f && epsilon <= 1.0f)) return raise(DCP_EFUNCUSE, __func__, "epsilon must lie in [0, 1]");
  if (int const rc = dcp_hip_set_epsilon(x->eng, epsilon)) return raise(rc, __func__, dcp_hip_strerror(x->eng));
  x->hmm->epsilon = epsilon; // the codons of the rows are decoded under the tables' error rate (scan_rows.h)
  return 0;
}

int dcp_scan_set_gencode(struct dcp_scan *x, int gencode_id)
{
  // the arguments first: without a GPU the codes are still told apart
  if (!x) return raise(DCP_EFUNCUSE, __func__);
  if (!x->eng || !x->hmm) return raise(DCP_EFUNCUSE, __func__, "the scan was not set up by dcp_scan_setup_hmm");
  {
    DcpNucltDist probe;
    float const zero[20] = {};
    if (!dcp_setup_nuclt_dist(gencode_id, zero, probe)) return raise(DCP_EGENCODEID, __func__);
  }
  // the distributions the rows' codons are decoded from are the ones the engine recomputes (scan_rows.h)
  if (int const rc = dcp_hip_set_gencode_sink(x->eng, gencode_id, x->hmm)) return raise(rc, __func__, dcp_hip_strerror(x->eng));
  return 0;
}

int dcp_scan_calibrate(struct dcp_scan *x, int nseq, int len, uint64_t seed, float const freq[4], float lambda)
{
  if (!x) return raise(DCP_EFUNCUSE, __func__);
  if (!x->eng) return raise(DCP_EFUNCUSE, __func__, "dcp_scan_setup has not succeeded");
  if (int const rc = dcp_hip_calibrate(x->eng, nseq, len, seed, freq, lambda)) return raise(rc, __func__, dcp_hip_strerror(x->eng));
  return 0;
}

int dcp_scan_set_evalue(struct dcp_scan *x, double z, double max)
{
  if (!x || isnan(z) || isnan(max)) return raise(DCP_EFUNCUSE, __func__);
  x->evalue_z = z;
  x->evalue_max = max;
  return 0;
}

float dcp_scan_profile_mu(struct dcp_scan const *x, int i) { return x && x->eng ? dcp_hip_profile_mu(x->eng, i) : NAN; }

int dcp_scan_calibrate_lengths(struct dcp_scan *x, int nseq, int nlen, int const *lens, uint64_t seed, float const freq[4], float lambda)
{
  if (!x) return raise(DCP_EFUNCUSE, __func__);
  if (!x->eng) return raise(DCP_EFUNCUSE, __func__, "dcp_scan_setup has not succeeded");
  if (int const rc = dcp_hip_calibrate_lengths(x->eng, nseq, nlen, lens, seed, freq, lambda))
    return raise(rc, __func__, dcp_hip_strerror(x->eng));
  return 0;
}

double dcp_scan_profile_mu_at(struct dcp_scan const *x, int i, int64_t len) { return x && x->eng ? dcp_hip_profile_mu_at(x->eng, i, len) : NAN; }

float dcp_scan_profile_lambda(struct dcp_scan const *x, int i) { return x && x->eng ? dcp_hip_profile_lambda(x->eng, i) : NAN; }

int dcp_scan_set_strands(struct dcp_scan *x, int strands)
{
  // no engine is asked: the mode belongs to the scan and reaches the GPU with the reads of the next run
  if (!x) return raise(DCP_EFUNCUSE, __func__);
  if (strands != DCP_STRANDS_PLUS && strands != DCP_STRANDS_BOTH)
    return raise(DCP_EFUNCUSE, __func__, "strands must be DCP_STRANDS_PLUS or DCP_STRANDS_BOTH");
  x->strands = strands;
  return 0;
}

int dcp_scan_strands(struct dcp_scan const *x) { return x ? x->strands : raise(DCP_EFUNCUSE, __func__); }

int dcp_scan_partition_range(struct dcp_scan const *x, int *first, int *count)
{
  if (!x || !first || !count) return DCP_EFUNCUSE;
  *first = x->index_offset;
  *count = x->num_proteins;
  return 0;
}


// The pairs are scored speculatively, chunk by chunk (csrc/scan_walk.h: the rules of the walk).  Two cost batches are
// kept in flight (dcp_hip_cost_hits_begin): the host builds, sorts and uploads the window list of the next chunk while
// the GPU scores this one, and the kernels of a chunk follow those of the chunk before class by class, so the GPU never
// drains in between.  The hits go through the path pass when the cost batches are through; what then needs scoring
// again goes in a few small rounds at the end.  Rows are emitted in the reference's order (profile, read, window)
// whatever the order of work (csrc/scan_rows.h).
int dcp_scan_run(struct dcp_scan *x, struct dcp_batch *batch, char const *product_dir)
{
  if (!x || !batch || !product_dir) return raise(DCP_EFUNCUSE, __func__);
  if (!x->eng) return raise(DCP_EFUNCUSE, __func__, "dcp_scan_setup has not succeeded");
  x->done_proteins = 0;
  x->interrupted = false;
  x->runs.reset();
  int rc = 0;
  Phase ph;
  Knobs const knobs;

  // batch_encode (c-core/batch.c:60-70): every read goes to HBM once -- on both strands too: the engine then holds
  // `nseq` = 2 x reads sequences, 2s read s as given and 2s + 1 its reverse complement, and all that follows (chunks,
  // walk, passes, the order of the rows) works on those.  The rows map a sequence back to (read, strand).
  bool const both = x->strands == DCP_STRANDS_BOTH;
  if (batch->seqs.size() > (size_t)(both ? INT_MAX / 2 : INT_MAX)) return raise(DCP_EFUNCUSE, __func__, "too many reads");
  int const nreads = (int)batch->seqs.size(), per = both ? 2 : 1, nseq = nreads * per;
  for (dcp_batch::Seq const &s : batch->seqs) // c-core/sequence.c:61-72
  {
    if (x->abc_name == "dna" && s.has_u) return raise(DCP_EDBDNASEQRNA, __func__);
    if (x->abc_name == "rna" && s.has_t) return raise(DCP_EDBRNASEQDNA, __func__);
  }
  std::vector<int64_t> off((size_t)nreads + 1, 0);
  for (int i = 0; i < nreads; ++i) off[(size_t)i + 1] = off[(size_t)i] + (int64_t)batch->seqs[(size_t)i].nt.size();
  std::vector<uint8_t> nt((size_t)off[(size_t)nreads]);
  for (int i = 0; i < nreads; ++i)
    memcpy(nt.data() + off[(size_t)i], batch->seqs[(size_t)i].nt.data(), batch->seqs[(size_t)i].nt.size());
  if ((rc = dcp_hip_set_sequences_strands(x->eng, nreads, nt.data(), off.data(), x->strands)))
    return raise(rc, __func__, dcp_hip_strerror(x->eng));

  // product_open (c-core/product.c:14-32)
  std::string const file = std::string(product_dir) + "/products.tsv";
  if ((rc = mkdir_p(product_dir))) return raise(rc, __func__, product_dir);
  ph.reads += ph.lap();

  int const nprof = dcp_hip_num_profiles(x->eng);
  std::vector<int32_t> K((size_t)std::max(nprof, 0)), len((size_t)nseq);
  for (int p = 0; p < nprof; ++p) K[(size_t)p] = dcp_hip_profile_core_size(x->eng, p);
  for (int s = 0; s < nseq; ++s) // (both strands: each read's length twice)
  {
    if (batch->seqs[(size_t)(s / per)].nt.size() > (size_t)INT_MAX) return raise(DCP_EFUNCUSE, __func__, "a read is longer than INT_MAX");
    len[(size_t)s] = (int32_t)batch->seqs[(size_t)(s / per)].nt.size();
  }
  // chunks (dcp_plan_chunks: profiles [p0, p1) x reads [s0, s1)): small enough for the window table of a chunk (2^21
  // pairs; DECIPHON_HIP_CHUNK_WINDOWS windows, 4 Mi by default -- a chunk holds every window of its pairs' no-hit
  // chains, and the host keeps its list, the pinned copy and per-window results for two chunks in flight); the first
  // one is kept short (~1e10 DP cells, a dozen milliseconds of cost pass) so that the GPU starts early and the host
  // builds the window list of the second chunk meanwhile (14 ms for the headline's 416 k windows; 4e10 cells while the
  // upload of that list still waited for the device, profiles/r03_exp_register_policy.txt: 0.497-0.499 -> 0.493-0.495 s).
  std::vector<DcpChunk> const chunks = dcp_plan_chunks(
      nprof, K.data(), nseq, len.data(), knobs.chunk_cells > 0 ? knobs.chunk_cells : DCP_SCAN_FIRST_CHUNK_CELLS,
      knobs.chunk_cells > 0 ? knobs.chunk_cells : HUGE_VAL, DCP_SCAN_CHUNK_PAIRS,
      knobs.chunk_windows >= 1 ? (int64_t)std::min(knobs.chunk_windows, 1.0e18) : DCP_SCAN_CHUNK_WINDOWS);
  // the engine takes a window list's length as int (only a single pair's chain is beyond the cap, and no read of
  // fewer than 2^31 nucleotides makes 2^31 windows, but DECIPHON_HIP_CHUNK_WINDOWS may raise the cap that far)
  for (DcpChunk const &c : chunks)
    if (c.windows > (int64_t)INT_MAX)
      return raise(DCP_EFUNCUSE, __func__, "a chunk holds more than INT_MAX windows: lower DECIPHON_HIP_CHUNK_WINDOWS");

  DcpScanWalk walk(nprof, K.data(), nseq, len.data());
  // (bytes below 2^63; what atof makes of no number is 0)
  int64_t const budget = knobs.product_mb >= 1.0e12 ? INT64_MAX : knobs.product_mb > 0 ? (int64_t)(knobs.product_mb * 1048576.0) : 0;
  x->runs.reset(new DcpProductRuns(product_dir, budget, both));
  DropRuns drop{x};
  // Z of the evalue column: the sequences this run scans (HMMER's Z, the number of targets) unless the caller set one
  DcpEvalueRule const evalue{x->evalue_z > 0 ? x->evalue_z : (double)nseq, x->evalue_max};
  DcpScanRows rows(x->eng, x->db.get(), x->index_offset, x->abc_name.c_str(), batch, x->runs.get(), both, evalue); // (after all that its threads read)
  Run r{x, walk, rows, ph};
  if (knobs.speculate)
  {
    std::deque<InFlight> flight;
    Drain drain{x->eng, &flight};
    int next = 0, released = 0; // chunks [0, next) are begun; the decoders of profiles [0, released) are gone
    int const nchunks = (int)chunks.size();
    // Path passes run once no cost batch is in flight.  When more than DECIPHON_HIP_PATH_DRAIN_HITS windows wait for
    // one, no new chunk is begun: the batches in flight end, the path passes run, the decoders of the profiles that
    // are through are released, and then the chunks go on.  Without that every hit would wait for the last chunk, and
    // the decoders of all profiles with hits would be held at once.  (The chains and speculated scores of the pairs
    // that hit stay for the whole scan either way.)  The default, 32768, is above the headline's ~2300 hits and the
    // 13 k of the stress scan: those run their path passes at the end.
    auto may_begin = [&]() { return next < nchunks && walk.path_waiting() <= knobs.drain_hits; };
    auto begin_next = [&]() {
      int const c = next++;
      return begin_chunk(r, flight, chunks[(size_t)c], c);
    };
    auto refill = [&]() -> int {
      while (may_begin() && flight.size() < 2 && !x->interrupted)
        if (int const brc = begin_next()) return brc;
      return 0;
    };
    if ((rc = refill())) return rc;
    while (!flight.empty())
    {
      InFlight f = std::move(flight.front());
      flight.pop_front();
      DcpChunk const &chunk = chunks[(size_t)f.chunk];
      std::vector<int32_t> hit_index(f.wins.size() + 1);
      std::vector<float> lrts(f.wins.size() + 1);
      int nh = 0;
      if ((rc = dcp_hip_cost_hits_end(x->eng, &nh, hit_index.data(), lrts.data())))
        return raise(rc, __func__, dcp_hip_strerror(x->eng));
      ph.cost += ph.lap();
      if (x->interrupted) continue; // (the batches still in flight are ended and dropped)
      if (may_begin() && (rc = begin_next())) return rc;
      walk.chunk_scored(chunk, f.base.data(), nh, hit_index.data(), lrts.data());
      r.progress(walk.take_queued());
      ph.windows += ph.lap();
      // The path passes of the hits so far -- once no batch is in flight (at the end, or after a drain): beside a
      // cost pass the path kernels, few wavefronts bound by memory latency, take several times as long and hold the
      // cost kernels up for as long (whichever priority their streams have: profiles/r03_scan_pipeline.txt), so the
      // scan gains nothing from the overlap and a short one loses.  What needs scoring again waits for the end.
      while ((flight.empty() || knobs.path_beside) && walk.path_waiting() && !x->interrupted)
        if ((rc = path_batch(r))) return rc;
      // a profile is through at its last chunk of reads
      int const through = chunk.s1 == nseq ? chunk.p1 : chunk.p0;
      x->done_proteins += through - chunk.p0;
      // Once the path passes have caught up, the decoders of the profiles that are through go: a Pfam-sized database
      // with hits on most profiles would pin gigabytes by the end of the scan.
      if (!walk.path_waiting())
      {
        rows.release_decoders(released, through);
        released = std::max(released, through);
      }
      if ((rc = refill())) return rc;
    }
  }
  else
  {
    walk.all_pairs();
    r.progress(walk.take_queued());
  }
  // the rounds of what is left: windows to score again (or, with nothing speculated, every window), their path passes
  while ((walk.cost_waiting() || walk.path_waiting()) && !x->interrupted)
  {
    if (walk.path_waiting() && (rc = path_batch(r))) return rc;
    if (walk.cost_waiting() && (rc = cost_batch(r))) return rc;
  }
  if (!knobs.speculate) x->done_proteins += nprof;
  rows.release_decoders(0, nprof);

  if ((rc = rows.join())) return raise(rc, __func__);
  ph.rows += ph.lap();
  if ((rc = rows.write(file))) return raise(rc, __func__, file.c_str());
  drop.keep = true;
  ph.write += ph.lap();
  {
    // (the progress callbacks of a batch are made while the GPU scores it: they count as cost pass)
    double const t[DCP_SCAN_TIMING_VALUES] = {ph.total(), ph.reads, ph.windows, ph.cost + ph.callbacks, ph.path, ph.rows, ph.write,
                                              (double)r.rounds, (double)walk.windows_walked(), (double)r.nhits,
                                              (double)r.chunks_begun, (double)r.largest_chunk, (double)r.path_batches};
    memcpy(x->timing, t, sizeof t);
  }
  if (knobs.timing)
    fprintf(stderr,
            "dcp_scan_run: %d rounds, %zu windows, %zu path passes in %d batches, %d chunks of at most %lld windows; "
            "windows %.3f s, cost pass %.3f s, path pass %.3f s, rows %.3f s, products.tsv %.3f s; of the cost pass "
            "%.3f s in progress callbacks\n",
            r.rounds, walk.windows_walked(), r.nhits, r.path_batches, r.chunks_begun, (long long)r.largest_chunk, ph.windows,
            ph.cost + ph.callbacks, ph.path, ph.rows, ph.write, ph.callbacks);
  return 0;
}

void dcp_scan_interrupt(struct dcp_scan *x)
{
  if (x) x->interrupted = true;
}

int dcp_scan_progress(struct dcp_scan const *x)
{
  if (!x || x->num_proteins <= 0) return 0;
  return (100 * x->done_proteins.load()) / x->num_proteins; // c-core/scan.c:224-227
}

long dcp_scan_num_products(struct dcp_scan const *x) { return x && x->runs ? x->runs->num_rows() : 0; }

int dcp_scan_product_stats(struct dcp_scan const *x, int64_t *out, int n)
{
  if (!x || (n > 0 && !out)) return 0;
  int64_t v[DCP_SCAN_PRODUCT_STATS_VALUES] = {0, 0, 0, 0};
  if (x->runs) x->runs->stats(v);
  for (int i = 0; i < n && i < DCP_SCAN_PRODUCT_STATS_VALUES; ++i) out[i] = v[i];
  return DCP_SCAN_PRODUCT_STATS_VALUES;
}

int dcp_scan_last_timing(struct dcp_scan const *x, double *out, int n)
{
  if (!x || (n > 0 && !out)) return 0;
  for (int i = 0; i < n && i < DCP_SCAN_TIMING_VALUES; ++i) out[i] = x->timing[i];
  return DCP_SCAN_TIMING_VALUES;
}

char const *dcp_scan_product(struct dcp_scan const *x, long i)
{
  return x && x->runs ? x->runs->row(i) : nullptr;
}

struct dcp_batch *dcp_batch_new(void) { return new (std::nothrow) dcp_batch; }

void dcp_batch_del(struct dcp_batch *x) { delete x; }

int dcp_batch_add(struct dcp_batch *x, long id, char const *name, char const *data)
{
  if (!x || !name || !data) return raise(DCP_EFUNCUSE, __func__);
  dcp_batch::Seq s;
  s.id = id;
  s.name = name;
  size_t const n = strlen(data);
  s.nt.resize(n);
  int rc = dcp_encode_sequence(data, (int64_t)n, s.nt.data());
  if (rc) return raise(rc, __func__);
  s.text.resize(n);
  for (size_t i = 0; i < n; ++i) s.text[i] = "ACGT"[s.nt[i]];
  // the reference keeps U as U in the stored text (c-core/disambiguate.c:14-21)
  for (size_t i = 0; i < n; ++i)
  {
    s.has_u = s.has_u || data[i] == 'U' || data[i] == 'u';
    s.has_t = s.has_t || data[i] == 'T' || data[i] == 't';
  }
  if (s.has_u)
    for (size_t i = 0; i < n; ++i)
      if (s.text[i] == 'T') s.text[i] = 'U';
  x->seqs.push_back(std::move(s));
  return 0;
}

void dcp_batch_reset(struct dcp_batch *x)
{
  if (x) x->seqs.clear();
}

} // extern "C"
