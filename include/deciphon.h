/* deciphon.h -- the reference's public C API (c-core/deciphon.h:9-32), as exported
 * by libdeciphon_hip.so, so that existing callers (python-core's CFFI binding,
 * python-core/deciphon_core/interface.h:1-40; c-core/test_scan.c:36-41) link
 * against the MI355X path unchanged.
 *
 * What differs from the reference, by design of this build:
 *  - dcp_scan_run scores every (profile x window) on the GPU; `num_threads` is
 *    accepted and ignored (one engine drives one GPU), `cache` likewise (profiles
 *    are always resident in HBM).
 *  - HMMER rescoring (the h3daemon TCP client of c-core/hmmer.c) is out of scope:
 *    `port` is ignored, no row is dropped for lack of a HMMER hit and no hmmer/
 *    directory with .h3r files is written.  The `evalue` column holds `nan` -- unless
 *    the scan is calibrated (dcp_scan_calibrate, below): it then holds the E-value of
 *    the row's own lrt under a Gumbel distribution fitted to the profile's scores on
 *    random reads, as HMMER calibrates its own scores, and rows at or beyond a limit
 *    are left out (dcp_scan_set_evalue).  That is not HMMER's E-value of the hit.
 *  - the codon and amino fields of the `match` column come from a restatement of third-party
 *    imm's imm_frame_cond_decode (csrc/host_logic.h), pinned by the reference's committed
 *    products.tsv only.
 *  - dcp_press_* reads HMMER3 text and builds the model on the host (csrc/hmm_model.h: a restatement of
 *    hmm_reader.c, the third-party hmr reader, model.c and the imm arithmetic it calls) and computes the
 *    emission tables on the GPU (csrc/press_kernel.hip).  It writes the current encoding (f32 arrays as `bin`,
 *    c-core/write.c:59-66).  dcp_press_open fails with DCP_EFUNCUSE, creating nothing, without a gfx950 at
 *    DECIPHON_HIP_DEVICE (default 0).
 */
#ifndef DECIPHON_AMD_DECIPHON_H
#define DECIPHON_AMD_DECIPHON_H

#include <stdbool.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

struct dcp_scan;
struct dcp_batch;
struct dcp_press;

/* scan: c-core/scan.c:40-227 */
struct dcp_scan *dcp_scan_new(void);
void dcp_scan_del(struct dcp_scan const *);
int dcp_scan_setup(struct dcp_scan *, char const *dbfile, int port, int num_threads, bool multi_hits,
                   bool hmmer3_compat, bool cache, void (*callback)(void *), void *userdata);
int dcp_scan_run(struct dcp_scan *, struct dcp_batch *, char const *product_dir);
void dcp_scan_interrupt(struct dcp_scan *);
int dcp_scan_progress(struct dcp_scan const *);

/* batch: c-core/batch.c:15-58 */
struct dcp_batch *dcp_batch_new(void);
void dcp_batch_del(struct dcp_batch *);
int dcp_batch_add(struct dcp_batch *, long id, char const *name, char const *data);
void dcp_batch_reset(struct dcp_batch *);

/* press: c-core/press.c:43-204, see above.  Call order: setup (while no press is open), open, next until end()
 * is true, close.  next before open, after end() or after a failed next is DCP_EFUNCUSE.  A parse error is returned
 * by the next that reaches that protein.  close after a failed next removes the output and returns 0; close
 * before end() writes the proteins pressed so far, as the reference does.  No call leaves a temporary file. */
struct dcp_press *dcp_press_new(void);
int dcp_press_setup(struct dcp_press *, int gencode_id, float epsilon);
int dcp_press_open(struct dcp_press *, char const *hmm, char const *db);
long dcp_press_nproteins(struct dcp_press const *);
int dcp_press_next(struct dcp_press *);
bool dcp_press_end(struct dcp_press const *);
int dcp_press_close(struct dcp_press *);
void dcp_press_del(struct dcp_press const *);

char const *dcp_error_string(int error_code);

/* The return codes, value for value c-core/deciphon.h:34-116: they are part of the ABI Python sees
 * through CFFI.  GPU failures are mapped onto existing codes (DCP_ENOMEM, DCP_EFUNCUSE). */
enum
{
  DCP_EDIFFABC = 1,
  DCP_EFCLOSE = 2,
  DCP_EFDATA = 3,
  DCP_EREFOPEN = 4,
  DCP_EFREAD = 5,
  DCP_EFSEEK = 6,
  DCP_EFTELL = 7,
  DCP_EFUNCUSE = 8,
  DCP_EFWRITE = 9,
  DCP_EGETPATH = 10,
  DCP_EZEROSEQ = 11,
  DCP_EZEROMODEL = 12,
  DCP_EZEROPART = 13,
  DCP_EDECODON = 14,
  DCP_ELARGEMODEL = 15,
  DCP_ELARGEPROTEIN = 16,
  DCP_EREADHMMER3 = 17,
  DCP_EMANYPARTS = 18,
  DCP_EMANYTRANS = 19,
  DCP_ENOMEM = 20,
  DCP_EOPENDB = 21,
  DCP_EOPENHMM = 22,
  DCP_EOPENTMP = 23,
  DCP_ETRUNCPATH = 24,
  DCP_EDPUNPACK = 25,
  DCP_EDPPACK = 26,
  DCP_ENUCLTDUNPACK = 27,
  DCP_ENUCLTDPACK = 28,
  DCP_ESETTRANS = 29,
  DCP_EADDSTATE = 30,
  DCP_EDPRESET = 31,
  DCP_EFSTAT = 32,
  DCP_EFOPEN = 33,
  DCP_ELARGEFILE = 34,
  DCP_ELONGPATH = 35,
  DCP_EIMMRESETTASK = 36,
  DCP_EIMMNEWTASK = 37,
  DCP_EIMMSETUPTASK = 38,
  DCP_EWRITEPROD = 39,
  DCP_EINVALPART = 40,
  DCP_ELONGACCESSION = 41,
  DCP_EMANYTHREADS = 42,
  DCP_ETMPFILE = 43,
  DCP_EFFLUSH = 44,
  DCP_EMKDIR = 45,
  DCP_EFORMAT = 46,
  DCP_ERMDIR = 47,
  DCP_ERMFILE = 48,
  DCP_ESETGENCODE = 49,
  DCP_EGENCODEID = 50,
  DCP_EH3CDIAL = 51,
  DCP_EH3CPUT = 52,
  DCP_EH3CPOP = 53,
  DCP_EH3CPACK = 54,
  DCP_EH3CMAXRETRY = 55,
  DCP_EH3CWARMUP = 56,
  DCP_ESEQABC = 57,
  DCP_EFDOPEN = 58,
  DCP_EMKSTEMP = 59,
  DCP_ELONGABC = 60,
  DCP_ELONGCONSENSUS = 61,
  DCP_ENOTDIALED = 62,
  DCP_ELARGECORESIZE = 63,
  DCP_EINVALSTATE = 64,
  DCP_EINVALSIZE = 65,
  DCP_EENDOFFILE = 66,
  DCP_EENDOFNODES = 67,
  DCP_EDBVERSION = 68,
  DCP_ENOTDBFILE = 69,
  DCP_EINVALSTATEID = 70,
  DCP_ENUCLTNOSUPPORT = 71,
  DCP_EDBDNASEQRNA = 72,
  DCP_EDBRNASEQDNA = 73,
  DCP_ENUCLTSEQTU = 74,
  DCP_ENOHIT = 75,
  DCP_EOPEN = 76,
  DCP_ECLOSE = 77,
  DCP_EDUP = 78,
  DCP_ETOOMANYPROTEINS = 79,
  DCP_EINVALNUMPROTEINS = 80,
};

/* Not in the reference: a scan that owns only partition `index` of `nparts`
 * contiguous profile partitions (partition_size, c-core/partition_size.c:13-16) on
 * HIP device `device` -- what one rank of a multi-GPU job calls instead of
 * dcp_scan_setup.  Its products.tsv rows are that partition's, in database order. */
int dcp_scan_setup_partition(struct dcp_scan *, char const *dbfile, int device, int index, int nparts,
                             bool multi_hits, bool hmmer3_compat, void (*callback)(void *), void *userdata);
/* The same with partition boundaries that balance the sum of core sizes instead of the number of profiles
 * (DP cells go with K): still contiguous and in database order, so the ranks' rows still
 * concatenate to the whole scan's.  dcp_scan_partition_range reports what a scan owns. */
int dcp_scan_setup_partition_balanced(struct dcp_scan *, char const *dbfile, int device, int index, int nparts,
                                      bool multi_hits, bool hmmer3_compat, void (*callback)(void *), void *userdata);
int dcp_scan_partition_range(struct dcp_scan const *, int *first, int *count);
/* Not in the reference: dcp_scan_setup from a HMMER3 file instead of a pressed database (device:
 * DECIPHON_HIP_DEVICE).  Rows are those of a scan of the file dcp_press_* writes from hmm at the same
 * gencode_id and epsilon.  Nothing is written: the emission tables are made on the GPU and stay there
 * (dcp_hip_load_hmm, whose error codes these are), and the scan keeps the nucleotide and codon distributions of
 * every node in host memory (516 bytes per node) for the codons of its rows.  Not partitioned. */
int dcp_scan_setup_hmm(struct dcp_scan *, char const *hmm, int gencode_id, float epsilon, bool multi_hits,
                       bool hmmer3_compat, void (*callback)(void *), void *userdata);
/* Not in the reference: a scan set up by dcp_scan_setup_hmm at another error rate, without reading the file again
 * (dcp_hip_set_epsilon: the tables are rewritten on the GPU, in place).  The next dcp_scan_run writes the rows a fresh
 * dcp_scan_setup_hmm at `epsilon` would, codons and amino acids included.  DCP_EFUNCUSE, with the scan left as it was,
 * for NULL, for a scan that is not set up or was set up from a pressed file, and for epsilon outside [0, 1] or NaN --
 * all checked before the GPU is touched.  Not to be called while dcp_scan_run runs on that scan (nothing locks).  The
 * rows of the last run (dcp_scan_product) stay valid. */
int dcp_scan_set_epsilon(struct dcp_scan *, float epsilon);
/* Not in the reference: a scan set up by dcp_scan_setup_hmm under another translation table, at the error rate it is
 * at, without reading the file again (dcp_hip_set_gencode: the nodes' distributions are derived again on the host from
 * their amino log-odds, the tables rewritten on the GPU, in place).  The scan's own distributions, which the codons of
 * its rows are decoded from, come from the same recomputation.  The next dcp_scan_run writes the rows a fresh
 * dcp_scan_setup_hmm at gencode_id would, codons and amino acids included.  DCP_EFUNCUSE for NULL, for a scan that is
 * not set up or was set up from a pressed file (a .dcp holds no amino log-odds), then DCP_EGENCODEID for a table not
 * held -- all checked before the GPU is touched, the scan left as it was.  Not to be called while dcp_scan_run runs on
 * that scan.  The rows of the last run (dcp_scan_product) stay valid. */
int dcp_scan_set_gencode(struct dcp_scan *, int gencode_id);
/* Not in the reference, whose E-values come from a HMMER daemon: the profiles of a scan calibrated on the GPU
 * (dcp_hip_calibrate, include/deciphon_hip.h, whose arguments and error codes these are): every profile is scored
 * against nseq random reads of len nucleotides (seed, freq[4] = frequencies of A, C, G, T or NULL for uniform:
 * csrc/calibrate.h) and the location mu of a Gumbel distribution of lrt is fitted at fixed lambda.  lrt is twice the
 * log-odds in nats: pass lambda = 0.5, HMMER's conjectured ln 2 per bit (what has been measured).
 * Valid after any setup and between runs, DCP_EFUNCUSE before; wanted again after dcp_scan_set_epsilon or
 * dcp_scan_set_gencode, which make the scan uncalibrated again.  dcp_scan_profile_mu: mu of local profile i, NaN when it
 * is not calibrated (or for a bad index or NULL).
 * A calibrated scan prints dcp_lrt_evalue(row lrt, mu of its profile, lambda, Z) (include/deciphon_host.h) with %.2g in
 * the evalue column, as c-core/product_thread.c:60 prints HMMER's, and leaves out the rows with E >= max.
 * dcp_scan_set_evalue: z <= 0, the default, makes Z the number of sequences the run scans -- its reads, twice that on
 * both strands: HMMER's Z, the number of targets; max is +inf by default, and the reference's rule is max = 1
 * (c-core/thread.c:192-201).  The window walk does not depend on the filter (thread.c:162 against thread.c:201): the
 * rows kept are, apart from that column, a subset in order of the unfiltered rows.  DCP_EFUNCUSE for NULL or NaN.
 * A scan that is not calibrated writes `nan` and keeps every row, whatever max is. */
int dcp_scan_calibrate(struct dcp_scan *, int nseq, int len, uint64_t seed, float const freq[4], float lambda);
int dcp_scan_set_evalue(struct dcp_scan *, double z, double max);
float dcp_scan_profile_mu(struct dcp_scan const *, int i);
/* The same over a ladder of read lengths (dcp_hip_calibrate_lengths, include/deciphon_hip.h, whose arguments and error
 * codes these are): a scan holds windows from a few hundred to 100 000 nucleotides and mu moves with the length, so
 * every profile gets a mu per length of lens[nlen], and with lambda == 0 a lambda of its own, fitted.  The evalue column
 * and the filter are then
 *   dcp_lrt_evalue(lrt, (float)mu of the profile at window_stop - window_start, lambda of the profile, Z)
 * with mu at a length by dcp_calib_mu_at (include/deciphon_host.h): linear in ln length between the rungs and beyond
 * them.  After dcp_scan_calibrate that is what it has always been: one rung, a constant mu, the lambda passed.  The
 * scan is uncalibrated again on the same events.  dcp_scan_profile_mu_at, dcp_scan_profile_lambda: of local profile i;
 * NaN when it is not calibrated. */
int dcp_scan_calibrate_lengths(struct dcp_scan *, int nseq, int nlen, int const *lens, uint64_t seed, float const freq[4],
                               float lambda);
double dcp_scan_profile_mu_at(struct dcp_scan const *, int i, int64_t len);
float dcp_scan_profile_lambda(struct dcp_scan const *, int i);
/* Not in the reference, which scans every read in the orientation it was given and no other (its GFF writer has
 * strand "+" for every hit): DCP_STRANDS_BOTH makes every later dcp_scan_run scan both strands of every read.  The reads
 * go to the GPU once; the code rows of the reverse complements are written there (dcp_hip_set_sequences_strands), and
 * the scan walks 2 x reads sequences.  The MINUS STRAND of a read is the reverse complement of the text dcp_batch_add
 * keeps -- uppercased and disambiguated first, then reversed with A<->T (A<->U for an RNA read) and C<->G -- not the
 * disambiguation of the reverse complement: the two differ only where c-core/disambiguate.c breaks a tie.
 * products.tsv then has a 13th column `strand`, + or -, and its rows are in (profile, read, strand with + first,
 * window) order.  window_start, window_stop, hit_start, hit_stop and the match column of a - row are on the scanned
 * strand, 0-based from the 5' end of the reverse complement: exactly what a plain scan of the reverse-complemented
 * read prints.  On the read as given a hit of a read of L nucleotides spans
 * [L - (window_start + hit_stop), L - (window_start + hit_start)).  DCP_STRANDS_PLUS, the default, is the reference's
 * behaviour and its 12 columns.  Allowed before or after any setup call and between runs; DCP_EFUNCUSE for NULL or
 * another value, without touching a GPU.  dcp_scan_strands: the mode a scan is in (DCP_EFUNCUSE for NULL). */
#ifndef DCP_STRANDS_PLUS /* (include/deciphon_hip.h has the same two) */
#define DCP_STRANDS_PLUS 0
#define DCP_STRANDS_BOTH 1
#endif
int dcp_scan_set_strands(struct dcp_scan *, int strands);
int dcp_scan_strands(struct dcp_scan const *);
/* Number of product rows the last dcp_scan_run wrote, and row i (without newline).  The pointer stands until the next
 * dcp_scan_run or dcp_scan_del of that scan.  Once the scan has spilled rows to run files (dcp_scan_product_stats:
 * runs > 0; DECIPHON_HIP_PRODUCT_MB) it stands only until the next dcp_scan_product on that scan, and
 * dcp_scan_product is then not to be called from two threads at once. */
long dcp_scan_num_products(struct dcp_scan const *);
char const *dcp_scan_product(struct dcp_scan const *, long i);
/* How the last dcp_scan_run held its product rows (csrc/product_runs.h).  Fills out[0..n) with, in order: the rows,
 * the sorted run files written to the product directory and removed again (0: every row stayed in memory), the most
 * bytes of row text held in memory at once, and the bytes of products.tsv.  Returns how many values exist
 * (DCP_SCAN_PRODUCT_STATS_VALUES). */
#define DCP_SCAN_PRODUCT_STATS_VALUES 4
int dcp_scan_product_stats(struct dcp_scan const *, int64_t *out, int n);
/* Where the wall time of the last dcp_scan_run went (measurement only; SURVEY 8d's wall definition: first H2D of the
 * reads to the last product row on the host).  Fills out[0..n) with, in order: total seconds, reads H2D + encode,
 * window bookkeeping, cost pass + LRT filter, path pass + unzip (the part the cost pass did not cover), row
 * formatting + decoding, products.tsv, then the counts of rounds, windows scored and path passes, and of the chunks
 * of speculated windows (cost batches begun ahead of the hits), the most windows one of them held and the path
 * batches.  Returns how many values exist (DCP_SCAN_TIMING_VALUES). */
#define DCP_SCAN_TIMING_VALUES 13
int dcp_scan_last_timing(struct dcp_scan const *, double *out, int n);
/* Where the time of the current (or last) press went, from open on (measurement only).  Fills out[0..n) with, in
 * order: seconds of parsing + model building (host), of uploads, of the emission kernel and of copy-back (GPU, from
 * HIP events), of the host waiting for the GPU, of writing (records + header at close), then the nodes written and
 * the bytes written.  Returns how many values exist (DCP_PRESS_TIMING_VALUES). */
#define DCP_PRESS_TIMING_VALUES 8
int dcp_press_last_timing(struct dcp_press const *, double *out, int n);

#ifdef __cplusplus
}
#endif

#endif
