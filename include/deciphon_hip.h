/* deciphon_hip.h -- C ABI of the MI355X-native Deciphon Viterbi scan path.
 *
 * This is the batched operator interface a libdeciphon build binds in place of
 * its per-thread DP engine: where c-core/thread.c:98-128 (process_window) calls
 * viterbi_null / viterbi_cost / viterbi_path on one (profile, window) at a time
 * through c-core/viterbi.h:38-52, a caller hands this library the same
 * parameters for many windows at once and gets the same numbers back.
 * Plain pointers and sizes only; every function returns 0 or a DCP_E* code of
 * c-core/deciphon.h:34-116 (the enum is part of the Python-visible ABI and is
 * reused, not extended).  The per-problem drop-in for viterbi.h itself is in
 * dcp_viterbi.h; the reference's outer dcp_scan_ / dcp_batch_ API is in
 * deciphon.h of this directory.
 *
 * There is no CPU fallback: every entry point that computes fails with
 * DCP_EFUNCUSE when no gfx950 device is usable.
 */
#ifndef DECIPHON_HIP_H
#define DECIPHON_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DCP_HIP_TABLE_SIZE 1364 /* viterbi_table_size(), c-core/viterbi.c:13,739 */
#define DCP_HIP_NUM_TRANS 8     /* enum core_trans_id, c-core/viterbi.h:22-32 */
#define DCP_HIP_NUM_XTRANS 13   /* enum extr_trans_id, c-core/viterbi.h:4-19 */

struct dcp_hip;

/* Number of usable HIP devices (0 when there is none; never fails). */
int dcp_hip_device_count(void);

/* One engine per GPU and per host thread (replaces the per-thread `struct work`
 * array of c-core/scan.c:28-33 / c-core/work.c:24-51).  NULL when the device
 * cannot be initialised. */
struct dcp_hip *dcp_hip_new(int device);
void dcp_hip_del(struct dcp_hip *);
char const *dcp_hip_strerror(struct dcp_hip const *); /* detail of the last failure */

/* ---- profiles (replaces work_setup -> protein_setup_viterbi, c-core/work.c:24-45) ----
 * dcp_hip_add_profile takes DP costs exactly as viterbi_set_core_trans /
 * _set_match / _set_null / _set_background receive them (c-core/viterbi.c:407-444):
 *   trans[8][K] in enum core_trans_id order, match[1364][K], null[1364], bg[1364].
 * dcp_hip_add_protein takes what protein_unpack yields (c-core/protein.c:283-351),
 * natural-log probabilities: node_trans[K+1][7] (MM,MI,MD,IM,II,DM,DD),
 * node_emission[K+1][1364], BMk[K], null/bg emission[1364], and applies the
 * mapping of protein_setup_viterbi (c-core/protein.c:353-394).
 * Both return the profile's index through *index.  Core sizes up to 16383 (state ids keep 14
 * bits for k + 1, c-core/state.h:27-39); DCP_ELARGECORESIZE beyond.  The delete costs MD, DD must
 * be non-negative (-log-probabilities are): the kernels take E = min M and bound delete runs
 * with that; DCP_EFUNCUSE / DCP_EFDATA otherwise. */
int dcp_hip_add_profile(struct dcp_hip *, int K, float const *trans, float const *match,
                        float const *null_cost, float const *bg_cost, int *index);
int dcp_hip_add_protein(struct dcp_hip *, int K, float const *node_trans, float const *node_emission,
                        float const *BMk, float const *null_lprob, float const *bg_lprob, int *index);
/* Reads proteins [first, first+count) of a pressed database (count < 0: to the
 * end); replaces database_reader_open + protein_reader + protein_iter_next
 * (c-core/database_reader.c:26-80, c-core/protein_reader.c:29-128). */
int dcp_hip_load_dcp(struct dcp_hip *, char const *path, int first, int count);
/* Reads profiles [first, first+count) of a HMMER3 text file (count < 0: to the end), builds their models on the host
 * (hmm_model.cpp), computes their emission tables under translation table gencode_id and error rate epsilon on the
 * GPU and leaves them in the pool as dcp_hip_load_dcp of the file dcp_press_* would write leaves them.  No file is
 * written.
 * As dcp_hip_load_dcp: profiles are appended behind what is resident, accessions kept, dcp_hip_commit_profiles
 * publishes.  Failures, in this order: NULL arguments DCP_EFUNCUSE; an unknown table DCP_EGENCODEID; epsilon outside
 * [0, 1] or NaN DCP_EFUNCUSE; a file that cannot be opened DCP_EOPENHMM; then, profile by profile in file order, the
 * reader's own codes (as dcp_press_next returns them) and DCP_ELARGECORESIZE beyond 16383 -- the file is read as it is
 * loaded, so of a profile too long and a broken one behind it the first in the file is reported; DCP_EINVALPART for
 * `first` out of range, once the file has been read; device errors.  The pool is sized once from the file's LENG
 * lines (and grown where they fall short).  On any
 * failure no profile is added: dcp_hip_num_profiles and dcp_hip_pool_bytes are what they were.  Profiles in front of
 * `first` are parsed and skipped; those behind the range are not read.  Batches as press makes them
 * (DECIPHON_HIP_PRESS_BATCH_NODES); DECIPHON_HIP_TIMING prints the seconds of parsing, upload, the emission kernel,
 * the rows kernel and waiting to stderr. */
int dcp_hip_load_hmm(struct dcp_hip *, char const *hmm, int gencode_id, float epsilon, int first, int count);
/* The profiles that came by dcp_hip_load_hmm again at another error rate, on the GPU and in place.  A load keeps what
 * its emission tables were made from in HBM beside the pool -- 528 bytes per node (nucltp[4], codonm[125]), against
 * 5456 or more of tables, and the null model and the background of each load (dcp_hip_dist_bytes: all of it) -- and
 * this call writes every profile's emission rows, their headers and the cost-order copies again from them: no file
 * is read and nothing but a list of workgroups goes up.  Afterwards the pool is, word for word, what dcp_hip_load_hmm
 * of the same files, ranges and translation tables leaves at `epsilon`; the transitions do not depend on the error
 * rate and are not touched.  Offsets and sizes stay, so nothing needs committing again.  It runs on the engine's
 * stream and returns when the tables are written.
 * Failures, in this order, each leaving the pool and every query as they were: NULL DCP_EFUNCUSE; cost batches
 * outstanding DCP_EFUNCUSE (as every call that changes the inputs); epsilon outside [0, 1] or NaN DCP_EFUNCUSE; a
 * profile, committed or not, that came by dcp_hip_add_profile, _add_protein or _load_dcp -- no distributions are
 * kept for those -- DCP_EFUNCUSE, dcp_hip_strerror naming the first; device errors.  Without profiles it returns 0 and
 * does nothing.  The translation table stays what it is: dcp_hip_set_gencode changes it.  DECIPHON_HIP_TIMING prints
 * profiles, nodes, bytes written and the kernel's seconds. */
int dcp_hip_set_epsilon(struct dcp_hip *, float epsilon);
/* the error rate profile `index` is at; NaN for a profile without kept distributions (and for a bad index or NULL) */
float dcp_hip_profile_epsilon(struct dcp_hip const *, int index);
/* The profiles that came by dcp_hip_load_hmm again under another translation table, without their files.  The kept
 * distributions themselves depend on the table, but what they are derived from does not: a load also keeps every
 * node's 20 amino log-odds, 80 bytes in host memory (not counted by dcp_hip_dist_bytes).  This call derives every
 * node's nucltp and codonm from them again under gencode_id -- on the host, by the function the load uses
 * (dcp_regencode_entries, include/deciphon_host.h), on up to 16 threads --, uploads them over the kept ones in chunks
 * (64 MiB of pinned memory, twice; DECIPHON_HIP_STAGE_MB shrinks them) with the table's null model and background for
 * every load, and writes the rows as dcp_hip_set_epsilon does, once per error rate among the profiles: every profile
 * keeps its own.  Afterwards the pool is, word for word, what dcp_hip_load_hmm of the same files and ranges at
 * (gencode_id, that profile's error rate) leaves, whatever tables the profiles were under; the table that is there
 * already is written all the same.  Offsets and sizes stay, nothing needs committing again, and it is a change of the
 * inputs (below) like dcp_hip_set_epsilon.
 * Failures, in this order, each leaving the pool, the kept distributions and every query as they were: NULL
 * DCP_EFUNCUSE; cost batches outstanding DCP_EFUNCUSE; a table not held DCP_EGENCODEID; a profile without kept
 * distributions DCP_EFUNCUSE, dcp_hip_strerror naming the first; allocations, all made before the first byte of device
 * memory changes, DCP_ENOMEM.  A device error after that is reported, and the tables and kept distributions are then
 * undefined until dcp_hip_clear_profiles.  Without profiles it returns 0 (after the checks above) and does nothing.
 * DECIPHON_HIP_TIMING prints one line "dcp_hip_set_gencode:" with profiles, nodes and the seconds of the host
 * recomputation, of the uploads and of the kernels. */
int dcp_hip_set_gencode(struct dcp_hip *, int gencode_id);
/* the translation table profile `index` is under; 0 for a profile without kept distributions, a bad index or NULL */
int dcp_hip_profile_gencode(struct dcp_hip const *, int index);
/* Bytes of HBM the kept distributions occupy: 528 per node of every profile loaded from a HMMER3 file, and 2 x 528 per
 * dcp_hip_load_hmm that added profiles (its null model and background).  dcp_hip_clear_profiles frees them. */
int64_t dcp_hip_dist_bytes(struct dcp_hip const *);
/* test hooks: floats profile i occupies in the pool (rows | trans | cost-order copy), and a copy of them */
int64_t dcp_hip_profile_floats(struct dcp_hip const *, int i);
int dcp_hip_profile_read(struct dcp_hip const *, int i, float *out, int64_t n);
/* how many staging chunks the last dcp_hip_load_dcp went through (256 MiB each; DECIPHON_HIP_STAGE_MB
 * shrinks them, never below one profile: a hook for tests of the double-buffered path) */
int dcp_hip_load_chunks(struct dcp_hip const *);
/* Bytes of HBM the resident profile tables occupy (rows + transitions, padded). */
int64_t dcp_hip_pool_bytes(struct dcp_hip const *);
int dcp_hip_num_profiles(struct dcp_hip const *);
int dcp_hip_profile_core_size(struct dcp_hip const *, int index);
char const *dcp_hip_profile_accession(struct dcp_hip const *, int index);
/* Uploads everything added so far to HBM (idempotent). */
int dcp_hip_commit_profiles(struct dcp_hip *);
/* Drops every profile.  While cost batches are outstanding it does nothing (the profiles stay, num_profiles
 * included) and leaves the reason in dcp_hip_strerror: the function returns no code. */
void dcp_hip_clear_profiles(struct dcp_hip *);

/* ---- sequences (replaces batch_encode -> sequence_encode, c-core/batch.c:60-70) ----
 * nt holds nucleotide indices A,C,G,T/U = 0..3 of nseq sequences back to back;
 * offsets[nseq+1].  dcp_hip_encode does what dcp_batch_add does to one string
 * (uppercase + disambiguate, c-core/sequence.c:15-45, c-core/disambiguate.c:37-86)
 * and writes n indices. */
int dcp_hip_encode(char const *data, int64_t n, uint8_t *out);
int dcp_hip_set_sequences(struct dcp_hip *, int nseq, uint8_t const *nt, int64_t const *offsets);
/* Not in the reference, which scans a read only as given: the same with both strands of every read.  DCP_STRANDS_PLUS
 * is dcp_hip_set_sequences.  With DCP_STRANDS_BOTH the engine holds 2 * nseq sequences: sequence 2s is read s as given,
 * sequence 2s + 1 its reverse complement rc[i] = 3 - nt[n-1-i].  The reads go up once; the code rows of both strands are
 * written by one kernel from them, and no reverse-complemented copy exists on either side of the bus.  struct
 * dcp_hip_window.seq addresses these internal indices, coordinates of sequence 2s + 1 counting from the 5' end of the
 * reverse complement; every cost and path entry point then works as on 2 * nseq plain reads.  The contract is that of
 * dcp_hip_set_sequences: everything is checked before anything is replaced, DCP_ESEQABC for an index above 3,
 * DCP_EFUNCUSE while batches are outstanding; and DCP_EFUNCUSE for nseq above INT_MAX / 2 or another value of strands. */
#ifndef DCP_STRANDS_PLUS /* (include/deciphon.h has the same two) */
#define DCP_STRANDS_PLUS 0
#define DCP_STRANDS_BOTH 1
#endif
int dcp_hip_set_sequences_strands(struct dcp_hip *, int nseq, uint8_t const *nt, int64_t const *offsets, int strands);
/* The number of internal sequences: nseq of the last dcp_hip_set_sequences, twice that on both strands. */
int dcp_hip_num_sequences(struct dcp_hip const *);
/* test hook, a read-only query like dcp_hip_profile_read: the code rows of internal sequence `seq` as they lie in HBM,
 * out[rows * 8] (struct DcpCodeRow, csrc/dcp_types.h; dcp_code_rows_of, include/deciphon_host.h, states them); rows
 * must be its length + 1. */
int dcp_hip_code_rows_read(struct dcp_hip const *, int seq, uint32_t *out, int64_t rows);

/* Not in the reference: a dcp_hip_set_sequences whose reads exist nowhere -- nseq random sequences of len nucleotides
 * each, whose code rows a kernel writes straight from a counter-based generator (csrc/calibrate.h states it;
 * dcp_random_nt, include/deciphon_host.h, gives the same nucleotides on the host).  freq[4]: the frequencies of A, C, G,
 * T, normalised by their sum; NULL: uniform.  The contract is that of dcp_hip_set_sequences: a change of the inputs,
 * DCP_EFUNCUSE while batches are outstanding, everything checked before anything is replaced -- nseq >= 0, len >= 0, a
 * freq that is not negative, NaN or all zero, nseq * (len + 1) code rows below 2^32, each DCP_EFUNCUSE.  Afterwards
 * dcp_hip_num_sequences, dcp_hip_code_rows_read and every cost and path entry point work as on nseq plain reads. */
int dcp_hip_set_random_sequences(struct dcp_hip *, int nseq, int len, uint64_t seed, float const freq[4]);

/* ---- calibration: what HMMER's p7_Calibrate does for its own scores, for lrt ------------------------------------
 * Sets the random sequences above and scores every committed profile against every whole sequence under the mode and
 * special transitions in force -- windows {p, s, 0, len}, profile-major, through the same stage, plan and launch path
 * as dcp_hip_cost, in chunks of whole profiles of at most DECIPHON_HIP_CALIB_WINDOWS windows (default: the 4 Mi of a
 * scan's chunk; one profile at the least) -- and fits, per profile, the location mu of a Gumbel distribution of
 * lrt = -2 * (null_loglik - alt_loglik) with lambda fixed, by maximum likelihood, on the GPU:
 *   mu = m - (1 / lambda) * log((1 / n') * sum exp(-lambda * (x_i - m))),  m = min x_i,
 * over the n' finite scores (fp64 sum, mu kept as fp32); the others are counted (dcp_hip_profile_calib_excluded), and
 * n' = 0 gives NaN.  lrt is twice the log-odds in nats, so HMMER's conjecture lambda = ln 2 per bit is lambda = 0.5:
 * the value to pass unless a measurement says otherwise.
 * DCP_EFUNCUSE, with nothing changed: batches outstanding, nseq < 1, len < 1, a bad freq, lambda <= 0, infinite or
 * NaN, profiles not committed, no dcp_hip_set_mode yet.  Without profiles it sets the sequences and returns 0.  The
 * random sequences stay resident: the caller sets its reads again.  DECIPHON_HIP_TIMING prints one line
 * "dcp_hip_calibrate:" with profiles, rungs (one), windows, cells and the seconds of generation, cost pass, gather and fit.
 * dcp_hip_profile_mu: NaN for a profile never calibrated, a bad index or NULL.  mu of every profile goes back to NaN on
 * whatever changes a score: dcp_hip_set_epsilon, _set_gencode, _set_mode, _set_xtrans_table, _clear_profiles; profiles
 * added after a calibration have none.  dcp_hip_calib_lambda: the lambda of the calibration in force, NaN without. */
int dcp_hip_calibrate(struct dcp_hip *, int nseq, int len, uint64_t seed, float const freq[4], float lambda);
float dcp_hip_profile_mu(struct dcp_hip const *, int i);
int dcp_hip_profile_calib_excluded(struct dcp_hip const *, int i);
float dcp_hip_calib_lambda(struct dcp_hip const *);

/* ---- calibration over a ladder of read lengths, and lambda fitted ------------------------------------------------
 * mu moves with the length of what is scored, and one scan holds windows of many lengths.  So:
 * the calibration above at every length of lens[nlen], 1 <= nlen <= DCP_CALIB_MAX_LENS, every length >= 1 and larger
 * than the one before.  Rung j scores every profile against exactly the reads of
 *   dcp_hip_set_random_sequences(nseq, lens[j], seed + j (mod 2^64), freq),
 * which dcp_random_nt(seed + j, ...) (include/deciphon_host.h) reproduces on the host -- part of the interface, like the
 * generator -- through the same cost pass in the same chunks; the reads of the last rung stay resident.  A kernel keeps
 * lrt of every profile x rung x read on the device, and one launch fits all profiles, one wavefront each, every sum in
 * fp64 in a fixed order (the same arguments give the same bits):
 *   lambda > 0   that lambda; mu of rung j is the formula above over the rung's finite scores and has the bits
 *                dcp_hip_calibrate(nseq, lens[j], seed + j, freq, lambda) gives -- which is this call with one rung.
 *   lambda == 0  one lambda per profile, common to its rungs, by maximum likelihood with a location per rung: with
 *                y = x - m_j and Tk_j = sum y^k exp(-lambda y) over the n'_j finite scores of rung j, the root of
 *                  g(lambda) = sum_j n'_j (1 / lambda - mean_j(y) + T1_j / T0_j)
 *                over the rungs with n'_j >= 2 and not all scores equal (g falls strictly from +inf to a negative
 *                limit: one root), by Newton's method inside a bracket until |step| <= 1e-13 lambda; then
 *                mu_j = m_j - log(T0_j / n'_j) / lambda for every rung with a finite score.  A profile without a rung
 *                that carries scale gets NaN for lambda and every mu: not calibrated.
 * lambda and mu are kept as fp32; a rung without a finite score has mu NaN; the scores left out are counted per rung.
 * DCP_EFUNCUSE, with nothing changed -- not the sequences, the calibration in force or any query: whatever
 * dcp_hip_calibrate refuses, for any rung; nlen or lens as they must not be; lambda negative, NaN or infinite;
 * lambda == 0 with nseq < 2.  DCP_ENOMEM, with nothing changed, when the scores find no room.  Without profiles it sets
 * the sequences of the last rung and returns 0.  The calibration goes when dcp_hip_calibrate's does.
 * DECIPHON_HIP_TIMING prints one line "dcp_hip_calibrate_lengths:" with profiles, rungs, windows, cells and the seconds
 * of generation, cost pass, gather and fit.
 * dcp_hip_calib_num_lengths: the rungs of the calibration in force, 0 without one (1 after dcp_hip_calibrate);
 * dcp_hip_calib_length: of rung j (0 for a bad j).  dcp_hip_profile_mu_rung, _calib_excluded_rung: profile i at rung j,
 * NaN and 0 for what is not calibrated; dcp_hip_profile_mu and dcp_hip_profile_calib_excluded answer for rung 0.
 * dcp_hip_profile_lambda: the fixed lambda or the profile's fitted one, NaN when it has none; dcp_hip_calib_lambda is
 * the `lambda` argument of the calibration in force: 0 when it was fitted.  dcp_hip_profile_mu_at: mu of profile i at a
 * window of len nucleotides, dcp_calib_mu_at (include/deciphon_host.h) of its rungs. */
#define DCP_CALIB_MAX_LENS 16
int dcp_hip_calibrate_lengths(struct dcp_hip *, int nseq, int nlen, int const *lens, uint64_t seed, float const freq[4],
                              float lambda);
int dcp_hip_calib_num_lengths(struct dcp_hip const *);
int dcp_hip_calib_length(struct dcp_hip const *, int j);
float dcp_hip_profile_mu_rung(struct dcp_hip const *, int i, int j);
int dcp_hip_profile_calib_excluded_rung(struct dcp_hip const *, int i, int j);
float dcp_hip_profile_lambda(struct dcp_hip const *, int i);
double dcp_hip_profile_mu_at(struct dcp_hip const *, int i, int64_t len);

/* ---- special transitions (replaces work_reset -> xtrans_setup, c-core/work.c:47-51) ---- */
int dcp_hip_set_mode(struct dcp_hip *, int multi_hits, int hmmer3_compat);
/* Overrides the special-transition costs for amino lengths 0..rows-1 with the
 * caller's own (what a caller of viterbi_set_extr_trans, c-core/viterbi.c:383-405,
 * may pass): xt[rows][13] in enum extr_trans_id order.  Lengths beyond the table
 * keep following dcp_hip_set_mode. */
int dcp_hip_set_xtrans_table(struct dcp_hip *, int rows, float const *xt);
/* The 13 costs xtrans_setup_viterbi would set for a window whose amino length
 * is seq_size (c-core/xtrans.c:21-68), in enum extr_trans_id order. */
void dcp_hip_xtrans(int seq_size, int multi_hits, int hmmer3_compat, float xt[DCP_HIP_NUM_XTRANS]);

/* ---- the DP ---------------------------------------------------------------------------
 * A window is the half-open range [start, stop) of sequence `seq` scored against
 * `profile`, i.e. one process_window call (c-core/thread.c:98-128).
 *
 * The inputs: every accepted call of dcp_hip_add_profile, _add_protein, _load_dcp, _load_hmm, _set_epsilon and
 * _set_gencode (with profiles resident), _commit_profiles,
 * _clear_profiles, _set_sequences, _set_random_sequences, _calibrate, _calibrate_lengths, _set_mode or _set_xtrans_table changes them, even one that sets what was
 * there already (a call refused for outstanding batches or for its arguments changes nothing).  Two things
 * outlive a call and are tied to the inputs they were made from: the staged window list (dcp_hip_stage) and the
 * trellis of the last dcp_hip_path, which is computed only when asked for.  Once the inputs have changed,
 * dcp_hip_run_staged, dcp_hip_fetch_staged and dcp_hip_path_trellis are DCP_EFUNCUSE until dcp_hip_stage /
 * dcp_hip_path is called again. */
struct dcp_hip_window
{
  int32_t profile;
  int32_t seq;
  int32_t start;
  int32_t stop;
};

/* viterbi_null + viterbi_cost for n windows (c-core/thread.c:114-117):
 * null_cost[i] / alt_cost[i] are the raw return values (the caller negates them
 * into log-likelihoods and forms lrt = -2*(null - alt), c-core/lrt.h:6-9). */
int dcp_hip_cost(struct dcp_hip *, int n, struct dcp_hip_window const *, float *null_cost, float *alt_cost);

/* The same followed by process_window's filter (c-core/thread.c:118-121) on the device: only the windows
 * whose lrt = -2 * (null - alt) (c-core/lrt.h:6-9) is finite and >= 0 come back -- *nhits of them, their indices
 * into the window array in increasing order and their lrt; hit_window and hit_lrt must hold n entries. */
int dcp_hip_cost_hits(struct dcp_hip *, int n, struct dcp_hip_window const *, int *nhits, int32_t *hit_window,
                      float *hit_lrt);
/* The same in two halves: _begin stages the windows and enqueues the kernels and returns while the GPU works;
 * _end waits for the OLDEST batch begun and delivers what dcp_hip_cost_hits would have.  Two batches may be
 * outstanding per engine (the second queues behind the first, so the GPU does not drain between them); a third
 * _begin is a DCP_EFUNCUSE.  While batches are outstanding -- in either buffer set, whichever began first -- the
 * engine accepts only _begin, _end, the read-only queries (dcp_hip_profile_read among them), dcp_hip_path, dcp_hip_path_trellis and
 * dcp_hip_path_reserve (the path pass has buffers and streams of its own); everything else is a DCP_EFUNCUSE, and
 * dcp_hip_clear_profiles does nothing (see there). */
int dcp_hip_cost_hits_begin(struct dcp_hip *, int n, struct dcp_hip_window const *);
int dcp_hip_cost_hits_end(struct dcp_hip *, int *nhits, int32_t *hit_window, float *hit_lrt);

/* viterbi_path + trellis_unzip for n windows (c-core/thread.c:124-126).  The steps and scores
 * (dcp_hip_path_nsteps, _steps, _steps_packed, _score) stay valid until the next dcp_hip_path /
 * dcp_hip_del, whatever is called between: they are host copies.  A dcp_hip_path that fails leaves
 * no results (nsteps -1, trellis DCP_EFUNCUSE).
 * The steps come from a fast pass (cost pass with the DP values kept in HBM + a traceback
 * that picks, at every visited state, the first candidate equal to the stored minimum --
 * the reference's strict-< rule); windows in which that meets an exact fp32 tie only the
 * reference's pass order resolves are redone with the literal pass-by-pass kernel.  The
 * trellis itself is produced (by the literal kernel, for the whole batch) only when
 * dcp_hip_path_trellis is called.  DECIPHON_HIP_PATH=literal forces the literal pass.
 * The fast pass never holds a window's whole DP table: it keeps checkpoints every DECIPHON_HIP_CKPT_ROWS rows (500)
 * and one table of that many rows per block being recomputed, within DECIPHON_HIP_PATH_BUDGET_MB.  A profile beyond
 * 4096 positions keeps the whole table of a window where that fits the budget (its rows are then walked once, not
 * twice) and goes in blocks like the others where it does not.  DECIPHON_HIP_PATH_STRICT=1 makes the budget a hard
 * limit -- DCP_ENOMEM instead of an allocation beyond it -- and, for profiles beyond 4096 positions, keeps an older
 * rule: a window whose WHOLE table exceeds the budget is refused, although its blocks might fit.  The literal pass
 * of such profiles replays the trellis from the DP table with 3 * K floats of scratch per row; it follows the same rule
 * for table + scratch: where the two exceed the budget (and it is not strict) the table comes block by block from the
 * same checkpoints and the scratch shrinks to a block's rows.  Only the trellis itself, (L + 1) * (4 + 2 K) bytes, the
 * output of dcp_hip_path_trellis, is held whole, outside the budget.
 * A window with no finite path at all (viterbi_cost = +inf, which the reference never sends
 * here: c-core/thread.c:118-121) yields 0 steps and score +inf. */
int dcp_hip_path(struct dcp_hip *, int n, struct dcp_hip_window const *);
/* Sets aside `bytes` of HBM for the DP tables of dcp_hip_path now (never shrinks).  VRAM is
 * cleared when allocated, in the background: called early (before the profiles are loaded) the
 * clearing overlaps the load and the cost pass.  Clamped to a quarter of the free device memory.
 * Optional: dcp_hip_path allocates on demand. */
int dcp_hip_path_reserve(struct dcp_hip *, int64_t bytes);
/* how many windows of the last dcp_hip_path needed the literal pass */
int dcp_hip_path_redone(struct dcp_hip const *);
/* The most bytes of DP tables, checkpoints and replay scratch that the last dcp_hip_path -- and the
 * dcp_hip_path_trellis calls that followed it -- had placed in HBM at one time.  Bytes PLACED in the engine's table
 * arena, which is kept and reused from call to call (and set aside by dcp_hip_path_reserve): not bytes allocated. */
int64_t dcp_hip_path_table_bytes(struct dcp_hip const *);
/* How many windows of profiles beyond 4096 positions the last dcp_hip_path took in blocks: those whose whole table
 * exceeded the budget in its fast pass, or, where DECIPHON_HIP_PATH=literal skipped that, those whose table + scratch
 * did in the literal pass.  A dcp_hip_path_trellis afterwards does not change the count (its literal pass adds the
 * scratch to the table, so it may take in blocks a window that the fast pass did not). */
int dcp_hip_path_blocked(struct dcp_hip const *);
/* number of steps of window i's path (S ... T) */
int dcp_hip_path_nsteps(struct dcp_hip const *, int i);
/* state ids (c-core/state.h:9-25, state.c:92-96) and emission lengths of every step */
int dcp_hip_path_steps(struct dcp_hip const *, int i, int32_t *state_ids, int32_t *seqsizes);
/* The same without a copy: *steps points at window i's *nsteps steps as the engine holds them, one word each --
 * state id in the low 16 bits, emission length in the high -- valid until the next dcp_hip_path / dcp_hip_del
 * (what struct imm_step carries apart from the score, c-core/trellis.c:147-167). */
int dcp_hip_path_steps_packed(struct dcp_hip const *, int i, uint32_t const **steps, int32_t *nsteps);
/* the packed back-pointers themselves: xnodes[L+1], nodes[(L+1)*K] (c-core/trellis.h:12-21), L and K of the
 * window and its profile as they were at the dcp_hip_path.  DCP_EFUNCUSE, with the steps left as they are, once
 * the inputs have changed since that dcp_hip_path (see "the inputs" above).  Allowed while cost batches are
 * outstanding; the cost calls and the staged list do not touch it. */
int dcp_hip_path_trellis(struct dcp_hip const *, int i, uint32_t const **xnodes, uint16_t const **nodes);
/* score of the path pass's own DP (equals alt_cost of dcp_hip_cost) */
float dcp_hip_path_score(struct dcp_hip const *, int i);

/* ---- measurement ------------------------------------------------------------------------
 * Stages n windows in HBM once, then times `reps` launches of the cost pass over
 * them with HIP events on the engine's own stream (inputs resident, nothing
 * copied inside the timed region).  *ms receives the mean milliseconds per
 * launch, *cells the DP cells (sum of K*L) one launch computes. */
int dcp_hip_cost_bench(struct dcp_hip *, int n, struct dcp_hip_window const *, int warmup, int reps,
                       float *ms, double *cells, float *null_cost, float *alt_cost);
/* The same in two steps: dcp_hip_stage copies the window list to HBM (untimed);
 * dcp_hip_run_staged launches the cost pass `reps` times over it and returns when the
 * last launch has finished; *ms = HIP-event time of all `reps` launches together,
 * *cells = DP cells of ONE launch.  dcp_hip_fetch_staged copies back the scores of the last
 * dcp_hip_run_staged with reps > 0 (DCP_EFUNCUSE before there is one).  Both may be called any
 * number of times over one staged list.  The list ends with a dcp_hip_stage that fails, and with
 * any dcp_hip_cost, _cost_hits, _cost_hits_begin or _cost_bench that gets past checking its
 * windows (they reuse its buffers); dcp_hip_path and dcp_hip_path_trellis leave it.  After a change
 * of the inputs (see "the inputs" above) both are DCP_EFUNCUSE until the list is staged again. */
int dcp_hip_stage(struct dcp_hip *, int n, struct dcp_hip_window const *);
int dcp_hip_run_staged(struct dcp_hip *, int reps, float *ms, double *cells);
int dcp_hip_fetch_staged(struct dcp_hip *, float *null_cost, float *alt_cost);
/* test hook, a read-only query like dcp_hip_profile_read (allowed while batches are outstanding): the launches of the
 * most recent cost pass of this engine (dcp_hip_cost, dcp_hip_cost_hits[_begin], dcp_hip_cost_bench,
 * dcp_hip_run_staged; with two batches in flight, of the one begun last), in launch order.  Returns their number (0
 * before the first pass, -1 for a null engine, a negative cap or cap > 0 without out) and writes up to cap records of
 * five int32 {kernel, index, first, count, windows_per_profile}, kernel coded as dcp_cost_schedule_of
 * (include/deciphon_host.h) codes it.  What the pass launched, not what a plan says it would: the tests of the cost
 * kernels read from it which kernel gave the scores they compare. */
int dcp_hip_last_cost_launches(struct dcp_hip const *, int cap, int32_t *out);

#ifdef __cplusplus
}
#endif

#endif
