/* deciphon_host.h -- C ABI of the host-side pieces that sit either side of the
 * GPU path: the pressed-database reader and the scalar bookkeeping of
 * process_window.  None of these touch the GPU; they exist so that a caller of
 * deciphon_hip.h (and the tests) can prepare inputs and interpret outputs
 * exactly as the reference does.  All return 0 or a DCP_E* code
 * (c-core/deciphon.h:34-116) unless stated otherwise.
 */
#ifndef DECIPHON_HOST_H
#define DECIPHON_HOST_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- .dcp reader: database_reader_open (c-core/database_reader.c:26-80),
 * protein_reader offsets (c-core/protein_reader.c:112-128) and protein_unpack
 * (c-core/protein.c:283-351) ---- */
struct dcp_db;
int dcp_db_open(char const *path, struct dcp_db **out);
void dcp_db_close(struct dcp_db *);
int dcp_db_num_proteins(struct dcp_db const *);
float dcp_db_epsilon(struct dcp_db const *);
int dcp_db_entry_dist(struct dcp_db const *);
int dcp_db_has_ga(struct dcp_db const *);
int64_t dcp_db_protein_offset(struct dcp_db const *, int i); /* byte offset in the file */
int dcp_db_protein_core_size(struct dcp_db const *, int i, int *core_size);
/* node_trans[(K+1)*7], node_emission[(K+1)*1364], BMk[K], null[1364], bg[1364],
 * accession[32], consensus[K+1]; any pointer may be NULL to skip it */
int dcp_db_read_protein(struct dcp_db const *, int i, float *node_trans, float *node_emission, float *BMk,
                        float *null_lprob, float *bg_lprob, char *accession, char *consensus);

/* The distributions quasi-codon decoding uses (decoder_setup, c-core/decoder.c:21-36): for entry 0 = null model,
 * 1 = background, 2 + n = node n (n = 0..K): nucltp[(K+3)*4] nucleotide log-probabilities and codonm[(K+3)*125]
 * codon marginals (5 x 5 x 5, index 4 = any nucleotide).  Any pointer may be NULL. */
int dcp_db_read_nuclt_dist(struct dcp_db const *, int i, float *nucltp, float *codonm, int *gencode);
/* decoder_decode (c-core/decoder.c:38-58; arithmetic of third-party imm's imm_frame_cond_decode restated, see
 * csrc/host_logic.h): the codon (nucleotide indices) that most likely produced the n = 1..5 nucleotides nt under
 * error rate epsilon.  Returns 0, or DCP_EDECODON.  dcp_gencode_amino_of: imm_gencode_decode, 0 = unknown table. */
int dcp_decode_quasi_codon(float epsilon, float const *nucltp4, float const *codonm125, uint8_t const *nt, int n,
                           uint8_t codon[3]);
char dcp_gencode_amino_of(int gencode_id, uint8_t const codon[3]);

/* ---- HMMER3 text reader and protein model of press (csrc/hmm_model.h): hmm_reader_next (c-core/hmm_reader.c:19-67),
 * model.c and the node layout of protein_absorb (c-core/protein.c:66-121).  dcp_hmm_open: DCP_EGENCODEID for an
 * unknown NCBI table, DCP_EFOPEN for an unreadable file; dcp_hmm_count: the HMMER3/f lines of the file.
 * dcp_hmm_next reads one profile (0, or DCP_EREADHMMER3, DCP_EENDOFFILE, DCP_EENDOFNODES, DCP_ELARGEMODEL,
 * DCP_ELONGACCESSION, DCP_EZEROMODEL); at the end of the file it returns 0 and dcp_hmm_end becomes 1.
 * dcp_hmm_read of the profile just read: trans[(K+1)*7] (node i: the transitions out of model node min(i + 1, K)),
 * BMk[K], nucltp[(K+3)*4] and codonm[(K+3)*125] (0 = null, 1 = background, 2 + n = node n, n = 0..K, as
 * dcp_db_read_nuclt_dist), accession[32], consensus[K+1]; any pointer may be NULL. ---- */
struct dcp_hmm;
int dcp_hmm_open(char const *path, int gencode_id, struct dcp_hmm **out);
void dcp_hmm_close(struct dcp_hmm *);
long dcp_hmm_count(struct dcp_hmm const *);
int dcp_hmm_next(struct dcp_hmm *);
int dcp_hmm_end(struct dcp_hmm const *);
int dcp_hmm_core_size(struct dcp_hmm const *);
int dcp_hmm_has_ga(struct dcp_hmm const *);
int dcp_hmm_read(struct dcp_hmm const *, float *trans, float *BMk, float *nucltp, float *codonm, char *accession,
                 char *consensus);
/* What of a profile depends on the translation table, and what it is derived from.  dcp_hmm_read_lodds: lodds[K*20] of
 * the profile just read, node n's 20 amino log-odds (match value minus the null model's, model_add_node,
 * c-core/model.c:67-69) -- the same words under whichever table the file was opened.  dcp_regencode_entries: the nucltp
 * and codonm of n nodes under table gencode_id from their lodds[n*20], by the reader's own function on at most
 * max_threads host threads (clamped to 1..16; the result does not depend on it), as the entries a load keeps
 * (csrc/press_kernel.h): entries[n*132], per node nucltp[4], codonm[125] and 3 floats of padding, 0.  DCP_EGENCODEID
 * for a table not held, DCP_EFUNCUSE for n < 0 or NULL with n > 0.  dcp_hmm_models: the null model, then the
 * background, under gencode_id, as entries 0 and 1 of dcp_hmm_read -- nucltp8[2*4], codonm250[2*125], either may be
 * NULL; no file is needed.  DCP_EGENCODEID for a table not held. */
int dcp_hmm_read_lodds(struct dcp_hmm const *, float *lodds);
int dcp_regencode_entries(int gencode_id, int64_t n, float const *lodds, int max_threads, float *entries);
int dcp_hmm_models(int gencode_id, float *nucltp8, float *codonm250);

/* partition_size (c-core/partition_size.c:13-16): proteins of partition idx out of nparts */
long dcp_partition_size(long nelems, long nparts, long idx);
/* core sizes of all proteins (read from the protein heads; nothing else of a protein is touched) */
int dcp_db_core_sizes(struct dcp_db const *, int32_t *core_sizes);
/* first[nparts + 1]: partition p holds proteins first[p] .. first[p+1]-1.  balanced = 0: the rule above, as
 * c-core/protein_reader.c:112-128 applies it.  balanced = 1: contiguous and in order all the same, boundaries
 * where the running sum of core sizes is closest to p/nparts of the total (DP cells go with K). */
int dcp_db_partition_bounds(struct dcp_db const *, int nparts, int balanced, int32_t *first);
/* the same rule on a plain array of n core sizes (core_sizes may be NULL when balanced = 0) */
int dcp_partition_bounds_of(int n, int32_t const *core_sizes, int nparts, int balanced, int32_t *first);

/* Windows of the chain of one (read, profile) pair that never hits: what dcp_window_setup / dcp_window_next
 * walk for a read of seq_size nucleotides and a profile of core_size nodes, counted in O(1) (0 for an empty
 * read or core_size < 1).  Returns the count. */
int64_t dcp_window_count(int64_t seq_size, int core_size);
/* The code rows of one read of n nucleotide indices 0..3, as the engine holds them in HBM (struct DcpCodeRow,
 * csrc/dcp_types.h): rows[(n + 1) * 8].  Row r holds in word t - 1, t = 1..5, the code of the t-mer y[r-t..r-1] --
 * off[t] + its base-4 value, the leftmost symbol the most significant digit, off = {0, 4, 20, 84, 340} -- and 0 where
 * r < t; words 5..7 are 0.  minus = 0: y = nt, what dcp_hip_set_sequences leaves.  minus != 0: y is the reverse
 * complement, y[i] = 3 - nt[n-1-i], what dcp_hip_set_sequences_strands leaves for the minus strand.  This function is
 * the statement (csrc/code_rows.h) the kernels of csrc/code_rows.hip are built from and tested against.
 * 0; DCP_EFUNCUSE for NULL or n < 0; DCP_ESEQABC for an index above 3 (nothing of rows is then defined). */
int dcp_code_rows_of(uint8_t const *nt, int64_t n, int minus, uint32_t *rows);
/* The cost-order copy of the emission rows that the cost kernel of Q positions per lane and W wavefronts reads
 * (csrc/host_logic.h dcp_cost_order_col): cols[k] receives the column of position k, k < 64*Q*W, counted from the
 * first column (behind the row's 32-float header), and the function returns the floats of one copy row (0 and
 * nothing written for Q < 1, W < 1 or Q*W > 64). */
int dcp_cost_order_map(int Q, int W, int32_t *cols);
/* The workgroups of dcp_hip_set_epsilon's kernel (csrc/press_reemit.h): one (profile, k0) pair per 64 positions of
 * every profile, k0 = 0, 64, ... below its padded length Kp[i] (a multiple of 64), profiles in order and k0 ascending
 * within each.  Returns the number of pairs, the sum of Kp[i] / 64, whatever `cap` is; the first min(count, cap) of them
 * are written to profile[] and k0[] and nothing beyond (cap = 0: the arrays may be NULL). */
int64_t dcp_reemit_tiles(int n, int32_t const *Kp, int32_t *profile, int32_t *k0, int64_t cap);
/* Which columns of an emission row the lanes of a cost kernel read for a profile of K positions (csrc/dcp_types.h
 * dcp_row_read_offset: a lane with no position below K reads with the last lane that has one).  layout 0: one
 * wavefront of 64 lanes x Q positions on the canonical rows; 1: the same on the cost-order copy; 2: one group of S
 * lanes x Q positions of a packed kernel, lane 0 its separator.  offsets[e * chunks + c] receives the byte offset
 * inside a row of chunk c of lane e -- chunks = (Q + 3) / 4 chunks of up to four floats for layouts 0 and 1, one
 * chunk of Q floats for layout 2 -- for the 64 (layout 2: S) lanes.  Returns the lanes that own at least one
 * position below K (layout 2: the separator not counted), or 0 with nothing written for a shape no kernel has
 * (Q < 1, Q > 16, K < 1, K beyond the shape's positions, S not 4, 8, 16 or 32). */
int dcp_row_lane_offsets(int layout, int Q, int S, int K, uint32_t *offsets);
/* Which windows of a cost launch share an XCD's L2 (csrc/dcp_types.h).  dcp_xcd_eighths_entry_of: the entry of a list
 * of n that workgroup b takes when XCD x = b % 8 is given the x-th contiguous eighth of the list (-1 unless
 * 0 <= b < n).  dcp_xcd_placement_of: the rule itself, 1 = eighths, 0 = the plain order, for a launch of `workgroups`
 * windows in profile order, windows_per_profile of them per profile, table_bytes of emission rows per profile, on a
 * kernel of which one XCD holds resident_per_xcd workgroups. */
int dcp_xcd_eighths_entry_of(int b, int n);
int dcp_xcd_placement_of(int workgroups, int windows_per_profile, int64_t table_bytes, int resident_per_xcd);
/* The memory plan of the path pass (csrc/path_plan.h dcp_plan_path: the rules), for n windows of L[i] rows of profiles
 * of K[i] positions, padded to Kp[i], on W[i] wavefronts, strip[i] != 0 for the strip class (K > 4096).  kind 0: the
 * fast pass over every window of a request; 1: the literal pass over its strip windows (strip[] is not read).  B: rows
 * between checkpoints (a multiple of 5; 0 = none); budget: bytes the table arena may hold; strict != 0: the budget is
 * a hard limit; largest_chunk: the largest chunk the arena holds already (0: none); group_override > 0: blocks side by
 * side whatever the budget says.  Per window: in_blocks (0 = the whole table), its blocks, the rows of replay scratch
 * (kind 1), the bytes from the start of its placement to its checkpoints (0: none) and to its scratch (kind 1), and the
 * bytes of the placement.  *G: blocks of a window side by side; *blocked: strip windows in blocks.  Returns 0, or
 * DCP_EFUNCUSE with nothing written. */
int dcp_path_plan_of(int kind, int n, int32_t const *L, int32_t const *K, int32_t const *Kp, int32_t const *W,
                     uint8_t const *strip, int B, int64_t budget, int strict, int64_t largest_chunk, int group_override,
                     int32_t *in_blocks, int32_t *blocks, int32_t *replay_rows, int64_t *ckpt_off, int64_t *scratch_off,
                     int64_t *bytes, int *G, int *blocked);
/* The plan of a window list (csrc/stage_plan.h plan_stage: the rules) -- what the engine stages for a cost or a path
 * pass, without an engine.  windows[n]; profiles[nprof][5] = {K, Kp, class, narrow, pack shape or -1} per profile;
 * seq_off, row_off[nseq + 1]: the nucleotides and the code rows in front of each read, and in all; arena_kind 0 = none,
 * 1 = trellises, 2 = DP tables at table_addr[n]; pack, pack_lds: what DECIPHON_HIP_PACK and _PACK_LDS say;
 * shapes[DCP_NUM_PACK_SHAPES = 11][2] = {windows of a pack, wavefronts of an LDS workgroup or 0}.
 * sizes[3]: on entry the elements that problems, packs and groups hold (not read for a NULL one), on return the
 * elements of the plan.  problems: struct DcpProblem (csrc/dcp_types.h, 32 bytes), packs: struct DcpPack (264 bytes),
 * groups: {first pack, count} pairs; c_begin[13], c_wide[12], c_profiles[12][2], pk_begin[12], pg_begin[12]: whose
 * share of those lists is whose (csrc/stage_plan.h StagedPlan); *cells = sum of K L, *arena_bytes, *max_xt_row.  Any
 * output may be NULL.  Returns 0; the engine's refusal (DCP_EFUNCUSE, DCP_EZEROSEQ, DCP_ELARGECORESIZE) with its
 * message in *what and nothing else written; DCP_EFUNCUSE with *what = "" for arguments no engine would pass (a pack
 * shape outside -1..10, a shape of more than 16 windows, ...); DCP_ENOMEM, with sizes set, when an array is too small. */
struct dcp_hip_window;
int dcp_stage_plan_of(int n, struct dcp_hip_window const *windows, int nprof, int32_t const *profiles, int nseq,
                      int64_t const *seq_off, int64_t const *row_off, int arena_kind, int64_t const *table_addr, int pack,
                      int pack_lds, int32_t const *shapes, int64_t sizes[3], void *problems, void *packs, int32_t *groups,
                      int32_t *c_begin, int32_t *c_wide, int32_t *c_profiles, int32_t *pk_begin, int32_t *pg_begin,
                      double *cells, int64_t *arena_bytes, int32_t *max_xt_row, char const **what);
/* The launches of a cost pass over a list with those shares (csrc/stage_plan.h cost_schedule), narrow: what
 * DECIPHON_HIP_NARROW says.  Returns their number; when it is at most cap, rows[..][6] = {kernel (0 none, 1 class,
 * 2 narrow, 3 fused, 4 packs, 5 packs with LDS tables), class or shape, first element, count, windows per profile,
 * branch (0 class, 1 narrow, 2 pack)} in launch order.  The pass forks when there is more than one.  -1: a NULL array. */
int dcp_cost_schedule_of(int32_t const *c_begin, int32_t const *c_wide, int32_t const *c_profiles, int32_t const *pk_begin,
                         int32_t const *pg_begin, int narrow, int cap, int32_t *rows);
/* Where the literal path pass puts the trellises of n windows of L[i] rows and K[i] positions (csrc/stage_plan.h
 * trellis_offsets): offsets[n] (may be NULL); returns the bytes of the arena, -1 for L < 0 or K < 1. */
int64_t dcp_trellis_arena_of(int n, int32_t const *L, int32_t const *K, int64_t *offsets);
/* What the engine decides for a profile of K positions, without a device: out[4] = {class, narrow, pack shape or -1,
 * Kp}; DCP_ELARGECORESIZE for a core size no class holds.  And for pack shape 0..10: out[2] = {windows of a pack,
 * wavefronts of an LDS workgroup or 0}; DCP_EFUNCUSE otherwise.  (The kernels' own tables, csrc/viterbi_kernels.h.) */
int dcp_engine_core_size(int K, int32_t out[4]);
int dcp_engine_pack_shape(int shape, int32_t out[2]);
/* How dcp_scan_run cuts profiles x reads into cost batches (csrc/host_logic.h dcp_plan_chunks: the rules).
 * dcp_scan_run plans with first_cells = DCP_SCAN_FIRST_CHUNK_CELLS, later_cells = unlimited (both
 * DECIPHON_HIP_CHUNK_CELLS when that is set), max_pairs = DCP_SCAN_CHUNK_PAIRS and max_windows =
 * DCP_SCAN_CHUNK_WINDOWS (or DECIPHON_HIP_CHUNK_WINDOWS).
 * Chunk i covers profiles [chunks[4i], chunks[4i+1]) x reads [chunks[4i+2], chunks[4i+3]) and holds windows[i]
 * windows.  *nchunks receives the number of chunks; with more than cap of them nothing is written and
 * DCP_ENOMEM is returned.  first_cells / later_cells: the DP-cell limits of the first / every later chunk;
 * max_pairs, max_windows >= 1. */
int dcp_scan_plan_chunks(int nprof, int32_t const *core_sizes, int nreads, int32_t const *read_lengths,
                         double first_cells, double later_cells, int64_t max_pairs, int64_t max_windows, int cap,
                         int32_t *chunks, int64_t *windows, int *nchunks);
#define DCP_SCAN_FIRST_CHUNK_CELLS 1.0e10
#define DCP_SCAN_CHUNK_PAIRS (1 << 21)
#define DCP_SCAN_CHUNK_WINDOWS (4 << 20)

/* ---- the window walk of dcp_scan_run (csrc/scan_walk.h: the rules), for tests: which windows of which (profile,
 * read) pairs a scan scores, keeps or scores again, given the verdicts of the cost and path passes.  Windows are
 * struct dcp_hip_window (include/deciphon_hip.h: int32 profile, seq, start, stop).  A chunk is {p0, p1, s0, s1} and
 * its window count, as dcp_scan_plan_chunks gives them.  Lists that a call returns belong to the walk and stand until
 * its next call of the same name. ---- */
struct dcp_scan_walk;
struct dcp_hip_window;
struct dcp_walk_hit /* a hit as dcp_scan_walk_path_walked reports it */
{
  int32_t batch_index; /* its window's index in the path batch */
  int32_t profile, seq, window, start, stop;
  float lrt;
};
struct dcp_scan_walk *dcp_scan_walk_new(int nprof, int32_t const *core_sizes, int nreads, int32_t const *read_lengths);
void dcp_scan_walk_del(struct dcp_scan_walk *);
/* wins[windows] and base[pairs + 1] (the first window of each pair, and the total) are filled; DCP_EFUNCUSE when the
 * chains do not make `windows` windows */
int dcp_scan_walk_chunk_windows(struct dcp_scan_walk *, int32_t const chunk[4], int64_t windows,
                                struct dcp_hip_window *wins, int64_t *base);
/* the nh windows of the chunk that passed the filter, ascending, and their lrt */
int dcp_scan_walk_chunk_scored(struct dcp_scan_walk *, int32_t const chunk[4], int64_t const *base, int nh,
                               int32_t const *hit_index, float const *lrts);
int dcp_scan_walk_all_pairs(struct dcp_scan_walk *); /* nothing speculated */
/* windows waiting for a cost round (which = 0) or a path pass (1); take: they become the batch, *wins its windows */
int64_t dcp_scan_walk_waiting(struct dcp_scan_walk const *, int which);
int64_t dcp_scan_walk_take(struct dcp_scan_walk *, int which, struct dcp_hip_window const **wins);
int dcp_scan_walk_cost_scored(struct dcp_scan_walk *, int nh, int32_t const *hit_index, float const *lrts);
/* is_hit[n], last_hit_pos[n] per window of the path batch; returns the number of hits, *hits as they stand before
 * their pairs move on */
int64_t dcp_scan_walk_path_walked(struct dcp_scan_walk *, uint8_t const *is_hit, int32_t const *last_hit_pos,
                                  struct dcp_walk_hit const **hits);
int64_t dcp_scan_walk_windows(struct dcp_scan_walk const *);  /* walked so far */
int64_t dcp_scan_walk_take_queued(struct dcp_scan_walk *);    /* queued for a cost round since the last call */

/* ---- the product rows of a scan in bounded memory (csrc/product_runs.h: the rules), for tests.  Rows are handed over
 * in any order and come out sorted by (profile, seq, window), equal keys in the order they were added; once more than
 * budget_bytes of text are held they go to sorted run files `<dir>/.products.NNN.run`, which close merges into `file`
 * behind the header line of products.tsv and removes.  add: n rows, text[i] NUL-terminated and without newline; 0,
 * DCP_EOPENTMP, DCP_EWRITEPROD -- the first error sticks.  close: 0, that error, DCP_EFOPEN or DCP_EWRITEPROD.
 * row: row i of the closed file without its newline, NULL out of range; once runs were written the pointer stands
 * until the next row.  stats: rows, runs written, most text bytes held, bytes of `file`; returns 4.  del removes any
 * run file still there. ---- */
struct dcp_product_runs;
struct dcp_product_runs *dcp_product_runs_new(char const *dir, int64_t budget_bytes);
int dcp_product_runs_add(struct dcp_product_runs *, int n, int32_t const *profile, int32_t const *seq,
                         int32_t const *window, char const *const *text);
int dcp_product_runs_close(struct dcp_product_runs *, char const *file);
long dcp_product_runs_num_rows(struct dcp_product_runs const *);
char const *dcp_product_runs_row(struct dcp_product_runs *, long i);
int dcp_product_runs_stats(struct dcp_product_runs const *, int64_t out[4]);
void dcp_product_runs_del(struct dcp_product_runs *);

/* ---- window iteration: window_setup / window_next / window_set_last_hit_position
 * (c-core/window.c:7-50) ---- */
struct dcp_window
{
  int32_t core_size, seq_size;
  int32_t start, stop, idx, last_hit_pos;
};
void dcp_window_setup(struct dcp_window *, int seq_size, int core_size);
int dcp_window_next(struct dcp_window *); /* 1 = a window was produced, 0 = end */

/* ---- trellis_unzip (c-core/trellis.c:147-167): steps of the traceback in path
 * order.  *nsteps receives the count; fails with DCP_ENOMEM when cap is too small. */
int dcp_trellis_unzip(int K, int L, uint32_t const *xnodes, uint16_t const *nodes, int cap, int32_t *state_ids,
                      int32_t *seqsizes, int *nsteps);

/* ---- the hit of a window (c-core/thread.c:130-166): from the first B to the last
 * E of the path.  Returns 1 and fills hit[5] = {hit_start, hit_stop, begin_step,
 * end_step, last_hit_pos}, or 0 when the path has no B. */
int dcp_path_hit(int nsteps, int32_t const *state_ids, int32_t const *seqsizes, int32_t hit[5]);

/* state_name (c-core/state.c:46-90); name must hold 8 bytes */
void dcp_state_name_of(int state_id, char *name);
int dcp_state_is_mute_id(int state_id);

/* lrt (c-core/lrt.h:6-9) */
float dcp_lrt_of(float null_loglik, float alt_loglik);

/* ---- the random reads of dcp_hip_set_random_sequences / dcp_hip_calibrate (csrc/calibrate.h is the one statement, for
 * the host and the kernel).  Nucleotide i of sequence s of a set of sequences of len nucleotides has the 64-bit index
 * idx = s * len + i, and
 *   z = seed + (idx + 1) * 0x9E3779B97F4A7C15 (mod 2^64);  z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9;
 *   z = (z ^ z >> 27) * 0x94D049BB133111EB;  u = (z ^ z >> 31) >> 32;  base = (u >= t[0]) + (u >= t[1]) + (u >= t[2])
 * -- splitmix64 addressed by position.  A seed gives the same reads in every later version.
 * dcp_random_thresholds: t[j] = min(floor(cum_j * 2^32), 2^32 - 1) from the four frequencies (NULL: uniform),
 * normalised by their sum, in double.  A frequency of 0 leaves its base no value of u (base 3 behind the clamp: the one
 * value u = 2^32 - 1).  DCP_EFUNCUSE for a negative, NaN, infinite or all-zero freq, or NULL t.
 * dcp_random_nt: out[i] = the base at index first_idx + i, i < n.  DCP_EFUNCUSE for NULL, first_idx < 0 or n < 0. */
int dcp_random_thresholds(float const freq[4], uint32_t t[3]);
int dcp_random_nt(uint64_t seed, uint32_t const t[3], int64_t first_idx, int64_t n, uint8_t *out);
/* The E-value of a row: the tail of the Gumbel distribution (mu, lambda) a calibration fitted to its profile
 * (dcp_hip_calibrate, include/deciphon_hip.h), times z targets:
 *   z * (-expm1(-exp(-(double)lambda * ((double)lrt - mu))))
 * -- the one place the tail is stated.  NaN when mu is NaN. */
double dcp_lrt_evalue(float lrt, float mu, float lambda, double z);
/* mu of a profile at a window of len nucleotides, from the nlen rungs (lens[j], mu[j]) of a calibration over a ladder of
 * read lengths (dcp_hip_calibrate_lengths, include/deciphon_hip.h) -- the one statement of the rule; dcp_hip_profile_mu_at
 * and the scan call it.  Piecewise linear in ln len through the points (ln lens[j], mu[j]) of the rungs whose mu is not
 * NaN: between the usable rungs a < b around len
 *   mu[a] + (mu[b] - mu[a]) * (log(len / lens[a]) / log(lens[b] / lens[a]))      in double,
 * and beyond either end the line of the end segment goes on (in theory mu is linear in ln L; clamping would freeze the
 * error a ladder is there to remove).  At len == lens[j] of a usable rung exactly (double)mu[j].  One usable rung: that
 * mu, a constant.  None: NaN.  NaN as well for nlen < 1, NULL, len < 1, a length below 1 or lens that do not increase. */
double dcp_calib_mu_at(int nlen, int const *lens, float const *mu, int64_t len);

#ifdef __cplusplus
}
#endif

#endif
