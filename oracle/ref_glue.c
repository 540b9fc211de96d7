/* ref_glue.c -- TEST INFRASTRUCTURE ONLY.
 *
 * Flat-array driver around the REFERENCE's own DP engine.  oracle/Makefile
 * compiles c-core/viterbi.c (+ error.c, loglevel.c) unmodified, straight from
 * /root/reference, and links them with this file into oracle/_ref/libdcp_ref.so.
 * The same library carries, equally unmodified, the other files of the path
 * that need only libc, the reference's own headers and the small imm
 * interfaces of oracle/imm_shim/ -- partition_size.c, state.c (+ bug.c),
 * disambiguate.c, uppercase.c, xtrans.c, trellis.c (+ xrealloc.c), window.c
 * -- whose functions the tests call directly (tests/test_reference_pins.py,
 * tests/test_reference_unzip.py).
 * Nothing of the reference is copied into this repository.
 *
 * trellis.c provides the trellis storage viterbi.c writes and trellis_unzip()
 * (ref_unzip); xtrans.c the special transitions (ref_xtrans); window.c the
 * window walk (ref_windows).  The one restatement left here is window.c's view
 * of a sequence: sequence_size() and sequence_slice() over a plain length.
 */
#include "imm_path.h"
#include "sequence.h"
#include "trellis.h"
#include "viterbi.h"
#include "window.h"
#include "xtrans.h"

#include <limits.h>
#include <math.h>
#include <omp.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

/* ---- what the reference's files need from outside them ------------------- */
/* restated: a sequence is its length here (c-core/sequence.c keeps it in imm_seq) */
int sequence_size(struct sequence const *x) { return x->imm.seq.size; }

struct sequence sequence_slice(struct sequence const *x, struct imm_range r)
{
  struct sequence s = *x;
  s.imm.seq.size = imm_range_size(r);
  return s;
}

/* xtrans_dump()'s printer; nothing the tests run calls it */
void imm_dump_array_f32(size_t size, float const *array, FILE *restrict fp)
{
  for (size_t i = 0; i < size; ++i) fprintf(fp, i ? ",%.9g" : "%.9g", (double)array[i]);
}

/* linked with -Wl,--wrap=viterbi_set_extr_trans: every call from another object
 * file (xtrans_setup_viterbi, ref_set_xtrans) lands here and goes on to
 * viterbi.c's own setter; ref_xtrans() records what xtrans.c hands over */
void __real_viterbi_set_extr_trans(struct viterbi *, enum extr_trans_id, float);
static _Thread_local float *xt_capture;

void __wrap_viterbi_set_extr_trans(struct viterbi *v, enum extr_trans_id id, float scalar)
{
  if (xt_capture && (int)id >= 0 && (int)id < 13) xt_capture[id] = scalar;
  __real_viterbi_set_extr_trans(v, id, scalar);
}

/* ---- flat driver ------------------------------------------------------------ */
struct ref
{
  struct viterbi *v;
  int K;
  /* borrowed parameter arrays of the last ref_setup(), for ref_fresh() */
  float const *trans, *match, *null_cost, *bg_cost;
  float xt[13];
};

struct codes
{
  uint16_t const *m; /* [pos][5], like imm_eseq's code matrix */
};

static int code_fn(int pos, int len, void *arg)
{
  struct codes const *c = arg;
  return c->m[(size_t)pos * 5 + (len - 1)];
}

static uint16_t *make_codes(uint8_t const *seq, int L)
{
  static int const off[6] = {0, 0, 4, 20, 84, 340};
  uint16_t *m = malloc(sizeof(uint16_t) * 5 * ((size_t)L + 1));
  for (int pos = 0; pos < L; ++pos)
    for (int len = 1; len <= 5; ++len)
    {
      int idx = 0;
      if (pos + len <= L)
        for (int i = 0; i < len; ++i) idx = idx * 4 + seq[pos + i];
      m[(size_t)pos * 5 + len - 1] = (uint16_t)(off[len] + idx);
    }
  return m;
}

void *ref_new(void)
{
  struct ref *r = malloc(sizeof(*r));
  r->v = viterbi_new();
  r->K = 0;
  r->trans = r->match = r->null_cost = r->bg_cost = NULL;
  return r;
}

void ref_del(void *p)
{
  struct ref *r = p;
  if (!r) return;
  viterbi_del(r->v);
  free(r);
}

/* trans[8][K] in enum core_trans_id order; costs, exactly what
 * protein_setup_viterbi would pass to the setters */
int ref_setup(void *p, int K, float const *trans, float const *match, float const *null_cost,
              float const *bg_cost)
{
  struct ref *r = p;
  int rc = viterbi_setup(r->v, K);
  if (rc) return rc;
  r->K = K;
  r->trans = trans;
  r->match = match;
  r->null_cost = null_cost;
  r->bg_cost = bg_cost;
  for (int id = 0; id < 8; ++id)
    for (int k = 0; k < K; ++k)
      viterbi_set_core_trans(r->v, (enum core_trans_id)id, trans[id * K + k], k);
  int T = viterbi_table_size();
  for (int c = 0; c < T; ++c)
  {
    viterbi_set_null(r->v, null_cost[c], c);
    viterbi_set_background(r->v, bg_cost[c], c);
    for (int k = 0; k < K; ++k) viterbi_set_match(r->v, match[(size_t)c * K + k], k, c);
  }
  return 0;
}

void ref_set_xtrans(void *p, float const xt[13])
{
  struct ref *r = p;
  memcpy(r->xt, xt, sizeof(r->xt));
  for (int id = 0; id < 13; ++id) viterbi_set_extr_trans(r->v, (enum extr_trans_id)id, xt[id]);
}

/* The reference never clears "row 0" of its DP ring between runs: cost()
 * (viterbi.c:471-473) only sets S and B, so N,J,E,C,T and M,D,I of row 0 still
 * hold the LAST row of whatever ran before on the same struct viterbi.  A run is
 * history-free only right after viterbi_setup() (viterbi.c:336-381 fills
 * everything with +inf).  ref_fresh() re-does setup + setters so the next run
 * starts from that defined state; the arrays given to ref_setup() must still
 * be alive. */
int ref_fresh(void *p)
{
  struct ref *r = p;
  float xt[13];
  memcpy(xt, r->xt, sizeof(xt));
  int rc = ref_setup(p, r->K, r->trans, r->match, r->null_cost, r->bg_cost);
  if (rc) return rc;
  ref_set_xtrans(p, xt);
  return 0;
}

float ref_null(void *p, uint8_t const *seq, int L)
{
  struct ref *r = p;
  uint16_t *m = make_codes(seq, L);
  struct codes c = {m};
  float x = viterbi_null(r->v, L, code_fn, &c);
  free(m);
  return x;
}

float ref_cost(void *p, uint8_t const *seq, int L)
{
  struct ref *r = p;
  uint16_t *m = make_codes(seq, L);
  struct codes c = {m};
  float x = viterbi_cost(r->v, L, code_fn, &c);
  free(m);
  return x;
}

int ref_path(void *p, uint8_t const *seq, int L, uint32_t *xnodes, uint16_t *nodes)
{
  struct ref *r = p;
  uint16_t *m = make_codes(seq, L);
  struct codes c = {m};
  int rc = viterbi_path(r->v, L, code_fn, &c);
  free(m);
  if (rc) return rc;
  struct trellis *t = viterbi_trellis(r->v);
  memcpy(xnodes, t->xnodes, sizeof(uint32_t) * ((size_t)L + 1));
  memcpy(nodes, t->nodes, sizeof(uint16_t) * ((size_t)L + 1) * (size_t)r->K);
  return 0;
}

/* CPU baseline: the reference's per-window work (viterbi_null + viterbi_cost,
 * c-core/thread.c:114-117) for `nprob` windows of one profile, spread over
 * `nthreads` OpenMP threads with one struct viterbi each, like the per-thread
 * works of c-core/scan.c:188-208.  Returns seconds; scores go to out[2*nprob]. */
double ref_bench(int K, float const *trans, float const *match, float const *null_cost,
                 float const *bg_cost, float const *xt /*[nprob][13]*/, uint8_t const *seqs,
                 int64_t const *offsets /*[nprob+1]*/, int nprob, int nthreads, int repeat, float *out)
{
  void **refs = malloc(sizeof(void *) * (size_t)nthreads);
  uint16_t **codes = malloc(sizeof(uint16_t *) * (size_t)nprob);
  for (int i = 0; i < nthreads; ++i)
  {
    refs[i] = ref_new();
    ref_setup(refs[i], K, trans, match, null_cost, bg_cost);
  }
  for (int i = 0; i < nprob; ++i)
    codes[i] = make_codes(seqs + offsets[i], (int)(offsets[i + 1] - offsets[i]));

  struct timespec t0, t1;
  clock_gettime(CLOCK_MONOTONIC, &t0);
#pragma omp parallel for schedule(dynamic, 1) num_threads(nthreads)
  for (int j = 0; j < nprob * repeat; ++j)
  {
    int i = j % nprob;
    struct ref *r = refs[omp_get_thread_num()];
    int L = (int)(offsets[i + 1] - offsets[i]);
    struct codes c = {codes[i]};
    ref_set_xtrans(r, xt + 13 * (size_t)i);
    out[2 * i + 0] = viterbi_null(r->v, L, code_fn, &c);
    out[2 * i + 1] = viterbi_cost(r->v, L, code_fn, &c);
  }
  clock_gettime(CLOCK_MONOTONIC, &t1);

  for (int i = 0; i < nprob; ++i) free(codes[i]);
  for (int i = 0; i < nthreads; ++i) ref_del(refs[i]);
  free(codes);
  free(refs);
  return (double)(t1.tv_sec - t0.tv_sec) + 1e-9 * (double)(t1.tv_nsec - t0.tv_nsec);
}

/* ---- the reference's xtrans.c, trellis.c and window.c ---------------------- */
/* xtrans_init -> xtrans_setup -> xtrans_setup_viterbi (c-core/thread.c:110-113):
 * out[13] = what xtrans.c hands to viterbi_set_extr_trans, by enum extr_trans_id */
int ref_xtrans(int seq_size, int multi_hits, int hmmer3_compat, float *out)
{
  if (seq_size <= 0) return -1; /* xtrans_setup's BUG_ON */
  struct viterbi *v = viterbi_new();
  if (!v) return -1;
  for (int i = 0; i < 13; ++i) out[i] = NAN;
  struct xtrans x;
  xtrans_init(&x);
  xtrans_setup(&x, multi_hits != 0, hmmer3_compat != 0, seq_size);
  xt_capture = out;
  xtrans_setup_viterbi(&x, v);
  xt_capture = NULL;
  viterbi_del(v);
  return 0;
}

/* trellis_unzip() on the trellis the last ref_path() left (L: its length).
 * -> number of steps, -1 when more than `cap` */
int ref_unzip(void *p, int L, int cap, int32_t *state_ids, int32_t *seqsizes)
{
  struct ref *r = p;
  struct imm_step *steps = malloc(sizeof(*steps) * (size_t)(cap > 0 ? cap : 1));
  if (!steps) return -1;
  struct imm_path path = {cap, 0, steps};
  int rc = trellis_unzip(viterbi_trellis(r->v), L, &path);
  int n = rc ? -1 : path.nsteps;
  for (int i = 0; i < n; ++i)
  {
    state_ids[i] = steps[i].state_id;
    seqsizes[i] = steps[i].seqsize;
  }
  free(steps);
  return n;
}

/* window_setup + window_next over a read of seq_size nucleotides; after window
 * i, window_set_last_hit_position(last_hit_pos[i]) unless that is INT_MIN (no
 * hit: the position stays what it was).  ranges[2 i], ranges[2 i + 1] = window
 * i's [start, stop).  -> number of windows; -1 when more than `cap`; -2 when a
 * position breaks the precondition window_next BUG_ONs on (-1 <= pos < size). */
int ref_windows(int seq_size, int core_size, int32_t const *last_hit_pos, int cap, int32_t *ranges)
{
  struct sequence seq;
  memset(&seq, 0, sizeof(seq));
  seq.imm.seq.size = seq_size;
  struct window w = window_setup(&seq, core_size);
  int n = 0;
  while (window_next(&w))
  {
    if (n >= cap) return -1;
    struct imm_range rg = window_range(&w);
    ranges[2 * n] = rg.start;
    ranges[2 * n + 1] = rg.stop;
    int32_t pos = last_hit_pos[n];
    ++n;
    if (pos == INT_MIN) continue;
    if (pos < -1 || pos >= imm_range_size(rg)) return -2;
    window_set_last_hit_position(&w, pos);
  }
  return n;
}
