// host_capi.cpp -- C ABI of include/deciphon_host.h over dcp_db / host_logic / scan_walk / path_plan / stage_plan.
#include "../../include/deciphon_host.h"
#include "calibrate.h"
#include "dcp_db.h"
#include "dcp_errors.h"
#include "dcp_types.h"
#include "host_logic.h"
#include "path_plan.h"
#include "scan_walk.h"
#include "stage_plan.h"

#include <math.h>
#include <string.h>
#include <string>
#include <vector>

struct dcp_db
{
  DcpDbReader reader;
};

struct dcp_scan_walk
{
  DcpScanWalk walk;
};

extern "C" {

int dcp_db_open(char const *path, struct dcp_db **out)
{
  if (!path || !out) return DCP_EFUNCUSE;
  dcp_db *x = new dcp_db;
  int rc = x->reader.open(path);
  if (rc)
  {
    delete x;
    *out = nullptr;
    return rc;
  }
  *out = x;
  return 0;
}

void dcp_db_close(struct dcp_db *x) { delete x; }
int dcp_db_num_proteins(struct dcp_db const *x) { return x ? x->reader.num_proteins() : 0; }
float dcp_db_epsilon(struct dcp_db const *x) { return x ? x->reader.header().epsilon : 0.0f; }
int dcp_db_entry_dist(struct dcp_db const *x) { return x ? x->reader.header().entry_dist : 0; }
int dcp_db_has_ga(struct dcp_db const *x) { return x ? (int)x->reader.header().has_ga : 0; }

int64_t dcp_db_protein_offset(struct dcp_db const *x, int i)
{
  if (!x || i < 0 || i > x->reader.num_proteins()) return -1;
  return x->reader.protein_offset(i);
}

int dcp_db_protein_core_size(struct dcp_db const *x, int i, int *core_size)
{
  if (!x || !core_size) return DCP_EFUNCUSE;
  std::string acc;
  return x->reader.read_protein_head(i, *core_size, acc);
}

int dcp_db_core_sizes(struct dcp_db const *x, int32_t *core_sizes)
{
  if (!x || !core_sizes) return DCP_EFUNCUSE;
  std::string acc;
  for (int i = 0; i < x->reader.num_proteins(); ++i)
  {
    int K = 0;
    int rc = x->reader.read_protein_head(i, K, acc);
    if (rc) return rc;
    core_sizes[i] = K;
  }
  return 0;
}

int dcp_db_partition_bounds(struct dcp_db const *x, int nparts, int balanced, int32_t *first)
{
  if (!x || !first) return DCP_EFUNCUSE;
  if (nparts < 1) return DCP_EZEROPART;
  int const n = x->reader.num_proteins();
  std::vector<int32_t> K;
  if (balanced)
  {
    K.resize((size_t)n);
    int rc = dcp_db_core_sizes(x, K.data());
    if (rc) return rc;
  }
  dcp_partition_bounds(n, balanced ? K.data() : nullptr, nparts, balanced != 0, first);
  return 0;
}

int dcp_db_read_nuclt_dist(struct dcp_db const *x, int i, float *nucltp, float *codonm, int *gencode)
{
  if (!x) return DCP_EFUNCUSE;
  DcpDecoder d;
  int rc = x->reader.read_decoder(i, d);
  if (rc) return rc;
  if (nucltp) memcpy(nucltp, d.nucltp.data(), d.nucltp.size() * sizeof(float));
  if (codonm) memcpy(codonm, d.codonm.data(), d.codonm.size() * sizeof(float));
  if (gencode) *gencode = d.gencode;
  return 0;
}

int dcp_decode_quasi_codon(float epsilon, float const *nucltp4, float const *codonm125, uint8_t const *nt, int n,
                           uint8_t codon[3])
{
  if (!nucltp4 || !codonm125 || !nt || !codon) return DCP_EFUNCUSE;
  for (int i = 0; i < n && i < 5; ++i)
    if (nt[i] > 3) return DCP_ESEQABC;
  return dcp_decode_codon(epsilon, nucltp4, codonm125, nt, n, codon) ? 0 : DCP_EDECODON;
}

char dcp_gencode_amino_of(int gencode_id, uint8_t const codon[3]) { return dcp_gencode_amino(gencode_id, codon); }

int dcp_cost_order_map(int Q, int W, int32_t *cols)
{
  if (Q < 1 || W < 1 || Q * W > 64 || !cols) return 0;
  for (int k = 0; k < 64 * Q * W; ++k) cols[k] = dcp_cost_order_col(Q, W, k);
  return dcp_cost_order_stride(Q, W);
}

int dcp_row_lane_offsets(int layout, int Q, int S, int K, uint32_t *offsets)
{
  bool const pack = layout == DCP_ROW_PACK;
  if (layout < DCP_ROW_CANON || layout > DCP_ROW_PACK || Q < 1 || Q > 16 || K < 1 || !offsets) return 0;
  if (pack && S != 4 && S != 8 && S != 16 && S != 32) return 0;
  int const lanes = pack ? S : 64, chunks = pack ? 1 : (Q + 3) / 4;
  if (K > (pack ? S - 1 : 64) * Q) return 0;
  for (int e = 0; e < lanes; ++e)
    for (int c = 0; c < chunks; ++c) offsets[e * chunks + c] = dcp_row_read_offset(layout, Q, S, K, (uint32_t)e, c);
  return dcp_row_read_lanes(layout, Q, S, K);
}

int64_t dcp_reemit_tiles(int n, int32_t const *Kp, int32_t *profile, int32_t *k0, int64_t cap)
{
  int64_t count = 0;
  for (int i = 0; i < n; ++i)
    for (int32_t k = 0; k < Kp[i]; k += 64, ++count)
      if (count < cap)
      {
        profile[count] = i;
        k0[count] = k;
      }
  return count;
}

int dcp_xcd_eighths_entry_of(int b, int n) { return b < 0 || b >= n ? -1 : dcp_xcd_eighths_entry(b, n); }

int dcp_xcd_placement_of(int workgroups, int windows_per_profile, int64_t table_bytes, int resident_per_xcd)
{
  return dcp_xcd_placement(workgroups, windows_per_profile, (long long)table_bytes, resident_per_xcd);
}

int dcp_path_plan_of(int kind, int n, int32_t const *L, int32_t const *K, int32_t const *Kp, int32_t const *W,
                     uint8_t const *strip, int B, int64_t budget, int strict, int64_t largest_chunk, int group_override,
                     int32_t *in_blocks, int32_t *blocks, int32_t *replay_rows, int64_t *ckpt_off, int64_t *scratch_off,
                     int64_t *bytes, int *G, int *blocked)
{
  if ((kind != DCP_PATH_FAST && kind != DCP_PATH_LITERAL) || n < 0 || B < 0 || budget < 0 || largest_chunk < 0 || !G || !blocked)
    return DCP_EFUNCUSE;
  if (n > 0 && (!L || !K || !Kp || !W || !strip || !in_blocks || !blocks || !replay_rows || !ckpt_off || !scratch_off || !bytes))
    return DCP_EFUNCUSE;
  std::vector<DcpPathWindow> w;
  for (int i = 0; i < n; ++i) w.push_back(DcpPathWindow{L[i], K[i], Kp[i], W[i], strip[i] != 0});
  DcpPathPlan const plan = dcp_plan_path((DcpPathKind)kind, n, w.data(), B, (size_t)budget, strict != 0, (size_t)largest_chunk,
                                         group_override);
  for (int i = 0; i < n; ++i)
  {
    DcpPathPlace const &p = plan.place[(size_t)i];
    in_blocks[i] = p.in_blocks;
    blocks[i] = p.blocks;
    replay_rows[i] = p.replay_rows;
    ckpt_off[i] = (int64_t)p.ckpt_off;
    scratch_off[i] = (int64_t)p.scratch_off;
    bytes[i] = (int64_t)p.bytes;
  }
  *G = plan.G;
  *blocked = plan.blocked;
  return 0;
}

int dcp_stage_plan_of(int n, struct dcp_hip_window const *windows, int nprof, int32_t const *profiles, int nseq,
                      int64_t const *seq_off, int64_t const *row_off, int arena_kind, int64_t const *table_addr, int pack,
                      int pack_lds, int32_t const *shapes, int64_t sizes[3], void *problems, void *packs, int32_t *groups,
                      int32_t *c_begin, int32_t *c_wide, int32_t *c_profiles, int32_t *pk_begin, int32_t *pg_begin,
                      double *cells, int64_t *arena_bytes, int32_t *max_xt_row, char const **what)
{
  using namespace dcp_engine;
  if (what) *what = "";
  if (n < 0 || nprof < 0 || nseq < 0 || (n && !windows) || (nprof && !profiles) || !seq_off || !row_off || !shapes || !sizes)
    return DCP_EFUNCUSE;
  if (arena_kind < ARENA_NONE || arena_kind > ARENA_TABLE || (arena_kind == ARENA_TABLE && n && !table_addr)) return DCP_EFUNCUSE;
  std::vector<StageProfile> prof((size_t)nprof);
  for (int i = 0; i < nprof; ++i)
  {
    int32_t const *p = profiles + 5 * (size_t)i;
    if (p[4] < -1 || p[4] >= DCP_NUM_PACK_SHAPES) return DCP_EFUNCUSE;
    prof[(size_t)i].K = p[0], prof[(size_t)i].Kp = p[1], prof[(size_t)i].cls = p[2], prof[(size_t)i].narrow = p[3] != 0, prof[(size_t)i].pack = p[4];
  }
  StageShape sh[DCP_NUM_PACK_SHAPES];
  for (int s = 0; s < DCP_NUM_PACK_SHAPES; ++s)
  {
    sh[s] = StageShape{shapes[2 * s], shapes[2 * s + 1]};
    if (sh[s].windows < 1 || sh[s].windows > 16 || sh[s].lds_waves < 0) return DCP_EFUNCUSE; // DcpPack holds 16 windows
  }
  StageInput const in{n,  windows, prof.data(), nprof, nseq, seq_off, row_off, (ArenaKind)arena_kind,
                      table_addr, pack != 0, pack_lds != 0, sh};
  Staged st;
  Refusal const refused = plan_stage(in, st);
  if (refused.code)
  {
    if (what) *what = refused.what;
    return refused.code;
  }
  int64_t const counts[3] = {(int64_t)st.problems.size(), (int64_t)st.packs.size(), (int64_t)st.pack_groups.size()};
  bool const fits = (!problems || sizes[0] >= counts[0]) && (!packs || sizes[1] >= counts[1]) && (!groups || sizes[2] >= counts[2]);
  memcpy(sizes, counts, sizeof counts);
  if (!fits) return DCP_ENOMEM;
  if (problems && counts[0]) memcpy(problems, st.problems.data(), st.problems.size() * sizeof(DcpProblem));
  if (packs && counts[1]) memcpy(packs, st.packs.data(), st.packs.size() * sizeof(DcpPack));
  if (groups && counts[2]) memcpy(groups, st.pack_groups.data(), st.pack_groups.size() * sizeof(PackGroup));
  if (c_begin) memcpy(c_begin, st.c_begin, sizeof st.c_begin);
  if (c_wide) memcpy(c_wide, st.c_wide, sizeof st.c_wide);
  if (c_profiles) memcpy(c_profiles, st.c_profiles, sizeof st.c_profiles);
  if (pk_begin) memcpy(pk_begin, st.pk_begin, sizeof st.pk_begin);
  if (pg_begin) memcpy(pg_begin, st.pg_begin, sizeof st.pg_begin);
  if (cells) *cells = st.cells;
  if (arena_bytes) *arena_bytes = (int64_t)st.arena_bytes;
  if (max_xt_row) *max_xt_row = st.max_xt_row;
  return 0;
}

int dcp_cost_schedule_of(int32_t const *c_begin, int32_t const *c_wide, int32_t const *c_profiles, int32_t const *pk_begin,
                         int32_t const *pg_begin, int narrow, int cap, int32_t *rows)
{
  using namespace dcp_engine;
  if (!c_begin || !c_wide || !c_profiles || !pk_begin || !pg_begin || cap < 0 || (cap && !rows)) return -1;
  StagedPlan st;
  memcpy(st.c_begin, c_begin, sizeof st.c_begin);
  memcpy(st.c_wide, c_wide, sizeof st.c_wide);
  memcpy(st.c_profiles, c_profiles, sizeof st.c_profiles);
  memcpy(st.pk_begin, pk_begin, sizeof st.pk_begin);
  memcpy(st.pg_begin, pg_begin, sizeof st.pg_begin);
  std::vector<CostLaunch> const s = cost_schedule(st, narrow != 0);
  static_assert(sizeof(CostLaunch) == 6 * sizeof(int32_t), "a launch goes out as a row of six int32");
  if (!s.empty() && (int)s.size() <= cap) memcpy(rows, s.data(), s.size() * sizeof(CostLaunch));
  return (int)s.size();
}

int64_t dcp_trellis_arena_of(int n, int32_t const *L, int32_t const *K, int64_t *offsets)
{
  using namespace dcp_engine;
  if (n < 0 || (n && (!L || !K))) return -1;
  std::vector<dcp_hip_window> w((size_t)n);
  std::vector<StageProfile> prof((size_t)n);
  for (int i = 0; i < n; ++i)
  {
    if (L[i] < 0 || K[i] < 1) return -1;
    w[(size_t)i].profile = i, w[(size_t)i].seq = 0, w[(size_t)i].start = 0, w[(size_t)i].stop = L[i];
    prof[(size_t)i].K = K[i];
  }
  std::vector<size_t> const off = trellis_offsets(n, w.data(), prof.data());
  for (int i = 0; offsets && i < n; ++i) offsets[i] = (int64_t)off[(size_t)i];
  return (int64_t)off[(size_t)n];
}

int dcp_partition_bounds_of(int n, int32_t const *core_sizes, int nparts, int balanced, int32_t *first)
{
  if (n < 0 || !first || (balanced && n > 0 && !core_sizes)) return DCP_EFUNCUSE;
  if (nparts < 1) return DCP_EZEROPART;
  dcp_partition_bounds(n, core_sizes, nparts, balanced != 0, first);
  return 0;
}

int dcp_db_read_protein(struct dcp_db const *x, int i, float *node_trans, float *node_emission, float *BMk,
                        float *null_lprob, float *bg_lprob, char *accession, char *consensus)
{
  if (!x) return DCP_EFUNCUSE;
  DcpProtein p;
  int rc = x->reader.read_protein(i, p);
  if (rc) return rc;
  if (node_trans) memcpy(node_trans, p.trans.data(), p.trans.size() * sizeof(float));
  if (node_emission) memcpy(node_emission, p.emission.data(), p.emission.size() * sizeof(float));
  if (BMk) memcpy(BMk, p.BMk.data(), p.BMk.size() * sizeof(float));
  if (null_lprob) memcpy(null_lprob, p.null_emission.data(), p.null_emission.size() * sizeof(float));
  if (bg_lprob) memcpy(bg_lprob, p.bg_emission.data(), p.bg_emission.size() * sizeof(float));
  if (accession)
  {
    strncpy(accession, p.accession.c_str(), 31);
    accession[31] = 0;
  }
  if (consensus) memcpy(consensus, p.consensus.c_str(), p.consensus.size() + 1);
  return 0;
}

void dcp_window_setup(struct dcp_window *w, int seq_size, int core_size)
{
  w->core_size = core_size;
  w->seq_size = seq_size;
  w->start = -1;
  w->stop = 0;
  w->idx = -1;
  w->last_hit_pos = -1;
}

int dcp_window_next(struct dcp_window *w)
{
  DcpWindow x(w->seq_size, w->core_size);
  x.start = w->start;
  x.stop = w->stop;
  x.idx = w->idx;
  x.last_hit_pos = w->last_hit_pos;
  bool ok = x.next();
  w->start = x.start;
  w->stop = x.stop;
  w->idx = x.idx;
  return ok ? 1 : 0;
}

int dcp_trellis_unzip(int K, int L, uint32_t const *xnodes, uint16_t const *nodes, int cap, int32_t *state_ids,
                      int32_t *seqsizes, int *nsteps)
{
  if (!xnodes || !nodes || !state_ids || !seqsizes || !nsteps || K < 1 || L < 0) return DCP_EFUNCUSE;
  std::vector<int32_t> ids, sizes;
  int rc = dcp_unzip(K, L, xnodes, nodes, ids, sizes);
  if (rc) return rc;
  *nsteps = (int)ids.size();
  if ((int)ids.size() > cap) return DCP_ENOMEM;
  memcpy(state_ids, ids.data(), ids.size() * sizeof(int32_t));
  memcpy(seqsizes, sizes.data(), sizes.size() * sizeof(int32_t));
  return 0;
}

struct dcp_scan_walk *dcp_scan_walk_new(int nprof, int32_t const *core_sizes, int nreads, int32_t const *read_lengths)
{
  if (nprof < 0 || nreads < 0 || (nprof && !core_sizes) || (nreads && !read_lengths)) return nullptr;
  return new dcp_scan_walk{DcpScanWalk(nprof, core_sizes, nreads, read_lengths)};
}

void dcp_scan_walk_del(struct dcp_scan_walk *x) { delete x; }

int dcp_scan_walk_chunk_windows(struct dcp_scan_walk *x, int32_t const c[4], int64_t windows, struct dcp_hip_window *wins,
                                int64_t *base)
{
  if (!x || !c || windows < 0 || (windows && !wins) || !base) return DCP_EFUNCUSE;
  return x->walk.chunk_windows(DcpChunk{c[0], c[1], c[2], c[3], windows}, wins, base);
}

int dcp_scan_walk_chunk_scored(struct dcp_scan_walk *x, int32_t const c[4], int64_t const *base, int nh,
                               int32_t const *hit_index, float const *lrts)
{
  if (!x || !c || !base || nh < 0 || (nh && (!hit_index || !lrts))) return DCP_EFUNCUSE;
  x->walk.chunk_scored(DcpChunk{c[0], c[1], c[2], c[3], 0}, base, nh, hit_index, lrts);
  return 0;
}

int dcp_scan_walk_all_pairs(struct dcp_scan_walk *x)
{
  if (!x) return DCP_EFUNCUSE;
  x->walk.all_pairs();
  return 0;
}

int64_t dcp_scan_walk_waiting(struct dcp_scan_walk const *x, int which)
{
  return !x ? 0 : (int64_t)(which ? x->walk.path_waiting() : x->walk.cost_waiting());
}

int64_t dcp_scan_walk_take(struct dcp_scan_walk *x, int which, struct dcp_hip_window const **wins)
{
  if (!x || !wins) return 0;
  std::vector<dcp_hip_window> const &w = which ? x->walk.take_path_batch() : x->walk.take_cost_round();
  *wins = w.data();
  return (int64_t)w.size();
}

int dcp_scan_walk_cost_scored(struct dcp_scan_walk *x, int nh, int32_t const *hit_index, float const *lrts)
{
  if (!x || nh < 0 || (nh && (!hit_index || !lrts))) return DCP_EFUNCUSE;
  x->walk.cost_scored(nh, hit_index, lrts);
  return 0;
}

int64_t dcp_scan_walk_path_walked(struct dcp_scan_walk *x, uint8_t const *is_hit, int32_t const *last_hit_pos,
                                  struct dcp_walk_hit const **hits)
{
  if (!x || !is_hit || !last_hit_pos || !hits) return 0;
  std::vector<dcp_walk_hit> const &h = x->walk.path_walked(is_hit, last_hit_pos);
  *hits = h.data();
  return (int64_t)h.size();
}

int64_t dcp_scan_walk_windows(struct dcp_scan_walk const *x) { return x ? (int64_t)x->walk.windows_walked() : 0; }
int64_t dcp_scan_walk_take_queued(struct dcp_scan_walk *x) { return x ? (int64_t)x->walk.take_queued() : 0; }

int dcp_path_hit(int nsteps, int32_t const *state_ids, int32_t const *seqsizes, int32_t hit[5])
{
  if (nsteps < 0 || !state_ids || !seqsizes || !hit) return 0;
  std::vector<int32_t> ids(state_ids, state_ids + nsteps), sizes(seqsizes, seqsizes + nsteps);
  DcpHit h;
  if (!dcp_find_hit(ids, sizes, h)) return 0;
  hit[0] = h.hit_start;
  hit[1] = h.hit_stop;
  hit[2] = h.begin_step;
  hit[3] = h.end_step;
  hit[4] = h.last_hit_pos;
  return 1;
}

void dcp_state_name_of(int state_id, char *name) { dcp_state_name(state_id, name); }
int dcp_state_is_mute_id(int state_id) { return dcp_state_is_mute(state_id) ? 1 : 0; }
float dcp_lrt_of(float null_loglik, float alt_loglik) { return dcp_lrt(null_loglik, alt_loglik); }

// ---- the random reads of a calibration (calibrate.h) and the tail of the fitted distribution ----
int dcp_random_thresholds(float const freq[4], uint32_t t[3])
{
  if (!t) return DCP_EFUNCUSE;
  return dcp_random_thresholds_of(freq, t) ? 0 : DCP_EFUNCUSE;
}

int dcp_random_nt(uint64_t seed, uint32_t const t[3], int64_t first_idx, int64_t n, uint8_t *out)
{
  if (!t || first_idx < 0 || n < 0 || (n > 0 && !out)) return DCP_EFUNCUSE;
  for (int64_t i = 0; i < n; ++i) out[i] = (uint8_t)dcp_random_base(seed, t[0], t[1], t[2], (uint64_t)first_idx + (uint64_t)i);
  return 0;
}

double dcp_lrt_evalue(float lrt, float mu, float lambda, double z)
{
  if (isnan(mu)) return NAN;
  return z * (-expm1(-exp(-(double)lambda * ((double)lrt - (double)mu))));
}

} // extern "C"
