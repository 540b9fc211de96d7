// engine_hmm.cpp -- the engine's profiles from a HMMER3 file: the load that presses them into HBM, and what presses the
// resident ones again in place, at another error rate (dcp_hip_set_epsilon) or under another translation table
// (dcp_hip_set_gencode).  Everything else about profiles: engine_profiles.cpp.
#include "engine_internal.h"
#include "engine_hmm.h"
#include "../../include/deciphon_host.h"
#include "press_batch.h"
#include "press_reemit.h"
#include "press_rows.h"

#include <limits.h>

// ---- from a HMMER3 file: the tables are made on the device and stay there ---------------------------------
// Profiles are parsed into batches as press does (press_batch.h).  Per batch, queued on the engine's stream: the
// nodes' distributions and the host-made transitions go up, the emission kernel (press_kernel.hip) writes the
// node-major tables into a scratch buffer of the slot, and the rows kernel (press_rows.hip) writes every profile's rows,
// cost-order copy and transitions into its slice of the pool.  Two slots: the host parses batch b + 1 while the GPU
// works on b.  Nothing comes back, and the profiles are published to the engine only when the whole range is in.
namespace
{

// where the rows and re-emission kernels write a profile's rows (press_out.h); src: its node 0 among the kernel's inputs
DcpRowsOut rows_out(HostProfile const &hp, int64_t src)
{
  ProfileLayout const lay(hp);
  DcpRowsOut o;
  o.src = src;
  o.rows_off = hp.pool_off + (int64_t)lay.rows;
  o.copy_off = hp.pool_off + (int64_t)lay.copy;
  o.K = hp.K;
  o.Kp = hp.Kp;
  o.stride = (int32_t)lay.stride;
  o.cQ = hp.cQ;
  o.poison = hp.poisoned;
  return o;
}

struct HmmSlot : DcpPressBatch
{
  PinBuf<float> h_in, h_trans;
  PinBuf<DcpRowsDesc> h_desc;
  DevBuf<float> d_em, d_trans; // (the inputs go up into the engine's kept distributions, dcp_hip::d_dist)
  DevBuf<DcpRowsDesc> d_desc;
  Event ev[4]; // before the uploads, after them, after the emission kernel, after the rows kernel
  bool launched = false;
};

struct HmmLoad
{
  dcp_hip *x;
  int gencode;
  float epsilon;
  HmmSlot slot[2];
  PinBuf<float> h_models;            // the null model and the background: two entries in, behind the engine's kept ones ...
  DevBuf<float> d_nullbg;            // ... and their tables, null[1364] then bg[1364]
  size_t used;                       // floats of the pool written so far, the resident profiles included
  // The engine keeps what the emission kernel reads (dcp_hip::d_dist, d_dist_models) for dcp_hip_set_epsilon: the
  // entries go up behind the kept ones and count as kept only when the whole load is in, as the pool's floats do.
  size_t dist_used;                  // node entries written so far, the kept ones included
  size_t const models_at;            // where this load's two model entries lie
  std::vector<HostProfile> added;
  bool const poison = cost_order_mode() == COST_ORDER_POISON;
  double t_parse = 0, t_upload = 0, t_emission = 0, t_rows = 0, t_wait = 0, t_grow = 0;
  int grown = 0; // times the pool was reallocated during the load
  StreamDrain drain; // (the last member: the stream is idle before the slots' buffers go)
  HmmLoad(dcp_hip *x_, int gencode_id, float eps)
      : x(x_), gencode(gencode_id), epsilon(eps), used(x_->pool_used), dist_used(x_->dist_used),
        models_at(x_->dist_models_used), drain{x_->cost_set.stream}
  {
  }

  int models(DcpHmmReader const &reader)
  {
    HIP_TRY(x, h_models.reserve(2 * DCP_PRESS_IN_STRIDE), DCP_ENOMEM);
    HIP_TRY(x, d_nullbg.reserve(2 * DCP_PRESS_TABLE), DCP_ENOMEM);
    if (int rc = grow_keeping(x, x->d_dist_models, (models_at + 2) * DCP_PRESS_IN_STRIDE, models_at * DCP_PRESS_IN_STRIDE))
      return rc;
    float *d_models = x->d_dist_models.p + models_at * DCP_PRESS_IN_STRIDE;
    dcp_press_put_entry(h_models.p, reader.null_dist());
    dcp_press_put_entry(h_models.p + DCP_PRESS_IN_STRIDE, reader.bg_dist());
    HIP_TRY(x, hipMemcpyAsync(d_models, h_models.p, 2 * DCP_PRESS_IN_STRIDE * sizeof(float), hipMemcpyHostToDevice, x->cost_set.stream),
            DCP_EFUNCUSE);
    if (dcp_press_emission_launch(d_models, d_nullbg.p, 2, epsilon, x->cost_set.stream))
      return fail(x, DCP_EFUNCUSE, "the emission kernel could not be launched");
    for (HmmSlot &s : slot)
      for (Event &e : s.ev) HIP_TRY(x, e.create(), DCP_ENOMEM);
    return 0;
  }

  // the kept distributions hold `entries` node entries; a reallocation keeps what is written, as grow() does
  int grow_dist(size_t entries)
  {
    return grow_keeping(x, x->d_dist, entries * DCP_PRESS_IN_STRIDE, dist_used * DCP_PRESS_IN_STRIDE);
  }

  // the pool holds `floats`; a reallocation waits for the stream and copies what is written (timed apart)
  int grow(size_t floats)
  {
    if (floats <= x->d_pool.cap) return 0;
    auto const t0 = std::chrono::steady_clock::now();
    int const rc = ensure_pool(x, floats, used);
    t_grow += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    ++grown;
    return rc;
  }

  // The pool is sized once, from the lengths the file's LENG lines announce for profiles [first, first + count): the
  // load then never reallocates, and nothing is held twice.  Only an estimate -- a file whose LENG lines are not one
  // per profile is not sized by them -- so launch() still grows the pool where it falls short.
  int presize(DcpHmmReader const &reader, long first, long count)
  {
    std::vector<long> const &len = reader.announced_lengths();
    if ((long)len.size() != reader.count()) return 0;
    long const last = count < 0 ? (long)len.size() : std::min((long)len.size(), first + count);
    size_t floats = 0, nodes = 0;
    for (long i = first; i < last; ++i)
    {
      HostProfile hp;
      if (len[(size_t)i] < 1 || len[(size_t)i] >= DCP_MODEL_MAX) return 0; // the load will fail there
      if (describe(x, (int)len[(size_t)i], nullptr, hp)) return 0;
      floats += ProfileLayout(hp).total;
      nodes += (size_t)hp.K;
    }
    if (!floats) return 0;
    if (int rc = grow(used + floats)) return rc;
    x->lodds.reserve((dist_used + nodes) * 20); // the kept distributions and log-odds are sized by the same lines
    return grow_dist(dist_used + nodes);
  }

  // the slot's batch is through: its buffers are free again
  int wait(HmmSlot &s)
  {
    if (!s.launched) return 0;
    s.launched = false;
    auto const t0 = std::chrono::steady_clock::now();
    HIP_TRY(x, hipEventSynchronize(s.ev[3].e), DCP_EFUNCUSE);
    t_wait += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    float ms[3] = {0, 0, 0};
    for (int i = 0; i < 3; ++i) HIP_TRY(x, hipEventElapsedTime(&ms[i], s.ev[i].e, s.ev[i + 1].e), DCP_EFUNCUSE);
    t_upload += ms[0] * 1e-3;
    t_emission += ms[1] * 1e-3;
    t_rows += ms[2] * 1e-3;
    return 0;
  }

  // the slot's pinned transition blocks and descriptors, profile i's block at toff[i] among the blocks
  int fill(HmmSlot &s, std::vector<HostProfile> const &hps, std::vector<size_t> const &toff)
  {
    for (size_t i = 0; i < hps.size(); ++i)
    {
      HostProfile const &hp = hps[i];
      DcpHmmProfile const &p = s.profiles[i];
      float *t = s.h_trans.p + toff[i];
      std::fill(t, s.h_trans.p + toff[i + 1], INFINITY);
      dcp_setup_trans(hp.K, hp.Kp, p.trans.data(), p.BMk.data(), t);
      if (!delete_costs_ok(t, hp.K, hp.Kp)) return fail(x, DCP_EFDATA, "positive (or NaN) delete log-probability in the profile");
      DcpRowsDesc &d = s.h_desc.p[i];
      d.out = rows_out(hp, s.first[i]);
      d.trans_off = hp.pool_off + (int64_t)ProfileLayout(hp).trans;
      d.trans_src = (int64_t)toff[i];
      d.trans_floats = (int32_t)(toff[i + 1] - toff[i]);
    }
    return 0;
  }

  // the slot's batch onto the stream: uploads, emission kernel, rows kernel, an event between each
  int queue(HmmSlot &s, size_t trans_floats, int max_Kp)
  {
    size_t const n = s.profiles.size(), entries = (size_t)s.entries;
    float *const d_in = x->d_dist.p + dist_used * DCP_PRESS_IN_STRIDE;
    hipStream_t const q = x->cost_set.stream;
    HIP_TRY(x, hipEventRecord(s.ev[0].e, q), DCP_EFUNCUSE);
    HIP_TRY(x, hipMemcpyAsync(d_in, s.h_in.p, entries * DCP_PRESS_IN_STRIDE * sizeof(float), hipMemcpyHostToDevice, q), DCP_EFUNCUSE);
    HIP_TRY(x, hipMemcpyAsync(s.d_trans.p, s.h_trans.p, trans_floats * sizeof(float), hipMemcpyHostToDevice, q), DCP_EFUNCUSE);
    HIP_TRY(x, hipMemcpyAsync(s.d_desc.p, s.h_desc.p, n * sizeof(DcpRowsDesc), hipMemcpyHostToDevice, q), DCP_EFUNCUSE);
    HIP_TRY(x, hipEventRecord(s.ev[1].e, q), DCP_EFUNCUSE);
    if (dcp_press_emission_launch(d_in, s.d_em.p, (int)entries, epsilon, q))
      return fail(x, DCP_EFUNCUSE, "the emission kernel could not be launched");
    HIP_TRY(x, hipEventRecord(s.ev[2].e, q), DCP_EFUNCUSE);
    if (dcp_press_rows_launch(s.d_em.p, d_nullbg.p, d_nullbg.p + DCP_PRESS_TABLE, s.d_trans.p, s.d_desc.p, (int)n, max_Kp,
                              x->d_pool.p, q))
      return fail(x, DCP_EFUNCUSE, "the rows kernel could not be launched");
    HIP_TRY(x, hipEventRecord(s.ev[3].e, q), DCP_EFUNCUSE);
    s.launched = true;
    return 0;
  }

  // describes the profiles of the slot's batch, builds their transitions and queues the batch
  int launch(HmmSlot &s, DcpHmmSink *sink)
  {
    size_t const n = s.profiles.size(), entries = (size_t)s.entries;
    std::vector<HostProfile> hps(n);
    std::vector<size_t> toff(n + 1, 0); // the transition blocks (trans and the padding behind it) as they are uploaded
    size_t floats = 0;
    int max_Kp = 0;
    for (size_t i = 0; i < n; ++i)
    {
      HostProfile &hp = hps[i];
      if (int rc = describe(x, s.profiles[i].core_size, s.profiles[i].accession.c_str(), hp)) return rc;
      ProfileLayout const lay(hp);
      hp.pool_off = (int64_t)(used + floats);
      hp.dist = (int64_t)dist_used + s.first[i];
      hp.dist_models = (int64_t)models_at;
      hp.epsilon = epsilon;
      hp.gencode = gencode;
      hp.poisoned = hp.cQ && poison;
      floats += lay.total;
      toff[i + 1] = toff[i] + (lay.pad_end - lay.trans);
      max_Kp = std::max(max_Kp, hp.Kp);
    }
    HIP_TRY(x, s.h_in.reserve(entries * DCP_PRESS_IN_STRIDE), DCP_ENOMEM);
    HIP_TRY(x, s.d_em.reserve(entries * DCP_PRESS_TABLE), DCP_ENOMEM);
    HIP_TRY(x, s.h_trans.reserve(toff[n]), DCP_ENOMEM);
    HIP_TRY(x, s.d_trans.reserve(toff[n]), DCP_ENOMEM);
    HIP_TRY(x, s.h_desc.reserve(n), DCP_ENOMEM);
    HIP_TRY(x, s.d_desc.reserve(n), DCP_ENOMEM);
    s.put_entries(s.h_in.p);
    if (int rc = fill(s, hps, toff)) return rc;
    if (int rc = grow(used + floats)) return rc;
    if (int rc = grow_dist(dist_used + entries)) return rc;
    if (int rc = queue(s, toff[n], max_Kp)) return rc;
    used += floats;
    dist_used += entries;
    // (behind the kept ones, in the order of the entries; dcp_hip_load_hmm_sink drops them again when the load fails)
    for (DcpHmmProfile const &p : s.profiles) x->lodds.insert(x->lodds.end(), p.lodds.begin(), p.lodds.end());
    if (sink)
      for (DcpHmmProfile const &p : s.profiles) sink->profile(p);
    added.insert(added.end(), hps.begin(), hps.end());
    return 0;
  }
};

// ---- resident profiles again, in place ----------------------------------------------------------------------
// The emission rows, cost-order copies and headers of every resident profile again from the kept distributions: per
// group of profiles at one error rate, the null and background tables of every load by the emission kernel, then the
// re-emission kernel (press_reemit.hip) over the (profile, 64 positions) pairs of the group's profiles.  The
// descriptors and the pair lists are built here and uploaded: 56 bytes per profile and 8 per pair.  Every profile of the
// engine is in exactly one group.
struct Reemit
{
  struct Group
  {
    float rate;                   // dcp_press_reemit_launch takes one
    std::vector<int32_t> members; // engine indices, ascending
  };
  dcp_hip *x;
  std::vector<Group> groups;
  std::vector<DcpReemitDesc> desc;             // per profile of the engine
  std::vector<int64_t> pair_begin;             // group g's pairs are [pair_begin[g], pair_begin[g + 1])
  std::vector<int32_t> pair_profile, pair_k0;  // (engine index, k0), the groups' lists one behind the other
  size_t nodes = 0, written = 0;               // of all profiles; floats the kernel writes
  DevBuf<DcpReemitDesc> d_desc;
  DevBuf<int32_t> d_pair_profile, d_pair_k0;
  DevBuf<float> d_tables; // per group, the null and background tables of every kept model entry at the group's rate
  Event ker[2];           // around the kernels

  Reemit(dcp_hip *x_, std::vector<Group> groups_) : x(x_), groups(std::move(groups_)), desc(x_->profiles.size()), pair_begin(groups.size() + 1, 0)
  {
    for (size_t i = 0; i < desc.size(); ++i)
    {
      HostProfile const &hp = x->profiles[i];
      ProfileLayout const lay(hp);
      desc[i].out = rows_out(hp, hp.dist);
      desc[i].null_row = (int32_t)hp.dist_models;
      desc[i].bg_row = desc[i].null_row + 1;
      nodes += (size_t)hp.K;
      written += (lay.trans - lay.rows) + (lay.total - lay.copy);
    }
    std::vector<std::vector<int32_t>> Kp(groups.size());
    for (size_t g = 0; g < groups.size(); ++g)
    {
      for (int32_t i : groups[g].members) Kp[g].push_back(x->profiles[(size_t)i].Kp);
      pair_begin[g + 1] = pair_begin[g] + dcp_reemit_tiles((int)Kp[g].size(), Kp[g].data(), nullptr, nullptr, 0);
    }
    pair_profile.resize((size_t)pair_begin.back());
    pair_k0.resize((size_t)pair_begin.back());
    for (size_t g = 0; g < groups.size(); ++g)
    {
      int64_t const count = pair_begin[g + 1] - pair_begin[g];
      int32_t *pp = pair_profile.data() + pair_begin[g];
      (void)dcp_reemit_tiles((int)Kp[g].size(), Kp[g].data(), pp, pair_k0.data() + pair_begin[g], count);
      for (int64_t j = 0; j < count; ++j) pp[j] = groups[g].members[(size_t)pp[j]]; // of the group -> of the engine
    }
  }

  // Everything of the run that can fail for want of memory, and the lists into it: nothing that the engine holds has
  // changed when this fails.
  int prepare()
  {
    size_t const n = desc.size(), pairs = pair_profile.size();
    HIP_TRY(x, d_desc.reserve(n), DCP_ENOMEM);
    HIP_TRY(x, d_pair_profile.reserve(pairs), DCP_ENOMEM);
    HIP_TRY(x, d_pair_k0.reserve(pairs), DCP_ENOMEM);
    HIP_TRY(x, d_tables.reserve(groups.size() * x->dist_models_used * DCP_PRESS_TABLE), DCP_ENOMEM);
    for (Event &e : ker) HIP_TRY(x, e.create(), DCP_ENOMEM);
    HIP_TRY(x, hipMemcpy(d_desc.p, desc.data(), n * sizeof(DcpReemitDesc), hipMemcpyHostToDevice), DCP_EFUNCUSE);
    HIP_TRY(x, hipMemcpy(d_pair_profile.p, pair_profile.data(), pairs * sizeof(int32_t), hipMemcpyHostToDevice), DCP_EFUNCUSE);
    HIP_TRY(x, hipMemcpy(d_pair_k0.p, pair_k0.data(), pairs * sizeof(int32_t), hipMemcpyHostToDevice), DCP_EFUNCUSE);
    return 0;
  }

  // queues the kernels of every group on the engine's stream, from the kept distributions as they are by then
  int run()
  {
    hipStream_t const q = x->cost_set.stream;
    size_t const models = x->dist_models_used;
    HIP_TRY(x, hipEventRecord(ker[0].e, q), DCP_EFUNCUSE);
    for (size_t g = 0; g < groups.size(); ++g)
    {
      float *tables = d_tables.p + g * models * DCP_PRESS_TABLE;
      if (dcp_press_emission_launch(x->d_dist_models.p, tables, (int)models, groups[g].rate, q))
        return fail(x, DCP_EFUNCUSE, "the emission kernel could not be launched");
      if (dcp_press_reemit_launch(x->d_dist.p, tables, d_desc.p, d_pair_profile.p + pair_begin[g], d_pair_k0.p + pair_begin[g],
                                  pair_begin[g + 1] - pair_begin[g], groups[g].rate, x->d_pool.p, q))
        return fail(x, DCP_EFUNCUSE, "the re-emission kernel could not be launched");
    }
    HIP_TRY(x, hipEventRecord(ker[1].e, q), DCP_EFUNCUSE);
    return 0;
  }

  // once the stream is idle: what the kernels took
  int kernel_seconds(double *s)
  {
    float ms = 0;
    HIP_TRY(x, hipEventElapsedTime(&ms, ker[0].e, ker[1].e), DCP_EFUNCUSE);
    *s = ms * 1e-3;
    return 0;
  }
};

// the first profile without kept distributions refuses dcp_hip_set_epsilon and dcp_hip_set_gencode
int refuse_without_dist(dcp_hip *x)
{
  for (size_t i = 0; i < x->profiles.size(); ++i)
    if (x->profiles[i].dist < 0)
    {
      char msg[128];
      snprintf(msg, sizeof msg, "profile %zu has no distributions kept: only dcp_hip_load_hmm keeps them", i);
      return fail(x, DCP_EFUNCUSE, msg);
    }
  return 0;
}

} // namespace

int dcp_hip_load_hmm_sink(struct dcp_hip *x, char const *hmm, int gencode_id, float epsilon, int first, int count,
                          DcpHmmSink *sink)
{
  if (!x || !hmm) return DCP_EFUNCUSE;
  if (outstanding_batches(x)) return refuse_outstanding(x);
  {
    DcpNucltDist probe;
    float const zero[20] = {};
    if (!dcp_setup_nuclt_dist(gencode_id, zero, probe)) return fail(x, DCP_EGENCODEID, "unknown translation table");
  }
  if (!(epsilon >= 0.0f && epsilon <= 1.0f)) return fail(x, DCP_EFUNCUSE, "epsilon must lie in [0, 1]");
  if (FILE *f = fopen(hmm, "rb")) fclose(f);
  else return fail(x, DCP_EOPENHMM, "cannot open the HMMER3 file");
  HIP_TRY(x, hipSetDevice(x->device), DCP_EFUNCUSE);
  DcpHmmReader reader;
  int rc = reader.open(hmm, gencode_id);
  if (rc) return fail(x, rc, "cannot read the HMMER3 file");
  // a `first` out of range is reported after what reading the file reports: everything is then in front of it
  bool const bad_first = first < 0 || (long)first > reader.count();
  long skip = bad_first ? LONG_MAX : first, limit = bad_first || count < 0 ? -1 : count;

  HmmLoad load(x, gencode_id, epsilon);
  // the amino log-odds go behind the kept ones batch by batch and count, as the entries in HBM do, once dist_used says so
  struct KeptLodds
  {
    dcp_hip *x;
    ~KeptLodds() { x->lodds.resize(x->dist_used * 20); }
  } kept_lodds{x};
  if ((rc = load.models(reader))) return rc;
  if (!bad_first && (rc = load.presize(reader, first, count))) return rc;
  if (sink) sink->models(reader.null_dist(), reader.bg_dist());
  DcpPressFeeder feeder;
  feeder.batch_nodes = dcp_press_batch_nodes();
  for (int b = 0;; b ^= 1)
  {
    HmmSlot &s = load.slot[b];
    if ((rc = load.wait(s))) break;
    auto const t0 = std::chrono::steady_clock::now();
    feeder.fill(reader, s, &skip, &limit);
    if (!s.profiles.empty()) rc = load.launch(s, sink);
    load.t_parse += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    if (rc) break;
    if (s.rc_after)
    {
      rc = fail(x, s.rc_after, "cannot read a profile of the HMMER3 file");
      break;
    }
    if (s.eof_after) break;
  }
  for (HmmSlot &s : load.slot)
    if (int const wrc = load.wait(s))
      if (!rc) rc = wrc;
  if (!rc) HIP_TRY(x, hipStreamSynchronize(x->cost_set.stream), DCP_EFUNCUSE); // (the null and background tables of an empty range)
  if (!rc && bad_first) rc = fail(x, DCP_EINVALPART, "first profile out of range");
  if (rc) return rc; // nothing of this load is kept: pool_used and the profiles are what they were
  if (getenv("DECIPHON_HIP_TIMING"))
    fprintf(stderr,
            "dcp_hip_load_hmm: %zu profiles, %.3f GB of tables; parse %.3f s, upload %.6f s, emission kernel %.6f s, "
            "rows kernel %.6f s, wait %.3f s; pool grown %d times in %.3f s (of parse); kept %zu bytes of distributions\n",
            load.added.size(), (double)(load.used - x->pool_used) * 4e-9, load.t_parse, load.t_upload, load.t_emission,
            load.t_rows, load.t_wait, load.grown, load.t_grow,
            (load.dist_used - x->dist_used + (load.added.empty() ? 0 : 2)) * DCP_PRESS_IN_STRIDE * sizeof(float));
  x->profiles.insert(x->profiles.end(), load.added.begin(), load.added.end());
  x->pool_used = load.used;
  x->dist_used = load.dist_used;
  if (!load.added.empty()) x->dist_models_used = load.models_at + 2; // (an empty range keeps no models either)
  ++x->gen;
  return 0;
}

// Every kept entry again under another table: the nodes' from their amino log-odds (dcp_hip::lodds) by
// dcp_regencode_entries, on the host threads, chunk by chunk into two pinned buffers whose uploads overlap the
// recomputation of the next chunk; the null model and the background of every load are the table's.  Then what
// dcp_hip_set_epsilon runs (Reemit), with one group per error rate among the profiles.
int dcp_hip_set_gencode_sink(struct dcp_hip *x, int gencode_id, DcpGencodeSink *sink)
{
  if (!x) return DCP_EFUNCUSE;
  if (outstanding_batches(x)) return refuse_outstanding(x);
  float null_lprobs[20];
  DcpNucltDist null, bg;
  if (!dcp_setup_models(gencode_id, null_lprobs, null, bg)) return fail(x, DCP_EGENCODEID, "unknown translation table");
  if (int rc = refuse_without_dist(x)) return rc;
  size_t const n = x->profiles.size();
  if (!n) return 0;
  if (x->lodds.size() != x->dist_used * 20) return fail(x, DCP_EFUNCUSE, "the kept amino log-odds do not match the kept distributions");
  HIP_TRY(x, hipSetDevice(x->device), DCP_EFUNCUSE);
  auto const t_begin = std::chrono::steady_clock::now();

  // the profiles by error rate, compared bit by bit
  std::vector<Reemit::Group> by_rate;
  for (size_t i = 0; i < n; ++i)
  {
    float const rate = x->profiles[i].epsilon;
    size_t g = 0;
    while (g < by_rate.size() && memcmp(&by_rate[g].rate, &rate, sizeof(float)) != 0) ++g;
    if (g == by_rate.size()) by_rate.push_back({rate, {}});
    by_rate[g].members.push_back((int32_t)i);
  }
  Reemit reemit(x, std::move(by_rate));

  // everything that can fail for want of memory, before the first byte of what the engine holds changes
  size_t const models = x->dist_models_used, kept = x->dist_used;
  size_t const entry_bytes = DCP_PRESS_IN_STRIDE * sizeof(float);
  size_t const chunk = std::min(std::max<size_t>(stage_bytes((size_t)64 << 20) / entry_bytes, 1), kept); // entries
  PinBuf<float> h_models, stage[2];
  Event up0[2], up1[2];
  if (int rc = reemit.prepare()) return rc;
  HIP_TRY(x, h_models.reserve(models * DCP_PRESS_IN_STRIDE), DCP_ENOMEM);
  for (int b = 0; b < 2; ++b)
  {
    HIP_TRY(x, stage[b].reserve(chunk * DCP_PRESS_IN_STRIDE), DCP_ENOMEM);
    HIP_TRY(x, up0[b].create(), DCP_ENOMEM);
    HIP_TRY(x, up1[b].create(), DCP_ENOMEM);
  }
  StreamDrain drain{x->cost_set.stream}; // (until the stream is idle the pinned buffers stay: an early return below waits for what it queued)

  // from here on the kept distributions change
  hipStream_t const q = x->cost_set.stream;
  if (sink) sink->regencoded(gencode_id, null, bg);
  for (size_t m = 0; m + 1 < models; m += 2)
  {
    dcp_press_put_entry(h_models.p + m * DCP_PRESS_IN_STRIDE, null);
    dcp_press_put_entry(h_models.p + (m + 1) * DCP_PRESS_IN_STRIDE, bg);
  }
  HIP_TRY(x, hipMemcpyAsync(x->d_dist_models.p, h_models.p, models * DCP_PRESS_IN_STRIDE * sizeof(float), hipMemcpyHostToDevice, q),
          DCP_EFUNCUSE);
  double t_host = 0, t_upload = 0, t_kernels = 0;
  bool busy[2] = {false, false};
  auto uploaded = [&](int b) -> int {
    if (!busy[b]) return 0;
    busy[b] = false;
    float ms = 0;
    HIP_TRY(x, hipEventSynchronize(up1[b].e), DCP_EFUNCUSE);
    HIP_TRY(x, hipEventElapsedTime(&ms, up0[b].e, up1[b].e), DCP_EFUNCUSE);
    t_upload += ms * 1e-3;
    return 0;
  };
  int b = 0;
  for (size_t c0 = 0; c0 < kept; c0 += chunk, b ^= 1)
  {
    size_t const c = std::min(chunk, kept - c0);
    if (int rc = uploaded(b)) return rc;
    auto const t0 = std::chrono::steady_clock::now();
    (void)dcp_regencode_entries(gencode_id, (int64_t)c, x->lodds.data() + 20 * c0, 16, stage[b].p); // (the table is held)
    t_host += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    if (sink) sink->entries(c0, c, stage[b].p);
    HIP_TRY(x, hipEventRecord(up0[b].e, q), DCP_EFUNCUSE);
    HIP_TRY(x, hipMemcpyAsync(x->d_dist.p + c0 * DCP_PRESS_IN_STRIDE, stage[b].p, c * entry_bytes, hipMemcpyHostToDevice, q),
            DCP_EFUNCUSE);
    HIP_TRY(x, hipEventRecord(up1[b].e, q), DCP_EFUNCUSE);
    busy[b] = true;
  }
  if (int rc = reemit.run()) return rc;
  for (int s = 0; s < 2; ++s)
    if (int rc = uploaded(s)) return rc;
  HIP_TRY(x, hipStreamSynchronize(q), DCP_EFUNCUSE);
  if (getenv("DECIPHON_HIP_TIMING"))
  {
    if (int rc = reemit.kernel_seconds(&t_kernels)) return rc;
    fprintf(stderr,
            "dcp_hip_set_gencode: %zu profiles, %zu nodes, table %d, %zu error rates; host recomputation %.6f s, upload %.6f s, "
            "kernels %.6f s, wall %.6f s\n",
            n, reemit.nodes, gencode_id, reemit.groups.size(), t_host, t_upload, t_kernels,
            std::chrono::duration<double>(std::chrono::steady_clock::now() - t_begin).count());
  }
  for (HostProfile &hp : x->profiles) hp.gencode = gencode_id;
  ++x->gen;
  drop_calibration(x);
  return 0;
}

extern "C" {

int dcp_hip_load_hmm(struct dcp_hip *x, char const *hmm, int gencode_id, float epsilon, int first, int count)
{
  return dcp_hip_load_hmm_sink(x, hmm, gencode_id, epsilon, first, count, nullptr);
}

// Every profile's rows, cost-order copy and headers again, at `epsilon`, from the kept distributions: Reemit with all
// profiles in one group, so one launch of the re-emission kernel over all (profile, 64 positions) pairs in engine order.
int dcp_hip_set_epsilon(struct dcp_hip *x, float epsilon)
{
  if (!x) return DCP_EFUNCUSE;
  if (outstanding_batches(x)) return refuse_outstanding(x);
  if (!(epsilon >= 0.0f && epsilon <= 1.0f)) return fail(x, DCP_EFUNCUSE, "epsilon must lie in [0, 1]");
  size_t const n = x->profiles.size();
  if (int rc = refuse_without_dist(x)) return rc;
  if (!n) return 0;
  HIP_TRY(x, hipSetDevice(x->device), DCP_EFUNCUSE);

  std::vector<Reemit::Group> all(1);
  all[0].rate = epsilon;
  for (size_t i = 0; i < n; ++i) all[0].members.push_back((int32_t)i);
  Reemit reemit(x, std::move(all));
  if (int rc = reemit.prepare()) return rc;
  if (int rc = reemit.run()) return rc;
  HIP_TRY(x, hipStreamSynchronize(x->cost_set.stream), DCP_EFUNCUSE);
  if (getenv("DECIPHON_HIP_TIMING"))
  {
    // (the seconds are Reemit's: with the emission kernel over the loads' null models and backgrounds in front)
    double s = 0;
    if (int rc = reemit.kernel_seconds(&s)) return rc;
    fprintf(stderr, "dcp_hip_set_epsilon: %zu profiles, %zu nodes, %zu bytes written; re-emission kernel %.6f s\n", n,
            reemit.nodes, reemit.written * sizeof(float), s);
  }
  for (HostProfile &hp : x->profiles) hp.epsilon = epsilon;
  ++x->gen;
  drop_calibration(x);
  return 0;
}

float dcp_hip_profile_epsilon(struct dcp_hip const *x, int i)
{
  if (!x || i < 0 || i >= (int)x->profiles.size() || x->profiles[(size_t)i].dist < 0) return NAN;
  return x->profiles[(size_t)i].epsilon;
}

int dcp_hip_set_gencode(struct dcp_hip *x, int gencode_id) { return dcp_hip_set_gencode_sink(x, gencode_id, nullptr); }

int dcp_hip_profile_gencode(struct dcp_hip const *x, int i)
{
  if (!x || i < 0 || i >= (int)x->profiles.size() || x->profiles[(size_t)i].dist < 0) return 0;
  return x->profiles[(size_t)i].gencode;
}

int64_t dcp_hip_dist_bytes(struct dcp_hip const *x)
{
  return x ? (int64_t)((x->dist_used + x->dist_models_used) * DCP_PRESS_IN_STRIDE * sizeof(float)) : 0;
}

} // extern "C"
